// bge_epochs.hpp — the two epochs the tick kernel's per-wave words (WorldView::rs_word) are compared with, and the bookkeeping of
// the deferred translation row (Row3State, below), of fused ticks (FuseClock, below) and of solo groups (SoloPlan, below).  Host-only, no HIP: tests/test_rest_epoch_cpu.py and tests/test_row3_epoch_cpu.py
// compile this header on its own.  Which tick takes which path, defers, fuses or goes out in solo groups is decided from these pieces
// in bge_tick_plan.hpp (TickPlan, TickGroups).
//   rows  what word 0 must equal for the translation-row path (TickParams::rs_epoch)
//   rest  what word 1 must equal for the rest path (TickParams::rest_epoch)
// A bump invalidates every word of its kind at once.  The rules:
//   host_edit()          every call that can write a body's or a Transform's state, the flags, or what kernels a tick launches:
//                        BOTH epochs move.  There is no way to move `rows` for an edit and leave `rest` behind.
//   tick_without_rows()  a tick that is launched without the translation-row path (another kernel of the tick writes euler, scale,
//                        world or quat, or the variant has no such path): only `rows` moves — the rest path is built to live there.
//   tick_without_rest()  a tick launched in a variant without the rest path: only `rest` moves.
// Each returns true when its epoch wrapped (after 2^32 - 1 bumps a word may still hold the new value): the caller zeroes the words.
#pragma once
#include <cstddef>
#include <cstdint>

namespace bge {

struct PathEpochs {
    uint32_t rows = 1, rest = 1; // (0 means "path off" in TickParams: never a live value)
    bool host_edit()
    {
        const bool a = bump(rows), b = bump(rest);
        return a || b;
    }
    bool tick_without_rows() { return bump(rows); }
    bool tick_without_rest() { return bump(rest); }

private:
    static bool bump(uint32_t& e)
    {
        if (++e != 0) return false;
        e = 1;
        return true;
    }
};

// The deferred translation row (DESIGN.md §4.1 "Deferred translation row"): host bookkeeping, no device state of its own.
// A deferring tick (TickParams::defer_row3) leaves world row 3 of every wave that takes the translation-row path unstored; until
// the next k_row3_sync, row 3 of slot s is  (pos[s], 1)  if  rs_word[wave(s)].x == pending  and what memory holds otherwise.
//   pending  the rows epoch the deferring ticks since the last sync ran under; 0: every stored row 3 is current.  Readers that
//            compose pass it on as their epoch (0 never equals a word of a live path: PathEpochs never hands out 0).
//   pinned   the world or position array was handed out as a raw pointer (bge_world_device_array): no tick defers again.
// The one rule the callers keep: take_sync() — and the kernel launch it asks for — comes BEFORE the rows epoch moves, before the
// words are zeroed, and before anything but a rows-path tick writes pos or world.
struct Row3State {
    uint32_t pending = 0;
    bool pinned = false;
    // May this tick defer?  Only a translation-row tick of a scene with a single pass and no frozen root: in any other scene a
    // child of a later pass (or a frozen root) reads a stored matrix from memory inside the tick.
    bool may_defer(bool rows_path, size_t n_passes, bool any_frozen, bool enabled) const
    {
        return rows_path && enabled && !pinned && n_passes == 1 && !any_frozen;
    }
    void deferred(uint32_t rows_epoch) { pending = rows_epoch; }
    // The epoch k_row3_sync has to run with, or 0 when nothing is due; memory counts as current from here on.
    uint32_t take_sync()
    {
        const uint32_t e = pending;
        pending = 0;
        return e;
    }
};

// Fused ticks (DESIGN.md §4.1 "Fused ticks"): the serials that the launches of a bge_world_tick_many call carry (TickParams::serial) and
// the per-wave words WorldView::adv are compared with.  Host bookkeeping only.  The K ticks of a call are cut into groups of at
// most T; launch i (0-based) of a group of n carries serial first + i and n_left = n - i, and a vouched wave that runs the n_left
// ticks in one launch writes adv = first + n - 1, the group's last serial.  Serials only ever rise, so a word written by one group
// is below every serial of every later group; groups never span calls, so between calls every wave's memory is at the same tick.
//   next         the first serial of the next group, >= 1 (0 is "off" in TickParams, and what a zeroed word holds)
//   begin_group  hands out n consecutive serials and returns the first.  *wrapped = true: the 32-bit range is used up, the serials
//                restart at 1 and the caller zeroes the adv array with a memset ordered on the stream BEFORE the group's launches
struct FuseClock {
    uint32_t next = 1;
    uint32_t begin_group(uint32_t n, bool* wrapped)
    {
        *wrapped = n > 0xffffffffu - next; // (next + n - 1 must be a serial, and next + n the next group's first)
        if (*wrapped) next = 1;
        const uint32_t first = next;
        next += n;
        return first;
    }
    // Ticks in the group that begins at tick t of a call of `ticks`, for groups of at most T (T >= 1): the last takes the remainder
    static uint32_t group_size(uint32_t t, uint32_t ticks, uint32_t T) { return ticks - t < T ? ticks - t : T; }
};

// Solo groups (DESIGN.md §4.1 "Solo groups"): in a scene whose every tile is flat (bge_flatten.hpp TileShape::all_flat) no wave reads
// what another wave writes during a tick, so a wave can run the ticks of a group one after the other inside ONE launch, and the
// host launches once per group and needs no answer from the device.  The groups are FuseClock's (same cut, same T); no serial is
// handed out and WorldView::adv is not touched.
//   wanted  the call goes out in solo groups: it is fusable, the scene is all-flat, and BGE_SOLO_GROUPS allows it
//   plan    tick i (0-based) of a group of n: does it launch, and with which TickParams::n_solo.  The first tick of a group of
//           n > 1 launches with n_solo = n and the others launch nothing; a group of one, and every tick of a call that is not in
//           solo groups, launches as a plain tick (n_solo = 0: the ordinary kernel).
struct SoloPlan {
    bool launch;
    uint32_t n_solo;
    static bool wanted(bool fusable, bool all_flat, bool enabled) { return fusable && all_flat && enabled; }
    static SoloPlan plan(bool solo, uint32_t i, uint32_t n)
    {
        if (!solo || n <= 1u) return SoloPlan{true, 0u};
        return i == 0u ? SoloPlan{true, n} : SoloPlan{false, 0u};
    }
};

} // namespace bge
