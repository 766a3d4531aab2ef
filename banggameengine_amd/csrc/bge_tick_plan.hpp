// bge_tick_plan.hpp — what a bge_world_tick_many call decides before its first launch (TickPlan: which paths of the tick kernel are
// on, whether the call goes out in fused or solo groups, and of what size) and what each tick's launch carries (TickGroups), from
// the tick flags, a few facts about the scene (TickScene) and the BGE_* switches (TickKnobs).  Host-only, no HIP, no state of its
// own: tests/cpp/tick_plan.cpp runs every combination against a transcription of the expressions this header replaced.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>

#include "../../include/bge_world.h"
#include "bge_epochs.hpp"

namespace bge {

constexpr uint32_t kFuseTicksDefault = 8; // ticks per fused group of a bge_world_tick_many call (BGE_FUSE_TICKS; DESIGN.md §4.1 "Fused ticks": measured)
constexpr uint32_t kSoloTicksDefault = 512; // ticks per solo group, where BGE_FUSE_TICKS is unset (DESIGN.md §4.1 "Lean fusion": measured again with the reduced loop — the smallest of 64 .. 1024 whose median lies within the parent's spread of the best)
constexpr double kNtThresholdBytes = 300.0e6; // measured crossover between 2 M (plain wins) and 4 M slots (nt wins)

// The k_tick instantiations that carry the translation-row path, the rest path and the flag word (and, with PHYS, fused ticks):
// transforms, with or without the default physics step, and nothing else.  The kernel (kRowsPath), launch_tick (the solo variant)
// and the host gate below all take it from here.
constexpr bool tick_variant_has_rows_path(bool xform, bool aabb, bool normal, bool basis) { return xform && !aabb && !normal && !basis; }

// The switches of the tick path, read from the environment once per call (tests change them between calls on a live world).
struct TickKnobs {
    int nt_stores = -1;       // BGE_NT_STORES=0/1 overrides TickPlan::nt_out either way (experiments); -1: unset
    bool world_rows = true;   // BGE_WORLD_ROWS=0 turns the translation-row path off (A/B runs)
    bool defer_row3 = true;   // BGE_DEFER_ROW3=0 turns the deferred translation row off (A/B runs)
    bool flag_word = true;    // BGE_FLAG_WORD=0 turns the flag-word block off (A/B runs)
    bool rest_path = true;    // BGE_REST_PATH=0 turns the rest path off (A/B runs)
    bool solo_groups = true;  // BGE_SOLO_GROUPS=0 turns solo groups off (A/B runs): round 9's scheme, one launch per tick
    uint32_t fuse_ticks = 0;  // BGE_FUSE_TICKS=T sets the group size; 1 is off (A/B runs).  0: unset, the defaults above apply
    static TickKnobs from_env()
    {
        const auto on = [](const char* name) {
            const char* e = std::getenv(name);
            return !e || std::atoi(e) != 0;
        };
        TickKnobs k;
        if (const char* e = std::getenv("BGE_NT_STORES")) k.nt_stores = std::atoi(e) != 0;
        k.world_rows = on("BGE_WORLD_ROWS");
        k.defer_row3 = on("BGE_DEFER_ROW3");
        k.flag_word = on("BGE_FLAG_WORD");
        k.rest_path = on("BGE_REST_PATH");
        k.solo_groups = on("BGE_SOLO_GROUPS");
        if (const char* e = std::getenv("BGE_FUSE_TICKS")) k.fuse_ticks = static_cast<uint32_t>(std::max(1, std::atoi(e)));
        return k;
    }
};

// What the decision reads from the world
struct TickScene {
    uint64_t n_slots = 0;
    size_t n_passes = 1;
    bool any_frozen = false;
    bool contact_stages = false; // ground plane, obstacles or Dynamic contacts are on
    bool all_flat = false, any_flat_all_dynamic = false; // bge_flatten.hpp TileShape
    int profiling = 0;           // 0 off, 1 one event pair per call, 2 one per tick
};

struct TickPlan {
    // Output stores: non-temporal once the tick's working set (~140 B per slot, 204 B with normal matrices) no longer
    // fits the 256 MiB Infinity Cache; BGE_NT_STORES=0/1 overrides (experiments)
    bool nt_out;
    bool contacts; // the tick runs the contact stage in front of the tick kernel
    // Translation-row fast path of the tick kernel (WorldView::rs_word): only in the variants it exists in (transforms, with or
    // without the default physics step, nothing else), and only where no other kernel of the tick writes euler, scale, world
    // or quat (ground plane, obstacles, Dynamic contacts).  Only while the working set fits the Infinity Cache, unless the
    // tick defers the row (below): beyond it a 16-B store into every 64-B matrix costs more than the whole matrix
    // (tools/ubench_world_rows.hip: 16 M slots, 2.7x).
    // BGE_WORLD_ROWS=0 turns it off (A/B runs); a tick without it moves the epoch on, so that no word outlives what it vouched for.
    bool rows_path;
    // Deferred translation row (bge_epochs.hpp Row3State): translation-row waves do not store row 3 either; the readers that run every
    // frame compose it, everything else stores it first (bge_world::ensure_row3_current).  BGE_DEFER_ROW3=0 turns it off (A/B runs).
    // A deferring tick writes no partial matrix line, so the Infinity Cache limit above does not apply to it (the first, full-path
    // ticks keep their non-temporal stores).
    bool defer_row3;
    // Vouched waves of the translation-row path (WorldView::rs_word, words 2 and 3): a wave whose 64 flag words are known to be one
    // clean value skips the flags read.  The words are kept whether or not the block runs; BGE_FLAG_WORD=0 turns the block off (A/B runs).
    bool flag_word;
    // Rest path of the tick kernel (WorldView::rs_word, word 1): waves whose bodies are all asleep read 12 B per body and store
    // nothing.  In the same variants as the translation-row path — but ON with the ground plane, obstacles and Dynamic contacts,
    // where a scene at rest spends its life: every kernel of the contact stage either leaves a sleeping body alone or marks its
    // flags, deactivation record or contact word.  It stores nothing, so the non-temporal regime needs no
    // exclusion.  BGE_REST_PATH=0 turns it off (A/B runs); a tick without it moves its epoch on.
    bool rest_path;
    // Fused ticks (bge_epochs.hpp FuseClock, TickParams::serial): the ticks of this call go out in groups of at most group_T launches, and
    // a vouched wave runs the ticks that remain of its group in the first launch that finds it vouched; the group's later launches
    // return at once for it.  Only the physics + transform tick on the translation-row path with the flag word, only in a scene of
    // one pass without a frozen root (Row3State::may_defer's conditions without `pinned`: in any other scene a child of a later pass
    // reads a flat root's matrix inside the tick, and that must be the matrix of that very tick), and not with an event pair per
    // tick, which wants launches of equal meaning.  BGE_FUSE_TICKS=T sets the group size; 1 is off (A/B runs).  Groups never span calls.
    // If a launch fails in the middle of a group, some waves are ahead of others: the error is returned as ever, and the world is
    // not usable after a failed tick call (include/bge_world.h).
    // (only a flat all-Dynamic tile can hold a vouched wave: without one, no launch loads a word that can never be set)
    bool fusable;
    // Solo groups (bge_epochs.hpp SoloPlan, TickParams::n_solo): where every tile is flat, the first tick of a group launches ONE
    // kernel in which every wave runs the group's ticks itself — fused in registers where it is vouched, one after the other by the
    // ordinary path where it is not — and the group's other ticks launch nothing.  They still do all of the tick loop's bookkeeping.
    // No serial, no adv.  BGE_SOLO_GROUPS=0 turns it off (A/B runs): round 9's scheme, one launch per tick.  Every fusable scene
    // that is not all-flat keeps that scheme.
    bool solo;
    uint32_t group_T; // ticks per group, >= 1 (a solo group costs one launch whatever its size: its default is its own)

    static TickPlan of(uint32_t flags, const TickScene& s, const TickKnobs& k, const Row3State& row3)
    {
        const bool phys = (flags & BGE_TICK_PHYSICS) != 0, xform = (flags & BGE_TICK_TRANSFORMS) != 0;
        const bool normal = (flags & BGE_TICK_NORMAL_MATRICES) != 0;
        // (nor in a tick that gathers its roots)
        const bool variant = tick_variant_has_rows_path(xform, (flags & (BGE_TICK_AABBS | BGE_TICK_BROADPHASE)) != 0, normal, (flags & BGE_TICK_BULLET_BASIS) != 0) &&
                             !(flags & BGE_TICK_GATHER_ROOTS);
        const bool can_defer = row3.may_defer(true, s.n_passes, s.any_frozen, k.defer_row3);
        TickPlan p{};
        p.nt_out = k.nt_stores >= 0 ? k.nt_stores != 0 : static_cast<double>(s.n_slots) * (normal ? 204.0 : 140.0) > kNtThresholdBytes;
        p.contacts = phys && s.contact_stages;
        p.rows_path = variant && !p.contacts && (!p.nt_out || can_defer) && k.world_rows;
        p.defer_row3 = p.rows_path && can_defer;
        p.flag_word = p.rows_path && k.flag_word;
        p.rest_path = variant && k.rest_path;
        p.fusable = phys && p.rows_path && p.flag_word && s.n_passes == 1 && !s.any_frozen && s.profiling != 2 && s.any_flat_all_dynamic;
        p.solo = SoloPlan::wanted(p.fusable, s.all_flat, k.solo_groups);
        p.group_T = k.fuse_ticks ? k.fuse_ticks : p.solo ? kSoloTicksDefault : kFuseTicksDefault;
        return p;
    }
};

// The groups of one call: next() is called once for every tick t = 0 .. ticks-1 that launches anything, in order, and says what
// that tick's launch carries.  Built on FuseClock's cut and serials and on SoloPlan; a solo group takes no serial.
class TickGroups {
public:
    struct Tick {
        uint32_t serial, n_left, n_solo; // TickParams' fields of the same names
        bool launch;                     // false: a later tick of a solo group — its work is in the group's launch
        bool clear_adv;                  // the clock wrapped: WorldView::adv is zeroed on the stream before this tick's launch
    };
    TickGroups(const TickPlan& plan, uint32_t ticks) : grouped_(plan.fusable && plan.group_T > 1u), solo_(plan.solo), T_(plan.group_T), ticks_(ticks) {}
    Tick next(uint32_t t, FuseClock& clock)
    {
        bool wrapped = false;
        if (grouped_ && t == t0_ + n_) {
            t0_ = t;
            n_ = FuseClock::group_size(t, ticks_, T_);
            if (!solo_) first_ = clock.begin_group(n_, &wrapped);
        }
        const uint32_t i = t - t0_;
        // (a group of one tick has nothing to fuse: it goes out as every tick did, and no word is loaded)
        const bool fused = grouped_ && n_ > 1u && !solo_;
        const SoloPlan solo = SoloPlan::plan(solo_ && T_ > 1u, i, n_);
        return Tick{fused ? first_ + i : 0u, fused ? n_ - i : 1u, solo.n_solo, solo.launch, wrapped};
    }

private:
    bool grouped_, solo_;
    uint32_t T_, ticks_;
    uint32_t first_ = 0, t0_ = 0, n_ = 0; // the group tick t belongs to: its first serial, its first tick, its size
};

} // namespace bge
