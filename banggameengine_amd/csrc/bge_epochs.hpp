// bge_epochs.hpp — the two epochs the tick kernel's per-wave words (WorldView::rs_word) are compared with.  Host-only, no HIP:
// tests/test_rest_epoch_cpu.py compiles this header on its own.
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

} // namespace bge
