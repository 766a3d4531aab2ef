// bge_fuse_math.hpp — the ticks of a vouched wave in registers (fused ticks, solo groups; DESIGN.md §4.1 "Lean fusion").
//
// Plain C++ that the kernel (bge_kernels.hip) and a host program (tests/cpp/fuse_math.cpp) both compile: what differs between
// them is the wave W and nothing else.
//   W::any(m)          is m true in any lane?  (kernel: a ballot; host: a loop over the lanes)
//   W::abs(v)          |v| per lane
//   W::same_bits(a, b) per lane: are a and b the same 32 bits?
// and the type of a lane value (float in the kernel, where the 64 lanes are the hardware's; a 64-float array with per-lane
// operators on the host).  T3 is any {x, y, z} of lane values.  Every operation is one IEEE binary32 rounding (the translation
// units are compiled with -ffp-contract=off), so both builds run the same expressions in the same order.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BGE_FUSE_FN __device__ __forceinline__
#else
#define BGE_FUSE_FN inline
#endif
#if defined(__clang__)
#define BGE_FUSE_UNROLL _Pragma("unroll 2")
#else
#define BGE_FUSE_UNROLL
#endif

namespace bge {
namespace fuse {

// What a tick adds, the same in every tick of a group: the gravity impulse c = (gf.xyz * gf.w) * dt (applyGravity), the step
// and the sleep threshold (the slow-lane ballot).
struct Step {
    float cx, cy, cz, dt, sleep_lin;
};

// How a wave's group was decided (the host test counts them; the kernel passes nullptr and the stores fold away).
//   kLean           the lean loop's answer stood
//   kExactAccepted  the end test refused, the exact loop accepted (a lane jumped the band)
//   kExactRefused   the end test refused, and so did the exact loop
//   kNotFixed       x / z velocity was no fixed point: the exact loop alone
//   kFirstTick      the first tick's own ballot refused
enum Path : uint32_t { kLean = 0, kExactAccepted = 1, kExactRefused = 2, kNotFixed = 3, kFirstTick = 4 };

// The exact rule, and the fallback: n ticks, each with the single tick's expressions — applyGravity, the slow-lane ballot,
// integrateTransforms — in their order.  false: a lane turned slow in one of them, and nothing is to be stored.
template <class W, class T3> BGE_FUSE_FN bool fuse_ticks_exact(const Step& c, uint32_t n, T3& vn, T3& xn)
{
    for (uint32_t i = 0; i < n; ++i) {
        vn = T3{vn.x + c.cx, vn.y + c.cy, vn.z + c.cz};
        if (W::any(!(W::abs(vn.y) >= c.sleep_lin))) return false;
        xn = T3{xn.x + vn.x * c.dt, xn.y + vn.y * c.dt, xn.z + vn.z * c.dt};
    }
    return true;
}

// The same answer — the same flag and, where true, the same bits in vn and xn — with only what changes from tick to tick inside
// the loop.  Stores nothing; every decision is wave-wide.
//   * Tick 1 is the single tick, ballot and all.
//   * If v1.x + cx and v1.z + cz give back the bits of v1.x and v1.z in every lane, every later tick forms the same sums from the
//     same operands: x and z velocity are fixed, and so are the products v1.x * dt and v1.z * dt.  (True wherever gravity has no
//     x or z part: v + 0 == v from the second tick on — the first may still turn a -0 into +0.)
//   * Ticks 2..n then have no compare and no exit: one add for v.y, one product, three adds for the position, each rounded as in
//     the exact loop and with its operands in the same order.
//   * v.y moves by one lane-constant step per tick and rounding is monotone, so the sequence is monotone: with its first and last
//     value on one side of the band, no tick's ballot could have seen the lane inside it.
// A wave with a lane that fails either test — it crosses the band or jumps over it, holds a NaN, feels a sideways gravity that is
// not absorbed, or the threshold is no ordinary one — runs the exact loop from the loaded values and takes its answer.  That is the
// rare wave: it has paid the lean loop for nothing, a few instructions per tick where the exact loop costs several times that.
template <class W, class T3> BGE_FUSE_FN bool fuse_ticks(const Step& c, uint32_t n, T3& vn, T3& xn, uint32_t* path = nullptr)
{
    if (n == 0u) return true;
    const T3 v1{vn.x + c.cx, vn.y + c.cy, vn.z + c.cz};
    if (W::any(!(W::abs(v1.y) >= c.sleep_lin))) {
        if (path) *path = kFirstTick;
        return false;
    }
    const bool fixed = !W::any(!(W::same_bits(v1.x + c.cx, v1.x) && W::same_bits(v1.z + c.cz, v1.z)));
    if (fixed) {
        const auto dx = v1.x * c.dt, dz = v1.z * c.dt;
        auto vy = v1.y;
        T3 x{xn.x + dx, xn.y + vy * c.dt, xn.z + dz};
        BGE_FUSE_UNROLL
        for (uint32_t i = 1; i < n; ++i) {
            vy = vy + c.cy;
            x = T3{x.x + dx, x.y + vy * c.dt, x.z + dz};
        }
        const float s = c.sleep_lin;
        if (!W::any(!((v1.y >= s && vy >= s) || (v1.y <= -s && vy <= -s)))) {
            if (path) *path = kLean;
            vn = T3{v1.x, vy, v1.z};
            xn = x;
            return true;
        }
    }
    // (one copy of the exact loop for both ways into it)
    const bool ok = fuse_ticks_exact<W>(c, n, vn, xn);
    if (path) *path = !fixed ? kNotFixed : ok ? kExactAccepted : kExactRefused;
    return ok;
}

} // namespace fuse
} // namespace bge
