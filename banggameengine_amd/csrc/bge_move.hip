// bge_move.hip — sphere moves: batched collide-and-slide against the device world (include/bge_world.h "Sphere moves",
// bge_world_sphere_move*).
//
// The mover sees the world only through the closest-hit sphere cast (bge_query.hip), so a batch of moves is BGE_MOVE_SLIDES + 1
// passes of that cast with a few lines of arithmetic per mover in between.  The three kernels here are that arithmetic, one
// thread per mover, and they never look at a body:
//   k_move_begin   validates the mover, initialises its state and writes the cast of round 0.
//   k_move_step    reads the hit of the round's pass, applies steps 3-7 of the rule and writes the next round's cast; after the
//                  last slide round it writes the ground probe's cast instead.
//   k_move_finish  reads the probe's hit and writes the 80-byte result.
// A mover that is finished (nothing left to spend, or it moved freely) or invalid asks a cast with layer_mask = 0, which by the
// cast's own rule hits nothing; no loop here or in the passes depends on the data.  The state lives in planes of float4
// (bge_move.hpp), so every access to it is 64 consecutive 16-byte words per wave; the caller's records and the cast / hit records
// are only 4-byte aligned by their ABI and are moved word by word, as the query kernels do.
// The expressions below are the header's, operation for operation (the build's -ffp-contract=off keeps one rounding each).
#include <hip/hip_runtime.h>

#include "../../include/bge_world.h"
#include "bge_move.hpp"
#include "bge_move_device.hpp"

namespace bge {

namespace {

constexpr uint32_t kThreads = 256;
using namespace slide; // dot3, write_cast, spent, the bits and the constants (bge_move_device.hpp)

__global__ void __launch_bounds__(kThreads) k_move_begin(MoveParams p)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= p.n) return;
    const uint32_t* m = static_cast<const uint32_t*>(p.moves) + 12ull * i;
    float v[10];
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 10; ++k) {
        v[k] = __uint_as_float(m[k]);
        finite = finite && __builtin_isfinite(v[k]);
    }
    const uint32_t mask = m[10];
    const bool valid = finite && v[6] >= 0.0f && v[7] > 0.0f && v[8] >= 0.0f && mask != 0u;
    const float4 pos = make_float4(v[0], v[1], v[2], v[6]);
    float4 r = make_float4(v[3], v[4], v[5], v[7]);
    uint32_t bits = 0u;
    if (!valid) {
        bits = BGE_MOVE_INVALID | kFinished;
        r.x = r.y = r.z = 0.0f;
    } else if (spent(r)) {
        bits = kFinished;
        r.x = r.y = r.z = 0.0f;
    }
    const uint64_t n = p.n;
    p.state[i] = pos;
    p.state[n + i] = r;
    p.state[2 * n + i] = make_float4(v[3], v[4], v[5], __uint_as_float(mask));
    p.state[3 * n + i] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(bits));
    p.state[4 * n + i] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(BGE_RAY_NO_ENTITY));
    p.state[5 * n + i] = make_float4(v[8], v[9], 0.0f, 0.0f);
    write_cast(p.casts, i, pos, r.x, r.y, r.z, 1.0f, (bits & kFinished) ? 0u : mask);
}

__global__ void __launch_bounds__(kThreads) k_move_step(MoveParams p, uint32_t last)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= p.n) return;
    const uint64_t n = p.n;
    float4 prev = p.state[3 * n + i];
    uint32_t bits = __float_as_uint(prev.w);
    // A finished mover's cast already asks nothing: the kernel that finished it (k_move_begin or an earlier step) wrote it with
    // layer_mask 0, and between the kernels of one call only these kernels write p.casts (world-owned scratch, rewritten in full
    // by every k_move_begin).  Scratch shared with another writer would break this; write the record here then.
    if ((bits & kFinished) && !last) return;
    float4 pos = p.state[i];
    const float4 d0 = p.state[2 * n + i];
    const uint32_t mask = __float_as_uint(d0.w);
    if (!(bits & kFinished)) {
        float4 r = p.state[n + i];
        // steps 2-7 of the rule: slide::one_round, shared with the step moves
        float4 lasthit;
        if (slide::one_round(pos, r, d0, prev, bits, lasthit, static_cast<const uint32_t*>(p.hits) + 10ull * i, last != 0u)) p.state[4 * n + i] = lasthit;
        prev.w = __uint_as_float(bits);
        p.state[i] = pos;
        p.state[n + i] = r;
        p.state[3 * n + i] = prev;
        if (!last) {
            write_cast(p.casts, i, pos, r.x, r.y, r.z, 1.0f, (bits & kFinished) ? 0u : mask);
            return;
        }
    }
    // after the last round: the ground probe straight down from where the mover came to rest
    const float probe = p.state[5 * n + i].x;
    write_cast(p.casts, i, pos, 0.0f, -1.0f, 0.0f, probe, (!(bits & BGE_MOVE_INVALID) && probe > 0.0f) ? mask : 0u);
}

__global__ void __launch_bounds__(kThreads) k_move_finish(MoveParams p)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= p.n) return;
    const uint64_t n = p.n;
    const float4 pos = p.state[i];
    const float4 r = p.state[n + i];
    const float4 prev = p.state[3 * n + i];
    const float4 lasthit = p.state[4 * n + i];
    const float4 probe = p.state[5 * n + i];
    const uint32_t bits = __float_as_uint(prev.w);
    uint32_t flags = bits & 0xffu;
    const uint32_t* h = static_cast<const uint32_t*>(p.hits) + 10ull * i;
    uint32_t gkind = BGE_RAY_MISS, gent = BGE_RAY_NO_ENTITY, gdist = 0u, gnx = 0u, gny = 0u, gnz = 0u;
    if (!(flags & BGE_MOVE_INVALID) && probe.x > 0.0f && h[0] != BGE_RAY_MISS) {
        gkind = h[0];
        gent = h[1];
        gdist = h[3];
        gnx = h[7];
        gny = h[8];
        gnz = h[9];
        flags |= BGE_MOVE_PROBE_HIT;
        if (__uint_as_float(gny) >= probe.y) flags |= BGE_MOVE_GROUNDED;
    }
    uint32_t* o = static_cast<uint32_t*>(p.results) + 20ull * i;
    o[0] = __float_as_uint(pos.x);
    o[1] = __float_as_uint(pos.y);
    o[2] = __float_as_uint(pos.z);
    o[3] = __float_as_uint(r.x);
    o[4] = __float_as_uint(r.y);
    o[5] = __float_as_uint(r.z);
    o[6] = flags;
    o[7] = (bits >> 8) & 0xffu;
    o[8] = (bits >> 16) & 3u;
    o[9] = __float_as_uint(lasthit.w);
    o[10] = __float_as_uint(lasthit.x);
    o[11] = __float_as_uint(lasthit.y);
    o[12] = __float_as_uint(lasthit.z);
    o[13] = gkind;
    o[14] = gent;
    o[15] = gdist;
    o[16] = gnx;
    o[17] = gny;
    o[18] = gnz;
    o[19] = 0u;
}

dim3 grid_of(uint32_t n) { return dim3((n + kThreads - 1u) / kThreads); }

} // namespace

hipError_t launch_move_begin(hipStream_t stream, const MoveParams& p)
{
    if (p.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_move_begin, grid_of(p.n), dim3(kThreads), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_move_step(hipStream_t stream, const MoveParams& p, uint32_t round)
{
    if (p.n == 0) return hipSuccess;
    if (round >= BGE_MOVE_SLIDES) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_move_step, grid_of(p.n), dim3(kThreads), 0, stream, p, round + 1u == BGE_MOVE_SLIDES ? 1u : 0u);
    return hipGetLastError();
}

hipError_t launch_move_finish(hipStream_t stream, const MoveParams& p)
{
    if (p.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_move_finish, grid_of(p.n), dim3(kThreads), 0, stream, p);
    return hipGetLastError();
}

} // namespace bge
