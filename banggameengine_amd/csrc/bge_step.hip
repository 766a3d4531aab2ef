// bge_step.hip — sphere step moves: collide-and-slide that steps up over low obstacles (include/bge_world.h "Sphere step moves",
// bge_world_sphere_step_move*).
//
// The rule is the caller's recipe of bge_world_sphere_move (up, forward, down, take it if it gained ground), run once on the device.
// Every mover has two lanes that share the closest-hit sphere-cast passes (bge_query.hip): lane A is the plain slide, lane B the
// step.  The kernels here are the arithmetic between the passes, one thread per mover, and they never look at a body:
//   k_step_begin    validates the mover, initialises both lanes and writes A's first cast and B's Up cast.
//   k_step_advance  stage 1: A's first round; the gate, the rise u from the Up hit, B's first Forward cast.
//                   stages 2 .. BGE_MOVE_SLIDES: a round of each lane.  Stage BGE_MOVE_SLIDES + 1: B's last round and its Down cast.
//                   stage BGE_MOVE_SLIDES + 2: the Down hit, Gain, the selection into lane A's planes, and the probe's cast.
//   k_step_finish   reads the probe's hit and writes the 80-byte result.
// A lane that is finished, failed or invalid asks a cast with layer_mask = 0, which hits nothing; no loop here or in the passes
// depends on the data, and there is no LDS and no atomic.  The state lives in planes of float4 (bge_step.hpp); the caller's records
// and the cast / hit records are only 4-byte aligned by their ABI and are moved word by word.
// The slide rounds are slide::one_round of bge_move_device.hpp, the expressions bge_move.hip runs; the rest below is the header's,
// operation for operation (the build's -ffp-contract=off keeps one rounding each).
#include <hip/hip_runtime.h>

#include "../../include/bge_world.h"
#include "bge_move_device.hpp"
#include "bge_step.hpp"

namespace bge {

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kFailed = 1u << 26; // lane B: the step is not taken (never asked, gate closed, no rise, no landing)
using namespace slide; // dot3, write_cast, spent, the bits and the constants (bge_move_device.hpp)

static_assert(kStepStages == BGE_MOVE_SLIDES + 2, "a stage per slide round of lane A, one more for lane B's last, one for the Down hit");

__global__ void __launch_bounds__(kThreads) k_step_begin(StepParams p)
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
    const float height = __uint_as_float(m[11]);
    const bool valid = finite && v[6] >= 0.0f && v[7] > 0.0f && v[8] >= 0.0f && mask != 0u && __builtin_isfinite(height) && height >= 0.0f;
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
    // Lane B is asked only where the gate can still pass: the parts of it known before the first pass (a mover with nothing to
    // spend never hits, so its gate is closed too)
    const bool ask = !(bits & kFinished) && height > 0.0f && v[3] * v[3] + v[5] * v[5] > kRestSq;
    const uint64_t n = p.n;
    p.state[i] = pos;
    p.state[n + i] = r;
    p.state[2 * n + i] = make_float4(v[3], v[4], v[5], __uint_as_float(mask));
    p.state[3 * n + i] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(bits));
    p.state[4 * n + i] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(BGE_RAY_NO_ENTITY));
    p.state[5 * n + i] = make_float4(v[8], v[9], valid ? height : 0.0f, 0.0f);
    p.state[6 * n + i] = pos;
    p.state[7 * n + i] = make_float4(v[3], 0.0f, v[5], v[7]);
    p.state[8 * n + i] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(ask ? 0u : (kFailed | kFinished)));
    p.state[9 * n + i] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(BGE_RAY_NO_ENTITY));
    write_cast(p.casts, i, pos, r.x, r.y, r.z, 1.0f, (bits & kFinished) ? 0u : mask);
    write_cast(p.casts, n + i, pos, 0.0f, 1.0f, 0.0f, ask ? height : 0.0f, ask ? mask : 0u); // Up
}

__global__ void __launch_bounds__(kThreads) k_step_advance(StepParams p, uint32_t stage)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= p.n) return;
    const uint64_t n = p.n;
    const float4 d0 = p.state[2 * n + i];
    const uint32_t mask = __float_as_uint(d0.w);
    const uint32_t* hits = static_cast<const uint32_t*>(p.hits);
    float4 bprev = p.state[8 * n + i];
    uint32_t bbits = __float_as_uint(bprev.w);

    if (stage == kStepStages) {
        // The Down hit, Gain, the selection into lane A's planes, the probe's cast
        float4 pos = p.state[i];
        float4 aprev = p.state[3 * n + i];
        uint32_t bits = __float_as_uint(aprev.w);
        float4 pr = p.state[5 * n + i];
        float rise = 0.0f;
        if (!(bbits & kFailed)) {
            const uint32_t* h = hits + 10ull * (n + i);
            const float4 bpos = p.state[6 * n + i];
            const float4 br = p.state[7 * n + i];
            bool ok = h[0] != BGE_RAY_MISS && __uint_as_float(h[8]) >= pr.y;
            if (ok) {
                float e = __uint_as_float(h[3]) - br.w;
                if (!(e > 0.0f)) e = 0.0f;
                const float sy = bpos.y - e;
                const uint32_t* m = static_cast<const uint32_t*>(p.moves) + 12ull * i;
                const float x0 = __uint_as_float(m[0]), z0 = __uint_as_float(m[2]);
                const float gs = (bpos.x - x0) * d0.x + (bpos.z - z0) * d0.z;
                const float gp = (pos.x - x0) * d0.x + (pos.z - z0) * d0.z;
                if (gs > gp) {
                    pos.x = bpos.x;
                    pos.y = sy;
                    pos.z = bpos.z;
                    rise = pr.w;
                    bits = (bbits & ~kFailed) | BGE_MOVE_STEPPED;
                    aprev = bprev;
                    p.state[n + i] = br;
                    p.state[4 * n + i] = p.state[9 * n + i];
                }
            }
        }
        bits |= bbits & BGE_MOVE_STEP_TRIED;
        aprev.w = __uint_as_float(bits);
        pr.z = rise;
        p.state[i] = pos;
        p.state[3 * n + i] = aprev;
        p.state[5 * n + i] = pr;
        write_cast(p.casts, i, pos, 0.0f, -1.0f, 0.0f, pr.x, (!(bits & BGE_MOVE_INVALID) && pr.x > 0.0f) ? mask : 0u);
        return;
    }

    // lane A: round stage - 1 of the plain slide.  A finished lane's cast already asks nothing (written with layer_mask 0 by the
    // kernel that finished it; only these kernels write p.casts between the kernels of one call)
    bool first_hit = false;
    float n1y = 0.0f;
    if (stage <= BGE_MOVE_SLIDES) {
        float4 prev = p.state[3 * n + i];
        uint32_t bits = __float_as_uint(prev.w);
        if (!(bits & kFinished)) {
            float4 pos = p.state[i];
            float4 r = p.state[n + i];
            float4 lasthit;
            if (one_round(pos, r, d0, prev, bits, lasthit, hits + 10ull * i, stage == BGE_MOVE_SLIDES)) {
                p.state[4 * n + i] = lasthit;
                first_hit = true;
                n1y = lasthit.y;
            }
            prev.w = __uint_as_float(bits);
            p.state[i] = pos;
            p.state[n + i] = r;
            p.state[3 * n + i] = prev;
            if (stage < BGE_MOVE_SLIDES) write_cast(p.casts, i, pos, r.x, r.y, r.z, 1.0f, (bits & kFinished) ? 0u : mask);
        }
    }

    // lane B
    float4 bpos = p.state[6 * n + i];
    if (stage == 1u) {
        // The gate (A's first round just ran: first_hit is P.n_hits >= 1, n1y its normal's y) and the rise from the Up hit
        float4 br = p.state[7 * n + i];
        if (!(bbits & kFailed)) {
            float4 pr = p.state[5 * n + i];
            if (first_hit && n1y < pr.y) {
                bbits |= BGE_MOVE_STEP_TRIED;
                const uint32_t* h = hits + 10ull * (n + i);
                float u = pr.z;
                if (h[0] != BGE_RAY_MISS) u = __uint_as_float(h[3]) - br.w;
                if (u > 0.0f) {
                    bpos.y = bpos.y + u;
                    pr.w = u;
                    p.state[5 * n + i] = pr;
                    p.state[6 * n + i] = bpos;
                } else {
                    bbits |= kFailed | kFinished;
                }
            } else {
                bbits |= kFailed | kFinished;
            }
            bprev.w = __uint_as_float(bbits);
            p.state[8 * n + i] = bprev;
        }
        write_cast(p.casts, n + i, bpos, br.x, br.y, br.z, 1.0f, (bbits & kFinished) ? 0u : mask); // Forward, round 1
        return;
    }
    // Forward round stage - 2
    const bool blast = stage == BGE_MOVE_SLIDES + 1u;
    if (!(bbits & kFinished)) {
        float4 br = p.state[7 * n + i];
        const float4 db = make_float4(d0.x, 0.0f, d0.z, 0.0f);
        float4 lasthit;
        if (one_round(bpos, br, db, bprev, bbits, lasthit, hits + 10ull * (n + i), blast)) p.state[9 * n + i] = lasthit;
        bprev.w = __uint_as_float(bbits);
        p.state[6 * n + i] = bpos;
        p.state[7 * n + i] = br;
        p.state[8 * n + i] = bprev;
        if (!blast) write_cast(p.casts, n + i, bpos, br.x, br.y, br.z, 1.0f, (bbits & kFinished) ? 0u : mask);
    }
    if (blast) {
        // Down from where Forward came to rest, by the rise plus the probe
        const float4 pr = p.state[5 * n + i];
        const bool failed = (bbits & kFailed) != 0u;
        write_cast(p.casts, n + i, bpos, 0.0f, -1.0f, 0.0f, failed ? 0.0f : pr.w + pr.x, failed ? 0u : mask);
    }
}

__global__ void __launch_bounds__(kThreads) k_step_finish(StepParams p)
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
    o[19] = __float_as_uint(probe.z); // step_rise
}

dim3 grid_of(uint32_t n) { return dim3((n + kThreads - 1u) / kThreads); }

} // namespace

hipError_t launch_step_begin(hipStream_t stream, const StepParams& p)
{
    if (p.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_step_begin, grid_of(p.n), dim3(kThreads), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_step_advance(hipStream_t stream, const StepParams& p, uint32_t stage)
{
    if (p.n == 0) return hipSuccess;
    if (stage < 1u || stage > kStepStages) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_step_advance, grid_of(p.n), dim3(kThreads), 0, stream, p, stage);
    return hipGetLastError();
}

hipError_t launch_step_finish(hipStream_t stream, const StepParams& p)
{
    if (p.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_step_finish, grid_of(p.n), dim3(kThreads), 0, stream, p);
    return hipGetLastError();
}

} // namespace bge
