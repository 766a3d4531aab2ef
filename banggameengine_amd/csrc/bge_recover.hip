// bge_recover.hip — sphere recovery: a batch of spheres pushed out of what they penetrate (include/bge_world.h "Sphere
// penetration and recovery", bge_world_sphere_recover*).
//
// A recovering sphere sees the world only through the penetration query (bge_query.hip, SpherePenetrationQuery), so a batch is
// BGE_RECOVER_ROUNDS + 1 passes of that query with one line of arithmetic per sphere in between.  The three kernels here are that
// arithmetic, one thread per sphere, and they never look at a body:
//   k_recover_begin   validates the record, initialises the state and writes the query of round 0.
//   k_recover_step    reads the hit of the round's pass; a miss finishes the sphere, a hit pushes it out by depth + skin along the
//                     hit's normal.  It writes the next pass's query — after the last round that is the final check.
//   k_recover_finish  reads the final check's hit and writes the 64-byte result.
// A sphere that is finished or invalid asks with layer_mask = 0, which by the query's own rule penetrates nothing; no loop here or
// in the passes depends on the data.  The state lives in planes of float4 (bge_recover.hpp); the caller's records and the query /
// hit records are only 4-byte aligned by their ABI and are moved word by word, as the query kernels do.
// The expressions below are the header's, operation for operation (the build's -ffp-contract=off keeps one rounding each).
#include <hip/hip_runtime.h>

#include "../../include/bge_world.h"
#include "bge_recover.hpp"

namespace bge {

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kFinished = 1u << 25;

// The query record of sphere i: mask = 0 asks nothing
__device__ __forceinline__ void write_query(void* queries, uint32_t i, const float4& p, uint32_t mask)
{
    uint32_t* q = static_cast<uint32_t*>(queries) + 5ull * i;
    q[0] = __float_as_uint(p.x);
    q[1] = __float_as_uint(p.y);
    q[2] = __float_as_uint(p.z);
    q[3] = __float_as_uint(p.w); // radius
    q[4] = mask;
}

__global__ void __launch_bounds__(kThreads) k_recover_begin(RecoverParams p)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= p.n) return;
    const uint32_t* m = static_cast<const uint32_t*>(p.records) + 7ull * i;
    float v[5];
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        v[k] = __uint_as_float(m[k]);
        finite = finite && __builtin_isfinite(v[k]);
    }
    const uint32_t mask = m[5];
    const bool valid = finite && v[3] >= 0.0f && v[4] > 0.0f && mask != 0u;
    const uint32_t bits = valid ? 0u : (BGE_RECOVER_INVALID | kFinished);
    const float4 pos = make_float4(v[0], v[1], v[2], v[3]);
    const uint64_t n = p.n;
    p.state[i] = pos;
    p.state[n + i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    p.state[2 * n + i] = make_float4(v[4], __uint_as_float(mask), __uint_as_float(bits), __uint_as_float(BGE_RAY_NO_ENTITY));
    write_query(p.queries, i, pos, valid ? mask : 0u);
}

__global__ void __launch_bounds__(kThreads) k_recover_step(RecoverParams p)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= p.n) return;
    const uint64_t n = p.n;
    float4 st = p.state[2 * n + i];
    uint32_t bits = __float_as_uint(st.z);
    // A finished sphere's query already asks nothing: the kernel that finished it (k_recover_begin or an earlier step) wrote it
    // with layer_mask 0, and between the kernels of one call only these kernels write p.queries (scratch of the recovery alone,
    // rewritten in full by every k_recover_begin).
    if (bits & kFinished) return;
    float4 pos = p.state[i];
    const uint32_t* h = static_cast<const uint32_t*>(p.hits) + 10ull * i;
    const uint32_t kind = h[0];
    if (kind == BGE_RAY_MISS) { // step 2: clear of everything
        bits |= kFinished;
    } else { // step 3: out along the normal by the depth and the skin
        const float e = __uint_as_float(h[2]);
        const float nx = __uint_as_float(h[6]), ny = __uint_as_float(h[7]), nz = __uint_as_float(h[8]);
        const float t = e + st.x;
        pos.x = pos.x + nx * t;
        pos.y = pos.y + ny * t;
        pos.z = pos.z + nz * t;
        bits = ((bits & ~(3u << 16)) | (kind << 16)) + (1u << 8); // the last push's kind, n_pushes + 1
        st.w = __uint_as_float(h[1]);
        p.state[i] = pos;
        p.state[n + i] = make_float4(nx, ny, nz, e);
    }
    st.z = __uint_as_float(bits);
    p.state[2 * n + i] = st;
    write_query(p.queries, i, pos, (bits & kFinished) ? 0u : __float_as_uint(st.y));
}

__global__ void __launch_bounds__(kThreads) k_recover_finish(RecoverParams p)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= p.n) return;
    const uint64_t n = p.n;
    const float4 pos = p.state[i];
    const float4 push = p.state[n + i];
    const float4 st = p.state[2 * n + i];
    const uint32_t bits = __float_as_uint(st.z);
    const uint32_t* m = static_cast<const uint32_t*>(p.records) + 7ull * i;
    const uint32_t* h = static_cast<const uint32_t*>(p.hits) + 10ull * i;
    uint32_t flags = bits & 0xffu;
    const uint32_t pushes = (bits >> 8) & 0xffu;
    uint32_t remaining = 0u;
    if (!(bits & kFinished) && h[0] != BGE_RAY_MISS) { // still in something after the last round
        flags |= BGE_RECOVER_STUCK;
        remaining = h[2];
    }
    if (pushes > 0u) flags |= BGE_RECOVER_MOVED;
    uint32_t* o = static_cast<uint32_t*>(p.results) + 16ull * i;
    // an invalid sphere echoes its position bit for bit (p is that position: nothing pushed it); pushed is 0 for it, not p - p
    const bool invalid = (flags & BGE_RECOVER_INVALID) != 0u;
    o[0] = __float_as_uint(pos.x);
    o[1] = __float_as_uint(pos.y);
    o[2] = __float_as_uint(pos.z);
    o[3] = invalid ? 0u : __float_as_uint(pos.x - __uint_as_float(m[0]));
    o[4] = invalid ? 0u : __float_as_uint(pos.y - __uint_as_float(m[1]));
    o[5] = invalid ? 0u : __float_as_uint(pos.z - __uint_as_float(m[2]));
    o[6] = flags;
    o[7] = pushes;
    o[8] = (bits >> 16) & 3u;
    o[9] = __float_as_uint(st.w);
    o[10] = __float_as_uint(push.x);
    o[11] = __float_as_uint(push.y);
    o[12] = __float_as_uint(push.z);
    o[13] = __float_as_uint(push.w);
    o[14] = remaining;
    o[15] = 0u;
}

dim3 grid_of(uint32_t n) { return dim3((n + kThreads - 1u) / kThreads); }

} // namespace

hipError_t launch_recover_begin(hipStream_t stream, const RecoverParams& p)
{
    if (p.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_recover_begin, grid_of(p.n), dim3(kThreads), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_recover_step(hipStream_t stream, const RecoverParams& p)
{
    if (p.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_recover_step, grid_of(p.n), dim3(kThreads), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_recover_finish(hipStream_t stream, const RecoverParams& p)
{
    if (p.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_recover_finish, grid_of(p.n), dim3(kThreads), 0, stream, p);
    return hipGetLastError();
}

} // namespace bge
