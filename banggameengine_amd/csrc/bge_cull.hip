// bge_cull.hip — frustum culling on the device (include/bge_world.h bge_world_visible*).
//
// The renderer of the reference submits every MeshRenderer whose Transform is clean (src/render/Renderer.cpp:606-665).  With the
// world matrices resident in HBM the visible set is found where they are: an oriented-box test of each entity's model-space
// bounds against up to 16 planes, then a stream compaction in ENTITY order.  Items are the entities through slot_of_entity, as
// bge_debug.hip walks them.  Bandwidth-bound: 4 + 1 + 24 + 64 bytes read per tested entity, 4 + 64 (+ 64) written per visible one.
// A translation row that the tick has deferred (CullParams::row3) is read from the position array instead: 12 bytes more per entity of
// such a wave, in the test and in the emit (the matrix line is fetched for rows 0..2 either way).
//   k_cull_test   one entity per lane; the matrix is loaded only by lanes that are renderable and clean.  One 64-bit ballot word
//                 per wave, one count per workgroup (256 entities).
//   k_cull_scan   one workgroup: exclusive sum of the workgroups' counts (64-bit), *total.  A thread sums a run of counts, so
//                 any number of workgroups is covered.
//   k_cull_emit   a workgroup owns the 256 entities of its four ballot words, hence one contiguous range of records.  A visible
//                 lane's rank is the workgroup's offset plus the popcounts before it; it writes its index and leaves its slot in
//                 LDS.  The matrices then move as 16-byte pieces, four consecutive lanes per record: a wave's store covers
//                 1 KiB of consecutive output bytes.  (The alternative, one lane copying its own 64 bytes: DESIGN.md 4.15.)
// No workgroup waits for another one: the three passes are three launches.
#include <hip/hip_runtime.h>

#include "bge_cull.hpp"
#include "bge_cull_device.hpp"

namespace bge {

namespace {

constexpr uint32_t kThreads = kCullEntitiesPerBlock;
constexpr uint32_t kWaves = kThreads / 64u;

__global__ void __launch_bounds__(kThreads) k_cull_test(CullParams p)
{
    __shared__ uint32_t s_count[kWaves];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t e = blockIdx.x * static_cast<uint64_t>(kThreads) + threadIdx.x;
    const bool vis = e < p.n_entities && entity_visible(p, e);
    const unsigned long long word = __ballot(vis);
    if (lane == 0u) {
        p.ballots[blockIdx.x * static_cast<uint64_t>(kWaves) + wave] = word;
        s_count[wave] = static_cast<uint32_t>(__popcll(word));
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t sum = 0;
#pragma unroll
        for (uint32_t w = 0; w < kWaves; ++w) sum += s_count[w];
        p.block_sum[blockIdx.x] = sum;
    }
}

__global__ void __launch_bounds__(1024) k_cull_scan(CullParams p)
{
    __shared__ unsigned long long s[1024];
    const uint32_t tid = threadIdx.x;
    const uint32_t per = (p.n_blocks + 1023u) / 1024u;
    const uint64_t b0 = static_cast<uint64_t>(tid) * per;
    const uint64_t b1 = b0 + per < p.n_blocks ? b0 + per : p.n_blocks;
    unsigned long long sum = 0;
    for (uint64_t b = b0; b < b1; ++b) sum += p.block_sum[b];
    s[tid] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024u; d <<= 1) {
        const unsigned long long t = tid >= d ? s[tid - d] : 0ull;
        __syncthreads();
        s[tid] += t;
        __syncthreads();
    }
    unsigned long long run = s[tid] - sum;
    for (uint64_t b = b0; b < b1; ++b) {
        p.block_off[b] = run;
        run += p.block_sum[b];
    }
    if (tid == 1023u) *p.total = s[1023];
}

__global__ void __launch_bounds__(kThreads) k_cull_emit(CullParams p)
{
    __shared__ uint32_t s_slot[kThreads]; // slot of the workgroup's k-th visible entity
    __shared__ float4 s_row3[kThreads];   // its translation row where the tick deferred it (CullParams::row3), w = 1; else w = 0: copy the stored one
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t count = p.block_sum[blockIdx.x];
    if (count == 0u) return;
    const uint64_t base = p.block_off[blockIdx.x]; // first record of this workgroup
    if (base >= p.cap) return;                     // (records beyond cap are counted, not written)
    const unsigned long long* words = p.ballots + blockIdx.x * static_cast<uint64_t>(kWaves);
    uint32_t before = 0;
    unsigned long long mine = 0;
#pragma unroll
    for (uint32_t w = 0; w < kWaves; ++w) {
        const unsigned long long x = words[w];
        if (w < wave) before += static_cast<uint32_t>(__popcll(x));
        if (w == wave) mine = x;
    }
    if ((mine >> lane) & 1ull) {
        const uint32_t k = before + static_cast<uint32_t>(__popcll(mine & ((1ull << lane) - 1ull)));
        const uint64_t e = blockIdx.x * static_cast<uint64_t>(kThreads) + threadIdx.x;
        const uint32_t s = p.slot_of_entity[e];
        s_slot[k] = s;
        // composed by the entity's own lane: consecutive lanes read consecutive positions, and the loads leave before the barrier
        if (p.out_world && p.row3.epoch != 0u) {
            const bool composed = dev::row3_deferred(s, p.row3.rs_word, p.row3.epoch);
            s_row3[k] = composed ? dev::world_row3(nullptr, s, p.row3.pos, true) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
        if (p.out_entities && base + k < p.cap) p.out_entities[base + k] = static_cast<uint32_t>(e);
    }
    if (!p.out_world && !p.out_normal) return;
    __syncthreads();
    const float4* world = reinterpret_cast<const float4*>(p.world);
    const float4* normal = reinterpret_cast<const float4*>(p.normal);
    float4* out_world = reinterpret_cast<float4*>(p.out_world);
    float4* out_normal = reinterpret_cast<float4*>(p.out_normal);
    for (uint32_t piece = threadIdx.x; piece < 4u * count; piece += kThreads) {
        const uint32_t k = piece >> 2, q = piece & 3u;
        if (base + k >= p.cap) break;
        const uint64_t src = 4ull * s_slot[k] + q, dst = 4ull * (base + k) + q;
        if (out_world) {
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (q == 3u && p.row3.epoch != 0u) v = s_row3[k];
            if (v.w == 0.0f) v = world[src]; // (a composed row has w = 1)
            out_world[dst] = v;
        }
        if (out_normal) out_normal[dst] = normal[src];
    }
}

__global__ void k_cull_scatter_bounds(const uint32_t* __restrict__ index, uint64_t first, uint64_t count, const float* __restrict__ center3,
                                      const float* __restrict__ half3, float* __restrict__ bounds)
{
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (i >= count) return;
    float* b = bounds + 6ull * (index ? index[i] : first + i);
#pragma unroll
    for (uint32_t k = 0; k < 3u; ++k) {
        b[k] = center3[3ull * i + k];
        b[3u + k] = half3[3ull * i + k];
    }
}

} // namespace

hipError_t launch_cull_count(hipStream_t stream, const CullParams& p)
{
    if (p.n_blocks) hipLaunchKernelGGL(k_cull_test, dim3(p.n_blocks), dim3(kThreads), 0, stream, p);
    return launch_cull_scan(stream, p);
}

hipError_t launch_cull_scan(hipStream_t stream, const CullParams& p)
{
    hipLaunchKernelGGL(k_cull_scan, dim3(1), dim3(1024), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_cull_emit(hipStream_t stream, const CullParams& p)
{
    if (p.n_blocks && p.cap && (p.out_entities || p.out_world || p.out_normal)) {
        hipLaunchKernelGGL(k_cull_emit, dim3(p.n_blocks), dim3(kThreads), 0, stream, p);
    }
    return hipGetLastError();
}

hipError_t launch_cull_scatter_bounds(hipStream_t stream, const uint32_t* index, uint64_t first, uint64_t count, const float* center3,
                                      const float* half3, float* bounds)
{
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(k_cull_scatter_bounds, dim3(static_cast<uint32_t>((count + 255) / 256)), dim3(256), 0, stream, index, first, count,
                       center3, half3, bounds);
    return hipGetLastError();
}

} // namespace bge
