// bge_batch.hip — draw batches on the device (include/bge_world.h bge_world_draw_batches*).
//
// The visible entities of bge_cull.hip, grouped by the caller's draw key: records sorted by (key, entity index) and one
// (first_instance, instance_count) per key.  Integer work on top of the visibility rule of bge_cull_device.hpp.
//   k_batch_test     k_cull_test with one more condition, key[e] < n_keys (tested first: an entity without a key loads no matrix).
//                    Same ballots and counts, so k_cull_scan gives the offsets and *total.
//   k_batch_compact  the members in ENTITY order as (key, entity) records: rank = workgroup offset + popcounts, as k_cull_emit.
//   then 0, 1 or 2 stable passes of a least-significant-digit radix sort with 8-bit digits (n_keys <= 1, <= 256, <= 65536).  Equal
//   keys keep their order, so the entity index is the tie-break without being a sort key.  A pass is three launches:
//   k_batch_hist     a tile of kBatchTile records per workgroup: counts per digit, digit-major table hist[d * tiles + tile].
//   k_batch_scan     one workgroup: exclusive sum over the table in that order = first position of (digit, tile).  A thread owns
//                    a run of entries and moves them as 16-byte pieces.
//   k_batch_scatter  position = table entry + records of the same digit in earlier rounds, in earlier waves of the round (LDS
//                    counts) and in lower lanes of the wave (eight ballots of the digit's bits).  Nothing depends on the order in
//                    which atomics arrive: the output is the same on every run.
//   k_batch_ranges   one thread per key: two binary searches in the sorted keys give first_instance and instance_count, for
//                    empty batches too.
//   k_batch_gather   256 records per workgroup: index out, slot into LDS, then the matrices as 16-byte pieces, four consecutive
//                    lanes per record (a wave's store covers 1 KiB of consecutive output bytes), as k_cull_emit.
// The record count is only known on the device: launches are sized by n_entities and workgroups beyond *total exit.  No workgroup
// waits for another one: every step is its own launch.
#include <hip/hip_runtime.h>

#include "bge_batch.hpp"
#include "bge_cull_device.hpp"

namespace bge {

namespace {

constexpr uint32_t kThreads = kCullEntitiesPerBlock;
constexpr uint32_t kWaves = kThreads / 64u;
constexpr uint32_t kRounds = kBatchTile / kThreads;
constexpr uint32_t kDigits = 256;
static_assert(kThreads == kDigits, "one thread per digit in the LDS tables");
static_assert(kBatchTile % kThreads == 0, "whole rounds");

__global__ void __launch_bounds__(kThreads) k_batch_test(BatchParams bp)
{
    __shared__ uint32_t s_count[kWaves];
    const CullParams& p = bp.cull;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t e = blockIdx.x * static_cast<uint64_t>(kThreads) + threadIdx.x;
    const bool member = bp.key && e < p.n_entities && bp.key[e] < bp.n_keys && entity_visible(p, e);
    const unsigned long long word = __ballot(member);
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

__global__ void __launch_bounds__(kThreads) k_batch_compact(BatchParams bp)
{
    const CullParams& p = bp.cull;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (p.block_sum[blockIdx.x] == 0u) return;
    const uint64_t base = p.block_off[blockIdx.x];
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
        const uint64_t k = base + before + static_cast<uint32_t>(__popcll(mine & ((1ull << lane) - 1ull)));
        const uint64_t e = blockIdx.x * static_cast<uint64_t>(kThreads) + threadIdx.x;
        if (k < p.n_entities) { // (always: a member has a rank below the member count)
            bp.sort_key[0][k] = bp.key[e];
            bp.sort_entity[0][k] = static_cast<uint32_t>(e);
        }
    }
}

// the lanes of the wave that are active and hold the same digit (every lane of the wave calls it)
__device__ __forceinline__ unsigned long long same_digit(uint32_t d, bool active)
{
    unsigned long long peers = __ballot(active);
#pragma unroll
    for (uint32_t b = 0; b < 8u; ++b) {
        const bool bit = (d >> b) & 1u;
        const unsigned long long set = __ballot(active && bit);
        peers &= bit ? set : ~set;
    }
    return peers;
}

__global__ void __launch_bounds__(kThreads) k_batch_hist(const uint32_t* __restrict__ keys, const unsigned long long* __restrict__ total,
                                                         uint32_t shift, uint32_t* __restrict__ hist)
{
    __shared__ uint32_t s_hist[kDigits];
    const uint64_t m = *total;
    const uint64_t t0 = blockIdx.x * static_cast<uint64_t>(kBatchTile);
    if (t0 >= m) return;
    const uint32_t tiles = static_cast<uint32_t>((m + kBatchTile - 1u) / kBatchTile);
    const uint32_t lane = threadIdx.x & 63u;
    s_hist[threadIdx.x] = 0u;
    __syncthreads();
    for (uint32_t r = 0; r < kRounds; ++r) {
        const uint64_t i = t0 + r * kThreads + threadIdx.x;
        const bool active = i < m;
        const uint32_t d = active ? (keys[i] >> shift) & 255u : 0u;
        const unsigned long long peers = same_digit(d, active);
        // one add per digit and wave; sums do not depend on the order of the adds
        if (active && (peers & ((1ull << lane) - 1ull)) == 0ull) atomicAdd(&s_hist[d], static_cast<uint32_t>(__popcll(peers)));
    }
    __syncthreads();
    hist[static_cast<uint64_t>(threadIdx.x) * tiles + blockIdx.x] = s_hist[threadIdx.x];
}

__global__ void __launch_bounds__(1024) k_batch_scan(const uint32_t* __restrict__ hist, const unsigned long long* __restrict__ total,
                                                     uint32_t* __restrict__ off)
{
    __shared__ uint32_t s[1024];
    const uint64_t m = *total;
    if (m == 0ull) return;
    const uint32_t tid = threadIdx.x;
    const uint32_t entries = kDigits * static_cast<uint32_t>((m + kBatchTile - 1u) / kBatchTile); // a multiple of 4
    const uint32_t per = (((entries + 1023u) / 1024u) + 3u) & ~3u;                                  // so is a thread's run
    const uint32_t b0 = tid * per < entries ? tid * per : entries;
    const uint32_t b1 = b0 + per < entries ? b0 + per : entries;
    const uint4* in4 = reinterpret_cast<const uint4*>(hist);
    uint4* out4 = reinterpret_cast<uint4*>(off);
    uint32_t sum = 0;
    for (uint32_t b = b0; b < b1; b += 4u) {
        const uint4 v = in4[b >> 2];
        sum += (v.x + v.y) + (v.z + v.w);
    }
    s[tid] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024u; d <<= 1) {
        const uint32_t t = tid >= d ? s[tid - d] : 0u;
        __syncthreads();
        s[tid] += t;
        __syncthreads();
    }
    uint32_t run = s[tid] - sum;
    for (uint32_t b = b0; b < b1; b += 4u) {
        const uint4 v = in4[b >> 2];
        uint4 o;
        o.x = run;
        o.y = o.x + v.x;
        o.z = o.y + v.y;
        o.w = o.z + v.z;
        run = o.w + v.w;
        out4[b >> 2] = o;
    }
}

__global__ void __launch_bounds__(kThreads) k_batch_scatter(const uint32_t* __restrict__ key_in, const uint32_t* __restrict__ entity_in,
                                                            uint32_t* __restrict__ key_out, uint32_t* __restrict__ entity_out,
                                                            const unsigned long long* __restrict__ total, uint32_t shift,
                                                            const uint32_t* __restrict__ off)
{
    __shared__ uint32_t s_base[kDigits];        // next position of each digit in this tile
    __shared__ uint32_t s_wave[kWaves][kDigits]; // records of each digit per wave, this round
    const uint64_t m = *total;
    const uint64_t t0 = blockIdx.x * static_cast<uint64_t>(kBatchTile);
    if (t0 >= m) return;
    const uint32_t tiles = static_cast<uint32_t>((m + kBatchTile - 1u) / kBatchTile);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    s_base[threadIdx.x] = off[static_cast<uint64_t>(threadIdx.x) * tiles + blockIdx.x];
#pragma unroll
    for (uint32_t w = 0; w < kWaves; ++w) s_wave[w][threadIdx.x] = 0u;
    __syncthreads();
    for (uint32_t r = 0; r < kRounds; ++r) {
        const uint64_t i = t0 + r * kThreads + threadIdx.x;
        const bool active = i < m;
        const uint32_t key = active ? key_in[i] : 0u;
        const uint32_t entity = active ? entity_in[i] : 0u;
        const uint32_t d = (key >> shift) & 255u;
        const unsigned long long peers = same_digit(d, active);
        const uint32_t rank = static_cast<uint32_t>(__popcll(peers & ((1ull << lane) - 1ull)));
        if (active && rank == 0u) s_wave[wave][d] = static_cast<uint32_t>(__popcll(peers));
        __syncthreads();
        if (active) {
            uint32_t pos = s_base[d] + rank;
#pragma unroll
            for (uint32_t w = 0; w < kWaves; ++w) pos += w < wave ? s_wave[w][d] : 0u;
            if (pos < m) { // (always: the table counts exactly these records)
                key_out[pos] = key;
                entity_out[pos] = entity;
            }
        }
        __syncthreads();
        uint32_t sum = 0;
#pragma unroll
        for (uint32_t w = 0; w < kWaves; ++w) {
            sum += s_wave[w][threadIdx.x];
            s_wave[w][threadIdx.x] = 0u;
        }
        s_base[threadIdx.x] += sum;
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kThreads) k_batch_ranges(const uint32_t* __restrict__ keys, const unsigned long long* __restrict__ total,
                                                           uint32_t n_keys, uint32_t* __restrict__ batches)
{
    const uint32_t k = blockIdx.x * kThreads + threadIdx.x;
    if (k >= n_keys) return;
    const uint32_t m = static_cast<uint32_t>(*total);
    uint32_t bound[2]; // first record whose key is >= k, >= k + 1
#pragma unroll
    for (uint32_t j = 0; j < 2u; ++j) {
        uint32_t lo = 0, hi = m;
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (keys[mid] < k + j) lo = mid + 1u;
            else hi = mid;
        }
        bound[j] = lo;
    }
    batches[2u * k] = bound[0];
    batches[2u * k + 1u] = bound[1] - bound[0];
}

__global__ void __launch_bounds__(kThreads) k_batch_gather(BatchParams bp, const uint32_t* __restrict__ entities)
{
    __shared__ uint32_t s_slot[kThreads];
    __shared__ float4 s_row3[kThreads]; // as in k_cull_emit: the deferred translation row composed by the record's own lane, or w = 0
    const CullParams& p = bp.cull;
    const uint64_t total = *p.total;
    const uint64_t m = total < p.cap ? total : p.cap;
    const uint64_t r0 = blockIdx.x * static_cast<uint64_t>(kThreads);
    if (r0 >= m) return;
    const uint32_t count = m - r0 < kThreads ? static_cast<uint32_t>(m - r0) : kThreads;
    if (threadIdx.x < count) {
        const uint32_t e = entities[r0 + threadIdx.x];
        const uint32_t s = e < p.n_entities ? p.slot_of_entity[e] : 0u; // (always a member's index)
        s_slot[threadIdx.x] = s;
        if (p.out_world && p.row3.epoch != 0u) {
            const bool composed = s < p.n_slots && dev::row3_deferred(s, p.row3.rs_word, p.row3.epoch);
            s_row3[threadIdx.x] = composed ? dev::world_row3(nullptr, s, p.row3.pos, true) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
        if (p.out_entities) p.out_entities[r0 + threadIdx.x] = e;
    }
    if (!p.out_world && !p.out_normal) return;
    __syncthreads();
    const float4* world = reinterpret_cast<const float4*>(p.world);
    const float4* normal = reinterpret_cast<const float4*>(p.normal);
    float4* out_world = reinterpret_cast<float4*>(p.out_world);
    float4* out_normal = reinterpret_cast<float4*>(p.out_normal);
    for (uint32_t piece = threadIdx.x; piece < 4u * count; piece += kThreads) {
        const uint32_t k = piece >> 2, q = piece & 3u;
        const uint32_t slot = s_slot[k];
        if (slot >= p.n_slots) continue; // (never: a member owns a slot)
        const uint64_t src = 4ull * slot + q, dst = 4ull * (r0 + k) + q;
        if (out_world) {
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (q == 3u && p.row3.epoch != 0u) v = s_row3[k];
            if (v.w == 0.0f) v = world[src]; // (a composed row has w = 1)
            out_world[dst] = v;
        }
        if (out_normal) out_normal[dst] = normal[src];
    }
}

__global__ void k_batch_scatter_keys(const uint32_t* __restrict__ index, uint64_t first, uint64_t count, const uint32_t* __restrict__ src,
                                     uint32_t* __restrict__ key)
{
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (i >= count) return;
    key[index ? index[i] : first + i] = src[i];
}

} // namespace

hipError_t launch_batch_count(hipStream_t stream, const BatchParams& p)
{
    if (p.cull.n_blocks) hipLaunchKernelGGL(k_batch_test, dim3(p.cull.n_blocks), dim3(kThreads), 0, stream, p);
    return launch_cull_scan(stream, p.cull);
}

hipError_t launch_batch_sort(hipStream_t stream, const BatchParams& p)
{
    const uint32_t passes = batch_passes(p.n_keys);
    if (p.cull.n_blocks) {
        hipLaunchKernelGGL(k_batch_compact, dim3(p.cull.n_blocks), dim3(kThreads), 0, stream, p);
        const uint32_t tiles = static_cast<uint32_t>((p.cull.n_entities + kBatchTile - 1u) / kBatchTile);
        for (uint32_t pass = 0; pass < passes; ++pass) {
            const uint32_t in = pass & 1u, out = in ^ 1u, shift = 8u * pass;
            hipLaunchKernelGGL(k_batch_hist, dim3(tiles), dim3(kThreads), 0, stream, p.sort_key[in], p.cull.total, shift, p.hist);
            hipLaunchKernelGGL(k_batch_scan, dim3(1), dim3(1024), 0, stream, p.hist, p.cull.total, p.hist_off);
            hipLaunchKernelGGL(k_batch_scatter, dim3(tiles), dim3(kThreads), 0, stream, p.sort_key[in], p.sort_entity[in], p.sort_key[out],
                               p.sort_entity[out], p.cull.total, shift, p.hist_off);
        }
    }
    if (p.batches) {
        hipLaunchKernelGGL(k_batch_ranges, dim3((p.n_keys + kThreads - 1u) / kThreads), dim3(kThreads), 0, stream, p.sort_key[passes & 1u],
                           p.cull.total, p.n_keys, p.batches);
    }
    return hipGetLastError();
}

hipError_t launch_batch_gather(hipStream_t stream, const BatchParams& p)
{
    const CullParams& c = p.cull;
    if (c.n_blocks && c.cap && (c.out_entities || c.out_world || c.out_normal)) {
        const uint64_t most = c.cap < c.n_entities ? c.cap : c.n_entities;
        hipLaunchKernelGGL(k_batch_gather, dim3(static_cast<uint32_t>((most + kThreads - 1u) / kThreads)), dim3(kThreads), 0, stream, p,
                           p.sort_entity[batch_passes(p.n_keys) & 1u]);
    }
    return hipGetLastError();
}

hipError_t launch_batch_scatter_keys(hipStream_t stream, const uint32_t* index, uint64_t first, uint64_t count, const uint32_t* src,
                                     uint32_t* key)
{
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(k_batch_scatter_keys, dim3(static_cast<uint32_t>((count + 255) / 256)), dim3(256), 0, stream, index, first, count, src,
                       key);
    return hipGetLastError();
}

} // namespace bge
