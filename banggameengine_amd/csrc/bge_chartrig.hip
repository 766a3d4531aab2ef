// bge_chartrig.hip — trigger events for the device's characters (include/bge_world.h "Character trigger events").
//
// State: two bitmaps of [triggers][ceil(n / 64)] 64-bit words, bit c of row t = character c overlaps trigger t.  One call is
//   k_ct_test        one thread per character, one grid row per chunk of kCharTrigChunk listed ghosts.  The chunk's boxes and filter
//                    words sit in LDS; a thread keeps its character's box, group and mask in registers and every ghost of the chunk
//                    costs one __ballot.  Lane 0 stores the word of `cur` and the word's two counts.  No atomics; a tail wave ballots
//                    with all its lanes (lanes past n vote 0), so bits beyond n stay zero.
//   k_ct_scan_rows   one workgroup per listed row: the counts of its words become offsets inside the row, and the row's totals.
//   k_ct_scan_total  one workgroup: the rows' totals become each row's base, in ghost-list order, and the call's count.
//   k_ct_emit        every lane recomputes its bit from prev and cur, ranks itself with popcll(word & lanemask_lt) and writes its
//                    record at base + in-row offset + rank unless that is at or beyond the capacity.
// Order between workgroups comes from the kernel boundaries on the one stream; nothing waits inside a launch.  The rows of triggers
// that are not listed are carried from prev to cur by the host's copy before k_ct_test.
#include <hip/hip_runtime.h>

#include "../../include/bge_world.h"
#include "bge_chartrig.hpp"

namespace bge {

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kStateWords = 20, kDescWords = 12; // words of bge_character_state / bge_character_desc (include/bge_world.h)

__global__ void __launch_bounds__(kThreads) k_ct_test(CharTrigParams p)
{
    __shared__ float s_box[kCharTrigChunk][6];
    __shared__ uint32_t s_group[kCharTrigChunk], s_mask[kCharTrigChunk], s_row[kCharTrigChunk];
    const uint32_t g0 = blockIdx.y * kCharTrigChunk;
    const uint32_t ng = min(kCharTrigChunk, p.n_ghosts - g0);
    if (threadIdx.x < ng) {
        const QueryGhost gh = p.ghosts[g0 + threadIdx.x];
        const float* b = p.aabb + 6ull * gh.trigger;
        for (int a = 0; a < 6; ++a) s_box[threadIdx.x][a] = b[a];
        s_group[threadIdx.x] = gh.group;
        s_mask[threadIdx.x] = gh.mask;
        s_row[threadIdx.x] = gh.trigger;
        if (blockIdx.x == 0) p.ghost_rec[g0 + threadIdx.x] = make_uint2(gh.trigger, gh.entity);
    }
    __syncthreads();
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    const bool in = i < p.n;
    float cmin[3] = {0.0f, 0.0f, 0.0f}, cmax[3] = {0.0f, 0.0f, 0.0f};
    uint32_t cgroup = 0u, cmask = 0u;
    if (in) {
        const float* s = static_cast<const float*>(p.state) + uint64_t(kStateWords) * i;
        const float r = static_cast<const float*>(p.desc)[uint64_t(kDescWords) * i + 3];
        for (int a = 0; a < 3; ++a) { // the sphere's AABB plus the contact threshold, one rounding each
            cmin[a] = (s[a] - r) - 0.02f;
            cmax[a] = (s[a] + r) + 0.02f;
        }
        cgroup = p.group[i];
        cmask = p.mask[i];
    }
    const uint32_t word = i >> 6; // (uniform in a wave: 256 is a multiple of 64)
    const bool store = (threadIdx.x & 63u) == 0u && word < p.words;
    for (uint32_t k = 0; k < ng; ++k) { // (uniform trip count: the ballot needs every lane)
        bool hit = in && (s_group[k] & cmask) != 0u && (cgroup & s_mask[k]) != 0u;
        for (int a = 0; a < 3; ++a) hit = hit && s_box[k][a] <= cmax[a] && s_box[k][3 + a] >= cmin[a];
        const unsigned long long now = __ballot(hit);
        if (store) {
            const uint64_t at = uint64_t(s_row[k]) * p.words + word;
            const unsigned long long was = p.prev[at];
            p.cur[at] = now;
            const uint32_t first = __popcll(p.stay ? now : now & ~was); // Enter (+ Stay)
            const uint32_t last = __popcll(was & ~now);                 // Exit
            p.counts[uint64_t(g0 + k) * p.words + word] = first | (static_cast<unsigned long long>(last) << 32);
        }
    }
}

// exclusive scan over the workgroup's 256 values; total = their sum.  s_wave: 4 words of LDS, free again on return.
__device__ unsigned long long block_scan(unsigned long long v, unsigned long long* s_wave, unsigned long long& total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned long long inc = v;
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const unsigned long long t = __shfl_up(inc, d, 64);
        if (lane >= d) inc += t;
    }
    if (lane == 63u) s_wave[wave] = inc;
    __syncthreads();
    unsigned long long before = 0;
    total = 0;
    for (uint32_t k = 0; k < kThreads / 64u; ++k) {
        if (k < wave) before += s_wave[k];
        total += s_wave[k];
    }
    __syncthreads();
    return before + inc - v;
}

// (both halves of a packed count stay below 2^31: a row has at most n <= 2^30 - 1 bits, so the halves never carry into each other)
__global__ void __launch_bounds__(kThreads) k_ct_scan_rows(CharTrigParams p)
{
    __shared__ unsigned long long s_wave[kThreads / 64u];
    unsigned long long* row = p.counts + uint64_t(blockIdx.x) * p.words;
    unsigned long long run = 0;
    for (uint32_t w0 = 0; w0 < p.words; w0 += kThreads) { // (uniform trip count)
        const uint32_t wd = w0 + threadIdx.x;
        const unsigned long long v = wd < p.words ? row[wd] : 0ull;
        unsigned long long total;
        const unsigned long long ex = block_scan(v, s_wave, total);
        if (wd < p.words) row[wd] = run + ex;
        run += total;
    }
    if (threadIdx.x == 0) p.row_total[blockIdx.x] = run;
}

__global__ void __launch_bounds__(kThreads) k_ct_scan_total(CharTrigParams p)
{
    __shared__ unsigned long long s_wave[kThreads / 64u];
    unsigned long long run = 0;
    for (uint32_t g0 = 0; g0 < p.n_ghosts; g0 += kThreads) {
        const uint32_t g = g0 + threadIdx.x;
        unsigned long long v = 0;
        if (g < p.n_ghosts) {
            const unsigned long long t = p.row_total[g];
            v = (t & 0xffffffffull) + (t >> 32);
        }
        unsigned long long total;
        const unsigned long long ex = block_scan(v, s_wave, total);
        if (g < p.n_ghosts) p.row_base[g] = run + ex;
        run += total;
    }
    if (threadIdx.x == 0) *p.count = run > 0xffffffffull ? 0xffffffffu : static_cast<uint32_t>(run);
}

__global__ void __launch_bounds__(kThreads) k_ct_emit(CharTrigParams p)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    const uint32_t word = i >> 6, lane = threadIdx.x & 63u;
    if (word >= p.words) return; // (a whole wave; nothing below needs the lanes it takes away)
    const uint32_t g0 = blockIdx.y * kCharTrigChunk;
    const uint32_t ng = min(kCharTrigChunk, p.n_ghosts - g0);
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t* out = static_cast<uint32_t*>(p.events);
    for (uint32_t k = 0; k < ng; ++k) {
        const uint32_t g = g0 + k;
        const uint2 rec = p.ghost_rec[g];
        const uint64_t at = uint64_t(rec.x) * p.words + word;
        const unsigned long long was = p.prev[at], now = p.cur[at];
        const unsigned long long first = p.stay ? now : now & ~was, last = was & ~now;
        if (((first | last) >> lane & 1ull) == 0ull) continue;
        const unsigned long long off = p.counts[uint64_t(g) * p.words + word];
        const unsigned long long base = p.row_base[g];
        uint64_t idx;
        uint32_t type;
        if (first >> lane & 1ull) {
            idx = base + (off & 0xffffffffull) + __popcll(first & below);
            type = (was >> lane & 1ull) ? BGE_CHAR_TRIGGER_STAY : BGE_CHAR_TRIGGER_ENTER;
        } else {
            idx = base + (p.row_total[g] & 0xffffffffull) + (off >> 32) + __popcll(last & below);
            type = BGE_CHAR_TRIGGER_EXIT;
        }
        if (idx < p.cap) {
            out[3 * idx + 0] = type;
            out[3 * idx + 1] = rec.y;
            out[3 * idx + 2] = i;
        }
    }
}

__global__ void __launch_bounds__(kThreads) k_ct_gather(uint32_t rows, uint32_t words, const uint32_t* __restrict__ src_row,
                                                        const unsigned long long* __restrict__ src, unsigned long long* __restrict__ dst)
{
    const uint64_t at = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (at >= uint64_t(rows) * words) return;
    const uint32_t r = static_cast<uint32_t>(at / words), wd = static_cast<uint32_t>(at % words);
    const uint32_t from = src_row[r];
    dst[at] = from == kCharTrigNoRow ? 0ull : src[uint64_t(from) * words + wd];
}

dim3 pair_grid(const CharTrigParams& p) { return dim3((p.n + kThreads - 1u) / kThreads, (p.n_ghosts + kCharTrigChunk - 1u) / kCharTrigChunk); }

} // namespace

hipError_t launch_chartrig(hipStream_t stream, const CharTrigParams& p)
{
    if (p.n == 0 || p.n_ghosts == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_ct_test, pair_grid(p), dim3(kThreads), 0, stream, p);
    hipLaunchKernelGGL(k_ct_scan_rows, dim3(p.n_ghosts), dim3(kThreads), 0, stream, p);
    hipLaunchKernelGGL(k_ct_scan_total, dim3(1), dim3(kThreads), 0, stream, p);
    hipLaunchKernelGGL(k_ct_emit, pair_grid(p), dim3(kThreads), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_chartrig_emit(hipStream_t stream, const CharTrigParams& p)
{
    if (p.n == 0 || p.n_ghosts == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_ct_emit, pair_grid(p), dim3(kThreads), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_chartrig_gather(hipStream_t stream, uint32_t rows, uint32_t words, const uint32_t* src_row, const unsigned long long* src,
                                  unsigned long long* dst)
{
    if (rows == 0 || words == 0) return hipSuccess;
    const uint64_t total = uint64_t(rows) * words;
    hipLaunchKernelGGL(k_ct_gather, dim3(static_cast<uint32_t>((total + kThreads - 1u) / kThreads)), dim3(kThreads), 0, stream, rows, words,
                       src_row, src, dst);
    return hipGetLastError();
}

} // namespace bge
