// bge_crowd.hip — crowd separation: every sphere of a batch against every other (include/bge_world.h "Crowd separation",
// bge_world_crowd_query .., bge_world_characters_crowd ..).
//
// The answer for sphere i is a maximum with a stated tie (the deepest overlapping j, lowest j first) and an integer count, so it
// depends on the batch alone: both paths below only choose which j are looked at, and every j looked at is tested by the rule.
//   small path  k_crowd_pack      the snapshot {center, radius} / {index, group, mask} in index order
//               k_crowd_pairs     all pairs: a workgroup walks the snapshot in LDS tiles of 256
//   grid path   k_crowd_rmax      the largest valid radius, where the host does not know it (the stateless query)
//               k_crowd_cells     cell -> bucket of a power-of-two table per valid sphere, its rank in the bucket (integer atomics)
//               (hipcub)          one exclusive scan of the bucket counts
//               k_crowd_scatter   the snapshot, scattered by bucket: one 16-byte {center, radius} and one 16-byte {index, group,
//                                 mask, cell key} record per valid sphere
//               k_crowd_search    per sphere the buckets of the cells its reach touches
//   either      k_crowd_none      r_max == 0 known on the host: nothing can overlap, only validity is written
// The searching kernel also applies the push (apply_position): thread i reads candidates from the snapshot only and writes
// position i only, so no lane reads what another lane of the pass writes.
//
// Which cells (DESIGN.md 4.23 has the argument): with h = max((2 r_max) * 1.001, 1e-18) two spheres the rule calls overlapping lie
// within h of each other on every axis in REAL numbers.  Sphere a visits the cells floor(fl(a - h) / h) .. floor(fl(a + h) / h) per
// axis.  Rounding, the division, floor and the clamp are all monotone, and b is a float with a - h <= b <= a + h, so b's cell lies
// in that range whatever the magnitude.  Coverage rests on monotonicity alone; the cell edge only decides how many cells that is
// (3 per axis, 4 at worst next to the clamp).
// A candidate is taken only from the visit of its OWN cell: the record carries the low 10 bits of its cell per axis, which tells
// the (at most 4) cells of a range apart.  So a bucket that two visited cells share, and a hash collision with a far cell, add
// candidates that are either dropped by the key or fail the rule; nobody is counted twice and no visited-list is kept.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cfloat>

#include "../../include/bge_world.h"
#include "bge_crowd.hpp"

namespace bge {

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kHitWords = 8;
constexpr uint32_t kNone = 0xffffffffu;
constexpr float kCellMax = 1048576.0f; // 2^20: cells are clamped here AS FLOATS, before the conversion

struct Sphere {
    float x, y, z, r;
    uint32_t group, mask;
    bool valid;
};

__device__ __forceinline__ Sphere load_sphere(const CrowdSource& s, uint32_t i)
{
    const uint32_t* c = s.center + uint64_t(s.center_stride) * i;
    Sphere o;
    o.x = __uint_as_float(c[0]);
    o.y = __uint_as_float(c[1]);
    o.z = __uint_as_float(c[2]);
    o.r = __uint_as_float(s.radius[uint64_t(s.radius_stride) * i]);
    o.group = s.group ? s.group[uint64_t(s.group_stride) * i] : 1u;
    o.mask = s.mask ? s.mask[uint64_t(s.mask_stride) * i] : 0xffffffffu;
    o.valid = __builtin_isfinite(o.x) && __builtin_isfinite(o.y) && __builtin_isfinite(o.z) && __builtin_isfinite(o.r) && o.r >= 0.0f;
    return o;
}

// The running answer of one sphere
struct Best {
    uint32_t other = kNone, n = 0u;
    float depth = 0.0f;
    float ox = 0.0f, oy = 0.0f, oz = 0.0f; // centre of `other`
};

// "Pair" of the header for candidate j (valid, j != i)
__device__ __forceinline__ void test_pair(const Sphere& s, uint32_t j, const float4& a, uint32_t group, uint32_t mask, Best& b)
{
    if ((s.group & mask) == 0u || (group & s.mask) == 0u) return;
    const float dx = s.x - a.x, dy = s.y - a.y, dz = s.z - a.z;
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    const float R = s.r + a.w;
    const float depth = R - __builtin_sqrtf(d2);
    if (!(depth > 0.0f)) return;
    b.n += 1u;
    if (b.other == kNone || depth > b.depth || (depth == b.depth && j < b.other)) {
        b.other = j;
        b.depth = depth;
        b.ox = a.x;
        b.oy = a.y;
        b.oz = a.z;
    }
}

// "Push" of the header, the hit record, and the apply
__device__ __forceinline__ void finish(const CrowdParams& p, uint32_t i, const Sphere& s, const Best& b)
{
    uint32_t* h = static_cast<uint32_t*>(p.hits) + uint64_t(kHitWords) * i;
    uint32_t flags = 0u;
    float px = 0.0f, pz = 0.0f;
    if (!s.valid) {
        flags = BGE_CROWD_INVALID;
    } else if (b.other != kNone) {
        const float dx = s.x - b.ox, dz = s.z - b.oz;
        const float hl2 = dx * dx + dz * dz;
        float mx, mz;
        if (hl2 > 1e-12f) {
            const float hl = __builtin_sqrtf(hl2);
            mx = dx / hl;
            mz = dz / hl;
        } else {
            mx = i < b.other ? 1.0f : -1.0f;
            mz = 0.0f;
        }
        float t = b.depth * 0.5f;
        flags = BGE_CROWD_PUSHED;
        if (p.max_push > 0.0f && t > p.max_push) {
            t = p.max_push;
            flags |= BGE_CROWD_CLAMPED;
        }
        px = mx * t;
        pz = mz * t;
    }
    h[0] = flags;
    h[1] = b.other;
    h[2] = b.n;
    h[3] = __float_as_uint(b.depth);
    h[4] = __float_as_uint(px);
    h[5] = 0u;
    h[6] = __float_as_uint(pz);
    h[7] = 0u;
    if (p.apply_position && (flags & BGE_CROWD_PUSHED)) {
        uint32_t* q = p.apply_position + 20ull * i;
        q[0] = __float_as_uint(s.x + px);
        q[2] = __float_as_uint(s.z + pz);
    }
}

// ---------------------------------------------------------------- small path
__global__ void __launch_bounds__(kThreads) k_crowd_pack(CrowdParams p)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= p.n) return;
    const Sphere s = load_sphere(p.src, i);
    static_cast<float4*>(p.rec_a)[i] = float4{s.x, s.y, s.z, s.r};
    static_cast<uint4*>(p.rec_b)[i] = uint4{s.valid ? i : kNone, s.group, s.mask, 0u};
}

__global__ void __launch_bounds__(kThreads) k_crowd_pairs(CrowdParams p)
{
    __shared__ float4 ta[kThreads];
    __shared__ uint4 tb[kThreads];
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    const float4* ra = static_cast<const float4*>(p.rec_a);
    const uint4* rb = static_cast<const uint4*>(p.rec_b);
    Sphere s{};
    if (i < p.n) {
        const float4 a = ra[i];
        const uint4 b = rb[i];
        s = Sphere{a.x, a.y, a.z, a.w, b.y, b.z, b.x != kNone};
    }
    Best best;
    for (uint32_t base = 0; base < p.n; base += kThreads) {
        const uint32_t j = base + threadIdx.x;
        __syncthreads(); // (the tile of the pass before is read out)
        if (j < p.n) {
            ta[threadIdx.x] = ra[j];
            tb[threadIdx.x] = rb[j];
        }
        __syncthreads();
        if (s.valid) {
            const uint32_t m = min(kThreads, p.n - base);
            for (uint32_t k = 0; k < m; ++k) {
                const uint4 b = tb[k];
                if (b.x == kNone || b.x == i) continue;
                test_pair(s, b.x, ta[k], b.y, b.z, best);
            }
        }
    }
    if (i < p.n) finish(p, i, s, best);
}

// ---------------------------------------------------------------- grid path
__device__ __forceinline__ float reach_of(float r_max)
{
    float h = (r_max * 2.0f) * 1.001f;
    if (!(h >= 1e-18f)) h = 1e-18f;
    if (!(h <= FLT_MAX)) h = FLT_MAX;
    return h;
}

__device__ __forceinline__ int cell_of(float x, float cell)
{
    // x may be +-inf (a +- h past FLT_MAX), cell is finite and > 0: never NaN
    const float q = __builtin_floorf(x / cell);
    return static_cast<int>(fminf(fmaxf(q, -kCellMax), kCellMax));
}

__device__ __forceinline__ uint32_t bucket_of(int x, int y, int z, uint32_t table)
{
    uint32_t h = static_cast<uint32_t>(x) * 73856093u ^ static_cast<uint32_t>(y) * 19349663u ^ static_cast<uint32_t>(z) * 83492791u;
    h ^= h >> 15;
    return h & (table - 1u);
}

// the low 10 bits of the cell per axis
__device__ __forceinline__ uint32_t key_of(int x, int y, int z)
{
    return (static_cast<uint32_t>(x) & 1023u) | (static_cast<uint32_t>(y) & 1023u) << 10 | (static_cast<uint32_t>(z) & 1023u) << 20;
}

__device__ __forceinline__ float r_max_of(const CrowdParams& p) { return p.r_max_device ? __uint_as_float(*p.r_max_device) : p.r_max_host; }

__global__ void __launch_bounds__(kThreads) k_crowd_rmax(CrowdParams p)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    float r = 0.0f;
    if (i < p.n) {
        const Sphere s = load_sphere(p.src, i);
        if (s.valid && s.r > 0.0f) r = s.r;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) r = fmaxf(r, __shfl_xor(r, off, 64));
    // (a float >= +0 orders like its bits)
    if ((threadIdx.x & 63u) == 0u && r > 0.0f) atomicMax(p.r_max_device, __float_as_uint(r));
}

__global__ void __launch_bounds__(kThreads) k_crowd_cells(CrowdParams p)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= p.n) return;
    const Sphere s = load_sphere(p.src, i);
    uint32_t bucket = kNone, rank = 0u;
    if (s.valid) {
        const float h = reach_of(r_max_of(p));
        bucket = bucket_of(cell_of(s.x, h), cell_of(s.y, h), cell_of(s.z, h), p.table);
        rank = atomicAdd(&p.count[bucket], 1u);
    }
    p.cell[2ull * i] = bucket;
    p.cell[2ull * i + 1u] = rank;
}

__global__ void __launch_bounds__(kThreads) k_crowd_scatter(CrowdParams p)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= p.n) return;
    const uint32_t bucket = p.cell[2ull * i];
    if (bucket == kNone) return;
    const Sphere s = load_sphere(p.src, i);
    const float h = reach_of(r_max_of(p));
    const uint32_t at = p.start[bucket] + p.cell[2ull * i + 1u]; // < n: the counts sum to the valid spheres
    static_cast<float4*>(p.rec_a)[at] = float4{s.x, s.y, s.z, s.r};
    static_cast<uint4*>(p.rec_b)[at] = uint4{i, s.group, s.mask, key_of(cell_of(s.x, h), cell_of(s.y, h), cell_of(s.z, h))};
}

__global__ void __launch_bounds__(kThreads) k_crowd_search(CrowdParams p)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= p.n) return;
    const Sphere s = load_sphere(p.src, i);
    Best best;
    const float r_max = r_max_of(p);
    if (s.valid && r_max > 0.0f) {
        const float h = reach_of(r_max);
        const float4* ra = static_cast<const float4*>(p.rec_a);
        const uint4* rb = static_cast<const uint4*>(p.rec_b);
        const int x0 = cell_of(s.x - h, h), x1 = cell_of(s.x + h, h);
        const int y0 = cell_of(s.y - h, h), y1 = cell_of(s.y + h, h);
        const int z0 = cell_of(s.z - h, h), z1 = cell_of(s.z + h, h);
        // (x1 - x0 <= 3 by the argument above; a range is walked as it is, so nothing bounds the loops but that)
        for (int z = z0; z <= z1; ++z) {
            for (int y = y0; y <= y1; ++y) {
                for (int x = x0; x <= x1; ++x) {
                    const uint32_t bucket = bucket_of(x, y, z, p.table);
                    const uint32_t key = key_of(x, y, z);
                    const uint32_t first = p.start[bucket];
                    const uint32_t end = min(first + p.count[bucket], p.n);
                    for (uint32_t k = first; k < end; ++k) {
                        const uint4 b = rb[k];
                        if (b.w != key || b.x == i) continue;
                        test_pair(s, b.x, ra[k], b.y, b.z, best);
                    }
                }
            }
        }
    }
    finish(p, i, s, best);
}

__global__ void __launch_bounds__(kThreads) k_crowd_none(CrowdParams p)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= p.n) return;
    finish(p, i, load_sphere(p.src, i), Best{});
}

dim3 grid_of(uint32_t n) { return dim3((n + kThreads - 1u) / kThreads); }

} // namespace

uint32_t crowd_table_size(uint64_t n)
{
    uint32_t t = 1024u;
    while (t < 2u * n && t < (1u << 30)) t <<= 1;
    return t;
}

size_t crowd_scan_bytes(uint32_t table)
{
    size_t bytes = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, static_cast<const uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr),
                                           static_cast<int>(table));
    return bytes;
}

hipError_t launch_crowd(hipStream_t stream, const CrowdParams& p)
{
    if (p.n == 0) return hipSuccess;
    const dim3 grid = grid_of(p.n), block(kThreads);
    if (!p.grid) {
        hipLaunchKernelGGL(k_crowd_pack, grid, block, 0, stream, p);
        hipLaunchKernelGGL(k_crowd_pairs, grid, block, 0, stream, p);
        return hipGetLastError();
    }
    if (!p.r_max_device && !(p.r_max_host > 0.0f)) {
        hipLaunchKernelGGL(k_crowd_none, grid, block, 0, stream, p);
        return hipGetLastError();
    }
    if (p.r_max_device) {
        if (hipError_t e = hipMemsetAsync(p.r_max_device, 0, sizeof(uint32_t), stream)) return e;
        hipLaunchKernelGGL(k_crowd_rmax, grid, block, 0, stream, p);
    }
    if (hipError_t e = hipMemsetAsync(p.count, 0, size_t(p.table) * sizeof(uint32_t), stream)) return e;
    hipLaunchKernelGGL(k_crowd_cells, grid, block, 0, stream, p);
    size_t bytes = p.scan_bytes;
    if (hipError_t e = hipcub::DeviceScan::ExclusiveSum(p.scan_tmp, bytes, p.count, p.start, static_cast<int>(p.table), stream)) return e;
    hipLaunchKernelGGL(k_crowd_scatter, grid, block, 0, stream, p);
    hipLaunchKernelGGL(k_crowd_search, grid, block, 0, stream, p);
    return hipGetLastError();
}

} // namespace bge
