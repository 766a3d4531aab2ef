// bge_qindex.hip — building the query index (bge_qindex.hpp; include/bge_world.h "Query index" is the rule).
//
//   k_qindex_cells    one thread per slot: the body as the queries' cull sees it (bge_query_body.hpp load_body — the members are
//                     exactly its candidates, rb its expression).  Absent; or wide (rb not finite or above the cap of the cell
//                     edge): appended to the wide list behind one atomic per wave ballot; or in the cell of its centre -> bucket of
//                     a power-of-two table, its rank in the bucket from one integer atomic.
//   (hipcub)          one exclusive scan of the bucket counts
//   k_qindex_scatter  one self-contained record per member: bucket runs from the front of the arrays, the wide list from the back
// The search is bge_query.hip's k_qindex_search: it needs the query descriptions.  Integer atomics only; no float is summed.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "bge_qindex.hpp"
#include "bge_qindex_math.hpp"
#include "bge_query.hpp"
#include "bge_query_body.hpp"

namespace bge {

namespace {

using namespace dev;

constexpr uint32_t kThreads = 256;
constexpr uint32_t kAbsent = 0xffffffffu, kWide = 0xfffffffeu;

struct BuildArgs {
    QueryCall q;
    QIndexBuild b;
};

__global__ void __launch_bounds__(kThreads) k_qindex_cells(BuildArgs a)
{
    const uint32_t s = blockIdx.x * kThreads + threadIdx.x; // (n_slots < 2^31: the host checks)
    const bool in = s < a.q.n_slots;
    const BodyLane body = load_body(a.q, s);                // (cand = false beyond the slots)
    const float h = a.q.qi.h;
    const bool is_wide = body.cand && qindex::wide(body.rb, h), is_cell = body.cand && !is_wide;
    uint32_t bucket = kAbsent, rank = 0u;
    const uint32_t lane = threadIdx.x & 63u;
    // the wide list: one atomic per wave
    const unsigned long long mw = __ballot(is_wide);
    if (mw != 0ull) {
        const uint32_t leader = static_cast<uint32_t>(__ffsll(static_cast<long long>(mw))) - 1u;
        uint32_t at = 0;
        if (lane == leader) at = atomicAdd(a.q.qi.words + kQiWide, static_cast<uint32_t>(__popcll(mw)));
        at = __shfl(at, static_cast<int>(leader), 64);
        if (is_wide) {
            bucket = kWide;
            rank = at + static_cast<uint32_t>(__popcll(mw & ((1ull << lane) - 1ull)));
        }
    }
    const unsigned long long mc = __ballot(is_cell);
    if (mc != 0ull && lane == static_cast<uint32_t>(__ffsll(static_cast<long long>(mc))) - 1u)
        atomicAdd(a.q.qi.words + kQiIndexed, static_cast<uint32_t>(__popcll(mc)));
    if (is_cell) {
        bucket = qindex::bucket(qindex::cell(body.c.x, h), qindex::cell(body.c.y, h), qindex::cell(body.c.z, h), a.q.qi.table);
        rank = atomicAdd(&a.b.count[bucket], 1u);
    }
    if (in) {
        a.b.cell[2ull * s] = bucket;
        a.b.cell[2ull * s + 1u] = rank;
    }
}

__global__ void __launch_bounds__(kThreads) k_qindex_scatter(BuildArgs a)
{
    const uint32_t s = blockIdx.x * kThreads + threadIdx.x;
    if (s >= a.q.n_slots) return;
    const uint32_t bucket = a.b.cell[2ull * s];
    if (bucket == kAbsent) return;
    const BodyLane body = load_body(a.q, s);
    const float h = a.q.qi.h;
    const uint32_t n_rec = a.q.qi.n_rec, rank = a.b.cell[2ull * s + 1u];
    // members <= n_slots = n_rec: the bucket runs (their counts sum to the cell members) and the wide list never meet
    const uint32_t at = bucket == kWide ? n_rec - 1u - rank : a.b.start[bucket] + rank;
    if (at >= n_rec) return;
    a.b.rec_a[at] = float4{body.c.x, body.c.y, body.c.z, body.rb};
    a.b.rec_b[at] = float4{body.dims.x, body.dims.y, body.dims.z, __uint_as_float(body.capsule ? 1u : 0u)};
    const uint32_t key = bucket == kWide ? 0u : qindex::key(qindex::cell(body.c.x, h), qindex::cell(body.c.y, h), qindex::cell(body.c.z, h));
    a.b.rec_c[at] = uint4{s, body.grp, key, a.q.entity_of_slot[s] & kQueryEntityMask};
}

} // namespace

uint32_t qindex_table_size(uint64_t n_slots)
{
    uint32_t t = 1024u;
    while (t < 2u * n_slots && t < (1u << 30)) t <<= 1;
    return t;
}

size_t qindex_scan_bytes(uint32_t table)
{
    size_t bytes = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, static_cast<const uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr),
                                           static_cast<int>(table));
    return bytes;
}

hipError_t launch_qindex_build(hipStream_t stream, const QueryCall& p, const QIndexBuild& b)
{
    if (p.n_slots == 0 || p.n_slots > 0x7fffffffull || p.qi.n_rec != p.n_slots) return hipErrorInvalidValue;
    const BuildArgs a{p, b};
    const dim3 grid(static_cast<uint32_t>((p.n_slots + kThreads - 1u) / kThreads)), block(kThreads);
    if (hipError_t e = hipMemsetAsync(p.qi.words, 0, kQiWords * sizeof(uint32_t), stream)) return e;
    if (hipError_t e = hipMemsetAsync(b.count, 0, size_t(p.qi.table) * sizeof(uint32_t), stream)) return e;
    hipLaunchKernelGGL(k_qindex_cells, grid, block, 0, stream, a);
    size_t bytes = b.scan_bytes;
    if (hipError_t e = hipcub::DeviceScan::ExclusiveSum(b.scan_tmp, bytes, b.count, b.start, static_cast<int>(p.qi.table), stream)) return e;
    hipLaunchKernelGGL(k_qindex_scatter, grid, block, 0, stream, a);
    return hipGetLastError();
}

} // namespace bge
