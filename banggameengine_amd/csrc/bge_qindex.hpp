// bge_qindex.hpp — the query index: a spatial hash of the bodies' cull spheres at their current poses (bge_qindex.hip builds it,
// bge_query.hip k_qindex_search reads it; include/bge_world.h "Query index" is the rule).  Built once at the head
// of a public call that queries; every body pass of that call reads it.  Nothing is kept across calls.
#pragma once

#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>

#include <cstddef>
#include <cstdint>

namespace bge {

struct QueryCall;

// The words the kernels count in (one read-back in bge_world_query_index_stats, none in a query call)
enum QIndexWord : uint32_t {
    kQiIndexed = 0, // bodies in cells
    kQiWide,        // bodies on the wide list
    kQiRoutedIndex, // queries that walked their cells, summed over the passes of the call
    kQiRoutedFar,   // queries that took the all-bodies pass, summed over the passes of the call
    kQiFarCount,    // length of the far list of the pass in flight (zeroed before every pass)
    kQiWords = 8
};

// What a body pass needs of a built index; on = 0: there is none and the all-bodies pass runs (part of a QueryCall)
struct QIndexView {
    uint32_t on;
    uint32_t table;      // buckets, a power of two
    float h;             // cell edge (bge_qindex_math.hpp edge())
    uint32_t max_cells;  // a query whose extent covers more goes far
    uint32_t n_rec;      // records the arrays hold room for (= n_slots): bucket runs from the front, the wide list from the back
    const uint32_t* start; // [table]
    const uint32_t* count; // [table]
    // one self-contained record per member, in bucket order (wide body i of the list at n_rec - 1 - i)
    const float4* rec_a; // centre, rb
    const float4* rec_b; // dims, capsule bit (as an integer's bits)
    const uint4* rec_c;  // slot, group, cell key bits, object code
    uint32_t* words;     // [kQiWords]
    uint32_t* far_list;  // [n_queries of the call] query indices of the pass in flight
};

// The buffers a build writes (grow-only, the world's)
struct QIndexBuild {
    uint32_t* count;  // [table]
    uint32_t* start;  // [table]
    uint32_t* cell;   // [n_slots][2] bucket (all ones: absent, all ones - 1: wide) and rank in it / on the wide list
    float4* rec_a;
    float4* rec_b;
    uint4* rec_c;
    void* scan_tmp;   // hipcub's temporary storage
    size_t scan_bytes;
};

uint32_t qindex_table_size(uint64_t n_slots);
size_t qindex_scan_bytes(uint32_t table);
// Classifies every slot of p (bodies, p.qi.h, p.qi.table, p.qi.words) and writes the records; p.qi names the same buffers as b.
hipError_t launch_qindex_build(hipStream_t stream, const QueryCall& p, const QIndexBuild& b);

} // namespace bge
