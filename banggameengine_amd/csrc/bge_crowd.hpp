// bge_crowd.hpp — crowd separation: a batch of spheres against EACH OTHER (bge_crowd.hip; include/bge_world.h "Crowd separation",
// bge_world_crowd_query .., bge_world_characters_crowd ..).  One enqueue answers the query for a batch that lies
// in the caller's records or in the character set's; with `apply` the search also adds the push to the character's position.  The
// host enqueues the launches on the world's stream and reads nothing in between.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

namespace bge {

// Where sphere i's words lie: word pointer + i * stride (in words).  A bge_crowd_sphere batch is one array with stride 6; the
// character set is state.position (stride 20), desc.radius (stride 12) and the filter arrays (stride 1).
struct CrowdSource {
    const uint32_t* center; // 3 words
    const uint32_t* radius; // 1 word
    const uint32_t* group;
    const uint32_t* mask;
    uint32_t center_stride, radius_stride, group_stride, mask_stride;
};

struct CrowdParams {
    CrowdSource src;
    uint32_t n;
    float max_push;           // 0 = no limit
    void* hits;               // [n] bge_crowd_hit (4-byte aligned, moved word by word)
    uint32_t* apply_position; // NULL, or the words of state.position (stride 20 words): x and z of a PUSHED sphere take the push
    // the snapshot: {center, radius} and {index, group, mask, cell key}; packed in index order (small path) or scattered by bucket
    void* rec_a;              // [n] float4
    void* rec_b;              // [n] uint4
    // grid path only
    uint32_t grid;            // 0: small path
    float r_max_host;         // used when r_max_device is NULL
    uint32_t* r_max_device;   // one word: the bits of the largest valid radius, reduced on the device (bge_world_crowd_query*)
    uint32_t table;           // buckets, a power of two
    uint32_t* count;          // [table]
    uint32_t* start;          // [table]
    uint32_t* cell;           // [n][2] bucket (all ones: invalid) and rank in it
    void* scan_tmp;           // hipcub's temporary storage
    size_t scan_bytes;
};

// buckets for n spheres; hipcub's temporary bytes for the scan over them
uint32_t crowd_table_size(uint64_t n);
size_t crowd_scan_bytes(uint32_t table);
hipError_t launch_crowd(hipStream_t stream, const CrowdParams& p);

} // namespace bge
