// bge_batch.hpp — launch entry points of the draw-batch pass (bge_batch.hip; include/bge_world.h bge_world_draw_batches*).
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "bge_cull.hpp"

namespace bge {

constexpr uint32_t kBatchTile = 2048;    // records one workgroup of a sort pass owns (256 threads x 8 rounds)
constexpr uint32_t kBatchMaxKeys = 65536; // two 8-bit digits

struct BatchParams {
    CullParams cull;             // the visibility part: desc, world arrays, ballots / block_sum / block_off, outputs, cap, total
    const uint32_t* key;         // [n_entities] draw key per ENTITY (null: nobody has one)
    uint32_t n_keys;             // 1 .. kBatchMaxKeys; an entity takes part iff key < n_keys
    // scratch
    uint32_t* sort_key[2];       // [n_entities] each: the keys of the records, ping-pong
    uint32_t* sort_entity[2];    // [n_entities] each: their entity indices
    uint32_t* hist;              // [256 * tiles] digit-major counts of one sort pass, tiles = ceil(n_entities / kBatchTile)
    uint32_t* hist_off;          // [256 * tiles] their exclusive sum
    // output (device), may be null
    uint32_t* batches;           // [n_keys][2] first_instance, instance_count
};

inline uint32_t batch_passes(uint32_t n_keys) { return n_keys <= 1u ? 0u : n_keys <= 256u ? 1u : 2u; }

// k_batch_test + k_cull_scan: the members' ballots, the workgroups' offsets and *p.cull.total
hipError_t launch_batch_count(hipStream_t stream, const BatchParams& p);
// compaction in entity order, then batch_passes(n_keys) stable sort passes by key digit; the sorted records end in
// sort_key / sort_entity [batch_passes(n_keys) & 1].  Then p.batches, when set.  (Same stream, after launch_batch_count.)
hipError_t launch_batch_sort(hipStream_t stream, const BatchParams& p);
// records [0, min(cap, total)) of out_entities / out_world / out_normal in sorted order (after launch_batch_sort)
hipError_t launch_batch_gather(hipStream_t stream, const BatchParams& p);
// key[entity] = src[i] for `count` rows: entity = index ? index[i] : first + i (entities already validated)
hipError_t launch_batch_scatter_keys(hipStream_t stream, const uint32_t* index, uint64_t first, uint64_t count, const uint32_t* src,
                                     uint32_t* key);

} // namespace bge
