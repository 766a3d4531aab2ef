// bge_cull.hpp — launch entry points of the frustum culling pass (bge_cull.hip; include/bge_world.h bge_world_visible*).
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "bge_kernels.hpp"

namespace bge {

constexpr uint32_t kCullEntitiesPerBlock = 256; // entities one workgroup tests and emits (four ballot words)
constexpr uint32_t kCullMaxPlanes = 16;

struct CullParams {
    uint32_t n_planes;
    float planes[kCullMaxPlanes][4];
    // entities in ENTITY order through slot_of_entity; bounds in entity order, matrices in slot order
    uint64_t n_entities, n_slots;
    const uint32_t* slot_of_entity;
    const uint32_t* flag_words;
    const float* bounds;            // [n_entities][6] centre, half extents (null: nobody is renderable)
    const float* world;             // [n_slots][16]
    Row3View row3;                  // translation rows the tick has deferred are composed from the position array (bge_kernels.hpp)
    const float* normal;            // [n_slots][16] (null unless out_normal is set)
    // scratch
    unsigned long long* ballots;    // [n_blocks * 4] one word per wave: the lanes whose entity is visible
    uint32_t* block_sum;            // [n_blocks] visible entities of each workgroup
    uint64_t* block_off;            // [n_blocks] exclusive sum of block_sum
    uint32_t n_blocks;
    // output (device); every array may be null
    uint32_t* out_entities;         // [cap]
    float* out_world;               // [cap][16], 16-byte aligned
    float* out_normal;              // [cap][16], 16-byte aligned
    uint64_t cap;
    unsigned long long* total;      // [1] visible entities, whether or not they fitted
};

// k_cull_test + k_cull_scan: the ballots, the workgroups' offsets and *p.total
hipError_t launch_cull_count(hipStream_t stream, const CullParams& p);
// k_cull_scan alone, over block_sum written by another test kernel (bge_batch.hip): the workgroups' offsets and *p.total
hipError_t launch_cull_scan(hipStream_t stream, const CullParams& p);
// k_cull_emit from the ballots and offsets launch_cull_count left (same stream, same state): records [0, min(cap, total))
hipError_t launch_cull_emit(hipStream_t stream, const CullParams& p);
// bounds[entity] = (centre, half extents) for `count` rows: entity = index ? index[i] : first + i (entities already validated)
hipError_t launch_cull_scatter_bounds(hipStream_t stream, const uint32_t* index, uint64_t first, uint64_t count, const float* center3,
                                      const float* half3, float* bounds);

} // namespace bge
