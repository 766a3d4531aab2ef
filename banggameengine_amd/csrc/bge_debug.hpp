// bge_debug.hpp — launch entry point of the physics debug overlay (bge_debug.hip; include/bge_world.h bge_world_debug_lines*).
#pragma once

#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>

#include <cstdint>

#include "bge_query.hpp"

namespace bge {

constexpr uint32_t kDebugItemsPerBlock = 256; // items (plane, entities, ghosts) one workgroup counts and emits
constexpr uint32_t kDebugBoxLines = 12, kDebugCapsuleLines = 120, kDebugPlaneLines = 12;

struct DebugParams {
    uint32_t flags;                 // bge_debug_flags
    uint32_t use_region;
    float region_min[3], region_max[3];
    // bodies (WorldView arrays, slot order) in ENTITY order through slot_of_entity
    uint64_t n_entities, n_slots;
    const uint32_t* slot_of_entity;
    const uint32_t* flag_words;
    const float* pos;
    const float* quat;
    const float4* cshape;
    const uint32_t* cinfo;
    // ghosts (the list the queries see, in the order of the uploaded trigger array) and the plane
    const QueryGhost* ghosts;
    uint32_t n_ghosts;
    const float* ghost_pose;        // [triggers][8]
    uint32_t plane;
    // contacts: null / 0 where a kind is off
    const float* manifold;          // [slots][32] plane manifolds (null: off)
    const uint32_t* bmanifold;      // [slots][kBoxManifolds][kBoxManifoldWords] obstacle manifolds (null: off)
    const uint64_t* pair_keys;      // [n_pairs] lower entity << 32 | higher entity
    const uint32_t* pair_man;       // [n_pairs][kBoxManifoldWords]
    uint32_t n_pairs;
    // scratch of the shapes section
    uint32_t* block_sum;            // [n_blocks] lines of each workgroup's items
    uint64_t* block_off;            // [n_blocks] exclusive sum of block_sum
    uint32_t n_blocks;              // over 1 + n_entities + n_ghosts items (0 without BGE_DEBUG_SHAPES)
    // output
    float* lines;                   // bge_debug_line[cap] (device), 7 dwords a line; may be null when cap == 0
    uint64_t cap;
    unsigned long long* total;      // [1] device: lines of both sections, whether or not they fitted
};

constexpr uint64_t debug_items(uint64_t n_entities, uint32_t n_ghosts) { return 1ull + n_entities + n_ghosts; }

// count, scan, emit, contacts: *p.total holds the number of lines when the stream reaches this point
hipError_t launch_debug_lines(hipStream_t stream, const DebugParams& p);

} // namespace bge
