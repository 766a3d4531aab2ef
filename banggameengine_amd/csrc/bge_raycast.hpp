// bge_raycast.hpp — launch entry points of the ray queries (bge_raycast.hip; include/bge_world.h bge_world_raycast*).
#pragma once

#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>

#include <cstdint>

namespace bge {

// A trigger ghost the rays can see (the host lists the ghosts that are in the world and posed; few per scene)
struct RayGhost {
    float dims[3];  // box: half extents with margin; capsule: radius, half height, radius
    uint32_t capsule;
    uint32_t trigger; // index into the trigger arrays (TriggerView::pose)
    uint32_t entity;
    uint32_t group, mask;
};
static_assert(sizeof(RayGhost) == 32, "32-byte ghost record");

// One record of the all-hits list: ray, object code, fraction, world normal
struct RayAllRec {
    uint32_t ray, code;
    float f;
    float n[3];
};
static_assert(sizeof(RayAllRec) == 24, "24-byte hit record");

// Object codes order the hits of one ray at equal fraction: bodies, then ghosts, then the plane, each by entity index.
constexpr uint32_t kRayCodeGhost = 1u << 30, kRayCodePlane = 2u << 30, kRayEntityMask = (1u << 30) - 1u;

struct RayParams {
    const void* rays;               // bge_ray[n_rays] (device)
    uint32_t n_rays;
    uint64_t n_slots;
    // bodies (WorldView arrays, slot order)
    const uint32_t* flags;
    const float* pos;
    const float* quat;
    const float4* cshape;
    const uint32_t* cinfo;
    const uint32_t* group;
    const uint32_t* mask;
    const uint32_t* entity_of_slot;
    const uint32_t* slot_of_entity;
    // ghosts and plane
    const RayGhost* ghosts;
    uint32_t n_ghosts;
    const float* ghost_pose;        // [triggers][8]: origin xyz, 0, quaternion xyzw (k_trigger_aabb)
    uint32_t plane;
    // closest hit
    unsigned long long* keys;       // [n_rays] all ones between calls (k_ray_finish puts them back)
    void* hits;                     // bge_ray_hit[n_rays] (device)
    // all hits
    RayAllRec* all;                 // [all_cap]
    uint32_t* all_count;            // [1] records found (may exceed all_cap: nothing beyond it is written)
    uint32_t all_cap;
};

// closest hit: the body pass, then one thread per ray (ghosts, plane, the record)
hipError_t launch_ray_closest(hipStream_t stream, const RayParams& p);
// all hits: appends every (ray, object) crossed to p.all behind p.all_count (zeroed before the call by the caller)
hipError_t launch_ray_all(hipStream_t stream, const RayParams& p);

} // namespace bge
