// bge_query.hpp — parameters, records and launch entry point of the batched queries against the device world (bge_query.hip;
// include/bge_world.h bge_world_raycast*, bge_world_sphere_cast*, bge_world_overlap_sphere, bge_world_sphere_penetration; DESIGN.md
// 4.11, 4.13, 4.14, 4.18).
#pragma once

#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>

#include <cstdint>

#include "bge_qindex.hpp"

namespace bge {

// A trigger ghost the queries and the debug overlay can see (the host lists the ghosts that are in the world and posed; few per
// scene)
struct QueryGhost {
    float dims[3];  // box: half extents with margin; capsule: radius, half height, radius
    uint32_t capsule;
    uint32_t trigger; // index into the trigger arrays (TriggerView::pose)
    uint32_t entity;
    uint32_t group, mask;
};
static_assert(sizeof(QueryGhost) == 32, "32-byte ghost record");

// One record of the list of all hits: query, object code, fraction (overlap: distance), world normal (overlap: zero)
struct QueryRec {
    uint32_t query, code;
    float f;
    float n[3];
};
static_assert(sizeof(QueryRec) == 24, "24-byte hit record");

// Object codes order the hits of one query at equal fraction: bodies, then ghosts, then the plane, each by entity index.
constexpr uint32_t kQueryCodeGhost = 1u << 30, kQueryCodePlane = 2u << 30, kQueryEntityMask = (1u << 30) - 1u;

// What is asked; the records of a batch are bge_ray, bge_sphere_cast or bge_sphere (overlap and penetration) accordingly
enum class QueryKind { Ray, SphereCast, SphereOverlap, SpherePenetration };

struct QueryParams {
    const void* records;            // [n_queries] records of the batch's kind (device)
    uint32_t n_queries;
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
    const QueryGhost* ghosts;
    uint32_t n_ghosts;
    const float* ghost_pose;        // [triggers][8]: origin xyz, 0, quaternion xyzw (k_trigger_aabb)
    uint32_t plane;
    // closest hit
    unsigned long long* keys;       // [n_queries] all ones between calls (k_query_finish puts them back)
    void* hits;                     // bge_ray_hit[n_queries], SpherePenetration: bge_penetration_hit[n_queries] (device)
    // all hits
    QueryRec* all;                  // [all_cap]
    uint32_t* all_count;            // [1] records found (may exceed all_cap: nothing beyond it is written)
    uint32_t all_cap;
};

// What a launch takes: the parameters, and the query index of this call (bge_qindex.hpp); qi.on = 0: every body is tested against
// every query.  The passes that do not read the index are handed the QueryParams alone.
struct QueryCall : QueryParams {
    QIndexView qi;
};

// The body pass, then one thread per query (ghosts, plane).  With p.qi.on the body pass is the index's: one wave per query over the
// cells its extent touches and the wide list, then the all-bodies pass over the queries that went far (same tests, same bytes).  all = false: the closest hit of each query into p.hits (rays and
// sphere casts; for a penetration the deepest; an overlap has no closest hit: hipErrorInvalidValue).  all = true: every (query,
// object) hit is appended to p.all behind p.all_count (zeroed before the call by the caller); an overlap's records carry the
// distance and no normal; a penetration has no list (the overlap is its list): hipErrorInvalidValue.
hipError_t launch_query(hipStream_t stream, QueryKind kind, const QueryCall& p, bool all);

} // namespace bge
