// bge_query_body.hpp — a body as the queries' cull sees it (device code; bge_query.hip's body pass and bge_qindex.hip's build read
// a slot through this one function, so "candidate" and the bounding radius are the same expression in both).
#pragma once

#include <hip/hip_runtime.h>

#include "bge_device_math.hpp"
#include "bge_flatten.hpp"
#include "bge_kernels.hpp"
#include "bge_query.hpp"

namespace bge {
namespace dev {

__device__ __forceinline__ float abs_sum(const F3& v) { return __builtin_fabsf(v.x) + __builtin_fabsf(v.y) + __builtin_fabsf(v.z); }

// The body of a lane as the cull needs it; cand = false when it is not in the world or no query can see it
struct BodyLane {
    bool cand, capsule;
    F3 c, dims;
    uint32_t grp;
    float rb; // bounding radius with the rounding of the cull's arithmetic on top
};

__device__ __forceinline__ BodyLane load_body(const QueryParams& p, uint64_t s)
{
    BodyLane b{false, false, F3{0.0f, 0.0f, 0.0f}, F3{0.0f, 0.0f, 0.0f}, 0u, 0.0f};
    if (s >= p.n_slots) return b;
    const uint32_t f = p.flags[s];
    // in Bullet's world: a body of any type, not uploaded since the last physics tick (EnsureRigidBody creates it then)
    if ((f & kTypeMask) == 0u || (f & kBDirty)) return b;
    b.grp = p.group[s];
    b.cand = b.grp != 0u && p.mask[s] != 0u;
    if (!b.cand) return b;
    b.c = ld3(p.pos, static_cast<uint32_t>(s));
    const float4 cs = p.cshape[s];
    b.dims = F3{cs.x, cs.y, cs.z};
    b.capsule = (p.cinfo[s] & kCiCapsule) != 0u;
    const float rad = b.capsule ? cs.x + cs.y : __builtin_sqrtf(cs.x * cs.x + cs.y * cs.y + cs.z * cs.z);
    b.rb = rad * 1.0001f + 1e-5f * abs_sum(b.c) + 1e-6f;
    return b;
}

} // namespace dev
} // namespace bge
