// bge_ray_device.hpp — exact ray tests of the ray queries (bge_query.hip): ray / box by slabs in the box frame, ray / capsule,
// ray / plane.  A ray is the segment from + delta * f, f in [0, 1] (delta = direction * max_distance, include/bge_world.h).
// Every function returns the fraction of the first entry into the shape, or -1 for no hit; a segment that starts inside or on
// the shape does not hit it (the stated rule of include/bge_world.h).  Built with the library's -ffp-contract=off: the same
// inputs give the same bits in every kernel that calls these.
#pragma once

#include <hip/hip_runtime.h>

#include "bge_device_math.hpp"

namespace bge {
namespace dev {

// world -> body frame: basis^T * v (btTransform::invXform without the translation); body -> world: basis * v
__device__ __forceinline__ F3 ray_to_local(const M3& r, const F3& v)
{
    return F3{r.m[0][0] * v.x + r.m[1][0] * v.y + r.m[2][0] * v.z, r.m[0][1] * v.x + r.m[1][1] * v.y + r.m[2][1] * v.z,
              r.m[0][2] * v.x + r.m[1][2] * v.y + r.m[2][2] * v.z};
}
__device__ __forceinline__ F3 ray_to_world(const M3& r, const F3& v)
{
    return F3{r.m[0][0] * v.x + r.m[0][1] * v.y + r.m[0][2] * v.z, r.m[1][0] * v.x + r.m[1][1] * v.y + r.m[1][2] * v.z,
              r.m[2][0] * v.x + r.m[2][1] * v.y + r.m[2][2] * v.z};
}

__device__ __forceinline__ float ray_axis(const F3& v, int a) { return a == 0 ? v.x : (a == 1 ? v.y : v.z); }

// Sharp box of half extents h centred at the origin of its frame; o, d in that frame.  n = outward normal of the face entered
// (the first axis of the largest entry fraction on a tie: an edge or a corner).
__device__ __forceinline__ float ray_box_local(const F3& o, const F3& d, const F3& h, F3& n)
{
    if (__builtin_fabsf(o.x) <= h.x && __builtin_fabsf(o.y) <= h.y && __builtin_fabsf(o.z) <= h.z) return -1.0f;
    float tn = -INFINITY, tf = INFINITY;
    int ax = -1;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float oa = ray_axis(o, a), da = ray_axis(d, a), ha = ray_axis(h, a);
        if (da == 0.0f) {
            if (__builtin_fabsf(oa) > ha) return -1.0f; // parallel to the slab and outside it
            continue;
        }
        const float t1 = (-ha - oa) / da, t2 = (ha - oa) / da;
        const float nearf = t1 < t2 ? t1 : t2, farf = t1 < t2 ? t2 : t1;
        if (nearf > tn) {
            tn = nearf;
            ax = a;
        }
        if (farf < tf) tf = farf;
    }
    if (ax < 0 || !(tn <= tf) || !(tn >= 0.0f) || !(tn <= 1.0f)) return -1.0f;
    const float s = ray_axis(d, ax) > 0.0f ? -1.0f : 1.0f;
    n = F3{ax == 0 ? s : 0.0f, ax == 1 ? s : 0.0f, ax == 2 ? s : 0.0f};
    return tn + 0.0f; // (+0, never -0: the fraction's bits are a sort key)
}

// Bullet's Y-axis capsule: the points within r of the segment (0, -hh, 0) .. (0, hh, 0).  The entry into the union of the side
// (a cylinder, where |y| <= hh) and the two cap spheres is the first entry into any of them, the segment starting outside all.
// The quadratics are solved about the point of closest approach (t0, then the half chord), which keeps a far origin from
// cancelling the radius away.  n = outward unit normal at the entry.
__device__ __forceinline__ float ray_capsule_local(const F3& o, const F3& d, float r, float hh, F3& n)
{
    const float cy = o.y < -hh ? -hh : (o.y > hh ? hh : o.y);
    const float oy = o.y - cy;
    const float r2 = r * r;
    if (o.x * o.x + oy * oy + o.z * o.z <= r2) return -1.0f;
    float best = INFINITY;
    F3 bn{0.0f, 0.0f, 0.0f};
    const float a = d.x * d.x + d.z * d.z;
    if (a > 0.0f) {
        const float t0 = -(o.x * d.x + o.z * d.z) / a;
        const float qx = o.x + d.x * t0, qz = o.z + d.z * t0;
        const float p2 = qx * qx + qz * qz;
        if (p2 <= r2) {
            const float t = t0 - __builtin_sqrtf((r2 - p2) / a);
            const float y = o.y + d.y * t;
            if (t >= 0.0f && t <= 1.0f && __builtin_fabsf(y) <= hh) {
                best = t;
                bn = F3{o.x + d.x * t, 0.0f, o.z + d.z * t};
            }
        }
    }
    const float aa = d.x * d.x + d.y * d.y + d.z * d.z;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const float c = s == 0 ? -hh : hh;
        const F3 m{o.x, o.y - c, o.z};
        const float t0 = -(m.x * d.x + m.y * d.y + m.z * d.z) / aa;
        const F3 q{m.x + d.x * t0, m.y + d.y * t0, m.z + d.z * t0};
        const float p2 = q.x * q.x + q.y * q.y + q.z * q.z;
        if (p2 <= r2) {
            const float t = t0 - __builtin_sqrtf((r2 - p2) / aa);
            if (t >= 0.0f && t <= 1.0f && t < best) {
                best = t;
                bn = F3{m.x + d.x * t, m.y + d.y * t, m.z + d.z * t};
            }
        }
    }
    if (!(best <= 1.0f)) return -1.0f;
    const float len = __builtin_sqrtf(bn.x * bn.x + bn.y * bn.y + bn.z * bn.z);
    n = len > 0.0f ? F3{bn.x / len, bn.y / len, bn.z / len} : F3{0.0f, 0.0f, 0.0f};
    return best + 0.0f;
}

// A body or a ghost at (origin, q): box of half extents dims, or capsule (dims.x = radius, dims.y = half height).  n in world space.
__device__ __forceinline__ float ray_shape(const F3& from, const F3& delta, const F3& origin, const Q4& q, bool capsule, const F3& dims, F3& n)
{
    const M3 basis = bt_mat_from_quat(q);
    const F3 o = ray_to_local(basis, F3{from.x - origin.x, from.y - origin.y, from.z - origin.z});
    const F3 d = ray_to_local(basis, delta);
    F3 nl{0.0f, 0.0f, 0.0f};
    const float f = capsule ? ray_capsule_local(o, d, dims.x, dims.y, nl) : ray_box_local(o, d, dims, nl);
    if (f >= 0.0f) n = ray_to_world(basis, nl);
    return f;
}

// The plane y = 0 as btTriangleRaycastCallback sees it, without back-face filtering: hit only when the two ends lie strictly on
// opposite sides; the normal faces the side the segment starts on.
__device__ __forceinline__ float ray_plane(float from_y, float to_y, F3& n)
{
    const bool cross = (from_y > 0.0f && to_y < 0.0f) || (from_y < 0.0f && to_y > 0.0f);
    if (!cross) return -1.0f;
    const float f = from_y / (from_y - to_y);
    n = F3{0.0f, from_y > 0.0f ? 1.0f : -1.0f, 0.0f};
    return f + 0.0f;
}

} // namespace dev
} // namespace bge
