// bge_sphere_device.hpp — exact tests of the sphere queries (bge_query.hip): closest points of a box and a capsule, and a
// moving sphere against them.  A sphere of radius r whose centre moves along o + d * f, f in [0, 1], touches a shape where the
// centre's ray enters the shape grown by r: a capsule of radius R + r, the ROUNDED box (sharp box + ball), the planes y = +-r.
// Every cast returns the fraction of the first touch, or -1; a sphere that starts touching or overlapping the shape does not
// hit it (include/bge_world.h).  Built with the library's -ffp-contract=off, as bge_ray_device.hpp is.
#pragma once

#include <hip/hip_runtime.h>

#include "bge_ray_device.hpp"

namespace bge {
namespace dev {

__device__ __forceinline__ float sph_clamp(float v, float lim) { return v < -lim ? -lim : (v > lim ? lim : v); }

// Sharp box of half extents h: q = the point of the box closest to p (p itself inside); returns the squared distance.
__device__ __forceinline__ float point_box_closest(const F3& p, const F3& h, F3& q)
{
    q = F3{sph_clamp(p.x, h.x), sph_clamp(p.y, h.y), sph_clamp(p.z, h.z)};
    const float ex = p.x - q.x, ey = p.y - q.y, ez = p.z - q.z;
    return ex * ex + ey * ey + ez * ez;
}

// Y-axis capsule (radius r, half height hh): returns the distance from p to the solid (0 inside).
__device__ __forceinline__ float point_capsule_closest(const F3& p, float r, float hh)
{
    const float ey = p.y - sph_clamp(p.y, hh);
    const float len = __builtin_sqrtf(p.x * p.x + ey * ey + p.z * p.z);
    return len > r ? len - r : 0.0f;
}

// v with components a and 1 exchanged (a = 1: unchanged): takes the box axis a to the Y axis of ray_capsule_local and back
__device__ __forceinline__ F3 sph_swap_y(const F3& v, int a) { return a == 0 ? F3{v.y, v.x, v.z} : (a == 2 ? F3{v.x, v.z, v.y} : v); }

__device__ __forceinline__ F3 sph_grown(const F3& h, int a, float r) { return F3{a == 0 ? h.x + r : h.x, a == 1 ? h.y + r : h.y, a == 2 ? h.z + r : h.z}; }

// The rounded box: every point within r of the sharp box of half extents h (Ericson, Real-Time Collision Detection 5.5.7).  The
// centre's ray first meets the box grown by r on every axis (slabs).  Where it enters over a face of the sharp box that is the
// touch.  Otherwise the entry lies beside an edge (outside two slabs) or a corner (outside three): the touch, if any, is on the
// capsule of radius r around that edge, or around one of the three edges of that corner (their end spheres are the corners).
// Should those miss, the ray may still cross into a face's slab within rounding of the edge's cylinder (always, for r = 0): the
// sharp box grown along one outside axis at a time decides.  n = outward unit normal at the touch: c(f) - the box's closest point.
__device__ __forceinline__ float sphere_box_local(const F3& o, const F3& d, const F3& h, float r, F3& n)
{
    F3 q;
    if (point_box_closest(o, h, q) <= r * r) return -1.0f; // starts touching or overlapping
    float tn = -INFINITY, tf = INFINITY;
    int ax = -1;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float oa = ray_axis(o, a), da = ray_axis(d, a), ea = ray_axis(h, a) + r;
        if (da == 0.0f) {
            if (__builtin_fabsf(oa) > ea) return -1.0f;
            continue;
        }
        const float t1 = (-ea - oa) / da, t2 = (ea - oa) / da;
        const float nearf = t1 < t2 ? t1 : t2, farf = t1 < t2 ? t2 : t1;
        if (nearf > tn) {
            tn = nearf;
            ax = a;
        }
        if (farf < tf) tf = farf;
    }
    if (ax < 0 || !(tn <= tf) || !(tf >= 0.0f) || !(tn <= 1.0f)) return -1.0f;
    if (tn < 0.0f) { // the centre starts inside the grown box, beside an edge or a corner
        tn = 0.0f;
        ax = -1;
    }
    const F3 p{o.x + d.x * tn, o.y + d.y * tn, o.z + d.z * tn};
    const bool out[3] = {ax == 0 || __builtin_fabsf(p.x) > h.x, ax == 1 || __builtin_fabsf(p.y) > h.y, ax == 2 || __builtin_fabsf(p.z) > h.z};
    const int n_out = int(out[0]) + int(out[1]) + int(out[2]);
    if (n_out < 2) {
        if (ax < 0) return -1.0f;
        const float s = ray_axis(d, ax) > 0.0f ? -1.0f : 1.0f;
        n = F3{ax == 0 ? s : 0.0f, ax == 1 ? s : 0.0f, ax == 2 ? s : 0.0f};
        return tn + 0.0f;
    }
    const F3 corner{p.x < 0.0f ? -h.x : h.x, p.y < 0.0f ? -h.y : h.y, p.z < 0.0f ? -h.z : h.z};
    float best = INFINITY;
    for (int a = 0; a < 3; ++a) { // the edge along axis a, when the entry is outside both other slabs
        if (!(out[(a + 1) % 3] && out[(a + 2) % 3])) continue;
        const F3 m{a == 0 ? o.x : o.x - corner.x, a == 1 ? o.y : o.y - corner.y, a == 2 ? o.z : o.z - corner.z};
        F3 nc;
        const float f = ray_capsule_local(sph_swap_y(m, a), sph_swap_y(d, a), r, ray_axis(h, a), nc);
        if (f >= 0.0f && f < best) {
            best = f;
            n = sph_swap_y(nc, a);
        }
    }
    if (best <= 1.0f) {
        // the fractions of an edge's cylinder and of its end sphere tie to rounding near their seam, and so may the three edges of a
        // corner: the normal is taken from the box's closest point, which does not depend on the part that won
        const F3 c{o.x + d.x * best, o.y + d.y * best, o.z + d.z * best};
        const float len = __builtin_sqrtf(point_box_closest(c, h, q));
        if (len > 0.0f) n = F3{(c.x - q.x) / len, (c.y - q.y) / len, (c.z - q.z) / len};
    } else {
        for (int a = 0; a < 3; ++a) {
            if (!out[a]) continue;
            F3 nf;
            const float f = ray_box_local(o, d, sph_grown(h, a, r), nf);
            if (f >= 0.0f && f < best) {
                best = f;
                n = nf;
            }
        }
    }
    return best <= 1.0f ? best : -1.0f;
}

// A body or a ghost at (origin, q) against the sphere cast (from, delta, radius): fraction or -1, n in world space.
__device__ __forceinline__ float sphere_cast_shape(const F3& from, const F3& delta, float radius, const F3& origin, const Q4& q, bool capsule,
                                                   const F3& dims, F3& n)
{
    const M3 basis = bt_mat_from_quat(q);
    const F3 o = ray_to_local(basis, F3{from.x - origin.x, from.y - origin.y, from.z - origin.z});
    const F3 d = ray_to_local(basis, delta);
    F3 nl{0.0f, 0.0f, 0.0f};
    const float f = capsule ? ray_capsule_local(o, d, dims.x + radius, dims.y, nl) : sphere_box_local(o, d, dims, radius, nl);
    if (f >= 0.0f) n = ray_to_world(basis, nl);
    return f;
}

// Distance from the point c to the same shape, 0 inside.
__device__ __forceinline__ float point_shape_distance(const F3& c, const F3& origin, const Q4& q, bool capsule, const F3& dims)
{
    const M3 basis = bt_mat_from_quat(q);
    const F3 p = ray_to_local(basis, F3{c.x - origin.x, c.y - origin.y, c.z - origin.z});
    if (capsule) return point_capsule_closest(p, dims.x, dims.y);
    F3 cl;
    return __builtin_sqrtf(point_box_closest(p, dims, cl));
}

// Signed distance from the point c to the same shape and the unit direction n out of it, in world space (include/bge_world.h
// "Signed distance").  Outside, the value is point_shape_distance's, from the same functions: point_box_closest,
// point_capsule_closest.  Inside a box: minus the distance to the nearest face, n that face's axis (ties to the lowest axis, a zero
// coordinate counts as positive).  A capsule: distance to the segment less the radius, n away from the segment; on the segment
// itself n is the capsule's local +x.
__device__ __forceinline__ float point_shape_signed(const F3& c, const F3& origin, const Q4& q, bool capsule, const F3& dims, F3& n)
{
    const M3 basis = bt_mat_from_quat(q);
    const F3 p = ray_to_local(basis, F3{c.x - origin.x, c.y - origin.y, c.z - origin.z});
    F3 nl;
    float sd;
    if (capsule) {
        const float ey = p.y - sph_clamp(p.y, dims.y);
        const float a = __builtin_sqrtf(p.x * p.x + ey * ey + p.z * p.z);
        const float out = point_capsule_closest(p, dims.x, dims.y);
        sd = out > 0.0f ? out : a - dims.x;
        nl = a > 0.0f ? F3{p.x / a, ey / a, p.z / a} : F3{1.0f, 0.0f, 0.0f};
    } else {
        const float ax = __builtin_fabsf(p.x), ay = __builtin_fabsf(p.y), az = __builtin_fabsf(p.z);
        if (ax > dims.x || ay > dims.y || az > dims.z) {
            F3 cl;
            sd = __builtin_sqrtf(point_box_closest(p, dims, cl));
            nl = F3{(p.x - cl.x) / sd, (p.y - cl.y) / sd, (p.z - cl.z) / sd};
        } else {
            const float mx = dims.x - ax, my = dims.y - ay, mz = dims.z - az;
            const int j = mx <= my ? (mx <= mz ? 0 : 2) : (my <= mz ? 1 : 2);
            const float m = j == 0 ? mx : (j == 1 ? my : mz);
            const float s = (j == 0 ? p.x : (j == 1 ? p.y : p.z)) < 0.0f ? -1.0f : 1.0f;
            sd = -m;
            nl = F3{j == 0 ? s : 0.0f, j == 1 ? s : 0.0f, j == 2 ? s : 0.0f};
        }
    }
    n = ray_to_world(basis, nl);
    return sd;
}

// The plane y = 0, two-sided as the casts treat it: |c.y|, n up for c.y >= 0 (-0 included) and down below.  It has no inside.
__device__ __forceinline__ float point_plane_signed(float cy, F3& n)
{
    n = F3{0.0f, cy >= 0.0f ? 1.0f : -1.0f, 0.0f};
    return __builtin_fabsf(cy);
}

// The plane y = 0 against a sphere of radius r moving from from_y to to_y: the centre's ray against y = r from above (it must
// start above r and end below it) or y = -r from below; a sphere that starts within r of the plane does not hit it.
__device__ __forceinline__ float sphere_cast_plane(float from_y, float to_y, float r, F3& n)
{
    const bool above = from_y > r && to_y < r, below = from_y < -r && to_y > -r;
    if (!above && !below) return -1.0f;
    const float f = (above ? from_y - r : from_y + r) / (from_y - to_y);
    n = F3{0.0f, above ? 1.0f : -1.0f, 0.0f};
    return f + 0.0f;
}

} // namespace dev
} // namespace bge
