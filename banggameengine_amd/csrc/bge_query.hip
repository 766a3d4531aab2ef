// bge_query.hip — batched queries against the device world: rays, sphere casts, sphere overlaps and sphere penetrations
// (include/bge_world.h bge_world_raycast*, bge_world_sphere_cast*, bge_world_overlap_sphere, bge_world_sphere_penetration*;
// DESIGN.md 4.11, 4.13, 4.14, 4.18).
//
// PhysicsSystem::Raycast / RaycastAll (src/physics/PhysicsSystem.cpp:1076-1146) ask Bullet's rayTest for one ray; the reference has
// no sphere query (they are the two primitives its btKinematicCharacterController is made of).  Here a batch of queries of one
// kind is tested against every body in one streaming pass over the body arrays.  The passes are written once, as templates over a
// QUERY DESCRIPTION (RayQuery, SphereCastQuery, SphereOverlapQuery, SpherePenetrationQuery below) that supplies only the arithmetic
// of its kind:
//   k_query_bodies<Q, ALL>  one body per lane, grid-stride over the slots.  The batch's queries are staged through LDS in chunks
//                  of 256; the body stays in registers while its workgroup walks every chunk, so the body arrays are read once
//                  per batch.  The cull reads flags, position, collider, contact word and the filter words (44 bytes a body) and
//                  tests the body's bounding sphere against the query; only a candidate reads its quaternion and runs the exact
//                  test.  Closest hit: one 64-bit atomicMin per hit on the query's key (fraction bits << 32 | object code) —
//                  f >= 0, so the bit order is the value order and the tie rule (lowest object code) holds by construction.  A
//                  penetration's value is its depth and the LARGEST wins: its key carries the complemented depth bits.  All
//                  hits: the (query, code, f, normal) records are appended behind one atomic per wave ballot.
//   k_query_finish<Q>      one thread per query: the trigger ghosts (few) and the plane, then the winning key is decoded, the
//                  normal of the winner recomputed with the same device functions, and the bge_ray_hit (bge_penetration_hit)
//                  written.  The key goes back to all ones.
//   k_query_all_finish<Q>  one thread per query: appends the ghosts' and the plane's hits to the list.
//   k_qindex_search<Q, ALL>  the body pass through the query index (bge_qindex.hpp; include/bge_world.h "Query index"; DESIGN.md
//                  4.24), when the call built one: one wave per query over the cells its extent touches and the wide list, the
//                  same cull and exact test per visited body.  Queries that go far are listed, and k_query_bodies<Q, ALL, true>
//                  runs the all-bodies pass over that list alone.
// Each (Q, ALL) is a kernel of its own; nothing inside the loops asks for the kind at run time.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/bge_world.h"
#include "bge_flatten.hpp"
#include "bge_kernels.hpp"
#include "bge_qindex_math.hpp"
#include "bge_query.hpp"
#include "bge_query_body.hpp"
#include "bge_ray_device.hpp"
#include "bge_sphere_device.hpp"

namespace bge {

namespace {

using namespace dev;

constexpr uint32_t kChunk = 256;      // queries staged per round (= threads of a workgroup)
constexpr uint32_t kMaxBlocks = 2048; // 8 workgroups per CU; more slots are walked grid-stride

__device__ __forceinline__ bool finite3(const F3& v)
{
    return __builtin_isfinite(v.x) && __builtin_isfinite(v.y) && __builtin_isfinite(v.z);
}

// The key of a hit of value f >= 0 by the object `code`: the smaller key wins.  Q::kLargest: the larger value wins instead (the
// bits complemented; an object code is never all ones, so no key of a hit is the all-ones "no hit").
template <class Q>
__device__ __forceinline__ unsigned long long query_key(float f, uint32_t code)
{
    const uint32_t bits = Q::kLargest ? ~__float_as_uint(f) : __float_as_uint(f);
    return (static_cast<unsigned long long>(bits) << 32) | code;
}
template <class Q>
__device__ __forceinline__ float key_value(unsigned long long key)
{
    const uint32_t bits = static_cast<uint32_t>(key >> 32);
    return __uint_as_float(Q::kLargest ? ~bits : bits);
}

// ---------------------------------------------------------------- the query descriptions
// A description Q supplies:
//   Prep, prep(records, i)    record i made ready for the tests; mask = 0 when it can hit nothing (include/bge_world.h "No hit")
//   Shared, stage(sh, t, pr)  what a chunk of 256 stages in LDS
//   Entry, entry(sh, k), mask(e)   what every lane reads back of entry k, the layer mask bits among it
//   Extra, extra(sh, k)       what only a lane whose body the mask lets through reads on top
//   cull(e, x, b)             may the body's bounding sphere be hit at all (conservative: the exact test decides)
//   exact(e, x, b, q, n)      the value of the hit (fraction; overlap: distance; penetration: depth) or -1, and the world normal
//   shape(pr, ...), plane(pr, n)   the same exact test from a Prep against a shape given in full, and against the plane y = 0
//   kClosest, kList, kLargest   whether the value competes for one winning hit, whether there is a list of all hits, and whether
//                             the largest value wins instead of the smallest
//   again(pr, ...), again_plane(pr, n)   the winner's test once more for its record: the normal, and a value handed to point()
//   point(pr, f, v, n, on_plane), write(o, pr, kind, entity, f, at, n)   the contact point of the winner, and its 10-word record

// Words 0..6 of a bge_ray or a bge_sphere_cast: the segment from + delta * f.  Returns whether it is one that can hit anything.
__device__ __forceinline__ bool segment_prep(const uint32_t* w, F3& from, F3& delta, float& max_distance, float& len2)
{
    from = F3{__uint_as_float(w[0]), __uint_as_float(w[1]), __uint_as_float(w[2])};
    const F3 dir{__uint_as_float(w[3]), __uint_as_float(w[4]), __uint_as_float(w[5])};
    max_distance = __uint_as_float(w[6]);
    // to - from = direction * max_distance (PhysicsSystem.cpp:1087: to = from + direction * maxDistance)
    delta = F3{dir.x * max_distance, dir.y * max_distance, dir.z * max_distance};
    len2 = delta.x * delta.x + delta.y * delta.y + delta.z * delta.z;
    return finite3(from) && finite3(dir) && __builtin_isfinite(max_distance) && max_distance > 0.0f &&
           (dir.x != 0.0f || dir.y != 0.0f || dir.z != 0.0f) && finite3(delta) && len2 > 0.0f && __builtin_isfinite(len2) &&
           __builtin_isfinite(from.y + delta.y);
}

// Bounding sphere (centre c, radius rr) against the segment a.xyz + d.xyz * t, t in [0, 1]; a.w = 1 / |d|^2
__device__ __forceinline__ bool segment_near(const float4& a, const float4& d, const F3& c, float rr)
{
    const float wx = c.x - a.x, wy = c.y - a.y, wz = c.z - a.z;
    float t = (wx * d.x + wy * d.y + wz * d.z) * a.w;
    t = t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t);
    const float ex = wx - d.x * t, ey = wy - d.y * t, ez = wz - d.z * t;
    return ex * ex + ey * ey + ez * ez <= rr * rr;
}

// A bge_ray_hit, word by word (the records are 4-byte aligned)
__device__ __forceinline__ void write_ray_hit(uint32_t* o, uint32_t kind, uint32_t entity, float f, float distance, const F3& at, const F3& n)
{
    o[0] = kind;
    o[1] = entity;
    o[2] = __float_as_uint(f);
    o[3] = __float_as_uint(distance);
    o[4] = __float_as_uint(at.x);
    o[5] = __float_as_uint(at.y);
    o[6] = __float_as_uint(at.z);
    o[7] = __float_as_uint(n.x);
    o[8] = __float_as_uint(n.y);
    o[9] = __float_as_uint(n.z);
}

struct SegmentEntry {
    float4 a, d; // from.xyz, 1 / |delta|^2; delta.xyz, layer mask bits (0: the query sees nothing)
};

// The box of the segment from .. from + delta, for the query index (include/bge_world.h "Query index": the extent)
__device__ __forceinline__ void segment_box(const F3& from, const F3& delta, float lo[3], float hi[3])
{
    const float a[3] = {from.x, from.y, from.z}, b[3] = {from.x + delta.x, from.y + delta.y, from.z + delta.z};
    for (int i = 0; i < 3; ++i) {
        lo[i] = __builtin_fminf(a[i], b[i]);
        hi[i] = __builtin_fmaxf(a[i], b[i]);
        if (!(a[i] == a[i]) || !(b[i] == b[i])) lo[i] = hi[i] = __builtin_nanf(""); // (fmin / fmax drop a NaN: keep it, the query is far)
    }
}

struct RayQuery { // bge_ray, 8 words
    static constexpr bool kClosest = true, kList = true, kLargest = false;
    struct Prep {
        F3 from, delta;
        float inv_len2, slack, max_distance;
        uint32_t mask;
    };
    static __device__ __forceinline__ Prep prep(const void* rays, uint32_t i)
    {
        const uint32_t* w = static_cast<const uint32_t*>(rays) + 8ull * i;
        Prep p;
        float len2;
        const bool ok = segment_prep(w, p.from, p.delta, p.max_distance, len2);
        p.mask = ok ? w[7] : 0u;
        p.inv_len2 = ok ? 1.0f / len2 : 0.0f;
        // rounding of the cull's closest-point arithmetic is a few ulp of the magnitudes involved: a generous bound keeps it
        // conservative (the exact test decides)
        p.slack = 1e-5f * (__builtin_fabsf(p.from.x) + __builtin_fabsf(p.from.y) + __builtin_fabsf(p.from.z) + __builtin_fabsf(p.delta.x) +
                           __builtin_fabsf(p.delta.y) + __builtin_fabsf(p.delta.z));
        return p;
    }

    struct Shared {
        float4 from[kChunk], delta[kChunk];
        float slack[kChunk];
    };
    static __device__ __forceinline__ void stage(Shared& sh, uint32_t t, const Prep& p)
    {
        sh.from[t] = make_float4(p.from.x, p.from.y, p.from.z, p.inv_len2);
        sh.delta[t] = make_float4(p.delta.x, p.delta.y, p.delta.z, __uint_as_float(p.mask));
        sh.slack[t] = p.slack;
    }
    using Entry = SegmentEntry;
    using Extra = float; // slack
    static __device__ __forceinline__ Entry entry(const Shared& sh, uint32_t k) { return Entry{sh.from[k], sh.delta[k]}; }
    static __device__ __forceinline__ uint32_t mask(const Entry& e) { return __float_as_uint(e.d.w); }
    static __device__ __forceinline__ Extra extra(const Shared& sh, uint32_t k) { return sh.slack[k]; }

    static __device__ __forceinline__ bool cull(const Entry& e, Extra slack, const BodyLane& b) { return segment_near(e.a, e.d, b.c, b.rb + slack); }
    // what the query index needs: the box of the segment, and what cull() adds to rb
    static __device__ __forceinline__ float extent(const Prep& p, float lo[3], float hi[3])
    {
        segment_box(p.from, p.delta, lo, hi);
        return p.slack;
    }
    static __device__ __forceinline__ float exact(const Entry& e, Extra, const BodyLane& b, const Q4& q, F3& n)
    {
        return ray_shape(F3{e.a.x, e.a.y, e.a.z}, F3{e.d.x, e.d.y, e.d.z}, b.c, q, b.capsule, b.dims, n);
    }

    static __device__ __forceinline__ float shape(const Prep& p, const F3& origin, const Q4& q, bool capsule, const F3& dims, F3& n)
    {
        return ray_shape(p.from, p.delta, origin, q, capsule, dims, n);
    }
    static __device__ __forceinline__ float plane(const Prep& p, F3& n) { return ray_plane(p.from.y, p.from.y + p.delta.y, n); }
    static __device__ __forceinline__ float again(const Prep& p, const F3& origin, const Q4& q, bool capsule, const F3& dims, F3& n)
    {
        return shape(p, origin, q, capsule, dims, n);
    }
    static __device__ __forceinline__ float again_plane(const Prep& p, F3& n) { return plane(p, n); }
    // (bge_world.cpp fill_ray_hit computes the same expressions on the host)
    static __device__ __forceinline__ F3 point(const Prep& p, float f, float, const F3&, bool)
    {
        return F3{p.from.x + p.delta.x * f, p.from.y + p.delta.y * f, p.from.z + p.delta.z * f};
    }
    static __device__ __forceinline__ void write(uint32_t* o, const Prep& p, uint32_t kind, uint32_t entity, float f, const F3& at, const F3& n)
    {
        write_ray_hit(o, kind, entity, f, f * p.max_distance, at, n);
    }
};

struct SphereCastQuery { // bge_sphere_cast, 10 words
    static constexpr bool kClosest = true, kList = true, kLargest = false;
    struct Prep {
        F3 from, delta;
        float inv_len2, slack, max_distance, radius;
        uint32_t mask;
    };
    static __device__ __forceinline__ Prep prep(const void* casts, uint32_t i)
    {
        const uint32_t* w = static_cast<const uint32_t*>(casts) + 10ull * i;
        Prep p;
        float len2;
        p.radius = __uint_as_float(w[7]);
        const bool ok = segment_prep(w, p.from, p.delta, p.max_distance, len2) && __builtin_isfinite(p.radius) && p.radius >= 0.0f;
        p.mask = ok ? w[8] : 0u;
        p.inv_len2 = ok ? 1.0f / len2 : 0.0f;
        // keeps the cull conservative against the rounding of its own arithmetic (the exact test decides)
        p.slack = 1e-5f * (abs_sum(p.from) + abs_sum(p.delta) + p.radius);
        return p;
    }

    struct Shared {
        float4 from[kChunk], delta[kChunk];
        float2 sr[kChunk];
    };
    static __device__ __forceinline__ void stage(Shared& sh, uint32_t t, const Prep& p)
    {
        sh.from[t] = make_float4(p.from.x, p.from.y, p.from.z, p.inv_len2);
        sh.delta[t] = make_float4(p.delta.x, p.delta.y, p.delta.z, __uint_as_float(p.mask));
        sh.sr[t] = make_float2(p.slack, p.radius);
    }
    using Entry = SegmentEntry;
    using Extra = float2; // slack, radius
    static __device__ __forceinline__ Entry entry(const Shared& sh, uint32_t k) { return Entry{sh.from[k], sh.delta[k]}; }
    static __device__ __forceinline__ uint32_t mask(const Entry& e) { return __float_as_uint(e.d.w); }
    static __device__ __forceinline__ Extra extra(const Shared& sh, uint32_t k) { return sh.sr[k]; }

    // the bounding sphere grown by the cast's radius against the segment of the centre
    static __device__ __forceinline__ bool cull(const Entry& e, Extra sr, const BodyLane& b)
    {
        return segment_near(e.a, e.d, b.c, b.rb + sr.y * 1.0001f + sr.x);
    }
    static __device__ __forceinline__ float extent(const Prep& p, float lo[3], float hi[3])
    {
        segment_box(p.from, p.delta, lo, hi);
        return p.radius * 1.0001f + p.slack;
    }
    static __device__ __forceinline__ float exact(const Entry& e, Extra sr, const BodyLane& b, const Q4& q, F3& n)
    {
        return sphere_cast_shape(F3{e.a.x, e.a.y, e.a.z}, F3{e.d.x, e.d.y, e.d.z}, sr.y, b.c, q, b.capsule, b.dims, n);
    }

    static __device__ __forceinline__ float shape(const Prep& p, const F3& origin, const Q4& q, bool capsule, const F3& dims, F3& n)
    {
        return sphere_cast_shape(p.from, p.delta, p.radius, origin, q, capsule, dims, n);
    }
    static __device__ __forceinline__ float plane(const Prep& p, F3& n) { return sphere_cast_plane(p.from.y, p.from.y + p.delta.y, p.radius, n); }
    // the contact point: the centre at the touch pulled back by the radius along the normal; on the plane y is 0 by definition
    // (bge_world.cpp fill_sphere_cast_hit computes the same expressions on the host)
    static __device__ __forceinline__ F3 point(const Prep& p, float f, float, const F3& n, bool on_plane)
    {
        const float py = (p.from.y + p.delta.y * f) - p.radius * n.y;
        return F3{(p.from.x + p.delta.x * f) - p.radius * n.x, on_plane ? 0.0f : py, (p.from.z + p.delta.z * f) - p.radius * n.z};
    }
    static __device__ __forceinline__ float again(const Prep& p, const F3& origin, const Q4& q, bool capsule, const F3& dims, F3& n)
    {
        return shape(p, origin, q, capsule, dims, n);
    }
    static __device__ __forceinline__ float again_plane(const Prep& p, F3& n) { return plane(p, n); }
    static __device__ __forceinline__ void write(uint32_t* o, const Prep& p, uint32_t kind, uint32_t entity, float f, const F3& at, const F3& n)
    {
        write_ray_hit(o, kind, entity, f, f * p.max_distance, at, n);
    }
};

struct SphereOverlapQuery { // bge_sphere, 5 words: every object whose distance to the centre is at most the radius, with that distance
    static constexpr bool kClosest = false, kList = true; // (no winner: no kLargest)
    struct Prep {
        F3 c;
        float radius, slack;
        uint32_t mask;
    };
    static __device__ __forceinline__ Prep prep(const void* spheres, uint32_t i)
    {
        const uint32_t* w = static_cast<const uint32_t*>(spheres) + 5ull * i;
        Prep p;
        p.c = F3{__uint_as_float(w[0]), __uint_as_float(w[1]), __uint_as_float(w[2])};
        p.radius = __uint_as_float(w[3]);
        p.mask = w[4];
        if (!(finite3(p.c) && __builtin_isfinite(p.radius) && p.radius >= 0.0f)) p.mask = 0u;
        p.slack = 1e-5f * (abs_sum(p.c) + p.radius);
        return p;
    }

    struct Shared {
        float4 c[kChunk];  // centre.xyz, radius
        float2 ms[kChunk]; // layer mask bits (0: the sphere reports nothing), slack
    };
    static __device__ __forceinline__ void stage(Shared& sh, uint32_t t, const Prep& p)
    {
        sh.c[t] = make_float4(p.c.x, p.c.y, p.c.z, p.radius);
        sh.ms[t] = make_float2(__uint_as_float(p.mask), p.slack);
    }
    struct Entry {
        float4 a;
        float2 ms;
    };
    struct Extra {};
    static __device__ __forceinline__ Entry entry(const Shared& sh, uint32_t k) { return Entry{sh.c[k], sh.ms[k]}; }
    static __device__ __forceinline__ uint32_t mask(const Entry& e) { return __float_as_uint(e.ms.x); }
    static __device__ __forceinline__ Extra extra(const Shared&, uint32_t) { return Extra{}; }

    static __device__ __forceinline__ bool cull(const Entry& e, Extra, const BodyLane& b)
    {
        const float ex = b.c.x - e.a.x, ey = b.c.y - e.a.y, ez = b.c.z - e.a.z;
        const float rr = b.rb + e.a.w * 1.0001f + e.ms.y;
        return ex * ex + ey * ey + ez * ez <= rr * rr;
    }
    // (the point form: the box is the centre)
    static __device__ __forceinline__ float extent(const Prep& p, float lo[3], float hi[3])
    {
        lo[0] = hi[0] = p.c.x;
        lo[1] = hi[1] = p.c.y;
        lo[2] = hi[2] = p.c.z;
        return p.radius * 1.0001f + p.slack;
    }
    static __device__ __forceinline__ float exact(const Entry& e, Extra, const BodyLane& b, const Q4& q, F3&)
    {
        const float dist = point_shape_distance(F3{e.a.x, e.a.y, e.a.z}, b.c, q, b.capsule, b.dims);
        return dist <= e.a.w ? dist : -1.0f;
    }

    static __device__ __forceinline__ float shape(const Prep& p, const F3& origin, const Q4& q, bool capsule, const F3& dims, F3&)
    {
        const float dist = point_shape_distance(p.c, origin, q, capsule, dims);
        return dist <= p.radius ? dist : -1.0f;
    }
    static __device__ __forceinline__ float plane(const Prep& p, F3&) { return __builtin_fabsf(p.c.y) <= p.radius ? __builtin_fabsf(p.c.y) : -1.0f; }
};

// bge_sphere, 5 words: the object that reaches deepest into the sphere.  The value is depth = radius - sd(centre, S) >= 0 over the
// objects the overlap reports (sd <= radius; outside a shape sd is the overlap's distance, from the same device functions); the
// largest wins.  The record is a bge_penetration_hit; its point needs sd itself, which again() returns.
struct SpherePenetrationQuery : SphereOverlapQuery {
    static constexpr bool kClosest = true, kList = false, kLargest = true;
    // radius - sd in one subtraction; + 0 makes the only possible zero of the other sign (-0 - +0) a +0, so that the bit order
    // of the key is the value order
    static __device__ __forceinline__ float depth(float sd, float radius) { return sd <= radius ? (radius - sd) + 0.0f : -1.0f; }
    static __device__ __forceinline__ float exact(const Entry& e, Extra, const BodyLane& b, const Q4& q, F3& n)
    {
        return depth(point_shape_signed(F3{e.a.x, e.a.y, e.a.z}, b.c, q, b.capsule, b.dims, n), e.a.w);
    }
    static __device__ __forceinline__ float again(const Prep& p, const F3& origin, const Q4& q, bool capsule, const F3& dims, F3& n)
    {
        return point_shape_signed(p.c, origin, q, capsule, dims, n);
    }
    static __device__ __forceinline__ float again_plane(const Prep& p, F3& n) { return point_plane_signed(p.c.y, n); }
    static __device__ __forceinline__ float shape(const Prep& p, const F3& origin, const Q4& q, bool capsule, const F3& dims, F3& n)
    {
        return depth(again(p, origin, q, capsule, dims, n), p.radius);
    }
    static __device__ __forceinline__ float plane(const Prep& p, F3& n) { return depth(again_plane(p, n), p.radius); }
    // centre - normal * sd: on the surface
    static __device__ __forceinline__ F3 point(const Prep& p, float, float sd, const F3& n, bool)
    {
        return F3{p.c.x - n.x * sd, p.c.y - n.y * sd, p.c.z - n.z * sd};
    }
    static __device__ __forceinline__ void write(uint32_t* o, const Prep&, uint32_t kind, uint32_t entity, float f, const F3& at, const F3& n)
    {
        o[0] = kind;
        o[1] = entity;
        o[2] = __float_as_uint(f);
        o[3] = __float_as_uint(at.x);
        o[4] = __float_as_uint(at.y);
        o[5] = __float_as_uint(at.z);
        o[6] = __float_as_uint(n.x);
        o[7] = __float_as_uint(n.y);
        o[8] = __float_as_uint(n.z);
        o[9] = 0u;
    }
};

// ---------------------------------------------------------------- the body pass
__device__ __forceinline__ void write_rec(const QueryParams& p, uint32_t at, uint32_t query, uint32_t code, float f, const F3& n)
{
    if (at >= p.all_cap) return; // (counted, not written: the host grows the list and runs the batch again)
    QueryRec& o = p.all[at];
    o.query = query;
    o.code = code;
    o.f = f;
    o.n[0] = n.x;
    o.n[1] = n.y;
    o.n[2] = n.z;
}

// Appends the records of the lanes with `hit` behind the counter: one atomic per wave
__device__ __forceinline__ void append_wave(const QueryParams& p, bool hit, uint32_t query, uint32_t code, float f, const F3& n)
{
    const unsigned long long m = __ballot(hit);
    if (m == 0ull) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t leader = static_cast<uint32_t>(__ffsll(static_cast<long long>(m))) - 1u;
    uint32_t at = 0;
    if (lane == leader) at = atomicAdd(p.all_count, static_cast<uint32_t>(__popcll(m)));
    at = __shfl(at, static_cast<int>(leader), 64);
    if (!hit) return;
    write_rec(p, at + static_cast<uint32_t>(__popcll(m & ((1ull << lane) - 1ull))), query, code, f, n);
}

__device__ __forceinline__ void append_one(const QueryParams& p, uint32_t query, uint32_t code, float f, const F3& n)
{
    write_rec(p, atomicAdd(p.all_count, 1u), query, code, f, n);
}

// the queries of a far pass' chunk (a function's own LDS: the other instantiations have none of it)
__device__ __forceinline__ uint32_t* far_chunk()
{
    __shared__ uint32_t q[kChunk];
    return q;
}

// FAR: the batch is the far list of the query index (p.qi.far_list, its length on the device); the same pass otherwise
template <class Q, bool ALL, bool FAR = false>
__global__ void __launch_bounds__(256) k_query_bodies(std::conditional_t<FAR, QueryCall, QueryParams> p)
{
    static_assert(ALL || Q::kClosest, "a list-only query has no closest-hit pass");
    __shared__ typename Q::Shared sh;
    const uint32_t tid = threadIdx.x;
    uint32_t n_queries = p.n_queries;
    uint32_t* qid = nullptr;
    if constexpr (FAR) {
        n_queries = p.qi.words[kQiFarCount];
        if (n_queries == 0u) return; // (uniform)
        if (n_queries > p.n_queries) n_queries = p.n_queries;
        qid = far_chunk();
    }
    for (uint64_t base = blockIdx.x * 256ull; base < p.n_slots; base += gridDim.x * 256ull) {
        const uint64_t s = base + tid;
        const BodyLane b = load_body(p, s);
        if (__syncthreads_or(b.cand) == 0) continue; // (uniform: a workgroup without candidates skips the queries)
        bool have_q = false;
        Q4 q{0.0f, 0.0f, 0.0f, 1.0f};
        for (uint32_t r0 = 0; r0 < n_queries; r0 += kChunk) {
            const uint32_t nr = n_queries - r0 < kChunk ? n_queries - r0 : kChunk;
            __syncthreads();
            if constexpr (FAR) {
                if (tid < nr) {
                    const uint32_t r = p.qi.far_list[r0 + tid];
                    qid[tid] = r;
                    Q::stage(sh, tid, Q::prep(p.records, r));
                }
            } else {
                if (tid < nr) Q::stage(sh, tid, Q::prep(p.records, r0 + tid));
            }
            __syncthreads();
            for (uint32_t k = 0; k < nr; ++k) {
                const typename Q::Entry e = Q::entry(sh, k);
                bool hit = false;
                float fh = 0.0f;
                F3 nh{0.0f, 0.0f, 0.0f};
                if (b.cand && (b.grp & Q::mask(e)) != 0u) {
                    const typename Q::Extra x = Q::extra(sh, k);
                    if (Q::cull(e, x, b)) {
                        if (!have_q) {
                            q = ld4(p.quat, static_cast<uint32_t>(s));
                            have_q = true;
                        }
                        F3 n{0.0f, 0.0f, 0.0f};
                        const float f = Q::exact(e, x, b, q, n);
                        if (f >= 0.0f) {
                            if constexpr (!ALL) {
                                if constexpr (FAR) atomicMin(p.keys + qid[k], query_key<Q>(f, p.entity_of_slot[s] & kQueryEntityMask));
                                else atomicMin(p.keys + r0 + k, query_key<Q>(f, p.entity_of_slot[s] & kQueryEntityMask));
                            } else {
                                hit = true;
                                fh = f;
                                nh = n;
                            }
                        }
                    }
                }
                if constexpr (ALL) append_wave(p, hit, FAR ? qid[k] : r0 + k, hit ? p.entity_of_slot[s] & kQueryEntityMask : 0u, fh, nh);
            }
        }
    }
}

// ---------------------------------------------------------------- the body pass through the query index
// One wave per query, four per workgroup.  The wave decides its query's cells (bge_qindex_math.hpp range(): uniform), walks the
// bucket of each and then the wide list with lanes striding over the records, and puts every record it accepts through the
// description's own cull and exact: the arithmetic of a visited body is k_query_bodies', operation for operation.  A record is
// accepted only on the visit of its OWN cell (its key bits): a bucket two visited cells share, or a hash collision, tests nobody
// twice.  A far query's index goes on the far list; k_query_bodies<Q, ALL, true> takes it from there.
constexpr uint32_t kSearchWaves = 4;

template <class Q, bool ALL>
__global__ void __launch_bounds__(64 * kSearchWaves) k_qindex_search(QueryCall p)
{
    static_assert(ALL || Q::kClosest, "a list-only query has no closest-hit pass");
    __shared__ typename Q::Shared sh; // (slots 0 .. 3: each lane reads back what it staged itself, no barrier)
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t r = blockIdx.x * kSearchWaves + wave;
    if (r >= p.n_queries) return; // (uniform per wave; no workgroup barrier below)
    const QIndexView& qi = p.qi;
    const typename Q::Prep pr = Q::prep(p.records, r);
    Q::stage(sh, wave, pr);
    const typename Q::Entry e = Q::entry(sh, wave);
    const typename Q::Extra x = Q::extra(sh, wave);
    float lo[3], hi[3];
    const float growth = Q::extent(pr, lo, hi);
    const qindex::Range rg = qindex::range(lo, hi, growth, qi.h, qi.max_cells);
    if (rg.far) {
        if (lane == 0u) {
            qi.far_list[atomicAdd(qi.words + kQiFarCount, 1u)] = r; // (< n_queries: one append per query)
            atomicAdd(qi.words + kQiRoutedFar, 1u);
        }
        return;
    }
    if (lane == 0u) atomicAdd(qi.words + kQiRoutedIndex, 1u);
    const uint32_t qmask = Q::mask(e);
    if (qmask == 0u) return; // (sees nothing)

    unsigned long long best = ~0ull;
    // record idx of this lane (live: there is one); keyed: only a record of the cell with these key bits
    auto visit = [&](uint32_t idx, bool live, bool keyed, uint32_t key) {
        bool hit = false;
        float fh = 0.0f;
        F3 nh{0.0f, 0.0f, 0.0f};
        uint32_t code = 0u;
        if (live) {
            const uint4 c = qi.rec_c[idx];
            if ((!keyed || c.z == key) && (c.y & qmask) != 0u) {
                const float4 ra = qi.rec_a[idx], rb = qi.rec_b[idx];
                const BodyLane b{true, __float_as_uint(rb.w) != 0u, F3{ra.x, ra.y, ra.z}, F3{rb.x, rb.y, rb.z}, c.y, ra.w};
                if (Q::cull(e, x, b)) {
                    const Q4 q = ld4(p.quat, c.x);
                    F3 n{0.0f, 0.0f, 0.0f};
                    const float f = Q::exact(e, x, b, q, n);
                    if (f >= 0.0f) {
                        if constexpr (!ALL) {
                            const unsigned long long k = query_key<Q>(f, c.w);
                            best = k < best ? k : best;
                        } else {
                            hit = true;
                            code = c.w;
                            fh = f;
                            nh = n;
                        }
                    }
                }
            }
        }
        if constexpr (ALL) append_wave(p, hit, r, code, fh, nh);
    };

    for (int cz = rg.lo[2]; cz <= rg.hi[2]; ++cz) {
        for (int cy = rg.lo[1]; cy <= rg.hi[1]; ++cy) {
            for (int cx = rg.lo[0]; cx <= rg.hi[0]; ++cx) {
                const uint32_t bucket = qindex::bucket(cx, cy, cz, qi.table);
                const uint32_t key = qindex::key(cx, cy, cz);
                const uint32_t first = qi.start[bucket];
                const uint32_t end = min(first + qi.count[bucket], qi.n_rec);
                for (uint32_t k0 = first; k0 < end; k0 += 64u) visit(k0 + lane, k0 + lane < end, true, key);
            }
        }
    }
    const uint32_t n_wide = min(qi.words[kQiWide], qi.n_rec);
    for (uint32_t k0 = 0; k0 < n_wide; k0 += 64u) visit(qi.n_rec - 1u - min(k0 + lane, n_wide - 1u), k0 + lane < n_wide, false, 0u);

    if constexpr (!ALL) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const uint32_t l = __shfl_xor(static_cast<uint32_t>(best), off, 64), h = __shfl_xor(static_cast<uint32_t>(best >> 32), off, 64);
            const unsigned long long o = static_cast<unsigned long long>(h) << 32 | l;
            best = o < best ? o : best;
        }
        if (lane == 0u && best != ~0ull) atomicMin(p.keys + r, best);
    }
}

// ---------------------------------------------------------------- the finish passes
// ghost g of the list against the query pr: value or -1, world normal.  AGAIN: the winner's test once more (Q::again)
template <class Q, bool AGAIN = false>
__device__ __forceinline__ float query_ghost(const QueryParams& p, const typename Q::Prep& pr, uint32_t g, F3& n)
{
    const QueryGhost gh = p.ghosts[g];
    if ((gh.group & pr.mask) == 0u || gh.mask == 0u) return -1.0f;
    const float* pose = p.ghost_pose + 8ull * gh.trigger;
    const F3 origin{pose[0], pose[1], pose[2]}, dims{gh.dims[0], gh.dims[1], gh.dims[2]};
    const Q4 q{pose[4], pose[5], pose[6], pose[7]};
    if constexpr (AGAIN) return Q::again(pr, origin, q, gh.capsule != 0u, dims, n);
    else return Q::shape(pr, origin, q, gh.capsule != 0u, dims, n);
}

__device__ __forceinline__ bool sees_plane(const QueryParams& p, uint32_t mask)
{
    return p.plane && (mask & 2u) != 0u; // group StaticFilter (2), mask AllFilter (PhysicsSystem.cpp:149-166)
}

template <class Q>
__global__ void __launch_bounds__(64) k_query_finish(QueryParams p)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= p.n_queries) return;
    const typename Q::Prep pr = Q::prep(p.records, r);
    unsigned long long key = p.keys[r];
    p.keys[r] = ~0ull; // ready for the next batch
    uint32_t gwin = 0;
    if (pr.mask != 0u) {
        for (uint32_t g = 0; g < p.n_ghosts; ++g) {
            F3 n;
            const float f = query_ghost<Q>(p, pr, g, n);
            if (f >= 0.0f) {
                const unsigned long long k = query_key<Q>(f, kQueryCodeGhost | (p.ghosts[g].entity & kQueryEntityMask));
                if (k < key) {
                    key = k;
                    gwin = g;
                }
            }
        }
        if (sees_plane(p, pr.mask)) {
            F3 n;
            const float f = Q::plane(pr, n);
            if (f >= 0.0f) {
                const unsigned long long k = query_key<Q>(f, kQueryCodePlane | kQueryEntityMask);
                if (k < key) key = k;
            }
        }
    } else {
        key = ~0ull;
    }
    uint32_t* o = static_cast<uint32_t*>(p.hits) + 10ull * r;
    if (key == ~0ull) {
        o[0] = BGE_RAY_MISS;
        o[1] = BGE_RAY_NO_ENTITY;
        for (int i = 2; i < 10; ++i) o[i] = 0u;
        return;
    }
    const float f = key_value<Q>(key);
    const uint32_t code = static_cast<uint32_t>(key);
    const uint32_t kind = code >> 30, ent = code & kQueryEntityMask;
    F3 n{0.0f, 0.0f, 0.0f};
    float v; // what the winner's test returns this time
    uint32_t out_kind, out_entity = ent;
    if (kind == 0u) {
        const uint32_t s = p.slot_of_entity[ent];
        const float4 cs = p.cshape[s];
        v = Q::again(pr, ld3(p.pos, s), ld4(p.quat, s), (p.cinfo[s] & kCiCapsule) != 0u, F3{cs.x, cs.y, cs.z}, n);
        out_kind = BGE_RAY_BODY;
    } else if (kind == 1u) {
        v = query_ghost<Q, true>(p, pr, gwin, n);
        out_kind = BGE_RAY_TRIGGER;
    } else {
        v = Q::again_plane(pr, n);
        out_kind = BGE_RAY_GROUND;
        out_entity = BGE_RAY_NO_ENTITY;
    }
    Q::write(o, pr, out_kind, out_entity, f, Q::point(pr, f, v, n, kind == 2u), n);
}

template <class Q>
__global__ void __launch_bounds__(64) k_query_all_finish(QueryParams p)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= p.n_queries) return;
    const typename Q::Prep pr = Q::prep(p.records, r);
    if (pr.mask == 0u) return;
    for (uint32_t g = 0; g < p.n_ghosts; ++g) {
        F3 n{0.0f, 0.0f, 0.0f};
        const float f = query_ghost<Q>(p, pr, g, n);
        if (f >= 0.0f) append_one(p, r, kQueryCodeGhost | (p.ghosts[g].entity & kQueryEntityMask), f, n);
    }
    if (sees_plane(p, pr.mask)) {
        F3 n{0.0f, 0.0f, 0.0f};
        const float f = Q::plane(pr, n);
        if (f >= 0.0f) append_one(p, r, kQueryCodePlane | kQueryEntityMask, f, n);
    }
}

// the body pass of a batch: through the index and then over its far list, or over every body
template <class Q, bool ALL>
hipError_t launch_bodies(hipStream_t stream, const QueryCall& p)
{
    if (p.n_slots == 0) return hipSuccess;
    const uint64_t blocks = (p.n_slots + 255) / 256;
    const dim3 body_grid(static_cast<uint32_t>(blocks < kMaxBlocks ? blocks : kMaxBlocks));
    if (!p.qi.on) {
        hipLaunchKernelGGL((k_query_bodies<Q, ALL>), body_grid, dim3(256), 0, stream, static_cast<const QueryParams&>(p));
        return hipSuccess;
    }
    if (hipError_t e = hipMemsetAsync(p.qi.words + kQiFarCount, 0, sizeof(uint32_t), stream)) return e;
    hipLaunchKernelGGL((k_qindex_search<Q, ALL>), dim3((p.n_queries + kSearchWaves - 1u) / kSearchWaves), dim3(64 * kSearchWaves), 0, stream, p);
    hipLaunchKernelGGL((k_query_bodies<Q, ALL, true>), body_grid, dim3(256), 0, stream, p);
    return hipSuccess;
}

template <class Q>
hipError_t launch(hipStream_t stream, const QueryCall& p, bool all)
{
    if (p.n_queries == 0) return hipSuccess;
    const dim3 finish_grid((p.n_queries + 63u) / 64u);
    if (all) {
        if constexpr (Q::kList) {
            if (hipError_t e = launch_bodies<Q, true>(stream, p)) return e;
            hipLaunchKernelGGL(k_query_all_finish<Q>, finish_grid, dim3(64), 0, stream, static_cast<const QueryParams&>(p));
        } else {
            return hipErrorInvalidValue;
        }
    } else if constexpr (Q::kClosest) {
        if (hipError_t e = launch_bodies<Q, false>(stream, p)) return e;
        hipLaunchKernelGGL(k_query_finish<Q>, finish_grid, dim3(64), 0, stream, static_cast<const QueryParams&>(p));
    } else {
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

} // namespace

hipError_t launch_query(hipStream_t stream, QueryKind kind, const QueryCall& p, bool all)
{
    switch (kind) {
    case QueryKind::Ray: return launch<RayQuery>(stream, p, all);
    case QueryKind::SphereCast: return launch<SphereCastQuery>(stream, p, all);
    case QueryKind::SphereOverlap: return launch<SphereOverlapQuery>(stream, p, all);
    case QueryKind::SpherePenetration: return launch<SpherePenetrationQuery>(stream, p, all);
    }
    return hipErrorInvalidValue;
}

} // namespace bge
