// bge_spherecast.hip — sphere casts and sphere overlap queries against the device world (include/bge_world.h
// bge_world_sphere_cast*, bge_world_overlap_sphere).  The reference has no such query; they are the two primitives
// its btKinematicCharacterController is made of (a swept volume, an overlap volume) for the one shape that is exact in closed form
// against every shape of the world.  The kernels have the shape of the ray queries' (bge_raycast.hip):
//   k_cast_bodies     one body per lane, grid-stride over the slots; the batch's casts staged through LDS in chunks of 256, so the
//                     body arrays are read once per batch.  Cull: the body's bounding sphere grown by the cast's radius against
//                     the segment of the centre; only a candidate reads its quaternion and runs the exact test
//                     (bge_sphere_device.hpp).  Closest touch: a 64-bit atomicMin on (fraction bits << 32 | object code); all
//                     touches: records appended behind one atomic per wave ballot.
//   k_cast_finish     one thread per cast: the trigger ghosts and the plane, then the winner's normal recomputed and the
//                     bge_ray_hit written (point = the centre at the touch pulled back by the radius along the normal).
//   k_cast_all_finish one thread per cast: the ghosts' and the plane's touches appended.
//   k_overlap_bodies / k_overlap_finish   the same two passes for bge_sphere records: every object whose distance to the centre is
//                     at most the radius is appended with that distance.
#include <hip/hip_runtime.h>

#include "../../include/bge_world.h"
#include "bge_flatten.hpp"
#include "bge_kernels.hpp"
#include "bge_sphere_device.hpp"
#include "bge_spherecast.hpp"

namespace bge {

namespace {

using namespace dev;

constexpr uint32_t kChunk = 256;      // queries staged per round (= threads of a workgroup)
constexpr uint32_t kMaxBlocks = 2048; // 8 workgroups per CU; more slots are walked grid-stride

__device__ __forceinline__ bool finite3(const F3& v)
{
    return __builtin_isfinite(v.x) && __builtin_isfinite(v.y) && __builtin_isfinite(v.z);
}
__device__ __forceinline__ float abs_sum(const F3& v) { return __builtin_fabsf(v.x) + __builtin_fabsf(v.y) + __builtin_fabsf(v.z); }

// A cast made ready for the tests: mask = 0 when it can touch nothing (include/bge_world.h "No hit")
struct CastPrep {
    F3 from, delta;
    float inv_len2, slack, max_distance, radius;
    uint32_t mask;
};

__device__ __forceinline__ CastPrep cast_prep(const void* casts, uint32_t r)
{
    const uint32_t* w = static_cast<const uint32_t*>(casts) + 10ull * r;
    CastPrep p;
    p.from = F3{__uint_as_float(w[0]), __uint_as_float(w[1]), __uint_as_float(w[2])};
    const F3 dir{__uint_as_float(w[3]), __uint_as_float(w[4]), __uint_as_float(w[5])};
    p.max_distance = __uint_as_float(w[6]);
    p.radius = __uint_as_float(w[7]);
    p.mask = w[8];
    p.delta = F3{dir.x * p.max_distance, dir.y * p.max_distance, dir.z * p.max_distance};
    const float len2 = p.delta.x * p.delta.x + p.delta.y * p.delta.y + p.delta.z * p.delta.z;
    const bool ok = finite3(p.from) && finite3(dir) && __builtin_isfinite(p.max_distance) && p.max_distance > 0.0f &&
                    (dir.x != 0.0f || dir.y != 0.0f || dir.z != 0.0f) && finite3(p.delta) && len2 > 0.0f && __builtin_isfinite(len2) &&
                    __builtin_isfinite(p.from.y + p.delta.y) && __builtin_isfinite(p.radius) && p.radius >= 0.0f;
    if (!ok) p.mask = 0u;
    p.inv_len2 = ok ? 1.0f / len2 : 0.0f;
    // keeps the cull conservative against the rounding of its own arithmetic (the exact test decides)
    p.slack = 1e-5f * (abs_sum(p.from) + abs_sum(p.delta) + p.radius);
    return p;
}

// An overlap sphere made ready: mask = 0 when it reports nothing
struct OverlapPrep {
    F3 c;
    float radius, slack;
    uint32_t mask;
};

__device__ __forceinline__ OverlapPrep overlap_prep(const void* spheres, uint32_t r)
{
    const uint32_t* w = static_cast<const uint32_t*>(spheres) + 5ull * r;
    OverlapPrep p;
    p.c = F3{__uint_as_float(w[0]), __uint_as_float(w[1]), __uint_as_float(w[2])};
    p.radius = __uint_as_float(w[3]);
    p.mask = w[4];
    if (!(finite3(p.c) && __builtin_isfinite(p.radius) && p.radius >= 0.0f)) p.mask = 0u;
    p.slack = 1e-5f * (abs_sum(p.c) + p.radius);
    return p;
}

__device__ __forceinline__ unsigned long long cast_key(float f, uint32_t code)
{
    return (static_cast<unsigned long long>(__float_as_uint(f)) << 32) | code;
}

// The body of a lane as the cull needs it; cand = false when it is not in the world or no query can see it
struct BodyLane {
    bool cand, capsule;
    F3 c, dims;
    uint32_t grp;
    float rb; // bounding radius with the rounding of the cull's arithmetic on top
};

__device__ __forceinline__ BodyLane load_body(const RayParams& p, uint64_t s)
{
    BodyLane b{false, false, F3{0.0f, 0.0f, 0.0f}, F3{0.0f, 0.0f, 0.0f}, 0u, 0.0f};
    if (s >= p.n_slots) return b;
    const uint32_t f = p.flags[s];
    // in the world: a body of any type, not uploaded since the last physics tick (as for rays)
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

// Appends the records of the lanes with `hit` behind the counter: one atomic per wave
__device__ __forceinline__ void append_wave(const RayParams& p, bool hit, uint32_t query, uint32_t code, float f, const F3& n)
{
    const unsigned long long m = __ballot(hit);
    if (m == 0ull) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t leader = static_cast<uint32_t>(__ffsll(static_cast<long long>(m))) - 1u;
    uint32_t at = 0;
    if (lane == leader) at = atomicAdd(p.all_count, static_cast<uint32_t>(__popcll(m)));
    at = __shfl(at, static_cast<int>(leader), 64);
    if (!hit) return;
    at += static_cast<uint32_t>(__popcll(m & ((1ull << lane) - 1ull)));
    if (at >= p.all_cap) return;
    RayAllRec& o = p.all[at];
    o.ray = query;
    o.code = code;
    o.f = f;
    o.n[0] = n.x;
    o.n[1] = n.y;
    o.n[2] = n.z;
}

__device__ __forceinline__ void append_one(const RayParams& p, uint32_t query, uint32_t code, float f, const F3& n)
{
    const uint32_t at = atomicAdd(p.all_count, 1u);
    if (at >= p.all_cap) return;
    RayAllRec& o = p.all[at];
    o.ray = query;
    o.code = code;
    o.f = f;
    o.n[0] = n.x;
    o.n[1] = n.y;
    o.n[2] = n.z;
}

template <bool ALL>
__global__ void __launch_bounds__(256) k_cast_bodies(RayParams p)
{
    __shared__ float4 s_from[kChunk];  // from.xyz, 1 / |delta|^2
    __shared__ float4 s_delta[kChunk]; // delta.xyz, layer mask bits (0: the cast touches nothing)
    __shared__ float2 s_sr[kChunk];    // slack, radius
    const uint32_t tid = threadIdx.x;
    for (uint64_t base = blockIdx.x * 256ull; base < p.n_slots; base += gridDim.x * 256ull) {
        const uint64_t s = base + tid;
        const BodyLane b = load_body(p, s);
        if (__syncthreads_or(b.cand) == 0) continue; // (uniform: a workgroup without candidates skips the casts)
        bool have_q = false;
        Q4 q{0.0f, 0.0f, 0.0f, 1.0f};
        for (uint32_t r0 = 0; r0 < p.n_rays; r0 += kChunk) {
            const uint32_t nr = p.n_rays - r0 < kChunk ? p.n_rays - r0 : kChunk;
            __syncthreads();
            if (tid < nr) {
                const CastPrep cp = cast_prep(p.rays, r0 + tid);
                s_from[tid] = make_float4(cp.from.x, cp.from.y, cp.from.z, cp.inv_len2);
                s_delta[tid] = make_float4(cp.delta.x, cp.delta.y, cp.delta.z, __uint_as_float(cp.mask));
                s_sr[tid] = make_float2(cp.slack, cp.radius);
            }
            __syncthreads();
            for (uint32_t k = 0; k < nr; ++k) {
                const float4 a = s_from[k], d = s_delta[k];
                bool hit = false;
                float fh = 0.0f;
                F3 nh{0.0f, 0.0f, 0.0f};
                if (b.cand && (b.grp & __float_as_uint(d.w)) != 0u) {
                    // bounding sphere, grown by the cast's radius, against the segment of the centre
                    const float2 sr = s_sr[k];
                    const float wx = b.c.x - a.x, wy = b.c.y - a.y, wz = b.c.z - a.z;
                    float t = (wx * d.x + wy * d.y + wz * d.z) * a.w;
                    t = t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t);
                    const float ex = wx - d.x * t, ey = wy - d.y * t, ez = wz - d.z * t;
                    const float rr = b.rb + sr.y * 1.0001f + sr.x;
                    if (ex * ex + ey * ey + ez * ez <= rr * rr) {
                        if (!have_q) {
                            q = ld4(p.quat, static_cast<uint32_t>(s));
                            have_q = true;
                        }
                        F3 n{0.0f, 0.0f, 0.0f};
                        const float fr = sphere_cast_shape(F3{a.x, a.y, a.z}, F3{d.x, d.y, d.z}, sr.y, b.c, q, b.capsule, b.dims, n);
                        if (fr >= 0.0f) {
                            if constexpr (!ALL) {
                                atomicMin(p.keys + r0 + k, cast_key(fr, p.entity_of_slot[s] & kRayEntityMask));
                            } else {
                                hit = true;
                                fh = fr;
                                nh = n;
                            }
                        }
                    }
                }
                if constexpr (ALL) append_wave(p, hit, r0 + k, hit ? p.entity_of_slot[s] & kRayEntityMask : 0u, fh, nh);
            }
        }
    }
}

__device__ __forceinline__ bool ghost_visible(const RayGhost& gh, uint32_t mask) { return (gh.group & mask) != 0u && gh.mask != 0u; }

// ghost g of the list against cast cp: fraction or -1, world normal
__device__ __forceinline__ float cast_ghost(const RayParams& p, const CastPrep& cp, uint32_t g, F3& n)
{
    const RayGhost gh = p.ghosts[g];
    if (!ghost_visible(gh, cp.mask)) return -1.0f;
    const float* pose = p.ghost_pose + 8ull * gh.trigger;
    return sphere_cast_shape(cp.from, cp.delta, cp.radius, F3{pose[0], pose[1], pose[2]}, Q4{pose[4], pose[5], pose[6], pose[7]},
                             gh.capsule != 0u, F3{gh.dims[0], gh.dims[1], gh.dims[2]}, n);
}

__device__ __forceinline__ bool sees_plane(const RayParams& p, uint32_t mask)
{
    return p.plane && (mask & 2u) != 0u; // group StaticFilter (2), mask AllFilter, as for rays
}

__global__ void __launch_bounds__(64) k_cast_finish(RayParams p)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= p.n_rays) return;
    const CastPrep cp = cast_prep(p.rays, r);
    unsigned long long key = p.keys[r];
    p.keys[r] = ~0ull; // ready for the next batch
    uint32_t gwin = 0;
    if (cp.mask != 0u) {
        for (uint32_t g = 0; g < p.n_ghosts; ++g) {
            F3 n;
            const float f = cast_ghost(p, cp, g, n);
            if (f >= 0.0f) {
                const unsigned long long k = cast_key(f, kRayCodeGhost | (p.ghosts[g].entity & kRayEntityMask));
                if (k < key) {
                    key = k;
                    gwin = g;
                }
            }
        }
        if (sees_plane(p, cp.mask)) {
            F3 n;
            const float f = sphere_cast_plane(cp.from.y, cp.from.y + cp.delta.y, cp.radius, n);
            if (f >= 0.0f) {
                const unsigned long long k = cast_key(f, kRayCodePlane | kRayEntityMask);
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
    const float f = __uint_as_float(static_cast<uint32_t>(key >> 32));
    const uint32_t code = static_cast<uint32_t>(key);
    const uint32_t kind = code >> 30, ent = code & kRayEntityMask;
    F3 n{0.0f, 0.0f, 0.0f};
    uint32_t out_kind, out_entity = ent;
    if (kind == 0u) {
        const uint32_t s = p.slot_of_entity[ent];
        const float4 cs = p.cshape[s];
        (void)sphere_cast_shape(cp.from, cp.delta, cp.radius, ld3(p.pos, s), ld4(p.quat, s), (p.cinfo[s] & kCiCapsule) != 0u,
                                F3{cs.x, cs.y, cs.z}, n);
        out_kind = BGE_RAY_BODY;
    } else if (kind == 1u) {
        (void)cast_ghost(p, cp, gwin, n);
        out_kind = BGE_RAY_TRIGGER;
    } else {
        (void)sphere_cast_plane(cp.from.y, cp.from.y + cp.delta.y, cp.radius, n);
        out_kind = BGE_RAY_GROUND;
        out_entity = BGE_RAY_NO_ENTITY;
    }
    // the contact point: the centre at the touch pulled back by the radius along the normal; on the plane y is 0 by definition
    // (bge_world_sphere_cast_all computes the same expressions on the host)
    const float py = (cp.from.y + cp.delta.y * f) - cp.radius * n.y;
    o[0] = out_kind;
    o[1] = out_entity;
    o[2] = __float_as_uint(f);
    o[3] = __float_as_uint(f * cp.max_distance);
    o[4] = __float_as_uint((cp.from.x + cp.delta.x * f) - cp.radius * n.x);
    o[5] = __float_as_uint(kind == 2u ? 0.0f : py);
    o[6] = __float_as_uint((cp.from.z + cp.delta.z * f) - cp.radius * n.z);
    o[7] = __float_as_uint(n.x);
    o[8] = __float_as_uint(n.y);
    o[9] = __float_as_uint(n.z);
}

__global__ void __launch_bounds__(64) k_cast_all_finish(RayParams p)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= p.n_rays) return;
    const CastPrep cp = cast_prep(p.rays, r);
    if (cp.mask == 0u) return;
    for (uint32_t g = 0; g < p.n_ghosts; ++g) {
        F3 n;
        const float f = cast_ghost(p, cp, g, n);
        if (f >= 0.0f) append_one(p, r, kRayCodeGhost | (p.ghosts[g].entity & kRayEntityMask), f, n);
    }
    if (sees_plane(p, cp.mask)) {
        F3 n;
        const float f = sphere_cast_plane(cp.from.y, cp.from.y + cp.delta.y, cp.radius, n);
        if (f >= 0.0f) append_one(p, r, kRayCodePlane | kRayEntityMask, f, n);
    }
}

__global__ void __launch_bounds__(256) k_overlap_bodies(RayParams p)
{
    __shared__ float4 s_c[kChunk];  // centre.xyz, radius
    __shared__ float2 s_ms[kChunk]; // layer mask bits (0: the sphere reports nothing), slack
    const uint32_t tid = threadIdx.x;
    for (uint64_t base = blockIdx.x * 256ull; base < p.n_slots; base += gridDim.x * 256ull) {
        const uint64_t s = base + tid;
        const BodyLane b = load_body(p, s);
        if (__syncthreads_or(b.cand) == 0) continue;
        bool have_q = false;
        Q4 q{0.0f, 0.0f, 0.0f, 1.0f};
        for (uint32_t r0 = 0; r0 < p.n_rays; r0 += kChunk) {
            const uint32_t nr = p.n_rays - r0 < kChunk ? p.n_rays - r0 : kChunk;
            __syncthreads();
            if (tid < nr) {
                const OverlapPrep op = overlap_prep(p.rays, r0 + tid);
                s_c[tid] = make_float4(op.c.x, op.c.y, op.c.z, op.radius);
                s_ms[tid] = make_float2(__uint_as_float(op.mask), op.slack);
            }
            __syncthreads();
            for (uint32_t k = 0; k < nr; ++k) {
                const float4 a = s_c[k];
                const float2 ms = s_ms[k];
                bool hit = false;
                float dist = 0.0f;
                if (b.cand && (b.grp & __float_as_uint(ms.x)) != 0u) {
                    const float ex = b.c.x - a.x, ey = b.c.y - a.y, ez = b.c.z - a.z;
                    const float rr = b.rb + a.w * 1.0001f + ms.y;
                    if (ex * ex + ey * ey + ez * ez <= rr * rr) {
                        if (!have_q) {
                            q = ld4(p.quat, static_cast<uint32_t>(s));
                            have_q = true;
                        }
                        dist = point_shape_distance(F3{a.x, a.y, a.z}, b.c, q, b.capsule, b.dims);
                        hit = dist <= a.w;
                    }
                }
                append_wave(p, hit, r0 + k, hit ? p.entity_of_slot[s] & kRayEntityMask : 0u, dist, F3{0.0f, 0.0f, 0.0f});
            }
        }
    }
}

__global__ void __launch_bounds__(64) k_overlap_finish(RayParams p)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= p.n_rays) return;
    const OverlapPrep op = overlap_prep(p.rays, r);
    if (op.mask == 0u) return;
    const F3 zero{0.0f, 0.0f, 0.0f};
    for (uint32_t g = 0; g < p.n_ghosts; ++g) {
        const RayGhost gh = p.ghosts[g];
        if (!ghost_visible(gh, op.mask)) continue;
        const float* pose = p.ghost_pose + 8ull * gh.trigger;
        const float dist = point_shape_distance(op.c, F3{pose[0], pose[1], pose[2]}, Q4{pose[4], pose[5], pose[6], pose[7]}, gh.capsule != 0u,
                                                F3{gh.dims[0], gh.dims[1], gh.dims[2]});
        if (dist <= op.radius) append_one(p, r, kRayCodeGhost | (gh.entity & kRayEntityMask), dist, zero);
    }
    if (sees_plane(p, op.mask) && __builtin_fabsf(op.c.y) <= op.radius) append_one(p, r, kRayCodePlane | kRayEntityMask, __builtin_fabsf(op.c.y), zero);
}

inline dim3 body_grid(uint64_t n_slots)
{
    const uint64_t b = (n_slots + 255) / 256;
    return dim3(static_cast<uint32_t>(b < kMaxBlocks ? b : kMaxBlocks));
}

} // namespace

hipError_t launch_sphere_cast_closest(hipStream_t stream, const RayParams& p)
{
    if (p.n_rays == 0) return hipSuccess;
    if (p.n_slots) hipLaunchKernelGGL(k_cast_bodies<false>, body_grid(p.n_slots), dim3(256), 0, stream, p);
    hipLaunchKernelGGL(k_cast_finish, dim3((p.n_rays + 63u) / 64u), dim3(64), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_sphere_cast_all(hipStream_t stream, const RayParams& p)
{
    if (p.n_rays == 0) return hipSuccess;
    if (p.n_slots) hipLaunchKernelGGL(k_cast_bodies<true>, body_grid(p.n_slots), dim3(256), 0, stream, p);
    hipLaunchKernelGGL(k_cast_all_finish, dim3((p.n_rays + 63u) / 64u), dim3(64), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_sphere_overlap(hipStream_t stream, const RayParams& p)
{
    if (p.n_rays == 0) return hipSuccess;
    if (p.n_slots) hipLaunchKernelGGL(k_overlap_bodies, body_grid(p.n_slots), dim3(256), 0, stream, p);
    hipLaunchKernelGGL(k_overlap_finish, dim3((p.n_rays + 63u) / 64u), dim3(64), 0, stream, p);
    return hipGetLastError();
}

} // namespace bge
