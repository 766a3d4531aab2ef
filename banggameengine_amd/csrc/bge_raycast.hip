// bge_raycast.hip — ray queries against the device world (include/bge_world.h bge_world_raycast*).
//
// PhysicsSystem::Raycast / RaycastAll (src/physics/PhysicsSystem.cpp:1076-1146) ask Bullet's rayTest for one ray.  Here a batch of
// rays is tested against every body in one streaming pass over the body arrays:
//   k_ray_bodies   one body per lane, grid-stride over the slots.  The batch's rays are staged through LDS in chunks of 256; the
//                  body stays in registers while its workgroup walks every chunk, so the body arrays are read once per batch.
//                  The cull reads flags, position, collider, contact word and the filter words (44 bytes a body) and tests the
//                  body's bounding sphere against the segment; only a candidate reads its quaternion and runs the exact test.
//                  Closest hit: one 64-bit atomicMin per hit on the ray's key (fraction bits << 32 | object code) — f >= 0, so the
//                  bit order is the value order and the tie rule (lowest object code) holds by construction.  All hits: the
//                  (ray, code, f, normal) records are appended behind one atomic per wave ballot.
//   k_ray_finish   one thread per ray: the trigger ghosts (few) and the plane, then the winning key is decoded, the normal of the
//                  winner recomputed with the same device functions, and the bge_ray_hit written.  The key goes back to all ones.
//   k_ray_all_finish  one thread per ray: appends the ghosts' and the plane's hits to the all-hits list.
#include <hip/hip_runtime.h>

#include "../../include/bge_world.h"
#include "bge_flatten.hpp"
#include "bge_kernels.hpp"
#include "bge_ray_device.hpp"
#include "bge_raycast.hpp"

namespace bge {

namespace {

using namespace dev;

constexpr uint32_t kRayChunk = 256;      // rays staged per round (= threads of a workgroup)
constexpr uint32_t kRayMaxBlocks = 2048; // 8 workgroups per CU; more slots are walked grid-stride

// A ray made ready for the tests: mask = 0 when it can see nothing (include/bge_world.h "No hit")
struct RayPrep {
    F3 from, delta;
    float inv_len2, slack, max_distance;
    uint32_t mask;
};

__device__ __forceinline__ bool finite3(const F3& v)
{
    return __builtin_isfinite(v.x) && __builtin_isfinite(v.y) && __builtin_isfinite(v.z);
}

__device__ __forceinline__ RayPrep ray_prep(const void* rays, uint32_t r)
{
    const uint32_t* w = static_cast<const uint32_t*>(rays) + 8ull * r;
    RayPrep p;
    p.from = F3{__uint_as_float(w[0]), __uint_as_float(w[1]), __uint_as_float(w[2])};
    const F3 dir{__uint_as_float(w[3]), __uint_as_float(w[4]), __uint_as_float(w[5])};
    p.max_distance = __uint_as_float(w[6]);
    p.mask = w[7];
    // to - from = direction * max_distance (PhysicsSystem.cpp:1087: to = from + direction * maxDistance)
    p.delta = F3{dir.x * p.max_distance, dir.y * p.max_distance, dir.z * p.max_distance};
    const float len2 = p.delta.x * p.delta.x + p.delta.y * p.delta.y + p.delta.z * p.delta.z;
    const bool ok = finite3(p.from) && finite3(dir) && __builtin_isfinite(p.max_distance) && p.max_distance > 0.0f &&
                    (dir.x != 0.0f || dir.y != 0.0f || dir.z != 0.0f) && finite3(p.delta) && len2 > 0.0f &&
                    __builtin_isfinite(len2) && __builtin_isfinite(p.from.y + p.delta.y);
    if (!ok) p.mask = 0u;
    p.inv_len2 = ok ? 1.0f / len2 : 0.0f;
    // rounding of the cull's closest-point arithmetic is a few ulp of the magnitudes involved: a generous bound keeps it
    // conservative (the exact test decides)
    p.slack = 1e-5f * (__builtin_fabsf(p.from.x) + __builtin_fabsf(p.from.y) + __builtin_fabsf(p.from.z) + __builtin_fabsf(p.delta.x) +
                       __builtin_fabsf(p.delta.y) + __builtin_fabsf(p.delta.z));
    return p;
}

__device__ __forceinline__ unsigned long long ray_key(float f, uint32_t code)
{
    return (static_cast<unsigned long long>(__float_as_uint(f)) << 32) | code;
}

template <bool ALL>
__global__ void __launch_bounds__(256) k_ray_bodies(RayParams p)
{
    __shared__ float4 s_from[kRayChunk];  // from.xyz, 1 / |delta|^2
    __shared__ float4 s_delta[kRayChunk]; // delta.xyz, layer mask bits (0: the ray sees nothing)
    __shared__ float s_slack[kRayChunk];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    for (uint64_t base = blockIdx.x * 256ull; base < p.n_slots; base += gridDim.x * 256ull) {
        const uint64_t s = base + tid;
        bool cand = false, capsule = false;
        F3 c{0.0f, 0.0f, 0.0f}, dims{0.0f, 0.0f, 0.0f};
        uint32_t grp = 0;
        float rb = 0.0f;
        if (s < p.n_slots) {
            const uint32_t f = p.flags[s];
            // in Bullet's world: a body of any type, not uploaded since the last physics tick (EnsureRigidBody creates it then)
            if ((f & kTypeMask) != 0u && !(f & kBDirty)) {
                grp = p.group[s];
                cand = grp != 0u && p.mask[s] != 0u;
                if (cand) {
                    c = ld3(p.pos, static_cast<uint32_t>(s));
                    const float4 cs = p.cshape[s];
                    dims = F3{cs.x, cs.y, cs.z};
                    capsule = (p.cinfo[s] & kCiCapsule) != 0u;
                    const float rad = capsule ? cs.x + cs.y : __builtin_sqrtf(cs.x * cs.x + cs.y * cs.y + cs.z * cs.z);
                    rb = rad * 1.0001f + 1e-5f * (__builtin_fabsf(c.x) + __builtin_fabsf(c.y) + __builtin_fabsf(c.z)) + 1e-6f;
                }
            }
        }
        if (__syncthreads_or(cand) == 0) continue; // (uniform: a workgroup without candidates skips the rays)
        bool have_q = false;
        Q4 q{0.0f, 0.0f, 0.0f, 1.0f};
        for (uint32_t r0 = 0; r0 < p.n_rays; r0 += kRayChunk) {
            const uint32_t nr = p.n_rays - r0 < kRayChunk ? p.n_rays - r0 : kRayChunk;
            __syncthreads();
            if (tid < nr) {
                const RayPrep rp = ray_prep(p.rays, r0 + tid);
                s_from[tid] = make_float4(rp.from.x, rp.from.y, rp.from.z, rp.inv_len2);
                s_delta[tid] = make_float4(rp.delta.x, rp.delta.y, rp.delta.z, __uint_as_float(rp.mask));
                s_slack[tid] = rp.slack;
            }
            __syncthreads();
            for (uint32_t k = 0; k < nr; ++k) {
                const float4 a = s_from[k], b = s_delta[k];
                bool hit = false;
                float fh = 0.0f;
                F3 nh{0.0f, 0.0f, 0.0f};
                if (cand && (grp & __float_as_uint(b.w)) != 0u) {
                    // bounding sphere against the segment
                    const float wx = c.x - a.x, wy = c.y - a.y, wz = c.z - a.z;
                    float t = (wx * b.x + wy * b.y + wz * b.z) * a.w;
                    t = t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t);
                    const float ex = wx - b.x * t, ey = wy - b.y * t, ez = wz - b.z * t;
                    const float rr = rb + s_slack[k];
                    if (ex * ex + ey * ey + ez * ez <= rr * rr) {
                        if (!have_q) {
                            q = ld4(p.quat, static_cast<uint32_t>(s));
                            have_q = true;
                        }
                        F3 n{0.0f, 0.0f, 0.0f};
                        const float fr = ray_shape(F3{a.x, a.y, a.z}, F3{b.x, b.y, b.z}, c, q, capsule, dims, n);
                        if (fr >= 0.0f) {
                            if constexpr (!ALL) {
                                atomicMin(p.keys + r0 + k, ray_key(fr, p.entity_of_slot[s] & kRayEntityMask));
                            } else {
                                hit = true;
                                fh = fr;
                                nh = n;
                            }
                        }
                    }
                }
                if constexpr (ALL) {
                    const unsigned long long m = __ballot(hit);
                    if (m != 0ull) {
                        const uint32_t leader = static_cast<uint32_t>(__ffsll(static_cast<long long>(m))) - 1u;
                        uint32_t at = 0;
                        if (lane == leader) at = atomicAdd(p.all_count, static_cast<uint32_t>(__popcll(m)));
                        at = __shfl(at, static_cast<int>(leader), 64);
                        if (hit) {
                            at += static_cast<uint32_t>(__popcll(m & ((1ull << lane) - 1ull)));
                            if (at < p.all_cap) {
                                RayAllRec& o = p.all[at];
                                o.ray = r0 + k;
                                o.code = p.entity_of_slot[s] & kRayEntityMask;
                                o.f = fh;
                                o.n[0] = nh.x;
                                o.n[1] = nh.y;
                                o.n[2] = nh.z;
                            }
                        }
                    }
                }
            }
        }
    }
}

// ghost g of the list against ray rp: fraction or -1, world normal
__device__ __forceinline__ float ray_ghost(const RayParams& p, const RayPrep& rp, uint32_t g, F3& n)
{
    const RayGhost gh = p.ghosts[g];
    if ((gh.group & rp.mask) == 0u || gh.mask == 0u) return -1.0f;
    const float* pose = p.ghost_pose + 8ull * gh.trigger;
    return ray_shape(rp.from, rp.delta, F3{pose[0], pose[1], pose[2]}, Q4{pose[4], pose[5], pose[6], pose[7]}, gh.capsule != 0u,
                     F3{gh.dims[0], gh.dims[1], gh.dims[2]}, n);
}

__device__ __forceinline__ bool ray_sees_plane(const RayParams& p, const RayPrep& rp)
{
    return p.plane && (rp.mask & 2u) != 0u; // group StaticFilter (2), mask AllFilter (PhysicsSystem.cpp:149-166)
}

__global__ void __launch_bounds__(64) k_ray_finish(RayParams p)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= p.n_rays) return;
    const RayPrep rp = ray_prep(p.rays, r);
    unsigned long long key = p.keys[r];
    p.keys[r] = ~0ull; // ready for the next batch
    uint32_t gwin = 0;
    if (rp.mask != 0u) {
        for (uint32_t g = 0; g < p.n_ghosts; ++g) {
            F3 n;
            const float f = ray_ghost(p, rp, g, n);
            if (f >= 0.0f) {
                const unsigned long long k = ray_key(f, kRayCodeGhost | (p.ghosts[g].entity & kRayEntityMask));
                if (k < key) {
                    key = k;
                    gwin = g;
                }
            }
        }
        if (ray_sees_plane(p, rp)) {
            F3 n;
            const float f = ray_plane(rp.from.y, rp.from.y + rp.delta.y, n);
            if (f >= 0.0f) {
                const unsigned long long k = ray_key(f, kRayCodePlane | kRayEntityMask);
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
        (void)ray_shape(rp.from, rp.delta, ld3(p.pos, s), ld4(p.quat, s), (p.cinfo[s] & kCiCapsule) != 0u, F3{cs.x, cs.y, cs.z}, n);
        out_kind = BGE_RAY_BODY;
    } else if (kind == 1u) {
        (void)ray_ghost(p, rp, gwin, n);
        out_kind = BGE_RAY_TRIGGER;
    } else {
        (void)ray_plane(rp.from.y, rp.from.y + rp.delta.y, n);
        out_kind = BGE_RAY_GROUND;
        out_entity = BGE_RAY_NO_ENTITY;
    }
    o[0] = out_kind;
    o[1] = out_entity;
    o[2] = __float_as_uint(f);
    o[3] = __float_as_uint(f * rp.max_distance);
    o[4] = __float_as_uint(rp.from.x + rp.delta.x * f);
    o[5] = __float_as_uint(rp.from.y + rp.delta.y * f);
    o[6] = __float_as_uint(rp.from.z + rp.delta.z * f);
    o[7] = __float_as_uint(n.x);
    o[8] = __float_as_uint(n.y);
    o[9] = __float_as_uint(n.z);
}

__device__ __forceinline__ void ray_append(const RayParams& p, uint32_t r, uint32_t code, float f, const F3& n)
{
    const uint32_t at = atomicAdd(p.all_count, 1u);
    if (at >= p.all_cap) return;
    RayAllRec& o = p.all[at];
    o.ray = r;
    o.code = code;
    o.f = f;
    o.n[0] = n.x;
    o.n[1] = n.y;
    o.n[2] = n.z;
}

__global__ void __launch_bounds__(64) k_ray_all_finish(RayParams p)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= p.n_rays) return;
    const RayPrep rp = ray_prep(p.rays, r);
    if (rp.mask == 0u) return;
    for (uint32_t g = 0; g < p.n_ghosts; ++g) {
        F3 n;
        const float f = ray_ghost(p, rp, g, n);
        if (f >= 0.0f) ray_append(p, r, kRayCodeGhost | (p.ghosts[g].entity & kRayEntityMask), f, n);
    }
    if (ray_sees_plane(p, rp)) {
        F3 n;
        const float f = ray_plane(rp.from.y, rp.from.y + rp.delta.y, n);
        if (f >= 0.0f) ray_append(p, r, kRayCodePlane | kRayEntityMask, f, n);
    }
}

inline dim3 body_grid(uint64_t n_slots)
{
    const uint64_t b = (n_slots + 255) / 256;
    return dim3(static_cast<uint32_t>(b < kRayMaxBlocks ? b : kRayMaxBlocks));
}

} // namespace

hipError_t launch_ray_closest(hipStream_t stream, const RayParams& p)
{
    if (p.n_rays == 0) return hipSuccess;
    if (p.n_slots) hipLaunchKernelGGL(k_ray_bodies<false>, body_grid(p.n_slots), dim3(256), 0, stream, p);
    hipLaunchKernelGGL(k_ray_finish, dim3((p.n_rays + 63u) / 64u), dim3(64), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_ray_all(hipStream_t stream, const RayParams& p)
{
    if (p.n_rays == 0) return hipSuccess;
    if (p.n_slots) hipLaunchKernelGGL(k_ray_bodies<true>, body_grid(p.n_slots), dim3(256), 0, stream, p);
    hipLaunchKernelGGL(k_ray_all_finish, dim3((p.n_rays + 63u) / 64u), dim3(64), 0, stream, p);
    return hipGetLastError();
}

} // namespace bge
