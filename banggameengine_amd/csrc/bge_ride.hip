// bge_ride.hip — characters ride moving platforms (include/bge_world.h "Character platform riding", bge_world_characters_ride ..;
// DESIGN.md 4.22).
//
// A character remembers the body it stood on when the last update call ended and that body's pose (the anchor).  The next call
// begins by moving the character with the body: its position in the anchor pose's frame is put into the body's current frame.
//   k_char_carry        before the first step: Carry of the header, writes the state's position and the record's flags, carried, turn.
//   k_char_anchor       after the last step: the anchor for the next call from the state's ground probe.
//   k_char_ride_forget  clears the anchors on entities [first, first + count): the host's hook in bge_world_upload_bodies (an entity
//                       index that gets a new body) and bge_world_set_topology (all of them).
// One thread per character.  A body is gathered by slot_of_entity from the arrays the queries read, and it is present exactly when
// load_body of bge_query.hip would load it.  No loop, no LDS, no atomic; the records are only 4-byte aligned by their ABI and are
// moved word by word.  The expressions are the header's, operation for operation (the build's -ffp-contract=off keeps one rounding
// each).
#include <hip/hip_runtime.h>

#include "../../include/bge_world.h"
#include "bge_flatten.hpp"
#include "bge_ride.hpp"

namespace bge {

namespace {

constexpr uint32_t kThreads = 256;
// words of the records (include/bge_world.h)
constexpr uint32_t kStateWords = 20, kRideWords = 16;
// words of a ride record
constexpr uint32_t kRFlags = 0, kREntity = 1, kRAnchor = 2, kRCarried = 9, kRTurn = 12;

struct V3 {
    float x, y, z;
};
struct Q {
    float x, y, z, w;
};

__device__ __forceinline__ Q conj(const Q& q) { return Q{-q.x, -q.y, -q.z, q.w}; }

__device__ __forceinline__ V3 rot(const Q& q, const V3& v)
{
    const float tx = (q.y * v.z - q.z * v.y) * 2.0f;
    const float ty = (q.z * v.x - q.x * v.z) * 2.0f;
    const float tz = (q.x * v.y - q.y * v.x) * 2.0f;
    V3 r;
    r.x = (v.x + q.w * tx) + (q.y * tz - q.z * ty);
    r.y = (v.y + q.w * ty) + (q.z * tx - q.x * tz);
    r.z = (v.z + q.w * tz) + (q.x * ty - q.y * tx);
    return r;
}

__device__ __forceinline__ Q mul(const Q& p, const Q& q)
{
    Q r;
    r.x = ((p.w * q.x + p.x * q.w) + p.y * q.z) - p.z * q.y;
    r.y = ((p.w * q.y + p.y * q.w) + p.z * q.x) - p.x * q.z;
    r.z = ((p.w * q.z + p.z * q.w) + p.x * q.y) - p.y * q.x;
    r.w = ((p.w * q.w - p.x * q.x) - p.y * q.y) - p.z * q.z;
    return r;
}

// The 7 words of the pose of entity e into pose[], if the body is present and rideable
__device__ __forceinline__ bool rideable_pose(const RideParams& p, uint32_t e, uint32_t pose[7])
{
    if (e >= p.n_entities) return false;
    const uint32_t s = p.slot_of_entity[e];
    if (s == kNone || s >= p.n_slots) return false;
    const uint32_t f = p.flags[s];
    // present: the test of load_body (bge_query.hip)
    if ((f & kTypeMask) == 0u || (f & kBDirty)) return false;
    // rideable: Static (1) or Kinematic (3); Dynamic (2) with BGE_CHAR_RIDE_DYNAMIC
    if ((f & kTypeMask) == 2u && !p.dynamic) return false;
    const uint32_t* ps = reinterpret_cast<const uint32_t*>(p.pos) + 3ull * s;
    const uint32_t* qs = reinterpret_cast<const uint32_t*>(p.quat) + 4ull * s;
    pose[0] = ps[0];
    pose[1] = ps[1];
    pose[2] = ps[2];
    pose[3] = qs[0];
    pose[4] = qs[1];
    pose[5] = qs[2];
    pose[6] = qs[3];
    return true;
}

__global__ void __launch_bounds__(kThreads) k_char_carry(RideParams p)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= p.n) return;
    uint32_t* s = static_cast<uint32_t*>(p.state) + uint64_t(kStateWords) * i;
    uint32_t* r = static_cast<uint32_t*>(p.ride) + uint64_t(kRideWords) * i;
    uint32_t flags = 0u;
    V3 carried{0.0f, 0.0f, 0.0f};
    Q turn{0.0f, 0.0f, 0.0f, 1.0f};
    const uint32_t entity = r[kREntity];
    if ((s[4] & BGE_CHAR_GROUNDED) != 0u && entity != BGE_RAY_NO_ENTITY) {
        uint32_t cur[7];
        if (!rideable_pose(p, entity, cur)) {
            flags = BGE_CHAR_RIDE_LOST;
        } else {
            bool moved = false;
#pragma unroll
            for (uint32_t k = 0; k < 7u; ++k) moved = moved || cur[k] != r[kRAnchor + k];
            if (moved) {
                const V3 pos{__uint_as_float(s[0]), __uint_as_float(s[1]), __uint_as_float(s[2])};
                const V3 ap{__uint_as_float(r[kRAnchor]), __uint_as_float(r[kRAnchor + 1]), __uint_as_float(r[kRAnchor + 2])};
                const Q aq{__uint_as_float(r[kRAnchor + 3]), __uint_as_float(r[kRAnchor + 4]), __uint_as_float(r[kRAnchor + 5]),
                           __uint_as_float(r[kRAnchor + 6])};
                const V3 cp{__uint_as_float(cur[0]), __uint_as_float(cur[1]), __uint_as_float(cur[2])};
                const Q cq{__uint_as_float(cur[3]), __uint_as_float(cur[4]), __uint_as_float(cur[5]), __uint_as_float(cur[6])};
                const Q ca = conj(aq);
                const V3 l = rot(ca, V3{pos.x - ap.x, pos.y - ap.y, pos.z - ap.z});
                const V3 m = rot(cq, l);
                const V3 t{cp.x + m.x, cp.y + m.y, cp.z + m.z};
                if (__builtin_isfinite(t.x) && __builtin_isfinite(t.y) && __builtin_isfinite(t.z)) {
                    carried = V3{t.x - pos.x, t.y - pos.y, t.z - pos.z};
                    turn = mul(cq, ca);
                    s[0] = __float_as_uint(t.x);
                    s[1] = __float_as_uint(t.y);
                    s[2] = __float_as_uint(t.z);
                    flags = BGE_CHAR_RIDE_CARRIED;
                } else {
                    flags = BGE_CHAR_RIDE_LOST;
                }
            }
        }
    }
    r[kRFlags] = flags;
    r[kRCarried] = __float_as_uint(carried.x);
    r[kRCarried + 1] = __float_as_uint(carried.y);
    r[kRCarried + 2] = __float_as_uint(carried.z);
    r[kRTurn] = __float_as_uint(turn.x);
    r[kRTurn + 1] = __float_as_uint(turn.y);
    r[kRTurn + 2] = __float_as_uint(turn.z);
    r[kRTurn + 3] = __float_as_uint(turn.w);
}

__global__ void __launch_bounds__(kThreads) k_char_anchor(RideParams p)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= p.n) return;
    const uint32_t* s = static_cast<const uint32_t*>(p.state) + uint64_t(kStateWords) * i;
    uint32_t* r = static_cast<uint32_t*>(p.ride) + uint64_t(kRideWords) * i;
    uint32_t entity = BGE_RAY_NO_ENTITY;
    uint32_t pose[7] = {0u, 0u, 0u, 0u, 0u, 0u, 0u};
    if ((s[4] & BGE_CHAR_GROUNDED) != 0u && s[5] == BGE_RAY_BODY) {
        uint32_t cur[7];
        if (rideable_pose(p, s[6], cur)) {
            entity = s[6];
#pragma unroll
            for (uint32_t k = 0; k < 7u; ++k) pose[k] = cur[k];
        }
    }
    r[kREntity] = entity;
#pragma unroll
    for (uint32_t k = 0; k < 7u; ++k) r[kRAnchor + k] = pose[k];
}

__global__ void __launch_bounds__(kThreads) k_char_ride_forget(void* ride, uint32_t n, uint64_t first, uint64_t count)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    uint32_t* r = static_cast<uint32_t*>(ride) + uint64_t(kRideWords) * i;
    const uint64_t entity = r[kREntity];
    if (entity == BGE_RAY_NO_ENTITY || entity < first || entity - first >= count) return;
    r[kREntity] = BGE_RAY_NO_ENTITY;
#pragma unroll
    for (uint32_t k = 0; k < 7u; ++k) r[kRAnchor + k] = 0u;
}

dim3 grid_of(uint32_t n) { return dim3((n + kThreads - 1u) / kThreads); }

} // namespace

hipError_t launch_char_carry(hipStream_t stream, const RideParams& p)
{
    if (p.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_char_carry, grid_of(p.n), dim3(kThreads), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_char_anchor(hipStream_t stream, const RideParams& p)
{
    if (p.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_char_anchor, grid_of(p.n), dim3(kThreads), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_char_ride_forget(hipStream_t stream, void* ride, uint32_t n, uint64_t first, uint64_t count)
{
    if (n == 0 || count == 0) return hipSuccess;
    hipLaunchKernelGGL(k_char_ride_forget, grid_of(n), dim3(kThreads), 0, stream, ride, n, first, count);
    return hipGetLastError();
}

} // namespace bge
