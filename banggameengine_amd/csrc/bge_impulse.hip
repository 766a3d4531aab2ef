// bge_impulse.hip — impulses on Dynamic bodies, and the stage Push of a character step (include/bge_world.h "Impulses", "Character
// push").
//
// The result must be the bytes Bullet's calls give when made one after the other, however many records name one body, so nothing
// is summed across threads and no float atomic is used:
//   k_imp_keys    one thread per record: Valid, entity -> slot; key = slot (all ones: skipped), value = record index; the status
//                 word of a skipped record
//   (hipcub)      one stable radix sort of (key, value): the records of a body become one run, in ascending record index
//   k_imp_apply   one thread per sorted position; the thread whose predecessor has another key owns the run: it loads the body
//                 once, walks the run record by record in the rule's arithmetic, stores the body once and writes the status words
// A run is walked by ONE thread, whatever its length: the order of the additions is the rule.  Every other thread of k_imp_apply
// reads two keys and leaves.  Two owners never share a slot, so no thread reads what another thread of the pass writes.
//   k_char_push   one thread per character: the push record of its step from the state the step left
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "../../include/bge_world.h"
// (of the contact paths' header only the inertia and vector helpers are used here: its two non-inline functions stay unemitted)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunneeded-internal-declaration"
#include "bge_contact_device.hpp"
#pragma clang diagnostic pop
#include "bge_impulse.hpp"
#include "bge_impulse_math.hpp"

namespace bge {

namespace {

constexpr uint32_t kThreads = 256;

static_assert(impulse::kAtPoint == BGE_IMPULSE_AT_POINT && impulse::kCentral == BGE_IMPULSE_CENTRAL && impulse::kTorque == BGE_IMPULSE_TORQUE &&
                  impulse::kWorldPoint == BGE_IMPULSE_WORLD_POINT,
              "bge_impulse_math.hpp restates bge_impulse_flags");
static_assert(impulse::kApplied == BGE_IMPULSE_APPLIED && impulse::kWoke == BGE_IMPULSE_WOKE && impulse::kInvalid == BGE_IMPULSE_INVALID &&
                  impulse::kNoBody == BGE_IMPULSE_NO_BODY,
              "bge_impulse_math.hpp restates bge_impulse_status");
static_assert(sizeof(bge_impulse) == impulse::kRecordWords * 4, "bge_impulse is 32 bytes");

struct Record {
    uint32_t entity, flags;
    float impulse[3], point[3];
};

__device__ __forceinline__ Record load_record(const uint32_t* __restrict__ records, uint32_t i)
{
    const uint32_t* r = records + uint64_t(impulse::kRecordWords) * i;
    Record o;
    o.entity = r[0];
    o.flags = r[1];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        o.impulse[a] = __uint_as_float(r[2 + a]);
        o.point[a] = __uint_as_float(r[5 + a]);
    }
    return o;
}

// the slot of the Dynamic body of an entity, or kNone
__device__ __forceinline__ uint32_t dynamic_slot(uint32_t entity, uint64_t n_entities, const uint32_t* __restrict__ slot_of_entity,
                                                 const uint32_t* __restrict__ flags)
{
    if (entity >= n_entities) return kNone;
    const uint32_t slot = slot_of_entity[entity];
    if (slot == kNone) return kNone;
    return (flags[slot] & kTypeMask) == 2u ? slot : kNone;
}

__global__ void __launch_bounds__(kThreads) k_imp_keys(ImpulseParams p, WorldView w)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= p.n) return;
    const Record r = load_record(p.records, i);
    uint32_t key = kNone;
    if (!impulse::record_ok(r.flags, r.impulse, r.point)) {
        if (p.status) p.status[i] = impulse::kInvalid;
    } else {
        key = dynamic_slot(r.entity, p.n_entities, p.slot_of_entity, w.flags);
        if (key == kNone && p.status) p.status[i] = impulse::kNoBody;
    }
    p.keys_in[i] = key;
    p.vals_in[i] = i;
}

__global__ void __launch_bounds__(kThreads) k_imp_apply(ImpulseParams p, WorldView w)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= p.n) return;
    const uint32_t slot = p.keys_out[i];
    if (slot == kNone) return;
    if (i > 0u && p.keys_out[i - 1u] == slot) return; // (the run's first thread walks it)
    const uint32_t f0 = w.flags[slot];
    const uint32_t cls = f0 >> kMassShift;
    const float inv_mass = cls != kMassClassArray ? w.mass_palette[cls].x : w.inv_mass[slot];
    F3 v = ld_vel(w.vel, slot);
    F3 av = ld3(w.angvel, slot);
    const bool woke = (f0 & kDrowsy) && w.deact[slot] != 0u;
    // the body's pose, and invI_world of it, once, and only for a run that turns the body
    bool posed = false;
    F3 origin{0.0f, 0.0f, 0.0f};
    M3 invI{};
    for (uint32_t j = i; j < p.n && p.keys_out[j] == slot; ++j) {
        const uint32_t at = p.vals_out[j];
        const Record r = load_record(p.records, at);
        const uint32_t kind = r.flags & impulse::kKindMask;
        const F3 imp{r.impulse[0], r.impulse[1], r.impulse[2]};
        if (kind != impulse::kTorque) {
            v.x = v.x + imp.x * inv_mass;
            v.y = v.y + imp.y * inv_mass;
            v.z = v.z + imp.z * inv_mass;
        }
        if (kind != impulse::kCentral) {
            if (!posed) {
                posed = true;
                origin = ld3(w.pos, slot);
                const float4 cs = w.cshape[slot];
                CtShape shape;
                shape.capsule = (w.cinfo[slot] & kCiCapsule) != 0;
                shape.dims = F3{cs.x, cs.y, cs.z};
                const M3 basis = bt_mat_from_quat(ld4(w.quat, slot));
                invI = ct_inv_inertia_world(basis, ct_inv_inertia_local(ct_local_inertia(shape, w.cmass[slot])));
            }
            F3 t = imp;
            if (kind == impulse::kAtPoint) {
                F3 rel{r.point[0], r.point[1], r.point[2]};
                if (r.flags & impulse::kWorldPoint) rel = sub3(rel, origin);
                t = cross3(rel, imp);
            }
            av = add3(av, mat_vec(invI, t));
        }
        if (p.status) p.status[at] = impulse::kApplied | ((j == i && woke) ? impulse::kWoke : 0u);
    }
    st_vel(w.vel, slot, v);
    st3(w.angvel, slot, av);
    // activate(): ACTIVE_TAG, m_deactivationTime = 0
    uint32_t f = f0 & ~kDrowsy;
    f = (av.x != 0.0f || av.y != 0.0f || av.z != 0.0f) ? (f | kSpin) : (f & ~kSpin);
    if (f0 & kDrowsy) w.deact[slot] = 0u;
    if (f != f0) w.flags[slot] = f;
}

__global__ void __launch_bounds__(kThreads) k_char_push(CharPushParams p, WorldView w)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= p.n) return;
    const uint32_t* s = p.state + 20ull * i;
    uint32_t entity = BGE_RAY_NO_ENTITY, flags = 0u;
    float ix = 0.0f, iy = 0.0f, iz = 0.0f;
    if (!(s[4] & BGE_CHAR_INVALID) && s[10] == BGE_RAY_BODY) {
        const uint32_t hit = s[11];
        const uint32_t slot = dynamic_slot(hit, p.n_entities, p.slot_of_entity, w.flags);
        const float nx = __uint_as_float(s[12]), ny = __uint_as_float(s[13]), nz = __uint_as_float(s[14]);
        if (slot != kNone && (w.group[slot] & p.body_mask) != 0u && __builtin_fabsf(ny) <= p.max_normal_y) {
            const float h = __builtin_sqrtf(nx * nx + nz * nz);
            const float m = p.force * p.dt;
            entity = hit;
            flags = impulse::kCentral;
            ix = (-nx / h) * m;
            iy = 0.0f * m;
            iz = (-nz / h) * m;
        }
    }
    uint32_t* r = p.records + uint64_t(impulse::kRecordWords) * i;
    r[0] = entity;
    r[1] = flags;
    r[2] = __float_as_uint(ix);
    r[3] = __float_as_uint(iy);
    r[4] = __float_as_uint(iz);
    r[5] = 0u;
    r[6] = 0u;
    r[7] = 0u;
}

dim3 grid_of(uint32_t n) { return dim3((n + kThreads - 1u) / kThreads); }

hipError_t sort_pairs(hipStream_t stream, void* tmp, size_t& bytes, const uint32_t* kin, uint32_t* kout, const uint32_t* vin, uint32_t* vout, uint32_t n)
{
    return hipcub::DeviceRadixSort::SortPairs(tmp, bytes, kin, kout, vin, vout, static_cast<int>(n), 0, 32, stream);
}

} // namespace

size_t impulse_sort_bytes(uint32_t n)
{
    size_t bytes = 0;
    (void)sort_pairs(nullptr, nullptr, bytes, nullptr, nullptr, nullptr, nullptr, n);
    return bytes;
}

hipError_t launch_impulses(hipStream_t stream, const ImpulseParams& p, const WorldView& w)
{
    if (p.n == 0) return hipSuccess;
    const dim3 grid = grid_of(p.n), block(kThreads);
    hipLaunchKernelGGL(k_imp_keys, grid, block, 0, stream, p, w);
    size_t bytes = p.sort_bytes;
    if (hipError_t e = sort_pairs(stream, p.sort_tmp, bytes, p.keys_in, p.keys_out, p.vals_in, p.vals_out, p.n)) return e;
    hipLaunchKernelGGL(k_imp_apply, grid, block, 0, stream, p, w);
    return hipGetLastError();
}

hipError_t launch_char_push(hipStream_t stream, const CharPushParams& p, const WorldView& w)
{
    if (p.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_char_push, grid_of(p.n), dim3(kThreads), 0, stream, p, w);
    return hipGetLastError();
}

} // namespace bge
