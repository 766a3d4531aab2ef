// bge_debug.hip — the physics debug overlay from the device (include/bge_world.h bge_world_debug_lines*).
//
// PhysicsSystem::CollectDebugLines + BulletDebugDrawer (src/physics/PhysicsSystem.cpp:1148-1175, BulletDebugDrawer.cpp) walk every
// collision object and every manifold point on the host.  Here the bodies, ghosts and manifolds live in HBM, so the lines are made
// there: a variable-length expansion (0 / 12 / 120 records of 28 bytes per item), write-bound.  The items are
//   [0] the plane, [1 .. n_entities] the entities in ENTITY order (through slot_of_entity), then the ghosts in list order,
// which is the fixed order of the shapes section.
//   k_debug_count     one item per lane: its line count, summed per workgroup (256 items).
//   k_debug_scan      one workgroup: exclusive sum of the workgroups' totals (64-bit), *total = lines of the shapes section.
//   k_debug_emit      a workgroup owns 256 consecutive items, hence one contiguous range of output bytes.  It stages the items
//                     (origin, basis or the capsule's normalised axes, dimensions, colour) in LDS once, repeats the in-workgroup
//                     scan, then walks its range 256 lines at a time: each lane finds its line's item by bisection over the
//                     offsets, builds the record and writes its seven dwords (a wave covers 1,792 consecutive bytes).  Staging the
//                     records in LDS and streaming them out as whole dwords / 16-byte pieces measured no faster for boxes and
//                     slower for capsules, so the plain form stays.
//   k_debug_contacts_bodies / _pairs   one entity / pair per lane; the points are visited twice (count, then write) and appended
//                     behind the shapes section with one 64-bit atomic per wave.
#include <hip/hip_runtime.h>

#include "../../include/bge_world.h"
#include "bge_debug.hpp"
#include "bge_device_math.hpp"
#include "bge_flatten.hpp"
#include "bge_kernels.hpp"

namespace bge {

namespace {

using namespace dev;

constexpr uint32_t kThreads = kDebugItemsPerBlock;
constexpr uint32_t kItemWords = 16;  // origin 3, basis / axes 9, dimensions 3, colour
constexpr uint32_t kColStatic = 0xff7f7f7fu, kColDynamic = 0xff00ffffu, kColTrigger = 0xffff00ffu, kColContact = 0xff0000ffu;

// cos / sin of (i / 24) * SIMD_2_PI and of (i / 12) * SIMD_HALF_PI, the angles formed in binary32 as BulletDebugDrawer.cpp:244-264
// forms them (SIMD_HALF_PI = SIMD_2_PI * 0.25f)
constexpr float kRingCos[25] = {1.0f,          0.965925813f,  0.866025388f,  0.707106769f,  0.49999997f,    0.258819073f, -4.37113883e-08f,
                                -0.258819044f, -0.50000006f,  -0.707106769f, -0.866025388f, -0.965925872f,  -1.0f,        -0.965925753f,
                                -0.866025388f, -0.70710665f,  -0.499999911f, -0.258818984f, 1.19248806e-08f, 0.258819461f, 0.499999911f,
                                0.707107008f,  0.866025567f,  0.965925872f,  1.0f};
constexpr float kRingSin[25] = {0.0f,          0.258819044f,  0.5f,          0.707106769f,  0.866025448f,  0.965925813f,  1.0f,
                                0.965925813f,  0.866025388f,  0.707106769f,  0.50000006f,   0.258818924f,  -8.74227766e-08f, -0.258819312f,
                                -0.49999997f,  -0.707106888f, -0.866025448f, -0.965925872f, -1.0f,         -0.965925694f, -0.866025448f,
                                -0.707106531f, -0.499999762f, -0.258818835f, 1.74845553e-07f};
constexpr float kHemiCos[13] = {1.0f,        0.991444886f, 0.965925813f, 0.923879504f, 0.866025388f, 0.793353319f,    0.707106769f,
                                0.60876143f, 0.49999997f,  0.382683426f, 0.258819073f, 0.130526125f, -4.37113883e-08f};
constexpr float kHemiSin[13] = {0.0f,         0.1305262f,   0.258819044f, 0.382683456f, 0.5f,         0.60876143f, 0.707106769f,
                                0.793353319f, 0.866025448f, 0.923879504f, 0.965925813f, 0.991444886f, 1.0f};

struct Item {
    F3 o;
    Q4 q;
    F3 dims;
    uint32_t colour;
    bool capsule;
};

// the closed box region_min <= v <= region_max in plain binary32 compares: a NaN or min > max admits nothing
__device__ __forceinline__ bool in_region(const DebugParams& p, const F3& v)
{
    if (!p.use_region) return true;
    return p.region_min[0] <= v.x && v.x <= p.region_max[0] && p.region_min[1] <= v.y && v.y <= p.region_max[1] &&
           p.region_min[2] <= v.z && v.z <= p.region_max[2];
}

// lines of item `it`; FULL also loads what the emit needs
template <bool FULL>
__device__ __forceinline__ uint32_t load_item(const DebugParams& p, uint64_t it, Item& d)
{
    d.capsule = false;
    if (it == 0) {
        d.o = F3{0.0f, 0.0f, 0.0f};
        d.colour = kColStatic; // the ground body is a static object
        return p.plane ? kDebugPlaneLines : 0u;
    }
    const uint64_t e = it - 1;
    if (e < p.n_entities) {
        const uint32_t s = p.slot_of_entity[e];
        if (s == kNone || s >= p.n_slots) return 0u;
        const uint32_t f = p.flag_words[s];
        // in Bullet's world: a body of any type, not uploaded since the last physics tick (the ray queries' rule)
        if ((f & kTypeMask) == 0u || (f & kBDirty)) return 0u;
        d.o = ld3(p.pos, s);
        if (!in_region(p, d.o)) return 0u;
        d.capsule = (p.cinfo[s] & kCiCapsule) != 0u;
        if constexpr (FULL) {
            d.q = ld4(p.quat, s);
            const float4 cs = p.cshape[s];
            d.dims = F3{cs.x, cs.y, cs.z};
            // isStaticObject(): a Kinematic body loses CF_STATIC_OBJECT in EnsureRigidBody (PhysicsSystem.cpp:443-465)
            d.colour = (f & kTypeMask) == 1u ? kColStatic : kColDynamic;
        }
        return d.capsule ? kDebugCapsuleLines : kDebugBoxLines;
    }
    const uint64_t g = e - p.n_entities;
    if (g >= p.n_ghosts) return 0u;
    const QueryGhost gh = p.ghosts[g];
    const float* pose = p.ghost_pose + 8ull * gh.trigger;
    d.o = F3{pose[0], pose[1], pose[2]};
    if (!in_region(p, d.o)) return 0u;
    d.capsule = gh.capsule != 0u;
    if constexpr (FULL) {
        d.q = Q4{pose[4], pose[5], pose[6], pose[7]};
        d.dims = F3{gh.dims[0], gh.dims[1], gh.dims[2]};
        d.colour = kColTrigger; // CF_NO_CONTACT_RESPONSE
    }
    return d.capsule ? kDebugCapsuleLines : kDebugBoxLines;
}

// exclusive sum over the 256 lanes of a workgroup (s_wave: 4 words); total = the workgroup's sum
__device__ __forceinline__ uint32_t block_exscan(uint32_t v, uint32_t* s_wave, uint32_t& total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t t = __shfl_up(inc, d, 64);
        if (lane >= d) inc += t;
    }
    if (lane == 63u) s_wave[wave] = inc;
    __syncthreads();
    uint32_t before = 0;
    total = 0;
#pragma unroll
    for (uint32_t w = 0; w < kThreads / 64u; ++w) {
        const uint32_t x = s_wave[w];
        if (w < wave) before += x;
        total += x;
    }
    __syncthreads();
    return before + inc - v;
}

__global__ void __launch_bounds__(kThreads) k_debug_count(DebugParams p)
{
    __shared__ uint32_t s_wave[kThreads / 64];
    const uint64_t it = blockIdx.x * static_cast<uint64_t>(kThreads) + threadIdx.x;
    Item d;
    const uint32_t c = it < debug_items(p.n_entities, p.n_ghosts) ? load_item<false>(p, it, d) : 0u;
    uint32_t total;
    (void)block_exscan(c, s_wave, total);
    if (threadIdx.x == 0) p.block_sum[blockIdx.x] = total;
}

__global__ void __launch_bounds__(1024) k_debug_scan(DebugParams p)
{
    __shared__ unsigned long long s[1024];
    const uint32_t tid = threadIdx.x;
    const uint32_t per = (p.n_blocks + 1023u) / 1024u;
    const uint64_t b0 = static_cast<uint64_t>(tid) * per;
    const uint64_t b1 = b0 + per < p.n_blocks ? b0 + per : p.n_blocks;
    unsigned long long sum = 0;
    for (uint64_t b = b0; b < b1; ++b) sum += p.block_sum[b];
    s[tid] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024u; d <<= 1) {
        const unsigned long long t = tid >= d ? s[tid - d] : 0ull;
        __syncthreads();
        s[tid] += t;
        __syncthreads();
    }
    unsigned long long run = s[tid] - sum;
    for (uint64_t b = b0; b < b1; ++b) {
        p.block_off[b] = run;
        run += p.block_sum[b];
    }
    if (tid == 1023u) *p.total = s[1023];
}

struct Line {
    F3 a, b;
};

__device__ __forceinline__ F3 add3(const F3& a, const F3& b) { return F3{a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ F3 sub3(const F3& a, const F3& b) { return F3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ F3 mul3(const F3& a, float s) { return F3{a.x * s, a.y * s, a.z * s}; }

// DrawStaticPlane (BulletDebugDrawer.cpp:149-188) for the plane ((0, 1, 0), 0) under the identity transform: btPlaneSpace1 gives
// u = (-1, 0, 0), v = (0, 0, 1); corners (u + v), (u - v), (-u - v), (-u + v) times 25
__device__ __forceinline__ F3 plane_corner(uint32_t c)
{
    return F3{c < 2u ? -25.0f : 25.0f, 0.0f, (c == 0u || c == 3u) ? 25.0f : -25.0f};
}
__device__ __forceinline__ F3 lerp3(const F3& a, const F3& b, float t)
{
    return F3{a.x + (b.x - a.x) * t, a.y + (b.y - a.y) * t, a.z + (b.z - a.z) * t};
}
__device__ __forceinline__ Line plane_line(uint32_t k)
{
    if (k < 4u) return Line{plane_corner(k), plane_corner((k + 1u) & 3u)};
    const uint32_t j = k - 4u;
    const float t = static_cast<float>(1u + (j >> 1)) / 5.0f; // btScalar(i) / btScalar(gridLines + 1)
    if ((j & 1u) == 0u) return Line{lerp3(plane_corner(0), plane_corner(3), t), lerp3(plane_corner(1), plane_corner(2), t)};
    return Line{lerp3(plane_corner(0), plane_corner(1), t), lerp3(plane_corner(3), plane_corner(2), t)};
}

// item i of the workgroup as staged in LDS (word w of item i at s_item[w * 256 + i])
struct Staged {
    const float* s;
    uint32_t i;
    __device__ __forceinline__ float w(uint32_t k) const { return s[k * kThreads + i]; }
    __device__ __forceinline__ F3 v(uint32_t k) const { return F3{w(k), w(k + 1), w(k + 2)}; }
};

// DrawBox (:190-220): corner c of +-half extents through the world transform (btTransform::operator(): row dots, then the origin)
__device__ __forceinline__ F3 box_corner(const Staged& it, uint32_t c)
{
    const F3 h = it.v(12);
    const uint32_t c4 = c & 3u;
    const float x = (c4 == 1u || c4 == 2u) ? h.x : -h.x, y = (c & 2u) ? h.y : -h.y, z = (c & 4u) ? h.z : -h.z;
    const F3 r0 = it.v(3), r1 = it.v(6), r2 = it.v(9), o = it.v(0);
    return F3{(r0.x * x + r0.y * y + r0.z * z) + o.x, (r1.x * x + r1.y * y + r1.z * z) + o.y, (r2.x * x + r2.y * y + r2.z * z) + o.z};
}
__device__ __forceinline__ Line box_line(const Staged& it, uint32_t k)
{
    // 0,1 1,2 2,3 3,0  4,5 5,6 6,7 7,4  0,4 1,5 2,6 3,7
    uint32_t a, b;
    if (k < 8u) {
        const uint32_t base = k & 4u;
        a = base + (k & 3u);
        b = base + ((k + 1u) & 3u);
    } else {
        a = k - 8u;
        b = a + 4u;
    }
    return Line{box_corner(it, a), box_corner(it, b)};
}

// DrawCapsule (:222-285), up axis Y.  The staged axes are the NORMALISED columns: "axisX" = column 2, "axisY" = column 1,
// "axisZ" = column 0 (getColumn((upAxis + 1) % 3), getColumn(upAxis), getColumn((upAxis + 2) % 3)).
__device__ __forceinline__ Line capsule_line(const Staged& it, uint32_t k)
{
    const F3 center = it.v(0), ax = it.v(3), ay = it.v(6), az = it.v(9);
    const float radius = it.w(12), hh = it.w(13);
    const F3 top = add3(center, mul3(ay, hh)), bottom = sub3(center, mul3(ay, hh));
    if (k < 72u) {
        const uint32_t i = k / 3u, which = k - 3u * i;
        const F3 dir0 = add3(mul3(ax, kRingCos[i]), mul3(az, kRingSin[i]));
        const F3 dir1 = add3(mul3(ax, kRingCos[i + 1u]), mul3(az, kRingSin[i + 1u]));
        const F3 top0 = add3(top, mul3(dir0, radius)), bottom0 = add3(bottom, mul3(dir0, radius));
        if (which == 0u) return Line{top0, add3(top, mul3(dir1, radius))};
        if (which == 1u) return Line{bottom0, add3(bottom, mul3(dir1, radius))};
        return Line{top0, bottom0};
    }
    const uint32_t j = k - 72u, i = j >> 2, which = j & 3u;
    const F3 side = which < 2u ? ax : az;
    const F3 offset0 = mul3(side, kHemiCos[i] * radius), offset1 = mul3(side, kHemiCos[i + 1u] * radius);
    const F3 up0 = mul3(ay, kHemiSin[i] * radius), up1 = mul3(ay, kHemiSin[i + 1u] * radius);
    if ((which & 1u) == 0u) return Line{add3(add3(top, offset0), up0), add3(add3(top, offset1), up1)};
    return Line{sub3(sub3(bottom, offset0), up0), sub3(sub3(bottom, offset1), up1)};
}

__device__ __forceinline__ F3 normalized(const F3& v)
{
    const float inv = 1.0f / __builtin_sqrtf(v.x * v.x + v.y * v.y + v.z * v.z); // btVector3::normalize: *this /= length()
    return mul3(v, inv);
}

__global__ void __launch_bounds__(kThreads) k_debug_emit(DebugParams p)
{
    __shared__ float s_item[kItemWords * kThreads];
    __shared__ uint32_t s_off[kThreads + 1];
    __shared__ uint32_t s_wave[kThreads / 64];
    const uint32_t tid = threadIdx.x;
    const uint64_t it = blockIdx.x * static_cast<uint64_t>(kThreads) + tid;
    Item d{};
    const uint32_t c = it < debug_items(p.n_entities, p.n_ghosts) ? load_item<true>(p, it, d) : 0u;
    if (c != 0u && it != 0u) {
        const M3 r = bt_mat_from_quat(d.q);
        float* w = s_item + tid;
        w[0 * kThreads] = d.o.x;
        w[1 * kThreads] = d.o.y;
        w[2 * kThreads] = d.o.z;
        if (d.capsule) {
            const F3 ax = normalized(F3{r.m[0][2], r.m[1][2], r.m[2][2]});
            const F3 ay = normalized(F3{r.m[0][1], r.m[1][1], r.m[2][1]});
            const F3 az = normalized(F3{r.m[0][0], r.m[1][0], r.m[2][0]});
            w[3 * kThreads] = ax.x, w[4 * kThreads] = ax.y, w[5 * kThreads] = ax.z;
            w[6 * kThreads] = ay.x, w[7 * kThreads] = ay.y, w[8 * kThreads] = ay.z;
            w[9 * kThreads] = az.x, w[10 * kThreads] = az.y, w[11 * kThreads] = az.z;
        } else {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
#pragma unroll
                for (int b = 0; b < 3; ++b) w[(3 + 3 * a + b) * kThreads] = r.m[a][b];
            }
        }
        w[12 * kThreads] = d.dims.x;
        w[13 * kThreads] = d.dims.y;
        w[14 * kThreads] = d.dims.z;
    }
    if (c != 0u) s_item[15 * kThreads + tid] = __uint_as_float(d.colour);
    uint32_t total;
    const uint32_t ex = block_exscan(c, s_wave, total);
    s_off[tid] = ex;
    if (tid == 0) s_off[kThreads] = total;
    __syncthreads();
    if (total == 0u) return;
    const uint64_t base = p.block_off[blockIdx.x]; // first line of this workgroup
    for (uint32_t l = tid; l < total; l += kThreads) {
        if (base + l >= p.cap) break; // (lines beyond cap are counted, not written)
        // the last item whose first line is <= l (items without lines share their successor's offset)
        uint32_t lo = 0, hi = kThreads - 1u;
        while (lo < hi) {
            const uint32_t mid = (lo + hi + 1u) >> 1;
            if (s_off[mid] <= l) lo = mid;
            else hi = mid - 1u;
        }
        const uint32_t k = l - s_off[lo];
        const uint32_t cnt = s_off[lo + 1u] - s_off[lo];
        const Staged st{s_item, lo};
        const bool plane = blockIdx.x == 0 && lo == 0u;
        const Line ln = plane ? plane_line(k) : (cnt == kDebugCapsuleLines ? capsule_line(st, k) : box_line(st, k));
        float* o = p.lines + (base + l) * 7ull;
        o[0] = ln.a.x, o[1] = ln.a.y, o[2] = ln.a.z;
        o[3] = ln.b.x, o[4] = ln.b.y, o[5] = ln.b.z;
        o[6] = st.w(15);
    }
}

// ---------------------------------------------------------------- contacts

// drawContactPoint (BulletDebugDrawer.cpp:44-58): from the point along the unit normal, 0.25 long; a degenerate normal is +y
__device__ __forceinline__ F3 contact_to(const F3& from, F3 n)
{
    if (n.x * n.x + n.y * n.y + n.z * n.z < 1.1920929e-07f) n = F3{0.0f, 1.0f, 0.0f}; // SIMD_EPSILON = FLT_EPSILON
    n = normalized(n);
    return add3(from, mul3(n, 0.25f));
}

struct CountPoints {
    uint32_t n = 0;
    __device__ __forceinline__ void operator()(const F3&, const F3&) { ++n; }
};
struct WritePoints {
    float* lines;
    uint64_t cap, at;
    __device__ __forceinline__ void operator()(const F3& from, const F3& normal)
    {
        if (at < cap) {
            const F3 to = contact_to(from, normal);
            float* o = lines + at * 7ull;
            o[0] = from.x, o[1] = from.y, o[2] = from.z;
            o[3] = to.x, o[4] = to.y, o[5] = to.z;
            o[6] = __uint_as_float(kColContact);
        }
        ++at;
    }
};

// the points of one 4-point manifold row (count, then 4 x 12 floats from word 4 on) whose body B is entity `b`
template <class F>
__device__ __forceinline__ void visit_manifold(const DebugParams& p, uint32_t b, uint32_t points, const uint32_t* row, F& f)
{
    if (b >= p.n_entities || points == 0u) return;
    const uint32_t sb = p.slot_of_entity[b];
    if (sb == kNone || sb >= p.n_slots) return;
    const F3 o = ld3(p.pos, sb);
    const M3 r = bt_mat_from_quat(ld4(p.quat, sb));
    const float* pts = reinterpret_cast<const float*>(row + 4);
    for (uint32_t j = 0; j < points && j < 4u; ++j) {
        const float* pt = pts + 12u * j;
        const float x = pt[3], y = pt[4], z = pt[5]; // localB
        const F3 from{(r.m[0][0] * x + r.m[0][1] * y + r.m[0][2] * z) + o.x, (r.m[1][0] * x + r.m[1][1] * y + r.m[1][2] * z) + o.y,
                      (r.m[2][0] * x + r.m[2][1] * y + r.m[2][2] * z) + o.z};
        if (in_region(p, from)) f(from, F3{pt[6], pt[7], pt[8]});
    }
}

// entity e's plane manifold and its manifolds with obstacle boxes
template <class F>
__device__ __forceinline__ void visit_body(const DebugParams& p, uint64_t e, F& f)
{
    if (e >= p.n_entities) return;
    const uint32_t s = p.slot_of_entity[e];
    if (s == kNone || s >= p.n_slots) return;
    const uint32_t ci = p.cinfo[s];
    if (p.manifold) {
        const uint32_t n = (ci >> kCiCountShift) & 7u;
        const float* m = p.manifold + 32ull * s;
        for (uint32_t j = 0; j < n && j < 4u; ++j) {
            const F3 from{m[8u * j + 4u], 0.0f, m[8u * j + 6u]}; // B is the plane, whose frame is the world's
            if (in_region(p, from)) f(from, F3{0.0f, 1.0f, 0.0f});
        }
    }
    if (p.bmanifold && (ci & kCiBoxes)) {
        for (uint32_t k = 0; k < kBoxManifolds; ++k) {
            const uint32_t* row = p.bmanifold + (static_cast<uint64_t>(s) * kBoxManifolds + k) * kBoxManifoldWords;
            if (row[0] != kBoxNone) visit_manifold(p, row[0], row[1], row, f);
        }
    }
}

// one 64-bit atomic per wave: every lane learns where its n records go (an index into the whole line list)
__device__ __forceinline__ uint64_t wave_append(unsigned long long* total, uint32_t n)
{
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t inc = n;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t t = __shfl_up(inc, d, 64);
        if (lane >= d) inc += t;
    }
    const uint32_t sum = __shfl(inc, 63, 64);
    if (sum == 0u) return 0;
    unsigned long long at = 0;
    if (lane == 63u) at = atomicAdd(total, static_cast<unsigned long long>(sum));
    at = __shfl(at, 63, 64);
    return at + inc - n;
}

__global__ void __launch_bounds__(256) k_debug_contacts_bodies(DebugParams p)
{
    const uint64_t e = blockIdx.x * 256ull + threadIdx.x;
    CountPoints cnt;
    visit_body(p, e, cnt);
    WritePoints wr{p.lines, p.cap, wave_append(p.total, cnt.n)};
    if (cnt.n) visit_body(p, e, wr);
}

__global__ void __launch_bounds__(256) k_debug_contacts_pairs(DebugParams p)
{
    const uint64_t k = blockIdx.x * 256ull + threadIdx.x;
    const bool live = k < p.n_pairs;
    const uint32_t* m = p.pair_man + (live ? k : 0ull) * kBoxManifoldWords;
    const uint32_t b = live ? static_cast<uint32_t>(p.pair_keys[k]) : 0u; // B = the higher entity of the pair
    const uint32_t points = live ? m[0] : 0u;
    CountPoints cnt;
    visit_manifold(p, b, points, m, cnt);
    WritePoints wr{p.lines, p.cap, wave_append(p.total, cnt.n)};
    if (cnt.n) visit_manifold(p, b, points, m, wr);
}

} // namespace

hipError_t launch_debug_lines(hipStream_t stream, const DebugParams& p)
{
    if (p.n_blocks) hipLaunchKernelGGL(k_debug_count, dim3(p.n_blocks), dim3(kThreads), 0, stream, p);
    hipLaunchKernelGGL(k_debug_scan, dim3(1), dim3(1024), 0, stream, p);
    if (p.n_blocks && p.cap) hipLaunchKernelGGL(k_debug_emit, dim3(p.n_blocks), dim3(kThreads), 0, stream, p);
    if (p.flags & BGE_DEBUG_CONTACTS) {
        if ((p.manifold || p.bmanifold) && p.n_entities) {
            hipLaunchKernelGGL(k_debug_contacts_bodies, dim3(static_cast<uint32_t>((p.n_entities + 255) / 256)), dim3(256), 0, stream, p);
        }
        if (p.n_pairs) hipLaunchKernelGGL(k_debug_contacts_pairs, dim3((p.n_pairs + 255u) / 256u), dim3(256), 0, stream, p);
    }
    return hipGetLastError();
}

} // namespace bge
