// ubench_world_rows.hip — what the store shape of the flat tick's world matrices costs on gfx950.
//
// The flat tick rewrites 64 B of world matrix per entity, of which rows 0..2 already hold exactly the bits it stores
// whenever the body neither re-posed nor spun.  Before the kernel learns to store row 3 alone,
// this program times the access shapes involved, over N slots of float[16], with plain and non-temporal stores:
//   a  full rows    64 B per slot, every store instruction 1 KiB contiguous (the tick's wave-local write-out)
//   b  row 3 only   16 B per slot at a 64-B stride, lane = slot
//   c  flat tick    read flags, pos, vel, euler, scale (SoA); write pos, vel and the full row (bx_mtx_srt, LDS write-out)
//   d  fast path    read flags, pos, vel; write pos, vel and row 3
//   b2 rows 2-3     32 B per slot at a 64-B stride (two 16-B stores per lane: whole 32-B sectors)
//   e  fast path, whole sectors: read flags, pos, vel and row 2; write pos, vel and rows 2-3
//   f  fast path, vel in per-wave component blocks (ld_vel / st_vel_changed): only vel.y changes, only vel.y is stored
//   g  as f with all three components stored (st_vel): the layout alone, without the skipped stores
//   h  as f without the per-lane flags load: one 16-B per-wave record through a wave-uniform address stands in for it
//   i  as h without the row-3 store: the translation row stays in the position array, no matrix line is dirtied
//   j  as i for n_ticks ticks in one launch: loads once, n_ticks updates in registers (each with the sleep-threshold ballot),
//      stores pos, vel.y and the per-wave word adv = serial + n_ticks - 1 ("memory holds the state after tick adv")
//   k  a follow-up launch of a group that (j) began: the wave loads its record and adv, finds adv >= serial and returns
//      sequences "(j), then T - 1 x (k)" for T in {2, 4, 8} are timed per launch (= per tick) between runs of T x (i)
//      solo sequences "(j) alone with n_ticks = T, once per T ticks" for T in {8, 16, 32, 64} (solo groups, DESIGN.md §4.1: no
//      follow-up launch at all), timed per TICK, alternated three times with "(j), then 7 x (k)" (UBENCH_SOLO_ONLY)
//   l  as j with the reduced loop of csrc/bge_fuse_math.hpp (fuse::fuse_ticks: x and z velocity a fixed point, the ballot decided
//      from v.y's first and last value), in two forms: (l) is the product's function (the compiler packs the adds and unrolls), (l1) keeps the v.y
//      add a single instruction.  "(l) alone with n_ticks = T, once per T ticks" against the same with (j) for T in {64, 256, 1024}, timed per
//      LAUNCH and per tick, alternated three times (UBENCH_LEAN_ONLY)
// Each kernel runs `reps` times back to back between two events after a warm-up; one JSON line per (kernel, store
// policy, size).  Built by tools/ubench_world_rows.sh; no part of the product library.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../banggameengine_amd/csrc/bge_device_math.hpp"
#include "../banggameengine_amd/csrc/bge_fuse_math.hpp"

using namespace bge::dev;

#define CK(x)                                                                                          \
    do {                                                                                               \
        hipError_t e_ = (x);                                                                           \
        if (e_ != hipSuccess) {                                                                        \
            std::fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_));     \
            std::exit(1);                                                                              \
        }                                                                                              \
    } while (0)

namespace {

constexpr uint32_t kBlock = 256;

template <bool NT> __device__ __forceinline__ void put4(float4* p, const float4& v)
{
    if (NT) {
        __builtin_nontemporal_store(v.x, &p->x);
        __builtin_nontemporal_store(v.y, &p->y);
        __builtin_nontemporal_store(v.z, &p->z);
        __builtin_nontemporal_store(v.w, &p->w);
    } else {
        *p = v;
    }
}

// (a) one float4 per lane, consecutive lanes consecutive float4s: 64 B per slot
template <bool NT> __global__ void __launch_bounds__(kBlock) k_full_rows(float4* __restrict__ world, uint32_t n_slots, float salt)
{
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(kBlock) + threadIdx.x;
    if (i >= 4ull * n_slots) return;
    put4<NT>(world + i, make_float4(salt, static_cast<float>(i & 1023u), 0.0f, 1.0f));
}

// (b) row 3 of slot = lane: 16 B at a 64-B stride
template <bool NT> __global__ void __launch_bounds__(kBlock) k_row3(float4* __restrict__ world, uint32_t n_slots, float salt)
{
    const uint32_t slot = blockIdx.x * kBlock + threadIdx.x;
    if (slot >= n_slots) return;
    put4<NT>(world + 4ull * slot + 3, make_float4(salt, static_cast<float>(slot & 1023u), 0.0f, 1.0f));
}

// (b2) rows 2 and 3 of slot = lane: the 32-B-aligned upper half of the matrix, whole 32-B sectors
template <bool NT> __global__ void __launch_bounds__(kBlock) k_rows23(float4* __restrict__ world, uint32_t n_slots, float salt)
{
    const uint32_t slot = blockIdx.x * kBlock + threadIdx.x;
    if (slot >= n_slots) return;
    put4<NT>(world + 4ull * slot + 2, make_float4(0.0f, 0.0f, salt, 0.0f));
    put4<NT>(world + 4ull * slot + 3, make_float4(salt, static_cast<float>(slot & 1023u), 0.0f, 1.0f));
}

struct Soa {
    uint32_t* flags;
    float *pos, *vel, *euler, *scale;
    float4* world;
};

// (c) the flat tick's traffic and transform work: integrate, bx_mtx_srt, wave-local LDS write-out of 1 KiB per instruction
template <bool NT> __global__ void __launch_bounds__(kBlock, 8) k_flat_full(Soa s, uint32_t n_slots, float dt)
{
    __shared__ float4 lds[kBlock * 4];
    const uint32_t tid = threadIdx.x;
    const uint32_t slot = blockIdx.x * kBlock + tid; // n_slots is a multiple of kBlock
    const uint32_t f = s.flags[slot];
    F3 pos = ld3(s.pos, slot), vel = ld3(s.vel, slot);
    const F3 eul = ld3(s.euler, slot), scl = ld3(s.scale, slot);
    const bool valid = (f & 1u) != 0;
    if (valid) {
        vel.y = vel.y + -9.81f * dt;
        pos.x = pos.x + vel.x * dt;
        pos.y = pos.y + vel.y * dt;
        pos.z = pos.z + vel.z * dt;
        st3(s.vel, slot, vel);
        st3(s.pos, slot, pos);
    }
    float m[16];
    bx_mtx_srt(m, scl, eul, pos);
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) lds[tid * 4u + (r ^ ((tid >> 2) & 3u))] = make_float4(m[4 * r], m[4 * r + 1], m[4 * r + 2], m[4 * r + 3]);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const unsigned long long valid_mask = __ballot(valid);
    const uint32_t lane = tid & 63u, wbase = tid & ~63u;
    float4* dst = s.world + 4ull * kBlock * blockIdx.x;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t qi = lane + 64u * k, nl = qi >> 2, n = wbase + nl;
        const uint32_t r = (qi & 3u) ^ ((n >> 2) & 3u);
        if ((valid_mask >> nl) & 1ull) put4<NT>(&dst[n * 4u + r], lds[wbase * 4u + qi]);
    }
}

// (d) the proposed fast path: rows 0..2 are current, only the translation row is stored
template <bool NT> __global__ void __launch_bounds__(kBlock, 8) k_flat_row3(Soa s, uint32_t n_slots, float dt)
{
    const uint32_t slot = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t f = s.flags[slot];
    F3 pos = ld3(s.pos, slot), vel = ld3(s.vel, slot);
    if (f & 1u) {
        vel.y = vel.y + -9.81f * dt;
        pos.x = pos.x + vel.x * dt;
        pos.y = pos.y + vel.y * dt;
        pos.z = pos.z + vel.z * dt;
        st3(s.vel, slot, vel);
        st3(s.pos, slot, pos);
        put4<NT>(s.world + 4ull * slot + 3, make_float4(pos.x, pos.y, pos.z, 1.0f));
    }
}

// (e) as (d), but row 2 is read back and stored again with row 3, so that every written 32-B sector is written whole
template <bool NT> __global__ void __launch_bounds__(kBlock, 8) k_flat_rows23(Soa s, uint32_t n_slots, float dt)
{
    const uint32_t slot = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t f = s.flags[slot];
    F3 pos = ld3(s.pos, slot), vel = ld3(s.vel, slot);
    const float4 row2 = s.world[4ull * slot + 2];
    if (f & 1u) {
        vel.y = vel.y + -9.81f * dt;
        pos.x = pos.x + vel.x * dt;
        pos.y = pos.y + vel.y * dt;
        pos.z = pos.z + vel.z * dt;
        st3(s.vel, slot, vel);
        st3(s.pos, slot, pos);
        put4<NT>(s.world + 4ull * slot + 2, row2);
        put4<NT>(s.world + 4ull * slot + 3, make_float4(pos.x, pos.y, pos.z, 1.0f));
    }
}

// (f) as (d) with vel in per-wave component blocks; a y-only gravity leaves x and z as loaded, so their lines stay clean
template <bool NT> __global__ void __launch_bounds__(kBlock, 8) k_flat_row3_vy(Soa s, uint32_t n_slots, float dt)
{
    const uint32_t slot = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t f = s.flags[slot];
    F3 pos = ld3(s.pos, slot), vel = ld_vel(s.vel, slot);
    if (f & 1u) {
        const F3 old = vel;
        vel.y = vel.y + -9.81f * dt;
        const bool cxz = vel_xz_changed(vel, old), cy = vel_y_changed(vel, old);
        pos.x = pos.x + vel.x * dt;
        pos.y = pos.y + vel.y * dt;
        pos.z = pos.z + vel.z * dt;
        st_vel_if(s.vel, slot, vel, cxz, cy);
        st3(s.pos, slot, pos);
        put4<NT>(s.world + 4ull * slot + 3, make_float4(pos.x, pos.y, pos.z, 1.0f));
    }
}

// (g) as (f), every component stored.  The x and z impulses are run-time zeros: a store of the very value just loaded is one
// the compiler may drop, and then (g) would be (f).
template <bool NT> __global__ void __launch_bounds__(kBlock, 8) k_flat_row3_vblk(Soa s, uint32_t n_slots, float dt, float gx, float gz)
{
    const uint32_t slot = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t f = s.flags[slot];
    F3 pos = ld3(s.pos, slot), vel = ld_vel(s.vel, slot);
    if (f & 1u) {
        vel.x = vel.x + gx * dt;
        vel.y = vel.y + -9.81f * dt;
        vel.z = vel.z + gz * dt;
        pos.x = pos.x + vel.x * dt;
        pos.y = pos.y + vel.y * dt;
        pos.z = pos.z + vel.z * dt;
        st_vel(s.vel, slot, vel);
        st3(s.pos, slot, pos);
        put4<NT>(s.world + 4ull * slot + 3, make_float4(pos.x, pos.y, pos.z, 1.0f));
    }
}

// (h) as (f), but no lane loads its flag word: the wave reads one 16-B record {rows epoch, -, flag word, flag epoch} through a
// wave-uniform address (one scalar load), proceeds when both epochs equal the launch's, and takes the flag word from the record
template <bool NT>
__global__ void __launch_bounds__(kBlock, 8) k_flat_row3_wave(Soa s, const uint4* __restrict__ words, uint32_t epoch, uint32_t n_slots, float dt)
{
    const uint32_t slot = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t wave = blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint4 w = words[wave];
    if (((w.x ^ epoch) | (w.w ^ epoch)) != 0u) return;
    const uint32_t f = w.z;
    F3 pos = ld3(s.pos, slot), vel = ld_vel(s.vel, slot);
    if (f & 1u) {
        const F3 old = vel;
        vel.y = vel.y + -9.81f * dt;
        const bool cxz = vel_xz_changed(vel, old), cy = vel_y_changed(vel, old);
        pos.x = pos.x + vel.x * dt;
        pos.y = pos.y + vel.y * dt;
        pos.z = pos.z + vel.z * dt;
        st_vel_if(s.vel, slot, vel, cxz, cy);
        st3(s.pos, slot, pos);
        put4<NT>(s.world + 4ull * slot + 3, make_float4(pos.x, pos.y, pos.z, 1.0f));
    }
}

// (i) as (h) with the translation row left where st3 has just put it: no store into the matrix array at all
__global__ void __launch_bounds__(kBlock, 8) k_flat_norow_wave(Soa s, const uint4* __restrict__ words, uint32_t epoch, uint32_t n_slots, float dt)
{
    const uint32_t slot = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t wave = blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint4 w = words[wave];
    if (((w.x ^ epoch) | (w.w ^ epoch)) != 0u) return;
    const uint32_t f = w.z;
    F3 pos = ld3(s.pos, slot), vel = ld_vel(s.vel, slot);
    if (f & 1u) {
        const F3 old = vel;
        vel.y = vel.y + -9.81f * dt;
        const bool cxz = vel_xz_changed(vel, old), cy = vel_y_changed(vel, old);
        pos.x = pos.x + vel.x * dt;
        pos.y = pos.y + vel.y * dt;
        pos.z = pos.z + vel.z * dt;
        st_vel_if(s.vel, slot, vel, cxz, cy);
        st3(s.pos, slot, pos);
    }
}

// (j) / (k) share one body, as the two kinds of launch share one kernel in the product: record, then adv against the launch's
// serial (wave-uniform, nothing stored), then n_ticks updates in registers.  A wave that fails a ballot has stored nothing; the
// product would go on into its single-tick path, here it returns (sleep_lin is a run-time 0: no lane ever fails).
__device__ __forceinline__ void fused_body(const Soa& s, const uint4* __restrict__ words, uint32_t* __restrict__ adv, uint32_t epoch, uint32_t serial,
                                           uint32_t n_ticks, float dt, float sleep_lin)
{
    const uint32_t slot = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t wave = blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint4 w = words[wave];
    if (adv[wave] >= serial) return;
    if (((w.x ^ epoch) | (w.w ^ epoch)) != 0u) return;
    if (!(w.z & 1u)) return;
    F3 pos = ld3(s.pos, slot);
    const F3 old = ld_vel(s.vel, slot);
    asm volatile("" : "+v"(pos.x), "+v"(pos.y), "+v"(pos.z));
    F3 vel = old;
    for (uint32_t t = 0; t < n_ticks; ++t) {
        vel.y = vel.y + -9.81f * dt;
        if (__ballot(!(fabsf(vel.y) >= sleep_lin)) != 0ull) return;
        pos.x = pos.x + vel.x * dt;
        pos.y = pos.y + vel.y * dt;
        pos.z = pos.z + vel.z * dt;
    }
    st_vel_if(s.vel, slot, vel, vel_xz_changed(vel, old), vel_y_changed(vel, old));
    st3(s.pos, slot, pos);
    if (n_ticks > 1u && (threadIdx.x & 63u) == 0u) adv[wave] = serial + n_ticks - 1u;
}
__global__ void __launch_bounds__(kBlock, 8)
k_flat_fused(Soa s, const uint4* __restrict__ words, uint32_t* __restrict__ adv, uint32_t epoch, uint32_t serial, uint32_t n_ticks, float dt, float sleep_lin)
{
    fused_body(s, words, adv, epoch, serial, n_ticks, dt, sleep_lin);
}
__global__ void __launch_bounds__(kBlock, 8)
k_flat_follow(Soa s, const uint4* __restrict__ words, uint32_t* __restrict__ adv, uint32_t epoch, uint32_t serial, uint32_t n_ticks, float dt, float sleep_lin)
{
    fused_body(s, words, adv, epoch, serial, n_ticks, dt, sleep_lin);
}

// (l) / (l1): (j)'s body around the reduced loop.  (l) is fuse::fuse_ticks itself, the product's function: the compiler packs the
// adds (v_pk_add_f32, v_mul_f32, v_pk_add_f32 per tick) and unrolls by four.  (l1) is the same loop written out with the v.y add
// behind an empty asm, which keeps it a single instruction (v_add_f32, v_mul_f32, v_add_f32 and one v_pk_add_f32 for x and z) and
// which the unroller does not duplicate.
struct UWave {
    static __device__ __forceinline__ bool any(bool m) { return __ballot(m) != 0ull; }
    static __device__ __forceinline__ float abs(float v) { return fabsf(v); }
    static __device__ __forceinline__ bool same_bits(float a, float b) { return __float_as_uint(a) == __float_as_uint(b); }
};
__device__ __forceinline__ bool lean_plain_add(const bge::fuse::Step& c, uint32_t n, F3& vn, F3& xn)
{
    if (n == 0u) return true;
    const F3 v1{vn.x + c.cx, vn.y + c.cy, vn.z + c.cz};
    if (UWave::any(!(fabsf(v1.y) >= c.sleep_lin))) return false;
    if (!UWave::any(!(UWave::same_bits(v1.x + c.cx, v1.x) && UWave::same_bits(v1.z + c.cz, v1.z)))) {
        const float dx = v1.x * c.dt, dz = v1.z * c.dt;
        float vy = v1.y;
        F3 x{xn.x + dx, xn.y + vy * c.dt, xn.z + dz};
        for (uint32_t i = 1; i < n; ++i) {
            vy = vy + c.cy;
            asm("" : "+v"(vy));
            x = F3{x.x + dx, x.y + vy * c.dt, x.z + dz};
        }
        const float s = c.sleep_lin;
        if (!UWave::any(!((v1.y >= s && vy >= s) || (v1.y <= -s && vy <= -s)))) {
            vn = F3{v1.x, vy, v1.z};
            xn = x;
            return true;
        }
    }
    return bge::fuse::fuse_ticks_exact<UWave>(c, n, vn, xn);
}
template <bool PLAIN_ADD>
__global__ void __launch_bounds__(kBlock, 8)
k_flat_lean(Soa s, const uint4* __restrict__ words, uint32_t* __restrict__ adv, uint32_t epoch, uint32_t serial, uint32_t n_ticks, float dt, float sleep_lin)
{
    const uint32_t slot = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t wave = blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint4 w = words[wave];
    if (adv[wave] >= serial) return;
    if (((w.x ^ epoch) | (w.w ^ epoch)) != 0u) return;
    if (!(w.z & 1u)) return;
    F3 pos = ld3(s.pos, slot);
    const F3 old = ld_vel(s.vel, slot);
    asm volatile("" : "+v"(pos.x), "+v"(pos.y), "+v"(pos.z));
    F3 vel = old;
    const bge::fuse::Step c{0.0f, -9.81f * dt, 0.0f, dt, sleep_lin};
    if (!(PLAIN_ADD ? lean_plain_add(c, n_ticks, vel, pos) : bge::fuse::fuse_ticks<UWave>(c, n_ticks, vel, pos))) return;
    st_vel_if(s.vel, slot, vel, vel_xz_changed(vel, old), vel_y_changed(vel, old));
    st3(s.pos, slot, pos);
    if (n_ticks > 1u && (threadIdx.x & 63u) == 0u) adv[wave] = serial + n_ticks - 1u;
}

constexpr uint32_t kEpoch = 7; // what words 0 and 3 of every record of (h) hold, and what its launches pass

template <typename F> float time_us(F launch, int warm, int reps)
{
    hipEvent_t a, b;
    CK(hipEventCreate(&a));
    CK(hipEventCreate(&b));
    for (int i = 0; i < warm; ++i) launch();
    CK(hipDeviceSynchronize());
    CK(hipEventRecord(a, nullptr));
    for (int i = 0; i < reps; ++i) launch();
    CK(hipEventRecord(b, nullptr));
    CK(hipEventSynchronize(b));
    float ms = 0.0f;
    CK(hipEventElapsedTime(&ms, a, b));
    CK(hipEventDestroy(a));
    CK(hipEventDestroy(b));
    return 1e3f * ms / static_cast<float>(reps);
}

void report(const char* kernel, bool nt, uint32_t n, float us, double bytes_per_slot)
{
    const double gbs = bytes_per_slot * n / (us * 1e-6) / 1e9;
    std::printf("{\"kernel\": \"%s\", \"nt\": %d, \"slots\": %u, \"us\": %.3f, \"bytes_per_slot\": %.0f, \"GB_s\": %.1f}\n", kernel, nt ? 1 : 0,
                n, us, bytes_per_slot, gbs);
    std::fflush(stdout);
}


// "(j), then T - 1 x (k)": launch i of a group carries serial s + i and n_left = T - i, as the product's launches would
struct FusedSeq {
    Soa s;
    const uint4* words;
    uint32_t* adv;
    uint32_t n, T, serial = 1, at = 0;
    float sleep_lin;
    void operator()()
    {
        const dim3 g(n / kBlock), blk(kBlock);
        if (at == 0)
            k_flat_fused<<<g, blk>>>(s, words, adv, kEpoch, serial, T, 1.0f / 60.0f, sleep_lin);
        else
            k_flat_follow<<<g, blk>>>(s, words, adv, kEpoch, serial, T - at, 1.0f / 60.0f, sleep_lin);
        ++serial;
        at = (at + 1u) % T;
    }
};

// (i), T = 2, 4, 8, three times over, and a fourth (i): the spread of the (i) lines is the yardstick.  Warm-up and reps are whole
// groups (multiples of 8); the serials go on rising from run to run, adv is never reset.
void run_fused(uint32_t n, int reps, Soa s, const uint4* words, uint32_t* adv, float sleep_lin)
{
    const int warm = 24;
    reps = (reps + 7) / 8 * 8;
    const dim3 blk(kBlock), g_slot(n / kBlock);
    uint32_t serial = 1;
    for (int round = 0; round < 4; ++round) {
        report("i_flat_norow_wave", false, n, time_us([&] { k_flat_norow_wave<<<g_slot, blk>>>(s, words, kEpoch, n, 1.0f / 60.0f); }, warm, reps), 40.25);
        if (round == 3) break;
        for (uint32_t T : {2u, 4u, 8u}) {
            FusedSeq seq{s, words, adv, n, T, serial, 0u, sleep_lin};
            char name[32];
            std::snprintf(name, sizeof name, "jk_fused_T%u", T);
            report(name, false, n, time_us([&] { seq(); }, warm, reps), 40.3125 / T);
            serial = seq.serial;
        }
    }
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
}

// Solo groups: "(j) alone with n_ticks = T, once per T ticks" against round 9's "(j), then 7 x (k)", three times over and a fourth
// round-9 run: the spread of the four jk_fused_T8 lines is the yardstick.  One launch of a solo sequence stands for T ticks, so its
// line is the time per launch divided by T; `reps` launches of either kind are timed (whole groups of 8 for the round-9 sequence).
void run_solo(uint32_t n, int reps, Soa s, const uint4* words, uint32_t* adv, float sleep_lin)
{
    const int warm = 24;
    reps = (reps + 7) / 8 * 8;
    const dim3 blk(kBlock), g_slot(n / kBlock);
    uint32_t serial = 1;
    for (int round = 0; round < 4; ++round) {
        {
            FusedSeq seq{s, words, adv, n, 8u, serial, 0u, sleep_lin};
            report("jk_fused_T8", false, n, time_us([&] { seq(); }, warm, reps), 40.3125 / 8);
            serial = seq.serial;
        }
        if (round == 3) break;
        for (uint32_t T : {8u, 16u, 32u, 64u}) {
            char name[32];
            std::snprintf(name, sizeof name, "j_solo_T%u", T);
            const float us = time_us([&] {
                k_flat_fused<<<g_slot, blk>>>(s, words, adv, kEpoch, serial, T, 1.0f / 60.0f, sleep_lin);
                serial += T;
            }, warm, reps);
            report(name, false, n, us / static_cast<float>(T), 40.3125 / T);
        }
    }
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
}

// The reduced loop: (j), (l), (l1), each "alone with n_ticks = T, once per T ticks", for T = 64, 256, 1024, three times over.  One line
// per run: us per LAUNCH, and the same per tick.  The spread of the three (j) lines of a T is the yardstick for that T.
void run_lean(uint32_t n, int reps, Soa s, const uint4* words, uint32_t* adv, float sleep_lin)
{
    const int warm = 24;
    const dim3 blk(kBlock), g_slot(n / kBlock);
    uint32_t serial = 1;
    auto line = [&](const char* kernel, uint32_t T, float us) {
        std::printf("{\"kernel\": \"%s\", \"T\": %u, \"slots\": %u, \"us_per_launch\": %.3f, \"us_per_tick\": %.4f}\n", kernel, T, n, us, us / static_cast<float>(T));
        std::fflush(stdout);
    };
    for (int round = 0; round < 3; ++round) {
        for (uint32_t T : {64u, 256u, 1024u}) {
            line("j_solo", T, time_us([&] {
                     k_flat_fused<<<g_slot, blk>>>(s, words, adv, kEpoch, serial, T, 1.0f / 60.0f, sleep_lin);
                     serial += T;
                 }, warm, reps));
            line("l_lean", T, time_us([&] {
                     k_flat_lean<false><<<g_slot, blk>>>(s, words, adv, kEpoch, serial, T, 1.0f / 60.0f, sleep_lin);
                     serial += T;
                 }, warm, reps));
            line("l1_lean_plain_add", T, time_us([&] {
                     k_flat_lean<true><<<g_slot, blk>>>(s, words, adv, kEpoch, serial, T, 1.0f / 60.0f, sleep_lin);
                     serial += T;
                 }, warm, reps));
        }
    }
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
}

template <bool NT> void run_size(uint32_t n, int reps, Soa s, const uint4* words, float zero)
{
    const int warm = 20;
    const dim3 blk(kBlock);
    const dim3 g_full((4ull * n + kBlock - 1) / kBlock), g_slot((n + kBlock - 1) / kBlock);
    report("a_full_rows", NT, n, time_us([&] { k_full_rows<NT><<<g_full, blk>>>(s.world, n, 1.0f); }, warm, reps), 64.0);
    report("b_row3", NT, n, time_us([&] { k_row3<NT><<<g_slot, blk>>>(s.world, n, 2.0f); }, warm, reps), 16.0);
    report("b2_rows23", NT, n, time_us([&] { k_rows23<NT><<<g_slot, blk>>>(s.world, n, 3.0f); }, warm, reps), 32.0);
    report("c_flat_full", NT, n, time_us([&] { k_flat_full<NT><<<g_slot, blk>>>(s, n, 1.0f / 60.0f); }, warm, reps), 140.0);
    report("d_flat_row3", NT, n, time_us([&] { k_flat_row3<NT><<<g_slot, blk>>>(s, n, 1.0f / 60.0f); }, warm, reps), 68.0);
    report("e_flat_rows23", NT, n, time_us([&] { k_flat_rows23<NT><<<g_slot, blk>>>(s, n, 1.0f / 60.0f); }, warm, reps), 100.0);
    // (d) again on either side of (f) and (g): the spread of the three (d) lines is the yardstick for the other two
    report("f_flat_row3_vy", NT, n, time_us([&] { k_flat_row3_vy<NT><<<g_slot, blk>>>(s, n, 1.0f / 60.0f); }, warm, reps), 60.0);
    report("d_flat_row3", NT, n, time_us([&] { k_flat_row3<NT><<<g_slot, blk>>>(s, n, 1.0f / 60.0f); }, warm, reps), 68.0);
    report("g_flat_row3_vblk", NT, n, time_us([&] { k_flat_row3_vblk<NT><<<g_slot, blk>>>(s, n, 1.0f / 60.0f, zero, zero); }, warm, reps), 68.0);
    report("d_flat_row3", NT, n, time_us([&] { k_flat_row3<NT><<<g_slot, blk>>>(s, n, 1.0f / 60.0f); }, warm, reps), 68.0);
    report("f_flat_row3_vy", NT, n, time_us([&] { k_flat_row3_vy<NT><<<g_slot, blk>>>(s, n, 1.0f / 60.0f); }, warm, reps), 60.0);
    // (h) between (f)s, the same way: with the (f) line above, three (f) lines around two (h) lines
    report("h_flat_row3_wave", NT, n, time_us([&] { k_flat_row3_wave<NT><<<g_slot, blk>>>(s, words, kEpoch, n, 1.0f / 60.0f); }, warm, reps), 56.25);
    report("f_flat_row3_vy", NT, n, time_us([&] { k_flat_row3_vy<NT><<<g_slot, blk>>>(s, n, 1.0f / 60.0f); }, warm, reps), 60.0);
    report("h_flat_row3_wave", NT, n, time_us([&] { k_flat_row3_wave<NT><<<g_slot, blk>>>(s, words, kEpoch, n, 1.0f / 60.0f); }, warm, reps), 56.25);
    report("f_flat_row3_vy", NT, n, time_us([&] { k_flat_row3_vy<NT><<<g_slot, blk>>>(s, n, 1.0f / 60.0f); }, warm, reps), 60.0);
    // (i) between (h)s: (h), (i), (h), (i), (h).  (i) stores nothing into the matrices, so it has no non-temporal form: plain pass only
    if (!NT) {
        report("h_flat_row3_wave", NT, n, time_us([&] { k_flat_row3_wave<NT><<<g_slot, blk>>>(s, words, kEpoch, n, 1.0f / 60.0f); }, warm, reps), 56.25);
        report("i_flat_norow_wave", NT, n, time_us([&] { k_flat_norow_wave<<<g_slot, blk>>>(s, words, kEpoch, n, 1.0f / 60.0f); }, warm, reps), 40.25);
        report("h_flat_row3_wave", NT, n, time_us([&] { k_flat_row3_wave<NT><<<g_slot, blk>>>(s, words, kEpoch, n, 1.0f / 60.0f); }, warm, reps), 56.25);
        report("i_flat_norow_wave", NT, n, time_us([&] { k_flat_norow_wave<<<g_slot, blk>>>(s, words, kEpoch, n, 1.0f / 60.0f); }, warm, reps), 40.25);
        report("h_flat_row3_wave", NT, n, time_us([&] { k_flat_row3_wave<NT><<<g_slot, blk>>>(s, words, kEpoch, n, 1.0f / 60.0f); }, warm, reps), 56.25);
    }
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
}

} // namespace

// usage: ubench_world_rows [slots ...]   (default 1048576 16777216; rounded up to whole 256-slot blocks)
//        env UBENCH_REPS: timed launches per kernel (default 200); UBENCH_GXZ: x and z gravity of kernel (g) (default 0);
//        UBENCH_FUSED_ONLY: time (i), (j), (k) alone; UBENCH_SOLO_ONLY: the solo sequences against "(j), then 7 x (k)" alone; UBENCH_SLEEP_LIN: the sleep threshold of (j) (default 0: every ballot passes);
//        UBENCH_LEAN_ONLY: (j) against (l) and (l1) alone
int main(int argc, char** argv)
{
    std::vector<uint32_t> sizes;
    for (int i = 1; i < argc; ++i) sizes.push_back(static_cast<uint32_t>(std::strtoul(argv[i], nullptr, 10)));
    if (sizes.empty()) sizes = {1u << 20, 1u << 24};
    const float zero = std::getenv("UBENCH_GXZ") ? static_cast<float>(std::atof(std::getenv("UBENCH_GXZ"))) : 0.0f; // (g)'s x / z gravity
    const bool fused_only = std::getenv("UBENCH_FUSED_ONLY") != nullptr; // kernels (i), (j), (k) alone
    const int reps = std::getenv("UBENCH_REPS") ? std::atoi(std::getenv("UBENCH_REPS")) : 200;
    for (uint32_t n0 : sizes) {
        const uint32_t n = (n0 + kBlock - 1) / kBlock * kBlock;
        Soa s{};
        CK(hipMalloc(&s.flags, 4ull * n));
        CK(hipMalloc(&s.pos, 12ull * n));
        CK(hipMalloc(&s.vel, 12ull * n));
        CK(hipMalloc(&s.euler, 12ull * n));
        CK(hipMalloc(&s.scale, 12ull * n));
        CK(hipMalloc(&s.world, 64ull * n));
        std::vector<uint32_t> fl(n, 1u);
        std::vector<float> v3(3ull * n);
        CK(hipMemcpy(s.flags, fl.data(), 4ull * n, hipMemcpyHostToDevice));
        for (size_t i = 0; i < v3.size(); ++i) v3[i] = 0.001f * static_cast<float>(i % 997);
        CK(hipMemcpy(s.pos, v3.data(), 12ull * n, hipMemcpyHostToDevice));
        CK(hipMemcpy(s.euler, v3.data(), 12ull * n, hipMemcpyHostToDevice));
        for (size_t i = 0; i < v3.size(); ++i) v3[i] = 1.0f + 0.0001f * static_cast<float>(i % 101);
        CK(hipMemcpy(s.scale, v3.data(), 12ull * n, hipMemcpyHostToDevice));
        CK(hipMemset(s.vel, 0, 12ull * n));
        CK(hipMemset(s.world, 0, 64ull * n));
        uint4* words = nullptr; // one record per wave of 64 slots
        std::vector<uint4> wr(n / 64u, uint4{kEpoch, 0u, 1u, kEpoch});
        CK(hipMalloc(&words, 16ull * wr.size()));
        CK(hipMemcpy(words, wr.data(), 16ull * wr.size(), hipMemcpyHostToDevice));
        uint32_t* adv = nullptr; // (j) / (k): one word per wave
        CK(hipMalloc(&adv, 4ull * wr.size()));
        CK(hipMemset(adv, 0, 4ull * wr.size()));
        const float sleep_lin = std::getenv("UBENCH_SLEEP_LIN") ? static_cast<float>(std::atof(std::getenv("UBENCH_SLEEP_LIN"))) : 0.0f;
        if (std::getenv("UBENCH_LEAN_ONLY")) {
            run_lean(n, reps, s, words, adv, sleep_lin);
        } else if (std::getenv("UBENCH_SOLO_ONLY")) {
            run_solo(n, reps, s, words, adv, sleep_lin);
        } else {
            if (!fused_only) {
                run_size<false>(n, reps, s, words, zero);
                run_size<true>(n, reps, s, words, zero);
            }
            run_fused(n, reps, s, words, adv, sleep_lin);
        }
        CK(hipFree(adv));
        CK(hipFree(words));
        CK(hipFree(s.flags));
        CK(hipFree(s.pos));
        CK(hipFree(s.vel));
        CK(hipFree(s.euler));
        CK(hipFree(s.scale));
        CK(hipFree(s.world));
    }
    return 0;
}
