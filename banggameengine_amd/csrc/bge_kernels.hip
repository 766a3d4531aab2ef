// bge_kernels.hip — hand-written gfx950 kernels of the world tick.
//
// k_tick<PHYS, XFORM, AABB, NORMAL, BASIS>: one workgroup (4 wave64) per 256-slot tile.
//   PHYS   rigid-body slice of PhysicsSystem::Update for free bodies
//          (src/physics/PhysicsSystem.cpp:952-989 re-pose rule, :863 one Bullet sub-step,
//           :916-950 write-back + mark dirty)
//   XFORM  TransformSystem::Update (src/ecs/TransformSystem.cpp:10-46): local = mtxSRT, then
//          world = parentWorld * local level by level inside the tile, the parents' world matrices
//          staged in LDS (16 KiB per workgroup).  Wave-local tiles (every subtree inside one 64-slot
//          group) run without any workgroup barrier; block tiles use one barrier per level
//   AABB   the per-body AABB Bullet feeds its broadphase (current pose U predicted pose, +0.02)
//   NORMAL the render feed's per-entity normal matrix transpose(inverse(world)) (src/render/Renderer.cpp:633-636)
//   BASIS  Bullet's own orientation bookkeeping for every Dynamic body (BGE_TICK_BULLET_BASIS): basis -> getRotation ->
//          integrateTransform -> setRotation each step, rotationEuler rewritten from it; without it a body with zero angular
//          velocity keeps its orientation and euler triple
//
// Memory plan (all streams indexed by slot, 256 consecutive slots per workgroup):
//   reads   flags 4 B (body type, dirty bits, level, in-tile parent index, mass class), pos/euler/scale 12 B
//           each, vel 12 B (Dynamic bodies only); parent slot 4 B only for nodes whose parent is in an earlier pass
//   writes  pos 12 B (Dynamic only), world 64 B; flags only when a bit changed; of vel only the components whose bits the
//           tick changed: 4 B (y) per body falling under a y-only gravity, 12 B under a gravity with x and z components
//   vel is stored in per-wave component blocks (bge_device_math.hpp: per 64 slots float2 xz[64], float y[64]), so that the y
//   store of a wave is 256 contiguous bytes and the xz lines stay clean; pos, euler, scale are rows of three floats.
//   Waves whose rotation rows are current (WorldView::rs_word) read neither euler nor scale and write only world row 3:
//   60 B per flat body instead of 132 B.
//   Of those, waves whose 64 flag words are vouched for (WorldView::rs_word words 2 and 3: one clean value, nothing has stored to
//   flags since) do not read flags either: the wave's 16-B record and one palette entry through wave-uniform addresses stand in
//   for 64 x 4 B, 56 B per flat body.  k_tick<PHYS, XFORM> only; BGE_FLAG_WORD=0 turns it off.
//   With TickParams::defer_row3 the translation-row waves do not store row 3 either — it is (pos, 1) of the position they store;
//   readers compose it, k_row3_sync stores it before anything else may write pos or world: 40 B per flat body.
//   With TickParams::serial (fused ticks) a vouched wave runs the n_left ticks that remain of its group of launches
//   in registers, stores once and says so in WorldView::adv; the group's later launches return at once for it.  k_tick<PHYS, XFORM>
//   only; BGE_FUSE_TICKS=1 turns it off.
//   With TickParams::n_solo (solo groups) ONE launch of the SOLO instantiation stands for a whole group of ticks of a
//   scene whose every tile is flat: a vouched wave as above, every other wave tick after tick by the ordinary path inside the
//   launch.  BGE_SOLO_GROUPS=0 turns it off.
//   Waves whose bodies are all asleep (rest word, WorldView::rs_word word 1) read flags, the deactivation record and the contact
//   word, 8..12 B per body, and store nothing.
//   The world matrices leave through LDS so that every wave-level store instruction writes 1 KiB of
//   contiguous memory (16 B per lane), whatever the per-node compute layout was.
//   The kernel is HBM-bound (~250 flop against >= 113 B per entity): no MFMA.
#include <hip/hip_runtime.h>

#include "bge_device_math.hpp"
#include "bge_flatten.hpp"
#include "bge_fuse_math.hpp"
#include "bge_kernels.hpp"
#include "bge_tick_plan.hpp"

namespace bge {

using namespace dev;

namespace {

// LDS image of the tile's world matrices: node n, row r lives at float4 index n*4 + (r ^ ((n>>2)&3)).
// The XOR spreads the four 64-B rows of consecutive nodes over all 64 banks for ds_read_b128
// (lanes n, n+4, n+8, n+12 of a 16-lane group would otherwise share a bank).
__device__ __forceinline__ uint32_t lds_row(uint32_t n, uint32_t r) { return n * 4u + (r ^ ((n >> 2) & 3u)); }

__device__ __forceinline__ void lds_put(float4* lds, uint32_t n, const float (&m)[16])
{
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) lds[lds_row(n, r)] = make_float4(m[4 * r], m[4 * r + 1], m[4 * r + 2], m[4 * r + 3]);
}

__device__ __forceinline__ void lds_get(const float4* lds, uint32_t n, float (&m)[16])
{
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) {
        const float4 v = lds[lds_row(n, r)];
        m[4 * r] = v.x;
        m[4 * r + 1] = v.y;
        m[4 * r + 2] = v.z;
        m[4 * r + 3] = v.w;
    }
}

// world = parent * local, a row at a time: the parent's row comes from the LDS image (or from memory, for a parent resolved by
// an earlier launch), the product's row goes straight into this node's place in the image.  (bx_mtx_mul on whole matrices held
// 48 registers here — parent, local, product — and with them the kernel's register allocation.)
__device__ __forceinline__ void lds_mul_put(float4* lds, uint32_t parent, uint32_t self, const float (&local)[16])
{
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) lds[lds_row(self, r)] = bx_mtx_mul_row(lds[lds_row(parent, r)], local);
}
__device__ __forceinline__ void world_mul_put(float4* lds, const float* __restrict__ world, uint32_t parent_slot, uint32_t self, const float (&local)[16])
{
    const float4* src = reinterpret_cast<const float4*>(world) + 4ull * parent_slot;
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) lds[lds_row(self, r)] = bx_mtx_mul_row(src[r], local);
}

// Root table for the per-frame all-gather, filled by the roots themselves (consecutive roots of a tile are
// consecutive lanes, so the 64-byte rows of a wave form one contiguous run).
__device__ __forceinline__ void store_root(float* __restrict__ root_out, uint32_t index, const float (&m)[16])
{
    // compact row, 48 bytes: a root's world matrix is its local matrix (Transform.cpp:32-35), whose fourth column is
    // exactly (0, 0, 0, 1) (bx::mtxSRT) — the gather moves the 12 floats that carry information
    float4* dst = reinterpret_cast<float4*>(root_out) + 3ull * index;
    dst[0] = make_float4(m[0], m[1], m[2], m[4]);
    dst[1] = make_float4(m[5], m[6], m[8], m[9]);
    dst[2] = make_float4(m[10], m[12], m[13], m[14]);
}

// A frozen root (WorldView::frozen): its stored world matrix goes where the freshly built local matrix would have gone — a
// row at a time, so that the rare path costs the kernel no registers.
__device__ __forceinline__ void lds_put_stored(float4* lds, uint32_t n, const float* __restrict__ world, uint32_t slot)
{
    const float4* src = reinterpret_cast<const float4*>(world) + 4ull * slot;
#pragma unroll 1
    for (uint32_t r = 0; r < 4; ++r) lds[lds_row(n, r)] = src[r];
}
__device__ __forceinline__ void store_root_stored(float* __restrict__ root_out, uint32_t index, const float* __restrict__ world, uint32_t slot)
{
    const float* m = world + 16ull * slot;
    float* dst = root_out + 12ull * index; // the packing of store_root
    const int pick[12] = {0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13, 14};
#pragma unroll 1
    for (int k = 0; k < 12; ++k) dst[k] = m[pick[k]];
}

// Stores of results the tick never reads again (world / normal matrices).  Non-temporal when the host asks for it:
// measured on MI355X, plain stores win while the tick's working set fits the 256 MiB Infinity Cache (1 M entities:
// 22.6 us plain, 24.5 us nt) and nt stores win beyond it (4 M: 95.0 us plain, 89.5 us nt) — the 64 B/entity output
// stream then no longer evicts lines the next tick re-reads.
__device__ __forceinline__ void store_out(float4* p, const float4& v, bool nt)
{
    if (nt) {
        __builtin_nontemporal_store(v.x, &p->x);
        __builtin_nontemporal_store(v.y, &p->y);
        __builtin_nontemporal_store(v.z, &p->z);
        __builtin_nontemporal_store(v.w, &p->w);
    } else {
        *p = v;
    }
}

// LDS hand-over between lanes of ONE wave: the hardware keeps a wave's DS operations in order; the fences
// keep the compiler from moving them across this point.
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Wave64 reductions with DPP (one VALU instruction per step, no LDS): after the six steps lane 63 holds the result.
// row_shr 1/2/4/8 make an inclusive scan inside each row of 16 lanes (min / max are idempotent, so overlapping windows are
// fine); row_bcast:15 carries each row's last lane into the next row (rows 1 and 3), row_bcast:31 lane 31 into rows 2 and 3.
// Lanes that must not contribute pass the identity.  Call with all 64 lanes active.
template <bool IS_MIN> __device__ __forceinline__ float wave_reduce_to_lane63(float v)
{
    const int ident = __float_as_int(IS_MIN ? INFINITY : -INFINITY);
#define BGE_DPP_STEP(ctrl, rmask)                                                                                      \
    {                                                                                                                 \
        const float o = __int_as_float(__builtin_amdgcn_update_dpp(ident, __float_as_int(v), ctrl, rmask, 0xf, false)); \
        v = IS_MIN ? fminf(v, o) : fmaxf(v, o);                                                                        \
    }
    BGE_DPP_STEP(0x111, 0xf) // row_shr:1
    BGE_DPP_STEP(0x112, 0xf) // row_shr:2
    BGE_DPP_STEP(0x114, 0xf) // row_shr:4
    BGE_DPP_STEP(0x118, 0xf) // row_shr:8
    BGE_DPP_STEP(0x142, 0xa) // row_bcast:15 -> rows 1, 3
    BGE_DPP_STEP(0x143, 0xc) // row_bcast:31 -> rows 2, 3
#undef BGE_DPP_STEP
    return v;
}

#ifndef BGE_AABB_MIN_WAVES
#define BGE_AABB_MIN_WAVES 4 /* waves per SIMD the AABB variant is compiled for: at 8 it spills 20 VGPRs (measured ~2 % slower at 4 M bodies) */
#endif
#ifndef BGE_BASIS_MIN_WAVES
#define BGE_BASIS_MIN_WAVES 8 /* the BGE_TICK_BULLET_BASIS variants without AABBs / normal matrices: 55 VGPRs since parent * local is formed a row at a time (80 before, 6 waves per SIMD) */
#endif
#ifndef BGE_XFORM_MIN_WAVES
#define BGE_XFORM_MIN_WAVES 8 /* the variants with the transform part and nothing else heavy (the headline kernel).  While parent * local was formed on whole matrices (48 registers) they needed 72 VGPRs — at 64 they spilled 12 B per lane, 8 B per entity of scratch writes that rocprofv3 WRITE_SIZE showed — and ran at 7 waves per SIMD; with the product formed a row at a time (lds_mul_put) they need 55 / 48 */
#endif
// The ticks of a vouched wave in registers (fused ticks, solo groups): n ticks, each with the single tick's expressions — applyGravity,
// the slow-lane ballot, integrateTransforms — in their order.  false: a lane turned slow in one of them, and nothing is to be stored.
// The arithmetic is bge_fuse_math.hpp's (fuse::fuse_ticks; fuse::fuse_ticks_exact is that very loop, and what a wave falls back
// to): x and z velocity are a fixed point from the second tick on wherever gravity has no x or z part, and v.y is
// monotone, so the loop carries four adds and a product per tick and the ballot is decided from v.y's first and last value.
// The wave here is the hardware's: a lane value is a float, "any lane" a ballot.
struct WaveLanes {
    static __device__ __forceinline__ bool any(bool m) { return __ballot(m) != 0ull; }
    static __device__ __forceinline__ float abs(float v) { return fabsf(v); }
    static __device__ __forceinline__ bool same_bits(float a, float b) { return __float_as_uint(a) == __float_as_uint(b); }
};
__device__ __forceinline__ bool fuse_ticks(const float4 gf, const TickParams& p, uint32_t n, F3& vn, F3& xn)
{
    const fuse::Step c{(gf.x * gf.w) * p.dt, (gf.y * gf.w) * p.dt, (gf.z * gf.w) * p.dt, p.dt, p.sleep_lin};
    return fuse::fuse_ticks<WaveLanes>(c, n, vn, xn);
}
// The exact loop alone, for SOLO's retry inside its loop over the ticks: the reduced loop there keeps two more lane values live
// across the whole tick body, 98 VGPRs where the variant has 96 — an occupancy step (5 -> 4 waves per SIMD) for every wave of the
// launch, to save instructions for the rare wave whose first attempt declined (DESIGN.md §4.1 "Lean fusion").
__device__ __forceinline__ bool fuse_ticks_exact(const float4 gf, const TickParams& p, uint32_t n, F3& vn, F3& xn)
{
    const fuse::Step c{(gf.x * gf.w) * p.dt, (gf.y * gf.w) * p.dt, (gf.z * gf.w) * p.dt, p.dt, p.sleep_lin};
    return fuse::fuse_ticks_exact<WaveLanes>(c, n, vn, xn);
}

// Solo groups: between two ticks of ONE wave inside a solo launch (k_tick<..., SOLO>).  false: that was the launch's last tick.
// The wave has just stored a tick's results and is about to read and overwrite them as the next launch would.  Its lanes are
// different threads to the memory model, and some of those accesses cross lanes:
//   * the full write-out stores matrix rows of OTHER lanes' slots (through LDS, 16 B per lane); on a pinned world
//     (defer_row3 == 0) the next tick's translation-row store writes the same 16 bytes from the slot's own lane;
//   * lane 0 stores the words of the wave's record, and the reload below reads them with lanes 0..3;
//   * the write-out reads the wave's part of the LDS image that the next tick's lds_put overwrites.
// A workgroup-scope fence orders all of them: on gfx950 it is the wait for the wave's outstanding memory operations and nothing
// else — no cache write-back, no invalidate (the waves of a workgroup share one L1).  Nothing here waits for another wave: every
// wave of a flat tile depends on its own memory only.
// The record comes back through a VECTOR load (a lane-dependent address, then readlane): the scalar cache is not coherent with
// the wave's own vector stores, so the wave-uniform load of the launch's first tick must not be repeated.
__device__ __forceinline__ bool solo_next(const WorldView& w, uint32_t tile, uint32_t wave, uint32_t tid, uint32_t& remaining, uint4& rec)
{
    if (--remaining == 0u) return false;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    const uint32_t word = w.rs_word[4u * (tile * 4u + wave) + (tid & 3u)];
    rec = make_uint4(__builtin_amdgcn_readlane(word, 0), __builtin_amdgcn_readlane(word, 1), __builtin_amdgcn_readlane(word, 2), __builtin_amdgcn_readlane(word, 3));
    return true;
}

// SOLO (solo groups, TickParams::n_solo): an instantiation of its own for k_tick<PHYS, XFORM> — nothing else pays
// for its loop.  The host vouches that every tile of the launch is flat, so the block-tile branch with its workgroup barriers is
// compiled out, and every wave runs the n_solo ticks itself: fused in registers where it is vouched, else one tick after the other
// by the ordinary path, with solo_next() in between.
#ifndef BGE_SOLO_MIN_WAVES
#define BGE_SOLO_MIN_WAVES 4 /* the SOLO variant: with the loop over the ticks around the body it needs 96 VGPRs; compiled for 6 waves per SIMD it spills 11 VGPRs, for 8 it spills 66 — scratch traffic in every tick, against a launch whose cost is shared by a whole group of ticks */
#endif
template <bool PHYS, bool XFORM, bool AABB, bool NORMAL, bool BASIS, bool SOLO = false>
// 8 waves per SIMD (<= 64 VGPRs): the kernel waits on memory and, in block tiles, on barriers; occupancy hides both
// (the NORMAL variant carries a 4x4 inverse: it gets 128 VGPRs instead of spilling)
__global__ void __launch_bounds__(kTile, SOLO ? BGE_SOLO_MIN_WAVES : NORMAL ? 4 : (AABB ? BGE_AABB_MIN_WAVES : (BASIS ? BGE_BASIS_MIN_WAVES : (XFORM ? BGE_XFORM_MIN_WAVES : 8)))) k_tick(WorldView w, TickParams p)
{
    __shared__ float4 lds[kTile * 4];
    // BASIS: Bullet's orientation step (getRotation -> exponential map -> safeNormalize -> setRotation: four square roots, ten
    // divisions) and the euler write-back behind it (asin, two atan2) change nothing for a body whose quaternion is a fixed
    // point of that round trip and does not spin — 88 % of the bodies in steady state; those carry kSettled and skip both.
    // The others are scattered over all waves, so no wave could skip the code: they queue (quaternion, angular velocity) here
    // and, after a barrier, the first n threads of the workgroup do the step for the n queued bodies (usually one wave
    // instead of four), writing the results over their queue entries, where the owners pick them up.
    // The queue lives in the matrix staging area, which the transform stage only touches after the barrier that ends its use.
    __shared__ uint32_t eq_count;
    float4* const eq_quat = lds;        // [kTile] in: quaternion; out: the new one
    float4* const eq_av = lds + kTile;  // [kTile] in: angular velocity | kEq* bits; out: euler angles | kEq* bits
    if (PHYS && BASIS) {
        if (threadIdx.x == 0) eq_count = 0;
        __syncthreads();
    }
    constexpr uint32_t kEqNone = 0xffffffffu;
    constexpr uint32_t kEqIntegrate = 1u;  // in: run the orientation step (else only the angles are wanted)
    constexpr uint32_t kEqForce = 2u;      // in: the pose was set or corrected in this tick: the angles are rewritten whatever the step does
    constexpr uint32_t kEqStoreQuat = 4u;  // out: the quaternion changed
    constexpr uint32_t kEqStoreEuler = 8u; // out: the angles are new
    constexpr uint32_t kEqSettled = 16u;   // out: the step left the quaternion of a non-spinning body as it was
    uint32_t eq_at = kEqNone; // this lane's queue entry

    const uint32_t tile = p.tile_begin + blockIdx.x;
    uint32_t tid = threadIdx.x; // (neither changes; SOLO hides both from the optimiser once per tick, below)
    uint32_t slot = tile * kTile + tid;
    static_assert(!SOLO || (PHYS && XFORM && !AABB && !NORMAL && !BASIS), "solo groups exist for k_tick<PHYS, XFORM> alone");
    // (SOLO: the host vouches that the tile is flat — bge_flatten.hpp hdr_is_flat — and the compiler may know it)
    const uint32_t hdr = SOLO ? ((w.tile_hdr[tile] & ~(kHdrFrozen | kHdrExt | kHdrLevelMask)) | kHdrWaveLocal) : w.tile_hdr[tile];
    const uint32_t count = (hdr >> kHdrCountShift) & kHdrCountMask;
    const uint32_t max_level = hdr & kHdrLevelMask;

    // Rotation rows current (WorldView::rs_word): a wave whose word equals p.rs_epoch had world rows 0..2 = bx_mtx_srt(scale,
    // euler) for every valid slot when it last ran, and nothing has written scale, euler or world since (the host bumps the
    // epoch on every call that could).  Unless a lane re-poses or spins in this tick, rows 0..2 would come out bit for bit as
    // they are stored: the wave skips the euler / scale loads and bx_mtx_srt and stores the translation row alone (DESIGN.md
    // §4.1: 68 instead of 140 B per flat body).  The word is loaded as a scalar next to the tile header.
    constexpr bool kRowsPath = tick_variant_has_rows_path(XFORM, AABB, NORMAL, BASIS);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // The wave's record {rows word, rest word, flag value, flag epoch} (WorldView::rs_word) in one wave-uniform 16-B load.
    uint4 rec = (kRowsPath && (p.rs_epoch | p.rest_epoch) != 0u) ? reinterpret_cast<const uint4*>(w.rs_word)[tile * 4u + wave] : make_uint4(0u, 0u, 0u, 0u);
    // Fused ticks (WorldView::adv, TickParams::serial / n_left; DESIGN.md §4.1 "Fused ticks"): the wave's state in memory is already
    // the state after the tick with serial adv — an earlier launch of this group ran the ticks up to it in registers — so a launch
    // whose serial is not beyond it has nothing to do.  Wave-uniform, nothing stored; only a flat wave-local tile can have set the
    // word, and those have no workgroup barrier to miss (the rest path returns per wave in the same way).
    constexpr bool kFuse = PHYS && kRowsPath;
    // (The test on the header bit is always true where the word can be that high.  It is there for the schedule: without it the
    //  compiler sinks the header's load behind the return, and a wave that goes on pays a second scalar round trip; with it header,
    //  record and word leave together and are waited for once, as header and record were.  An empty asm would pin the load as well,
    //  but counts as a store to memory: the palette entry below then comes through a vector load.)
    if (kFuse && p.serial != 0u) {
        if (w.adv[tile * 4u + wave] >= p.serial && (hdr & kHdrWaveLocal) != 0u) return;
    }
    // Solo groups: the ticks this launch still owes the wave, and whether the fused block below is worth a try (not in the first
    // tick by the ordinary path: the first attempt has just declined).
    [[maybe_unused]] uint32_t remaining = SOLO ? p.n_solo : 1u;
    [[maybe_unused]] bool solo_retry = false;
    if constexpr (SOLO) {
        // First attempt: the vouched test and the fused block of the ordinary code below, for all n_solo ticks, BEFORE any store of
        // the launch — so that header, record and palette entry come through scalar loads, as in a group's first launch (inside
        // the loop, behind the wave's own stores, the same loads are vector loads).  The headline's path: one store, and out.
        if (p.rs_epoch != 0u && rec.x == p.rs_epoch && !(p.rest_epoch != 0u && rec.y == p.rest_epoch) && p.flag_word != 0u && rec.w == p.rs_epoch &&
            (hdr & kHdrAllDynamic) && p.cinfo_in == nullptr) {
            const float4 gf = w.grav_palette[rec.z >> kMassShift];
            if (gf.w != 0.0f) {
                F3 x0 = ld3(w.pos, slot);
                const F3 v = ld_vel(w.vel, slot);
                asm volatile("" : "+v"(x0.x), "+v"(x0.y), "+v"(x0.z)); // (as below: both loads leave together)
                F3 vn = v, xn = x0;
                // (Expected, and with a mark of its own behind the stores: left to itself the compiler shares these stores with the fused
                //  block inside the loop, in one exit block laid out behind the loop, and the twelve values then count as live across
                //  all of it — spills on this very path.)
                if (__builtin_expect(fuse_ticks(gf, p, remaining, vn, xn), 1)) {
                    st_vel_if(w.vel, slot, vn, vel_xz_changed(vn, v), vel_y_changed(vn, v));
                    st3(w.pos, slot, xn);
                    if (p.defer_row3 == 0u) reinterpret_cast<float4*>(w.world)[4ull * slot + 3u] = make_float4(xn.x, xn.y, xn.z, 1.0f);
                    asm volatile("; solo group: fused at the first attempt");
                    return;
                }
            }
        }
    }
solo_tick:; // (SOLO alone jumps here: the next tick of the launch, `rec` reloaded by solo_next)
    // (Opaque per tick: otherwise every address a tick forms from the lane's slot is hoisted out of the loop over the ticks and
    //  stays live across it — the variant then wants more than 128 VGPRs and spills on the first attempt's way out.)
    if constexpr (SOLO) asm volatile("" : "+v"(slot), "+v"(tid));
    const uint32_t rs_old = p.rs_epoch != 0u ? rec.x : 0u;
    // (header: wave-local, max level 0, no frozen root, no external parent)
    const bool flat_tile = kRowsPath && (hdr & (kHdrWaveLocal | kHdrFrozen | kHdrExt | kHdrLevelMask)) == kHdrWaveLocal;
    const bool rs_tile = flat_tile && p.rs_epoch != 0u;
    const bool rs_hint = rs_tile && rs_old == p.rs_epoch;

    // Rest path (WorldView::rs_word, word 1): a wave whose rest word equals p.rest_epoch ended its last full tick with every lane at
    // rest — no dirty bit, no spin, a Dynamic body ISLAND_SLEEPING with zero velocities stored, or no Dynamic body at all — and with
    // all four world rows = bx_mtx_srt(scale, euler, pos) of what is in memory; the host has not touched the world since (it bumps the
    // epoch on every call that could).  Only a kernel of this tick's contact stage can have changed that, and whichever does leaves a
    // mark in the flags, the deactivation record or the contact word (the audit table).  So the wave reads those 12 B per
    // body and, when one ballot finds no mark, returns: a sleeping body is not integrated, its zero velocity and its matrix would be
    // stored over the same bits, and its flags end the tick as they started (kTDirty is set and cleared within it).  Otherwise the
    // lanes go on into the ordinary path below.  Wave-local tiles of these variants have no workgroup barrier to miss.
    const uint32_t rest_old = p.rest_epoch != 0u ? rec.y : 0u;
    const bool rest_tile = flat_tile && p.rest_epoch != 0u;
    uint32_t f0;
    if (rest_tile && rest_old == p.rest_epoch) { // (wave-uniform)
        f0 = w.flags[slot];
        // (both read whether or not the flags say they matter: one round trip instead of two; the arrays cover whole tiles)
        const uint32_t dz_r = PHYS ? w.deact[slot] : 0u;
        const uint32_t ci_r = (PHYS && p.cinfo_in) ? p.cinfo_in[slot] : 0u;
        const uint32_t type_r = f0 & kTypeMask;
        bool moved;
        if (f0 & kValid) {
            moved = (f0 & (kTDirty | kSpin | kExtParent | kLevelMask)) != 0;
            if (PHYS) {
                moved = moved || (f0 & kBDirty) || type_r == 3u;
                // (the bits of the contact word this kernel obeys or consumes; kCiNoGravity, which k_island_begin sets on every sleeper,
                //  is read by the island kernels alone and stays)
                if (type_r == 2u) moved = moved || !(f0 & kDrowsy) || dz_r != kDeactSleeping || (ci_r & (kCiSolved | kCiMoved | kCiIsland));
            }
        } else {
            moved = PHYS && type_r != 0u; // an orphaned body is stepped: never on this path
        }
        // (SOLO: the wave leaves the launch with ticks still owed.  Nothing but the wave itself writes its memory between its ticks
        //  and this exit stores nothing, so every tick that remains would read the same words and leave by the same exit.)
        if (__ballot(moved) == 0ull) return;
    } else {
        // Vouched wave (WorldView::rs_word words 2 and 3, DESIGN.md §4.1 "flag word"): flag epoch == p.rs_epoch means that every one
        // of the wave's 64 flag words in memory is the record's flag value F, and F is kValid | Dynamic | mass class with no other bit:
        // awake with no deactivation record, not spinning, not dirty, no parent.  With the rows word current as well, all the ordinary
        // path would take from the 64 flag loads is F.  So the wave integrates with the palette entry of F's class (a uniform address)
        // and, unless a lane is slow enough to look at its deactivation record, stores what the ordinary path would store — velocity,
        // position, row 3; the flags end the tick as they are, kTDirty set and cleared — and returns.  It writes neither flags nor
        // words and touches neither the deactivation records nor the contact words; a wave that declines has stored nothing and goes
        // on into the ordinary path.  Every condition is wave-uniform.
        if (PHYS && kRowsPath && rs_hint && p.flag_word != 0u && rec.w == p.rs_epoch && (hdr & kHdrAllDynamic) && p.cinfo_in == nullptr) {
            const float4 gf = w.grav_palette[rec.z >> kMassShift];
            if (gf.w != 0.0f) {
                F3 x0 = ld3(w.pos, slot);
                const F3 v = ld_vel(w.vel, slot);
                // (pins the position load here, next to the velocity loads: the compiler otherwise sinks it behind the ballot below,
                //  a second memory round trip in the wave's life)
                asm volatile("" : "+v"(x0.x), "+v"(x0.y), "+v"(x0.z));
                // Fused ticks: nothing can observe the state between the ticks of one bge_world_tick_many call, and a vouched wave's tick
                // is lane-local arithmetic on six floats — so the wave runs the n_left ticks that remain of its group here, each with the
                // single tick's expressions and its ballot, and touches memory once.  It decides before any store: if a lane turns slow
                // in any of the ticks, nothing is stored and the wave goes on as a launch with n_left = 1 does (below); the launches
                // that follow in the group give it the same chance again with what is left.
                if (kFuse && p.serial != 0u && p.n_left > 1u && !SOLO) {
                    F3 vn = v, xn = x0;
                    // (The exact loop, written out as round 9 left it and not taken from bge_fuse_math.hpp: this kernel also runs every call
                    //  of ONE tick and every hierarchy scene.  With the reduced loop here its ISA was no longer the parent's and a call of one
                    //  tick measured 2 % slower, depth-4 chains 0.9 %; the exact loop through the header changes the ISA as well.  As it
                    //  stands the kernel is the parent's, instruction for instruction.  DESIGN.md §4.1 "Lean fusion".)
                    bool all_fast = true;
                    for (uint32_t i = 0; i < p.n_left; ++i) {
                        vn = F3{vn.x + (gf.x * gf.w) * p.dt, vn.y + (gf.y * gf.w) * p.dt, vn.z + (gf.z * gf.w) * p.dt};
                        if (__ballot(!(fabsf(vn.y) >= p.sleep_lin)) != 0ull) {
                            all_fast = false;
                            break;
                        }
                        xn = F3{xn.x + vn.x * p.dt, xn.y + vn.y * p.dt, xn.z + vn.z * p.dt};
                    }
                    if (all_fast) {
                        st_vel_if(w.vel, slot, vn, vel_xz_changed(vn, v), vel_y_changed(vn, v));
                        st3(w.pos, slot, xn);
                        if (p.defer_row3 == 0u) reinterpret_cast<float4*>(w.world)[4ull * slot + 3u] = make_float4(xn.x, xn.y, xn.z, 1.0f);
                        if ((tid & 63u) == 0u) w.adv[tile * 4u + wave] = p.serial + p.n_left - 1u;
                        return;
                    }
                }
                // Solo groups: the same for the ticks the launch still owes the wave (by the exact loop: see fuse_ticks_exact), and no word to set —
                // the wave's launch ends with it.
                if constexpr (SOLO) {
                    if (solo_retry && remaining > 1u) {
                        F3 vn = v, xn = x0;
                        if (fuse_ticks_exact(gf, p, remaining, vn, xn)) {
                            st_vel_if(w.vel, slot, vn, vel_xz_changed(vn, v), vel_y_changed(vn, v));
                            st3(w.pos, slot, xn);
                            if (p.defer_row3 == 0u) reinterpret_cast<float4*>(w.world)[4ull * slot + 3u] = make_float4(xn.x, xn.y, xn.z, 1.0f);
                            return;
                        }
                    }
                }
                // (the expressions of applyGravity and integrateTransforms below, in their order)
                const F3 v1{v.x + (gf.x * gf.w) * p.dt, v.y + (gf.y * gf.w) * p.dt, v.z + (gf.z * gf.w) * p.dt};
                if (__ballot(!(fabsf(v1.y) >= p.sleep_lin)) == 0ull) {
                    st_vel_if(w.vel, slot, v1, vel_xz_changed(v1, v), vel_y_changed(v1, v));
                    const F3 x1{x0.x + v1.x * p.dt, x0.y + v1.y * p.dt, x0.z + v1.z * p.dt};
                    st3(w.pos, slot, x1);
                    // (deferred: the row is (x1, 1) of the position just stored; readers compose it, k_row3_sync stores it — DESIGN.md §4.1)
                    if (p.defer_row3 == 0u) reinterpret_cast<float4*>(w.world)[4ull * slot + 3u] = make_float4(x1.x, x1.y, x1.z, 1.0f);
                    if constexpr (SOLO) {
                        if (solo_next(w, tile, wave, tid, remaining, rec)) {
                            solo_retry = true;
                            goto solo_tick;
                        }
                    }
                    return;
                }
            }
        }
        f0 = w.flags[slot];
    }
    // The component loads do not wait for the flag word: every array is allocated for whole tiles, so the loads of a slot
    // that turns out to be empty (or of a velocity nobody integrates) are harmless, and issuing them together with the flags
    // takes one memory round trip instead of two out of a workgroup's life.  Measured at
    // 1 M flat bodies: 24.4 -> 23.7 us per tick; velocities are only loaded early in tiles whose slots all carry a Dynamic body
    // (loading them everywhere cost 64-node subtrees, 1 body in 64 entities, 4 % more time)
    F3 pos = ld3(w.pos, slot), eul{0.0f, 0.0f, 0.0f}, scl{1.0f, 1.0f, 1.0f}, vel_early{0.0f, 0.0f, 0.0f};
    if (!rs_hint) {
        eul = ld3(w.euler, slot);
        if (XFORM) scl = ld3(w.scale, slot);
    }
    if (PHYS && (hdr & kHdrAllDynamic)) vel_early = ld_vel(w.vel, slot); // (elsewhere most slots have no velocity to read)
    // The mass palette entry (gravity force, inverse mass) is one more dependent round trip behind the flag word.  In tiles whose
    // slots all carry a Dynamic body every lane fetches palette entry (lane) with the loads above and takes its class's entry
    // from lane (class) once the flags are there (classes are < 64; outside any divergent branch: a permute reads active lanes).
    // 1 M flat bodies: 23.4 -> 23.15 us per tick (three alternating runs).  Doing this — and the early velocity load — in every tile
    // with at least one Dynamic body in eight slots made depth-4 chains (bodies on the roots) 3 % SLOWER (22.5 -> 23.2 us): there
    // the extra loads cost more than the round trip they hide.  Not in the Bullet-basis variant either: 31.9 -> 32.1 us with it (and
    // with the queue counter's barrier moved behind the first loads), three alternating runs.
    float4 gf_early = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const bool palette_early = PHYS && !BASIS && (hdr & kHdrAllDynamic);
    if (palette_early) {
        const float4 mine = w.grav_palette[tid & 63u];
        const int cls0 = static_cast<int>((f0 >> kMassShift) & 63u);
        gf_early = make_float4(__shfl(mine.x, cls0, 64), __shfl(mine.y, cls0, 64), __shfl(mine.z, cls0, 64), __shfl(mine.w, cls0, 64));
    }
    // Ground plane on (p.cinfo_in): the contact word k_ground left and the deactivation record — most bodies of a scene at rest
    // are asleep — are two more dependent round trips behind the flag word; in all-dynamic tiles they are requested with the
    // first loads (8 B per body more, only in ticks that follow a k_ground launch).
    uint32_t ci_early = 0, dz_early = 0;
    const bool ground_early = PHYS && p.cinfo_in != nullptr && (hdr & kHdrAllDynamic);
    if (ground_early) {
        ci_early = p.cinfo_in[slot];
        dz_early = w.deact[slot];
    }
    uint32_t f = f0;
    const bool valid = (f & kValid) != 0;
    // A slot with a body but no Transform: the entity lost its Transform while its RigidBody stayed.  The reference keeps that
    // Bullet body in the world (EnsureRigidBody returns before it looks at the runtime, PhysicsSystem.cpp:389-393; nothing
    // removes it while the component exists): it is stepped, collides and enters trigger volumes like any other, but it is
    // never re-posed or re-created and nothing is written back.  Here: the physics part runs, the transform part does not.
    const bool orphan_body = PHYS && !valid && (f & kTypeMask) != 0;
    if (!valid && !orphan_body) {
        pos = eul = F3{0.0f, 0.0f, 0.0f};
        scl = F3{1.0f, 1.0f, 1.0f};
    }
    // The flags confirm the word: no valid lane re-poses (which rewrites euler), spins (which turns it), has an external parent
    // or a parent in the tile.  (Orphaned bodies never read euler / scale here.)  Otherwise the lanes load what they skipped.
    bool rs_fast = false;
    if (rs_hint) {
        const bool repose_now = PHYS && p.no_repose == 0u && (f & (kTDirty | kBDirty)) != 0;
        const bool stale = valid && (repose_now || (PHYS && (f & kSpin)) || (f & (kExtParent | kLevelMask)));
        rs_fast = __ballot(stale) == 0ull;
        if (!rs_fast && (valid || orphan_body)) {
            eul = ld3(w.euler, slot);
            scl = ld3(w.scale, slot);
        }
    }

    // (AABB variants) this lane's fed box for the wave's broadphase partial: identity when the slot carries no body
    float box_mn[3] = {INFINITY, INFINITY, INFINITY}, box_mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    bool has_box = false;
    bool asleep = false; // a Dynamic body that ends this tick ISLAND_SLEEPING with zero velocities stored (the rest word)
    if (PHYS) {
        const uint32_t type = f & kTypeMask;
        if (type != 0) { // (type bits exist only on slots that carry a body: with a Transform, or orphaned)
            const bool dynamic = type == 2u;
            // (p.no_repose: a later sub-step of the same stepSimulation call — the teleport rule ran before the first one)
            const bool repose = valid && p.no_repose == 0u && (f & (kTDirty | kBDirty)) != 0;
            bool spin = (f & kSpin) != 0;
            // BASIS (BGE_TICK_BULLET_BASIS): Bullet's own orientation scheme.  Its state is the 3x3 basis, which every step
            // goes basis -> getRotation -> exponential map -> safeNormalize -> setRotation for EVERY non-static body, spinning
            // or not.  The basis is always setRotation(q) of a stored quaternion, so q stays the state here and the basis
            // is recomputed from it: same bits, 16 instead of 36 bytes.
            bool advanced = false;
            // ground plane on: k_ground collided this body with the plane before this kernel ran and, if it is in contact (or
            // spinning), solved it — its velocities are final (gravity impulse included), its fed AABB is written
            uint32_t ci = 0;
            if (p.cinfo_in && dynamic) ci = ground_early ? ci_early : p.cinfo_in[slot];
            const bool solved = (ci & kCiSolved) != 0;
            // whatever writes the quaternion (re-pose, spin, the split impulse) takes kSettled away
            if (repose || spin || (ci & kCiMoved)) f &= ~kSettled;
            bool turn = BASIS ? (dynamic && !(f & kSettled)) : spin;
            Q4 q{0.0f, 0.0f, 0.0f, 1.0f};
            F3 v{0.0f, 0.0f, 0.0f};
            F3 av{0.0f, 0.0f, 0.0f};
            if (repose) {
                // SyncKinematicBodiesToPhysics / EnsureRigidBody: pose from the LOCAL Transform, zero velocities
                q = bt_quat_from_transform_euler(eul);
                st4(w.quat, slot, q);
                if (spin) { // (of whatever type the re-created body is: the record the download reads is the new body's)
                    st3(w.angvel, slot, av);
                    spin = false;
                    f &= ~kSpin;
                    if (!BASIS) turn = false; // its angular velocity is zero now: the default scheme leaves the re-posed quaternion alone
                }
            } else {
                if (dynamic) v = (hdr & kHdrAllDynamic) ? vel_early : ld_vel(w.vel, slot);
                if (spin) av = ld3(w.angvel, slot);
                if (turn || AABB) q = ld4(w.quat, slot);
            }

            if (AABB && solved) {
                const float* bb = w.aabb + 6ull * slot; // written by k_ground from the pre-solve state
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    box_mn[a] = bb[a];
                    box_mx[a] = bb[3 + a];
                }
                has_box = true;
            }
            if (AABB && !solved) {
                const F3 he = ld3(w.half_extent, slot);
                const M3 r = bt_mat_from_quat(q);
                float mn[3], mx[3];
                bt_aabb_of_pose(pos, r, he, mn, mx);
                if (dynamic) {
                    // interpolation transform of predictUnconstraintMotion: velocity before the gravity impulse
                    const F3 pp{pos.x + v.x * p.dt, pos.y + v.y * p.dt, pos.z + v.z * p.dt};
                    float mn2[3], mx2[3];
                    if (turn) {
                        const M3 r2 = bt_mat_from_quat(bt_integrate_orientation(BASIS ? bt_quat_from_mat(r) : q, av, p.dt));
                        bt_aabb_of_pose(pp, r2, he, mn2, mx2);
                    } else {
                        bt_aabb_of_pose(pp, r, he, mn2, mx2);
                    }
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        mn[a] = mn2[a] < mn[a] ? mn2[a] : mn[a];
                        mx[a] = mx2[a] > mx[a] ? mx2[a] : mx[a];
                    }
                }
                float* bb = w.aabb + 6ull * slot;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    bb[a] = mn[a];
                    bb[3 + a] = mx[a];
                    box_mn[a] = mn[a];
                    box_mx[a] = mx[a];
                }
                has_box = true;
            }

            if (dynamic) {
                // mass class -> (gravity force, inv_mass) from the world's palette (a few distinct masses per scene,
                // L1/L2-resident); class 63 falls back to the per-slot array.  The force is btRigidBody::setGravity's
                // m_gravity = acceleration / m_inverseMass — a DIVISION per component in the reference's build
                // (oracle/tools/check_bullet_order.py) — which the host evaluates once per class and gravity vector.
                const uint32_t cls = f >> kMassShift;
                float inv_mass;
                F3 force;
                if (cls != kMassClassArray) {
                    const float4 gf = palette_early ? gf_early : w.grav_palette[cls];
                    inv_mass = gf.w;
                    force = F3{gf.x, gf.y, gf.z};
                } else {
                    inv_mass = w.inv_mass[slot];
                    force = F3{p.gx / inv_mass, p.gy / inv_mass, p.gz / inv_mass};
                }
                // Deactivation record: untouched (and unread) while the body is fast and its timer is zero.
                // (kDrowsy <=> record != 0; body (re)creation clears the bit: a new btRigidBody is ACTIVE_TAG, timer 0)
                const uint32_t dz0 = (f & kDrowsy) ? (ground_early ? dz_early : w.deact[slot]) : 0u;
                uint32_t dz = dz0;
                // buildIslands: a free body is an island of its own; WANTS_DEACTIVATION -> ISLAND_SLEEPING
                // (kCiIsland: an island of several bodies with an active body in it keeps this one awake — bge_island.hip k_island_flags)
                if (dz == kDeactWants && !(ci & kCiIsland)) dz = kDeactSleeping;
                if (inv_mass != 0.0f && dz == kDeactSleeping) {
                    // asleep: no gravity, not solved, not integrated; updateActivationState zeroes the velocities
                    v = F3{0.0f, 0.0f, 0.0f};
                    st_vel(w.vel, slot, v);
                    asleep = true;
                    if (spin) {
                        st3(w.angvel, slot, v);
                        spin = false;
                        f &= ~kSpin;
                    }
                } else if (inv_mass != 0.0f) {
                    // applyGravity (F = g * (1/invMass)) + solver write-back of the external force impulse
                    // Of the velocity only the components whose bits the impulse changed are stored: a y-only gravity leaves the xz
                    // lines of the velocity blocks clean (8 B per falling body less to write back).  A solved body's velocity is
                    // what k_ground stored; a re-posed body's zero was not loaded, so it is stored whole.  Stored here and not next
                    // to the position below: neither the loaded components nor the compares then stay live across the turn.
                    if (!solved) {
                        const F3 v1{v.x + (force.x * inv_mass) * p.dt, v.y + (force.y * inv_mass) * p.dt, v.z + (force.z * inv_mass) * p.dt};
                        st_vel_if(w.vel, slot, v1, repose || vel_xz_changed(v1, v), repose || vel_y_changed(v1, v));
                        v = v1;
                    } else if (repose) {
                        st_vel(w.vel, slot, v);
                    }
                    // integrateTransforms
                    pos.x = pos.x + v.x * p.dt;
                    pos.y = pos.y + v.y * p.dt;
                    pos.z = pos.z + v.z * p.dt;
                    if (turn && BASIS && !AABB) {
                        // queued: the first threads of the workgroup run the step after the barrier below
                        eq_at = atomicAdd(&eq_count, 1u);
                        eq_quat[eq_at] = make_float4(q.x, q.y, q.z, q.w);
                        eq_av[eq_at] = make_float4(av.x, av.y, av.z, __uint_as_float(kEqIntegrate | ((repose || (ci & kCiMoved)) ? kEqForce : 0u)));
                    } else if (turn) {
                        const Q4 qn = bt_integrate_orientation(BASIS ? bt_quat_from_mat(bt_mat_from_quat(q)) : q, av, p.dt);
                        // BASIS: a quaternion the round trip maps onto itself (88 % of the non-spinning bodies in steady state)
                        // needs neither the store nor new angles — rotationEuler already holds getEulerZYX of exactly these bits
                        const bool same = BASIS && !repose && __float_as_uint(qn.x) == __float_as_uint(q.x) && __float_as_uint(qn.y) == __float_as_uint(q.y) &&
                                          __float_as_uint(qn.z) == __float_as_uint(q.z) && __float_as_uint(qn.w) == __float_as_uint(q.w);
                        q = qn;
                        if (!same) {
                            st4(w.quat, slot, q);
                            advanced = true;
                        } else if (!spin && !(ci & kCiMoved)) {
                            f |= kSettled;
                        }
                    }
                    st3(w.pos, slot, pos);
                    // updateActivationState: updateDeactivation + wantsSleeping.  The kernel is close to VALU-bound, so the
                    // common case is decided by one compare: |v.y| >= threshold implies |v|^2 >= threshold^2 in float
                    // arithmetic too (rounding is monotone and the other two squares are >= 0), i.e. "not slow".
                    // (Measured at 1 M bodies: sleeping support costs 1.4 % of the tick this way, 2.0 % with the full test on
                    // every body, 2.9 % with the record handling moved behind a separate branch.)
                    if (!(fabsf(v.y) >= p.sleep_lin) || dz != 0u) {
                        const float lin2 = v.x * v.x + v.y * v.y + v.z * v.z;
                        const float ang2 = av.x * av.x + av.y * av.y + av.z * av.z;
                        const bool slow = lin2 < p.sleep_lin2 && ang2 < p.sleep_ang2;
                        if (dz == kDeactWants) {
                            // kept awake by its island: wantsSleeping() is true for the state itself while the body is slow; faster
                            // than the thresholds it is ACTIVE_TAG again, timer 0
                            if (!slow) dz = 0u;
                        } else if (slow || dz != 0u) {
                            const float t = slow ? __uint_as_float(dz) + p.dt : 0.0f;
                            dz = (p.sleep_time != 0.0f && t > p.sleep_time) ? kDeactWants : __float_as_uint(t);
                        }
                    }
                }
                if (dz != dz0) {
                    w.deact[slot] = dz;
                    f = dz ? (f | kDrowsy) : (f & ~kDrowsy);
                }
                if (inv_mass == 0.0f && repose) {
                    st_vel(w.vel, slot, v);
                }
                // SyncRigidBodiesFromPhysics: rotationEuler <- getEulerZYX(basis) whenever the orientation was
                // (re)posed or advanced; a non-spinning body keeps its euler triple bit for bit
                if (eq_at == kEqNone && (repose || advanced || (ci & kCiMoved))) {
                    if (!(repose || advanced) && !(turn || AABB)) q = ld4(w.quat, slot); // the split impulse moved a body whose quaternion was not read
                    if (BASIS) {
                        eq_at = atomicAdd(&eq_count, 1u);
                        eq_quat[eq_at] = make_float4(q.x, q.y, q.z, q.w);
                        eq_av[eq_at] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(kEqForce));
                    } else {
                        eul = bt_transform_euler_from_mat(bt_mat_from_quat(q));
                        st3(w.euler, slot, eul);
                    }
                }
                if (ci & (kCiSolved | kCiMoved | kCiIsland)) w.cinfo[slot] = ci & ~(kCiSolved | kCiMoved | kCiIsland); // consumed
                if (valid) f |= kTDirty; // transform->MarkDirty()
            }
            if (valid) f &= ~kBDirty; // (an orphaned body is not re-created: its dirty bit waits for the Transform)
        }
    }

    if (PHYS && BASIS) {
        __syncthreads();
        const uint32_t n_queued = eq_count;
        // (rotating the wave that takes the first 64 entries with the workgroup index, so that not every resident workgroup's
        //  wave 0 does this work, changed nothing: 32.1 against 31.8 us)
        const uint32_t et = tid;
        if (et < n_queued) {
            const float4 qq = eq_quat[et], aa = eq_av[et];
            const uint32_t in = __float_as_uint(aa.w);
            Q4 q{qq.x, qq.y, qq.z, qq.w};
            uint32_t out = (in & kEqForce) ? kEqStoreEuler : 0u;
            if (in & kEqIntegrate) {
                const Q4 qn = bt_integrate_orientation(bt_quat_from_mat_sel(bt_mat_from_quat(q)), F3{aa.x, aa.y, aa.z}, p.dt);
                const bool same = !(in & kEqForce) && __float_as_uint(qn.x) == __float_as_uint(q.x) && __float_as_uint(qn.y) == __float_as_uint(q.y) &&
                                  __float_as_uint(qn.z) == __float_as_uint(q.z) && __float_as_uint(qn.w) == __float_as_uint(q.w);
                // (a re-posed or corrected body stores what the step made of its quaternion even when the bits did not move:
                //  what the inline form of this step does, and the next tick finds it settled)
                if (!same) out |= kEqStoreQuat | kEqStoreEuler;
                else if (aa.x == 0.0f && aa.y == 0.0f && aa.z == 0.0f) out |= kEqSettled;
                q = qn;
            }
            F3 e{0.0f, 0.0f, 0.0f};
            if (out & kEqStoreEuler) e = bt_transform_euler_from_mat<true>(bt_mat_from_quat(q));
            eq_quat[et] = make_float4(q.x, q.y, q.z, q.w);
            eq_av[et] = make_float4(e.x, e.y, e.z, __uint_as_float(out));
        }
        __syncthreads();
        if (eq_at != kEqNone) {
            const float4 e = eq_av[eq_at];
            const uint32_t out = __float_as_uint(e.w);
            if (out & kEqStoreQuat) {
                const float4 qq = eq_quat[eq_at];
                st4(w.quat, slot, Q4{qq.x, qq.y, qq.z, qq.w});
            }
            if (out & kEqStoreEuler) {
                eul = F3{e.x, e.y, e.z};
                st3(w.euler, slot, eul);
            }
            if (out & kEqSettled) f |= kSettled;
        }
        if (XFORM) __syncthreads(); // the staging area is handed to the transform stage
    }

    if (AABB && PHYS) {
        // Broadphase partial of this wave (replaces a pass of k_bp_bounds over all AABBs): bounds, body count, widest box.
        // The extent is the expression the sort's large-body test evaluates (bge_broadphase.hip body_is_large).
        if (p.bp_partial) { // uniform
            float ext = fmaxf(fmaxf(box_mx[0] - box_mn[0], box_mx[1] - box_mn[1]), box_mx[2] - box_mn[2]);
            if (!(has_box && ext > 0.0f && ext < INFINITY)) ext = -INFINITY;
            const unsigned long long boxes = __ballot(has_box);
            float r[7];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                r[a] = wave_reduce_to_lane63<true>(box_mn[a]);
                r[3 + a] = wave_reduce_to_lane63<false>(box_mx[a]);
            }
            r[6] = wave_reduce_to_lane63<false>(ext);
            if ((tid & 63u) == 63u) {
                float4* dst = p.bp_partial + 2ull * (4ull * tile + (tid >> 6));
                dst[0] = make_float4(r[0], r[1], r[2], r[6]);
                dst[1] = make_float4(r[3], r[4], r[5], __uint_as_float(static_cast<uint32_t>(__popcll(boxes))));
            }
        }
    }

    if (kRowsPath && rs_fast) {
        // rows 0..2 in memory are what bx_mtx_srt would store; row 3 is (pos, 1) (bx::mtxSRT, m[12..15]).  16 B at a 64-B stride,
        // plain stores: tools/ubench_world_rows.hip measured non-temporal ones twice as slow for this shape, and the host keeps
        // the path off where the working set outgrows the Infinity Cache (16 M slots: partially written lines cost 2.7x whole ones)
        // unless the tick defers the row, which writes no partial line at all
        // With p.defer_row3 not even that: pos in memory is this lane's pos (stored above if it moved), and the wave's rows word stays
        // current, which is what tells every reader to take the row from there (world_row3)
        if (valid && p.defer_row3 == 0u) reinterpret_cast<float4*>(w.world)[4ull * slot + 3u] = make_float4(pos.x, pos.y, pos.z, 1.0f);
        f &= ~kTDirty; // transform->dirty = false
        if (kRowsPath && PHYS && p.rest_epoch != 0u) {
            // rows 0..2 were current and row 3 is stored: the rest word says so when every lane ends the tick at rest (written only when it changes)
            const uint32_t type = f & kTypeMask;
            const bool rests = valid ? (!(f & (kTDirty | kBDirty | kSpin | kExtParent | kLevelMask)) && type != 3u && (type != 2u || asleep)) : !orphan_body;
            const uint32_t rest_new = (rest_tile && __ballot(!rests) == 0ull) ? p.rest_epoch : 0u;
            if (rest_new != rest_old && (tid & 63u) == 0u) w.rs_word[4u * (tile * 4u + wave) + 1u] = rest_new;
        }
        if (PHYS && kRowsPath && p.rs_epoch != 0u) {
            // flag word (words 2 and 3): the wave's 64 flag words end the tick equal and of the vouched form, or the flag epoch is 0
            const uint32_t f_end = f;
            const uint32_t f_first = __builtin_amdgcn_readfirstlane(f_end);
            const bool vouch = rs_tile && (hdr & kHdrAllDynamic) && __ballot(f_end != f_first) == 0ull &&
                               (f_first & ~kMassMask) == (kValid | 2u) && (f_first >> kMassShift) != kMassClassArray;
            const uint32_t fe_new = vouch ? p.rs_epoch : 0u;
            if ((fe_new != rec.w || (vouch && f_first != rec.z)) && (tid & 63u) == 0u)
                reinterpret_cast<uint2*>(w.rs_word)[2u * (tile * 4u + wave) + 1u] = make_uint2(f_first, fe_new);
        }
    } else if (XFORM) {
        float local[16];
        bx_mtx_srt(local, scl, eul, pos);
        const uint32_t level = (f & kLevelMask) >> kLevelShift;
        float4* dst = reinterpret_cast<float4*>(w.world) + 4ull * kTile * tile;
        bool keep_world = false;
        // A root that became one because its parent entity lost its Transform: the reference does not recompute it until it is
        // dirty (nothing marked it), so it keeps the stored parent * local matrix; the first dirty tick ends that.
        if ((hdr & kHdrFrozen) && valid && level == 0 && !(f & kExtParent)) { // (the header bit is uniform and almost never set)
            const uint32_t bit = 1u << (slot & 31u);
            if (w.frozen[slot >> 5] & bit) {
                if (f & kTDirty) atomicAnd(&w.frozen[slot >> 5], ~bit);
                else keep_world = true;
            }
        }

        if (hdr & kHdrWaveLocal) {
            // Singletons at level 0 only (bge_flatten.hpp kHdrWaveLocal): the write-out needs no workgroup barrier — DS
            // operations of one wave execute in order.
            if (valid && level == 0) {
                if (f & kExtParent) {
                    world_mul_put(lds, w.world, w.parent[slot], tid, local);
                } else {
                    lds_put(lds, tid, local); // root: world = local (Transform.cpp:32-35)
                    if (keep_world) lds_put_stored(lds, tid, w.world, slot);
                    if (p.root_out && !(f & kHasParent)) {
                        if (keep_world) store_root_stored(p.root_out, w.root_index[slot], w.world, slot);
                        else store_root(p.root_out, w.root_index[slot], local);
                    }
                }
            }
            wave_lds_sync();
            // write-out of this wave's own 4 KiB: lane l stores float4 number l + 64k of the group's image
            const unsigned long long valid_mask = __ballot(valid);
            const uint32_t lane = tid & 63u;
            const uint32_t wbase = tid & ~63u;
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                const uint32_t qi = lane + 64u * k;      // float4 index inside the group's image
                const uint32_t nl = qi >> 2;             // node inside the group
                const uint32_t n = wbase + nl;
                const uint32_t r = (qi & 3u) ^ ((n >> 2) & 3u);
                if ((valid_mask >> nl) & 1ull) store_out(&dst[n * 4u + r], lds[wbase * 4u + qi], p.nt_out != 0);
            }
            if (kRowsPath && p.rs_epoch != 0u) {
                // the rows just stored are bx_mtx_srt of the scale and euler in memory; the word says so when the next tick can use
                // it: every valid lane ends the tick without spin in a tile of the fast path's shape (written only when it changes)
                const bool keeps = rs_tile && __ballot(valid && (f & (kSpin | kExtParent | kLevelMask))) == 0ull;
                const uint32_t rs_new = keeps ? p.rs_epoch : 0u;
                if (rs_new != rs_old && (tid & 63u) == 0u) w.rs_word[4u * (tile * 4u + wave)] = rs_new;
            }
            if (kRowsPath && PHYS && p.rest_epoch != 0u) {
                // all four rows just stored are bx_mtx_srt of what is in memory; kTDirty ends the tick cleared (below)
                const uint32_t type = f & kTypeMask;
                const bool rests = valid ? (!(f & (kBDirty | kSpin | kExtParent | kLevelMask)) && type != 3u && (type != 2u || asleep)) : !orphan_body;
                const uint32_t rest_new = (rest_tile && __ballot(!rests) == 0ull) ? p.rest_epoch : 0u;
                if (rest_new != rest_old && (tid & 63u) == 0u) w.rs_word[4u * (tile * 4u + wave) + 1u] = rest_new;
            }
            if (PHYS && kRowsPath && p.rs_epoch != 0u) {
                // flag word (words 2 and 3): the wave's 64 flag words end the tick equal and of the vouched form, or the flag epoch is 0
                const uint32_t f_end = f & ~kTDirty /* (cleared below) */;
                const uint32_t f_first = __builtin_amdgcn_readfirstlane(f_end);
                const bool vouch = rs_tile && (hdr & kHdrAllDynamic) && __ballot(f_end != f_first) == 0ull &&
                                   (f_first & ~kMassMask) == (kValid | 2u) && (f_first >> kMassShift) != kMassClassArray;
                const uint32_t fe_new = vouch ? p.rs_epoch : 0u;
                if ((fe_new != rec.w || (vouch && f_first != rec.z)) && (tid & 63u) == 0u)
                    reinterpret_cast<uint2*>(w.rs_word)[2u * (tile * 4u + wave) + 1u] = make_uint2(f_first, fe_new);
            }
            if (NORMAL) {
                // render feed: normalMtx = transpose(inverse(world)) (Renderer.cpp:633-636), same LDS round trip
                float m[16], nm[16];
                if (valid) lds_get(lds, tid, m);
                wave_lds_sync();
                if (valid) {
                    bx_normal_matrix(nm, m);
                    lds_put(lds, tid, nm);
                }
                wave_lds_sync();
                float4* ndst = reinterpret_cast<float4*>(w.normal) + 4ull * kTile * tile;
#pragma unroll
                for (uint32_t k = 0; k < 4; ++k) {
                    const uint32_t qi = lane + 64u * k;
                    const uint32_t nl = qi >> 2;
                    const uint32_t n = wbase + nl;
                    const uint32_t r = (qi & 3u) ^ ((n >> 2) & 3u);
                    if ((valid_mask >> nl) & 1ull) store_out(&ndst[n * 4u + r], lds[wbase * 4u + qi], p.nt_out != 0);
                }
            }
        } else {
            // block tile (a subtree of 65..256 nodes, or the breadth-first prefix of a larger one): levels are
            // separated by workgroup barriers, parents staged in LDS
            const uint32_t parent = (f & kParentMask) >> kParentShift;
            if (valid && level == 0) {
                if (f & kExtParent) {
                    // parent resolved by an earlier launch: read its world matrix from memory
                    world_mul_put(lds, w.world, w.parent[slot], tid, local);
                } else {
                    lds_put(lds, tid, local);
                    if (keep_world) lds_put_stored(lds, tid, w.world, slot);
                    if (p.root_out && !(f & kHasParent)) {
                        if (keep_world) store_root_stored(p.root_out, w.root_index[slot], w.world, slot);
                        else store_root(p.root_out, w.root_index[slot], local);
                    }
                }
            }
            for (uint32_t d = 1; d <= max_level; ++d) {
                __syncthreads();
                if (valid && level == d) lds_mul_put(lds, parent, tid, local); // parent * local — the reference's order
            }
            __syncthreads();
            // coalesced write-out: lane t stores float4 #(t + 256k) of the tile's 16 KiB image
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                const uint32_t qi = tid + kTile * k;
                const uint32_t n = qi >> 2;
                const uint32_t r = (qi & 3u) ^ ((n >> 2) & 3u);
                if (n < count) store_out(&dst[n * 4u + r], lds[qi], p.nt_out != 0);
            }
            if (NORMAL) {
                float m[16], nm[16];
                if (valid) lds_get(lds, tid, m);
                __syncthreads();
                if (valid) {
                    bx_normal_matrix(nm, m);
                    lds_put(lds, tid, nm);
                }
                __syncthreads();
                float4* ndst = reinterpret_cast<float4*>(w.normal) + 4ull * kTile * tile;
#pragma unroll
                for (uint32_t k = 0; k < 4; ++k) {
                    const uint32_t qi = tid + kTile * k;
                    const uint32_t n = qi >> 2;
                    const uint32_t r = (qi & 3u) ^ ((n >> 2) & 3u);
                    if (n < count) store_out(&ndst[n * 4u + r], lds[qi], p.nt_out != 0);
                }
            }
        }
        f &= ~kTDirty; // transform->dirty = false
    }

    if (f != f0) w.flags[slot] = f;
    if constexpr (SOLO) {
        if (solo_next(w, tile, wave, tid, remaining, rec)) {
            solo_retry = true;
            goto solo_tick;
        }
    }
}

// PhysicsSystem::Update with a stepSimulation that runs no sub-step (Bullet's accumulator, src/physics/PhysicsSystem.cpp:855-863:
// m_localTime has not reached fixedStep yet).  What still happens around the step: EnsureRigidBody /
// SyncKinematicBodiesToPhysics re-pose every body whose Transform or RigidBody is dirty and zero a Dynamic one's
// velocities (:952-989); SyncRigidBodiesFromPhysics writes every Dynamic body's pose back and marks its Transform dirty
// (:916-950).  Position needs no copy (Transform::position and the body origin share storage); rotationEuler is rewritten
// when the body was re-posed, or always in Bullet's own orientation scheme (BASIS).
template <bool BASIS>
__global__ void __launch_bounds__(256) k_pose_only(WorldView w, uint64_t n_slots)
{
    const uint64_t slot64 = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (slot64 >= n_slots) return;
    const uint32_t slot = static_cast<uint32_t>(slot64);
    const uint32_t f0 = w.flags[slot];
    uint32_t f = f0;
    const uint32_t type = f & kTypeMask;
    if (!(f & kValid) || type == 0) return;
    const bool dynamic = type == 2u;
    const bool repose = (f & (kTDirty | kBDirty)) != 0;
    Q4 q{0.0f, 0.0f, 0.0f, 1.0f};
    if (repose) {
        q = bt_quat_from_transform_euler(ld3(w.euler, slot));
        st4(w.quat, slot, q);
        f &= ~kSettled;
        const F3 zero{0.0f, 0.0f, 0.0f};
        if (dynamic) st_vel(w.vel, slot, zero);
        if (f & kSpin) {
            st3(w.angvel, slot, zero);
            f &= ~kSpin;
        }
    }
    if (dynamic) {
        if (repose || BASIS) {
            if (!repose) q = ld4(w.quat, slot);
            st3(w.euler, slot, bt_transform_euler_from_mat(bt_mat_from_quat(q)));
        }
        f |= kTDirty; // transform->MarkDirty()
    }
    f &= ~kBDirty;
    if (f != f0) w.flags[slot] = f;
}

// ------------------------------------------------------------------ component scatter / gather (entity order <-> slots)
// stage holds `count` rows of `width` 32-bit words for entities [first, first+count).
// `index` (nullable) selects entities explicitly: row i belongs to entity index[i] instead of first + i.
// `vel_blocks`: the device array is WorldView::vel — rows of three words on the host side, per-wave component blocks on the device
// (bge_device_math.hpp, vel_word).
__global__ void k_scatter_rows(const uint32_t* __restrict__ slot_of_entity, const uint32_t* __restrict__ index,
                               uint64_t first, uint64_t count,
                               uint32_t width, const uint32_t* __restrict__ stage, uint32_t* __restrict__ dst,
                               uint32_t* __restrict__ flags, uint32_t or_bits, uint32_t need_bits, bool vel_blocks)
{
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (i >= count) return;
    const uint32_t slot = slot_of_entity[index ? index[i] : first + i];
    if (slot == kNone) return;
    // need_bits = kValid: Transform data and dirty marks go to slots that hold a Transform — not to a body whose entity lost its
    // Transform (there the position array is the body's origin, and nothing marks what does not exist)
    if (need_bits && (flags[slot] & need_bits) != need_bits) return;
    if (dst) {
        for (uint32_t k = 0; k < width; ++k) dst[vel_blocks ? vel_word(slot, k) : static_cast<uint64_t>(slot) * width + k] = stage[i * width + k];
    }
    if (flags && or_bits) flags[slot] |= or_bits;
}

__global__ void k_gather_rows(const uint32_t* __restrict__ slot_of_entity, const uint32_t* __restrict__ index,
                              uint64_t first, uint64_t count,
                              uint32_t width, const uint32_t* __restrict__ src, uint32_t* __restrict__ stage, bool vel_blocks)
{
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (i >= count) return;
    const uint32_t slot = slot_of_entity[index ? index[i] : first + i];
    for (uint32_t k = 0; k < width; ++k) {
        stage[i * width + k] = slot == kNone ? 0u : src[vel_blocks ? vel_word(slot, k) : static_cast<uint64_t>(slot) * width + k];
    }
}

// k_gather_rows of the world matrices with the deferred translation rows composed (launch_gather_world).  A slot without a
// Transform (a body kept without one) has no row the tick would have stored: memory as it is.
__global__ void k_gather_world(const uint32_t* __restrict__ slot_of_entity, const uint32_t* __restrict__ index, uint64_t first, uint64_t count,
                               const float4* __restrict__ world, const uint32_t* __restrict__ flags, Row3View d, float4* __restrict__ stage)
{
    const uint64_t t = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    const uint64_t i = t >> 2;
    if (i >= count) return;
    const uint32_t r = static_cast<uint32_t>(t & 3u);
    const uint32_t slot = slot_of_entity[index ? index[i] : first + i];
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (slot != kNone) {
        v = (r == 3u && (flags[slot] & kValid)) ? world_row3(world, slot, d.pos, row3_deferred(slot, d.rs_word, d.epoch)) : world[4ull * slot + r];
    }
    stage[t] = v;
}

// The deferred translation rows into memory: one workgroup per tile, the wave's rows word through a wave-uniform address as in k_tick.
// What a deferring tick skipped, lane for lane: valid slots of waves whose word equals `epoch` get row 3 = (pos, 1).
__global__ void __launch_bounds__(kTile) k_row3_sync(WorldView w, uint32_t epoch)
{
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (w.rs_word[4u * (blockIdx.x * 4u + wave)] != epoch) return;
    const uint32_t slot = blockIdx.x * kTile + threadIdx.x;
    if (!(w.flags[slot] & kValid)) return;
    const F3 x = ld3(w.pos, slot);
    reinterpret_cast<float4*>(w.world)[4ull * slot + 3u] = make_float4(x.x, x.y, x.z, 1.0f);
}

// Body upload: type/shape bits + dirty, inverse mass, AABB half extents, group/mask.
__global__ void k_scatter_bodies(const uint32_t* __restrict__ slot_of_entity, const uint32_t* __restrict__ index,
                                 uint64_t first, uint64_t count,
                                 const uint32_t* __restrict__ type_bits, const float* __restrict__ inv_mass,
                                 const float* __restrict__ half_extent3, const uint32_t* __restrict__ group,
                                 const uint32_t* __restrict__ mask, const uint32_t* __restrict__ filter_class, WorldView w,
                                 const float* __restrict__ cdims3, const float* __restrict__ cmass, const uint32_t* __restrict__ cbits)
{
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (i >= count) return;
    const uint32_t slot = slot_of_entity[index ? index[i] : first + i];
    if (slot == kNone) return;
    // a body whose entity has no Transform is never re-created (EnsureRigidBody returns first): only its removal reaches it
    if (!(w.flags[slot] & kValid) && (type_bits[i] & kTypeMask) != 0) return;
    if (cdims3) {
        // a (re)created body starts without contacts: removeRigidBody dropped its pair with the ground and the manifold with it
        w.cshape[slot] = make_float4(cdims3[3 * i], cdims3[3 * i + 1], cdims3[3 * i + 2], 0.0f);
        w.cmass[slot] = cmass[i];
        w.cinfo[slot] = cbits[i];
    }
    w.filter_class[slot] = filter_class[i];
    uint32_t f = w.flags[slot];
    // a (re)created body is ACTIVE_TAG with its timer at zero.  kSpin stays: the body is re-created by the next physics tick
    // (EnsureRigidBody), whose re-pose rule zeroes the angular velocity record and takes the bit away
    f &= ~(kTypeMask | kBDirty | kMassMask | kDrowsy);
    f |= type_bits[i]; // body type, kBDirty and the mass class
    if ((f & kTypeMask) == 0) f &= ~kSpin;
    w.flags[slot] = f;
    w.inv_mass[slot] = inv_mass[i];
    w.half_extent[3ull * slot + 0] = half_extent3[3 * i + 0];
    w.half_extent[3ull * slot + 1] = half_extent3[3 * i + 1];
    w.half_extent[3ull * slot + 2] = half_extent3[3 * i + 2];
    w.group[slot] = group[i];
    w.mask[slot] = mask[i];
    if ((f & kTypeMask) == 0) {
        // body removed: forget its state
        st_vel(w.vel, slot, F3{0.0f, 0.0f, 0.0f});
        w.angvel[3ull * slot] = w.angvel[3ull * slot + 1] = w.angvel[3ull * slot + 2] = 0.0f;
    }
}

__global__ void k_scatter_velocities(const uint32_t* __restrict__ slot_of_entity, uint64_t first, uint64_t count,
                                     const float* __restrict__ lin, const float* __restrict__ ang, WorldView w)
{
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (i >= count) return;
    const uint32_t slot = slot_of_entity[first + i];
    if (slot == kNone) return;
    uint32_t f = w.flags[slot];
    if ((f & kTypeMask) != 2u) return; // only Dynamic bodies carry velocity
    if (lin) {
        st_vel(w.vel, slot, F3{lin[3 * i + 0], lin[3 * i + 1], lin[3 * i + 2]});
    }
    if (ang) {
        const float ax = ang[3 * i + 0], ay = ang[3 * i + 1], az = ang[3 * i + 2];
        w.angvel[3ull * slot + 0] = ax;
        w.angvel[3ull * slot + 1] = ay;
        w.angvel[3ull * slot + 2] = az;
        const uint32_t nf = (ax != 0.0f || ay != 0.0f || az != 0.0f) ? (f | kSpin) : (f & ~kSpin);
        if (nf != f) w.flags[slot] = nf;
    }
}

__global__ void k_init_slots(uint64_t n_slots, const uint32_t* __restrict__ structural_flags, WorldView w)
{
    const uint64_t s = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (s >= n_slots) return;
    const uint32_t sf = structural_flags[s];
    w.flags[s] = (sf & kValid) ? (sf | kTDirty) : sf; // Transform::Transform(): dirty = true
    w.pos[3 * s] = w.pos[3 * s + 1] = w.pos[3 * s + 2] = 0.0f;
    w.euler[3 * s] = w.euler[3 * s + 1] = w.euler[3 * s + 2] = 0.0f;
    w.scale[3 * s] = w.scale[3 * s + 1] = w.scale[3 * s + 2] = 1.0f;
    st_vel(w.vel, static_cast<uint32_t>(s), F3{0.0f, 0.0f, 0.0f});
    w.angvel[3 * s] = w.angvel[3 * s + 1] = w.angvel[3 * s + 2] = 0.0f;
    w.quat[4 * s] = w.quat[4 * s + 1] = w.quat[4 * s + 2] = 0.0f;
    w.quat[4 * s + 3] = 1.0f;
    w.inv_mass[s] = 0.0f;
    w.deact[s] = 0u;
    w.half_extent[3 * s] = w.half_extent[3 * s + 1] = w.half_extent[3 * s + 2] = 0.5f;
    w.group[s] = 1u;
    w.mask[s] = 0xffffffffu;
    w.filter_class[s] = 0u;
    w.cshape[s] = make_float4(0.5f, 0.5f, 0.5f, 0.0f);
    w.cmass[s] = 0.0f;
    w.cfriction[s] = 0.5f; // RigidBody::friction default (src/ecs/PhysicsComponents.h:32)
    w.crestitution[s] = 0.0f; // RigidBody::restitution default (:33)
    w.cinfo[s] = kCiGroundMask;
    // mtxIdentity(local), mtxIdentity(world)
    for (int k = 0; k < 16; ++k) w.world[16 * s + k] = (k % 5 == 0) ? 1.0f : 0.0f;
    for (int k = 0; k < 6; ++k) w.aabb[6 * s + k] = 0.0f;
}

// Scene::CountDirtyTransforms: per-lane predicate -> wave ballot popcount -> one atomic per wave.
__global__ void k_count_dirty(uint64_t n_slots, const uint32_t* __restrict__ flags, unsigned long long* __restrict__ out)
{
    uint64_t s = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    unsigned long long local = 0;
    for (; s < n_slots; s += stride) {
        const uint32_t f = flags[s];
        local += ((f & kValid) && (f & kTDirty)) ? 1ull : 0ull;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) local += __shfl_down(local, off, 64);
    if ((threadIdx.x & 63u) == 0 && local) atomicAdd(out, local);
}

__global__ void k_dirty_bytes(const uint32_t* __restrict__ slot_of_entity, uint64_t first, uint64_t count,
                              const uint32_t* __restrict__ flags, uint8_t* __restrict__ out)
{
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (i >= count) return;
    const uint32_t slot = slot_of_entity[first + i];
    out[i] = (slot != kNone && (flags[slot] & kTDirty)) ? 1 : 0;
}

// Compact root rows (12 floats, see store_root): 3 lanes per root, 16 B each.
// (a root's slot holds a Transform: its deferred translation row is composed, Row3View)
__global__ void k_pack_roots_compact(uint64_t n_roots, const uint32_t* __restrict__ root_slots, const float* __restrict__ world, Row3View d,
                                     float4* __restrict__ dst)
{
    const uint64_t t = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    const uint64_t r = t / 3;
    if (r >= n_roots) return;
    const uint32_t q = static_cast<uint32_t>(t - 3 * r);
    const uint32_t slot = root_slots[r];
    const float* m = world + 16ull * slot;
    float v[4];
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t cidx = 4u * q + k; // position in the compact row -> element of the 4x4 (skip column 3)
        v[k] = m[cidx + cidx / 3u];
    }
    if (q == 2u) { // compact floats 9..11 are m[12..14]
        const float4 r3 = world_row3(reinterpret_cast<const float4*>(world), slot, d.pos, row3_deferred(slot, d.rs_word, d.epoch));
        v[1] = r3.x;
        v[2] = r3.y;
        v[3] = r3.z;
    }
    dst[t] = make_float4(v[0], v[1], v[2], v[3]);
}

// Full 4x4 rows (the torch.distributed path of sharding.RootTable): 4 lanes per root, 16 B each.
__global__ void k_pack_roots(uint64_t n_roots, const uint32_t* __restrict__ root_slots, const float4* __restrict__ world, Row3View d,
                             float4* __restrict__ dst)
{
    const uint64_t t = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    const uint64_t r = t >> 2;
    if (r >= n_roots) return;
    const uint32_t slot = root_slots[r];
    dst[t] = (t & 3u) == 3u ? world_row3(world, slot, d.pos, row3_deferred(slot, d.rs_word, d.epoch)) : world[4ull * slot + (t & 3u)];
}

// ---- trigger volumes (ghost objects): AABB of the ghost at its entity's Transform, taken BEFORE the tick integrates
// (EnsureTrigger sets the ghost's pose at the start of PhysicsSystem::Update, src/physics/PhysicsSystem.cpp:575)
__global__ void k_trigger_aabb(uint32_t n_triggers, TriggerView t, WorldView w)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_triggers) return;
    const uint32_t slot = t.slot[i];
    float* bb = t.aabb + 6ull * i;
    if (slot == kFrozenGhost) return; // posed for the last time before its entity lost its Transform
    if (slot == kNone || !t.active[i]) {
        // an inactive ghost is not in the world: an empty box never overlaps
        bb[0] = bb[1] = bb[2] = INFINITY;
        bb[3] = bb[4] = bb[5] = -INFINITY;
        return;
    }
    const F3 pos = ld3(w.pos, slot);
    const F3 eul = ld3(w.euler, slot);
    const F3 he = ld3(t.half_extent, i);
    const Q4 q = bt_quat_from_transform_euler(eul);
    const M3 r = bt_mat_from_quat(q);
    float mn[3], mx[3];
    bt_aabb_of_pose(pos, r, he, mn, mx);
    for (int a = 0; a < 3; ++a) {
        bb[a] = mn[a];
        bb[3 + a] = mx[a];
    }
    float* ps = t.pose + 8ull * i;
    ps[0] = pos.x;
    ps[1] = pos.y;
    ps[2] = pos.z;
    ps[3] = 0.0f;
    ps[4] = q.x;
    ps[5] = q.y;
    ps[6] = q.z;
    ps[7] = q.w;
}

// every body against every trigger (scenes carry a handful of triggers; n_bodies x n_triggers box tests); hits are
// ballot-compacted per wave and appended behind one atomic per wave and trigger.  With `list` only the list[0 .. *list_count)
// triggers are tested: the ones Broadphase::query_boxes left over (boxes that span too much of the grid to walk it).
__global__ void __launch_bounds__(256) k_trigger_pairs(uint64_t n_slots, uint32_t n_triggers, TriggerView t, WorldView w,
                                                       const uint32_t* __restrict__ entity_of_slot, uint32_t* __restrict__ count,
                                                       uint2* __restrict__ out, uint32_t cap, const uint32_t* __restrict__ list,
                                                       const uint32_t* __restrict__ list_count)
{
    const uint32_t n_tested = list ? *list_count : n_triggers;
    if (n_tested == 0) return;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    const uint64_t first = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    const uint64_t rounds = (n_slots + stride - 1) / stride; // uniform trip count: the ballot needs every lane
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t r = 0; r < rounds; ++r) {
        const uint64_t s = first + r * stride;
        bool body = false;
        float bmn[3] = {0, 0, 0}, bmx[3] = {0, 0, 0};
        uint32_t grp = 0, msk = 0, ent = 0;
        if (s < n_slots) {
            const uint32_t f = w.flags[s];
            // every rigid body of whatever type: Bullet's pair cache pairs the ghost with Static bodies too (the reference hands
            // Bullet custom groups, PhysicsSystem.cpp:473,577; oracle/physics_ref.h has the reasoning)
            body = (f & kTypeMask) != 0u; // (with or without a Transform: an orphaned body is still in the world)
            if (body) {
                const float* b = w.aabb + 6 * s;
                for (int a = 0; a < 3; ++a) {
                    bmn[a] = b[a];
                    bmx[a] = b[3 + a];
                }
                grp = w.group[s];
                msk = w.mask[s];
                ent = entity_of_slot[s];
            }
        }
        for (uint32_t k = 0; k < n_tested; ++k) {
            const uint32_t i = list ? list[k] : k;
            const float* tb = t.aabb + 6ull * i;
            bool hit = body && ent != t.entity[i] && (t.group[i] & msk) != 0 && (grp & t.mask[i]) != 0;
            if (hit) {
                for (int a = 0; a < 3; ++a) hit = hit && tb[a] <= bmx[a] && tb[3 + a] >= bmn[a];
            }
            const unsigned long long m = __ballot(hit);
            if (m == 0) continue;
            const uint32_t leader = static_cast<uint32_t>(__ffsll(static_cast<long long>(m))) - 1u;
            uint32_t base = 0;
            if (lane == leader) base = atomicAdd(count, static_cast<uint32_t>(__popcll(m)));
            base = __shfl(base, static_cast<int>(leader), 64);
            if (hit) {
                const uint32_t at = base + static_cast<uint32_t>(__popcll(m & ((1ull << lane) - 1ull)));
                if (at < cap) out[at] = make_uint2(i, ent);
            }
        }
    }
}

// every ghost against every other ghost: both are registered collision objects, so the pair cache lists each in the other
// (btGhostPairCallback::addOverlappingPair serves both proxies).  Workgroup (x, y): the 256 ghosts i of tile x, one per thread,
// against the 64 ghosts j of tile y, which pass through LDS (one thread per i looping over ALL j took 352 us at 1000 ghosts: four
// workgroups, a thousand dependent trips each); a hit is (i | kGhostHit, j) — trigger INDICES, the host maps j to its entity and
// knows whether j is still in the world when i is processed (a one-shot ghost that fired earlier in ProcessTriggerEvents' loop is
// not).  An inactive ghost carries an empty box and overlaps nothing.
constexpr uint32_t kGhostTileJ = 64;
__global__ void __launch_bounds__(256) k_trigger_ghost_pairs(uint32_t n_triggers, TriggerView t, uint32_t* __restrict__ count,
                                                             uint2* __restrict__ out, uint32_t cap)
{
    __shared__ float s_box[kGhostTileJ][6];
    __shared__ uint32_t s_group[kGhostTileJ], s_mask[kGhostTileJ];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    float b[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    uint32_t grp = 0, msk = 0;
    if (i < n_triggers) {
#pragma unroll
        for (int a = 0; a < 6; ++a) b[a] = t.aabb[6ull * i + a];
        grp = t.group[i];
        msk = t.mask[i];
    }
    const uint32_t j0 = blockIdx.y * kGhostTileJ;
    const uint32_t jl = j0 + threadIdx.x;
    if (threadIdx.x < kGhostTileJ && jl < n_triggers) {
#pragma unroll
        for (int a = 0; a < 6; ++a) s_box[threadIdx.x][a] = t.aabb[6ull * jl + a];
        s_group[threadIdx.x] = t.group[jl];
        s_mask[threadIdx.x] = t.mask[jl];
    }
    __syncthreads();
    const uint32_t nj = min(kGhostTileJ, n_triggers - j0); // (uniform trip count: the ballots need every lane)
    for (uint32_t k = 0; k < nj; ++k) {
        const uint32_t j = j0 + k;
        bool hit = i < n_triggers && j != i && (grp & s_mask[k]) != 0u && (s_group[k] & msk) != 0u;
        if (hit) {
#pragma unroll
            for (int a = 0; a < 3; ++a) hit = hit && b[a] <= s_box[k][3 + a] && b[3 + a] >= s_box[k][a];
        }
        const unsigned long long m = __ballot(hit);
        if (m == 0) continue;
        const uint32_t leader = static_cast<uint32_t>(__ffsll(static_cast<long long>(m))) - 1u;
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(count, static_cast<uint32_t>(__popcll(m)));
        base = __shfl(base, static_cast<int>(leader), 64);
        if (hit) {
            const uint32_t at = base + static_cast<uint32_t>(__popcll(m & ((1ull << lane) - 1ull)));
            if (at < cap) out[at] = make_uint2(i | kGhostHit, j);
        }
    }
}

inline dim3 grid_for(uint64_t n, uint32_t block) { return dim3(static_cast<uint32_t>((n + block - 1) / block)); }

} // namespace

// ------------------------------------------------------------------ launch wrappers
static_assert(kTickPhysics == BGE_TICK_PHYSICS && kTickTransforms == BGE_TICK_TRANSFORMS && kTickAabb == (BGE_TICK_BROADPHASE | BGE_TICK_AABBS) &&
              kTickNormal == BGE_TICK_NORMAL_MATRICES && kTickBasis == BGE_TICK_BULLET_BASIS, "bge_kernels.hpp names the bits of bge_tick_flags");
hipError_t launch_tick(hipStream_t stream, const WorldView& w, const TickParams& p, uint32_t n_tiles, uint32_t flags)
{
    if (n_tiles == 0) return hipSuccess;
    const bool phys = (flags & kTickPhysics) != 0, xform = (flags & kTickTransforms) != 0, aabb = (flags & kTickAabb) != 0, normal = (flags & kTickNormal) != 0;
    const dim3 grid(n_tiles), block(kTile);
    const bool basis = phys && (flags & kTickBasis) != 0;
    if (p.n_solo > 1u) {
        // a solo group: the variant exists for the physics + transform tick alone, and a launch that asks for another is an error
        if (!phys || !tick_variant_has_rows_path(xform, aabb, normal, basis) || p.serial != 0u || p.n_left != 1u) return hipErrorInvalidValue;
        hipLaunchKernelGGL((k_tick<true, true, false, false, false, true>), grid, block, 0, stream, w, p);
        return hipGetLastError();
    }
#define BGE_LAUNCH(P, X, A, N)                                                                      \
    do {                                                                                            \
        if (basis) hipLaunchKernelGGL((k_tick<P, X, A, N, P>), grid, block, 0, stream, w, p);       \
        else hipLaunchKernelGGL((k_tick<P, X, A, N, false>), grid, block, 0, stream, w, p);         \
    } while (0)
    if (normal && xform) {
        if (phys && aabb) BGE_LAUNCH(true, true, true, true);
        else if (phys) BGE_LAUNCH(true, true, false, true);
        else BGE_LAUNCH(false, true, false, true);
    } else if (phys && xform && aabb) BGE_LAUNCH(true, true, true, false);
    else if (phys && xform) BGE_LAUNCH(true, true, false, false);
    else if (phys && aabb) BGE_LAUNCH(true, false, true, false);
    else if (phys) BGE_LAUNCH(true, false, false, false);
    else if (xform) BGE_LAUNCH(false, true, false, false);
#undef BGE_LAUNCH
    return hipGetLastError();
}

hipError_t launch_pose_only(hipStream_t stream, const WorldView& w, uint64_t n_slots, bool bullet_basis)
{
    if (n_slots == 0) return hipSuccess;
    if (bullet_basis) hipLaunchKernelGGL(k_pose_only<true>, grid_for(n_slots, 256), dim3(256), 0, stream, w, n_slots);
    else hipLaunchKernelGGL(k_pose_only<false>, grid_for(n_slots, 256), dim3(256), 0, stream, w, n_slots);
    return hipGetLastError();
}

hipError_t launch_scatter_rows(hipStream_t stream, const uint32_t* slot_of_entity, uint64_t first, uint64_t count,
                               uint32_t width, const void* stage, void* dst, uint32_t* flags, uint32_t or_bits,
                               const uint32_t* index, uint32_t need_bits, bool vel_blocks)
{
    if (count == 0) return hipSuccess;
    if (vel_blocks && width != 3) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_scatter_rows, grid_for(count, 256), dim3(256), 0, stream, slot_of_entity, index, first, count, width,
                       static_cast<const uint32_t*>(stage), static_cast<uint32_t*>(dst), flags, or_bits, need_bits, vel_blocks);
    return hipGetLastError();
}

hipError_t launch_gather_rows(hipStream_t stream, const uint32_t* slot_of_entity, uint64_t first, uint64_t count,
                              uint32_t width, const void* src, void* stage, const uint32_t* index, bool vel_blocks)
{
    if (count == 0) return hipSuccess;
    if (vel_blocks && width != 3) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_gather_rows, grid_for(count, 256), dim3(256), 0, stream, slot_of_entity, index, first, count, width,
                       static_cast<const uint32_t*>(src), static_cast<uint32_t*>(stage), vel_blocks);
    return hipGetLastError();
}

hipError_t launch_gather_world(hipStream_t stream, const uint32_t* slot_of_entity, uint64_t first, uint64_t count, const WorldView& w,
                               const Row3View& d, void* stage, const uint32_t* index)
{
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(k_gather_world, grid_for(count * 4, 256), dim3(256), 0, stream, slot_of_entity, index, first, count,
                       reinterpret_cast<const float4*>(w.world), w.flags, d, static_cast<float4*>(stage));
    return hipGetLastError();
}

hipError_t launch_scatter_bodies(hipStream_t stream, const uint32_t* slot_of_entity, uint64_t first, uint64_t count,
                                 const uint32_t* type_bits, const float* inv_mass, const float* half_extent3,
                                 const uint32_t* group, const uint32_t* mask, const uint32_t* filter_class, const WorldView& w,
                                 const uint32_t* index, const float* cdims3, const float* cmass, const uint32_t* cbits)
{
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(k_scatter_bodies, grid_for(count, 256), dim3(256), 0, stream, slot_of_entity, index, first, count,
                       type_bits, inv_mass, half_extent3, group, mask, filter_class, w, cdims3, cmass, cbits);
    return hipGetLastError();
}

hipError_t launch_scatter_velocities(hipStream_t stream, const uint32_t* slot_of_entity, uint64_t first, uint64_t count,
                                     const float* lin, const float* ang, const WorldView& w)
{
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(k_scatter_velocities, grid_for(count, 256), dim3(256), 0, stream, slot_of_entity, first, count,
                       lin, ang, w);
    return hipGetLastError();
}

hipError_t launch_init_slots(hipStream_t stream, uint64_t n_slots, const uint32_t* structural_flags, const WorldView& w)
{
    if (n_slots == 0) return hipSuccess;
    hipLaunchKernelGGL(k_init_slots, grid_for(n_slots, 256), dim3(256), 0, stream, n_slots, structural_flags, w);
    return hipGetLastError();
}

hipError_t launch_count_dirty(hipStream_t stream, uint64_t n_slots, const uint32_t* flags, unsigned long long* out)
{
    if (n_slots == 0) return hipSuccess;
    const uint64_t blocks = (n_slots + 255) / 256;
    hipLaunchKernelGGL(k_count_dirty, dim3(static_cast<uint32_t>(blocks < 2048 ? blocks : 2048)), dim3(256), 0, stream,
                       n_slots, flags, out);
    return hipGetLastError();
}

hipError_t launch_dirty_bytes(hipStream_t stream, const uint32_t* slot_of_entity, uint64_t first, uint64_t count,
                              const uint32_t* flags, uint8_t* out)
{
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(k_dirty_bytes, grid_for(count, 256), dim3(256), 0, stream, slot_of_entity, first, count, flags, out);
    return hipGetLastError();
}

hipError_t launch_trigger_aabb(hipStream_t stream, uint32_t n_triggers, const TriggerView& t, const WorldView& w)
{
    if (n_triggers == 0) return hipSuccess;
    hipLaunchKernelGGL(k_trigger_aabb, grid_for(n_triggers, 64), dim3(64), 0, stream, n_triggers, t, w);
    return hipGetLastError();
}

hipError_t launch_trigger_pairs(hipStream_t stream, uint64_t n_slots, uint32_t n_triggers, const TriggerView& t, const WorldView& w,
                                const uint32_t* entity_of_slot, uint32_t* count, void* out_pairs, uint32_t cap, const uint32_t* list,
                                const uint32_t* list_count)
{
    if (n_triggers == 0 || n_slots == 0) return hipSuccess;
    const uint64_t blocks = (n_slots + 255) / 256;
    hipLaunchKernelGGL(k_trigger_pairs, dim3(static_cast<uint32_t>(blocks < 2048 ? blocks : 2048)), dim3(256), 0, stream, n_slots,
                       n_triggers, t, w, entity_of_slot, count, static_cast<uint2*>(out_pairs), cap, list, list_count);
    return hipGetLastError();
}

// ---- trigger overlap diff (bge_kernels.hpp TriggerDiff)
namespace {
constexpr uint32_t kTrigProbeLimit = 4096;

__device__ __forceinline__ uint32_t trig_hash(uint64_t key, uint32_t log2_cap)
{
    return static_cast<uint32_t>((key * 0x9E3779B97F4A7C15ull) >> (64u - log2_cap));
}

// 0 = was there already, 1 = inserted, 2 = no room within the probe limit
__device__ __forceinline__ int trig_insert(uint64_t* table, uint32_t log2_cap, uint64_t key)
{
    const uint32_t mask = (1u << log2_cap) - 1u;
    uint32_t h = trig_hash(key, log2_cap);
    for (uint32_t probe = 0; probe < kTrigProbeLimit; ++probe) {
        const unsigned long long old = atomicCAS(reinterpret_cast<unsigned long long*>(table + h), static_cast<unsigned long long>(kTrigKeyEmpty),
                                                 static_cast<unsigned long long>(key));
        if (old == kTrigKeyEmpty) return 1;
        if (old == key) return 0;
        h = (h + 1u) & mask;
    }
    return 2;
}

__device__ __forceinline__ bool trig_contains(const uint64_t* table, uint32_t log2_cap, uint64_t key)
{
    const uint32_t mask = (1u << log2_cap) - 1u;
    uint32_t h = trig_hash(key, log2_cap);
    for (uint32_t probe = 0; probe <= mask; ++probe) {
        const uint64_t k = table[h];
        if (k == key) return true;
        if (k == kTrigKeyEmpty) return false;
        h = (h + 1u) & mask;
    }
    return false;
}

__device__ __forceinline__ void trig_append(const TriggerDiff& d, bool mine, uint64_t record)
{
    const unsigned long long m = __ballot(mine);
    if (m == 0ull) return;
    const int lane = static_cast<int>(threadIdx.x & 63u);
    uint32_t base = 0;
    if (lane == __ffsll(static_cast<long long>(m)) - 1) base = atomicAdd(d.header + 0, static_cast<uint32_t>(__popcll(m)));
    base = __shfl(base, __ffsll(static_cast<long long>(m)) - 1);
    if (mine) {
        const uint32_t at = base + static_cast<uint32_t>(__popcll(m & ((1ull << lane) - 1ull)));
        if (at < d.delta_cap) d.deltas[at] = record;
    }
}

// this tick's hits into the current table; the ones last tick's table does not hold are Enters
__global__ void __launch_bounds__(256) k_trigger_diff_cur(TriggerDiff d)
{
    const uint32_t hits = d.count[0];
    const uint32_t n = hits < d.pair_cap ? hits : d.pair_cap;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        d.header[3] = hits;
        d.header[4] = d.count[1];
        d.header[5] = d.count[2];
    }
    const uint32_t stride = gridDim.x * blockDim.x;
    const uint32_t rounds = (n + stride - 1u) / stride; // every lane of a wave makes the same number of trips (ballots inside)
    for (uint32_t r = 0; r < rounds; ++r) {
        const uint32_t k = r * stride + blockIdx.x * blockDim.x + threadIdx.x;
        bool fresh = false, enter = false;
        uint64_t key = 0;
        if (k < n) {
            const uint2 hit = d.pairs[k];
            key = (static_cast<uint64_t>(hit.x & ~kGhostHit) << 33) | ((hit.x & kGhostHit) ? (1ull << 32) : 0ull) | hit.y;
            const int how = trig_insert(d.cur, d.log2_cap, key);
            if (how == 2) d.header[2] = 1u;
            fresh = how == 1;
            enter = fresh && !trig_contains(d.prev, d.log2_cap, key);
        }
        const unsigned long long f = __ballot(fresh);
        if ((threadIdx.x & 63u) == 0u && f) atomicAdd(d.header + 1, static_cast<uint32_t>(__popcll(f)));
        trig_append(d, enter, key);
    }
}

// last tick's keys that this tick's table does not hold are Exits
__global__ void __launch_bounds__(256) k_trigger_diff_prev(TriggerDiff d)
{
    const uint32_t cap = 1u << d.log2_cap;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t base = 0; base < cap; base += stride) {
        const uint32_t slot = base + blockIdx.x * blockDim.x + threadIdx.x;
        uint64_t key = kTrigKeyEmpty;
        if (slot < cap) key = d.prev[slot];
        const bool gone = key != kTrigKeyEmpty && !trig_contains(d.cur, d.log2_cap, key);
        trig_append(d, gone, key | kTrigKeyExit);
    }
}

__global__ void __launch_bounds__(256) k_trigger_table_build(uint64_t* table, uint32_t log2_cap, const uint64_t* keys, uint32_t n, uint32_t* header)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n && trig_insert(table, log2_cap, keys[k]) == 2) header[2] = 1u;
}
} // namespace

hipError_t launch_trigger_diff(hipStream_t stream, const TriggerDiff& d)
{
    hipLaunchKernelGGL(k_trigger_diff_cur, dim3(256), dim3(256), 0, stream, d);
    hipLaunchKernelGGL(k_trigger_diff_prev, dim3(256), dim3(256), 0, stream, d);
    return hipGetLastError();
}

hipError_t launch_trigger_table_build(hipStream_t stream, uint64_t* table, uint32_t log2_cap, const uint64_t* keys, uint32_t n, uint32_t* header)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_trigger_table_build, grid_for(n, 256), dim3(256), 0, stream, table, log2_cap, keys, n, header);
    return hipGetLastError();
}

hipError_t launch_trigger_ghost_pairs(hipStream_t stream, uint32_t n_triggers, const TriggerView& t, uint32_t* count, void* out_pairs,
                                      uint32_t cap)
{
    if (n_triggers < 2) return hipSuccess;
    hipLaunchKernelGGL(k_trigger_ghost_pairs, dim3((n_triggers + 255u) / 256u, (n_triggers + kGhostTileJ - 1u) / kGhostTileJ), dim3(256), 0, stream,
                       n_triggers, t, count, static_cast<uint2*>(out_pairs), cap);
    return hipGetLastError();
}

hipError_t launch_pack_roots(hipStream_t stream, uint64_t n_roots, const uint32_t* root_slots, const float* world, const Row3View& d,
                             float* dst, bool compact)
{
    if (n_roots == 0) return hipSuccess;
    if (compact) {
        hipLaunchKernelGGL(k_pack_roots_compact, grid_for(n_roots * 3, 256), dim3(256), 0, stream, n_roots, root_slots, world, d,
                           reinterpret_cast<float4*>(dst));
    } else {
        hipLaunchKernelGGL(k_pack_roots, grid_for(n_roots * 4, 256), dim3(256), 0, stream, n_roots, root_slots,
                           reinterpret_cast<const float4*>(world), d, reinterpret_cast<float4*>(dst));
    }
    return hipGetLastError();
}

hipError_t launch_row3_sync(hipStream_t stream, const WorldView& w, uint32_t n_tiles, uint32_t epoch)
{
    if (n_tiles == 0 || epoch == 0u) return hipSuccess;
    hipLaunchKernelGGL(k_row3_sync, dim3(n_tiles), dim3(kTile), 0, stream, w, epoch);
    return hipGetLastError();
}

} // namespace bge
