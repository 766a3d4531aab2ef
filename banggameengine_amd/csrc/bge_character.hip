// bge_character.hip — sphere characters: the state that persists between frames and the arithmetic that makes a recovery and a step
// move a controller (include/bge_world.h "Characters", bge_world_characters_*).
//
// A character sees the world only through bge_world_sphere_recover and bge_world_sphere_step_move, so a step of the set is a batch
// of each with three kernels around them, one thread per character, and they never look at a body:
//   k_char_begin   validates the input, consumes the JUMP edge on the first step of a call, writes the bge_sphere_recover record.
//   k_char_move    reads the recovery's result, runs Vertical (jump, gravity, the clamps), writes the bge_sphere_step_move record
//                  and the step's scratch (vv, invalid, jumped).
//   k_char_finish  reads the step move's result, runs Ground, Head and State, and writes the 80-byte state.
// An invalid character hands both batches a record with layer_mask = 0: by their own rules such a record is INVALID, asks nothing
// of any pass and comes back with its position echoed.  No loop, no LDS, no atomic; the records are only 4-byte aligned by their
// ABI and are moved word by word.  The expressions below are the header's, operation for operation (the build's
// -ffp-contract=off keeps one rounding each).
#include <hip/hip_runtime.h>

#include "../../include/bge_world.h"
#include "bge_character.hpp"

namespace bge {

namespace {

constexpr uint32_t kThreads = 256;
// words of the records (include/bge_world.h)
constexpr uint32_t kDescWords = 12, kInputWords = 4, kStateWords = 20;
constexpr uint32_t kRecoverWords = 7, kRecoverResultWords = 16, kStepWords = 12, kStepResultWords = 20;

__global__ void __launch_bounds__(kThreads) k_char_begin(CharacterParams p, uint32_t first)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= p.n) return;
    const uint32_t* d = static_cast<const uint32_t*>(p.desc) + uint64_t(kDescWords) * i;
    uint32_t* in = static_cast<uint32_t*>(p.input) + uint64_t(kInputWords) * i;
    const uint32_t* s = static_cast<const uint32_t*>(p.state) + uint64_t(kStateWords) * i;
    const bool valid = __builtin_isfinite(__uint_as_float(in[0])) && __builtin_isfinite(__uint_as_float(in[1]));
    uint32_t bits = valid ? 0u : kCharStepInvalid;
    if (first) { // the edge is read and cleared, whether or not it leads to a jump
        const uint32_t buttons = in[2];
        if (buttons & BGE_CHAR_BUTTON_JUMP) {
            bits |= kCharStepJumped; // (pressed; k_char_move makes it "jumped" where the character was on the ground)
            in[2] = buttons & ~uint32_t(BGE_CHAR_BUTTON_JUMP);
        }
    }
    p.scratch[i] = make_uint2(0u, bits);
    uint32_t* r = static_cast<uint32_t*>(p.recover_in) + uint64_t(kRecoverWords) * i;
    r[0] = s[0];
    r[1] = s[1];
    r[2] = s[2];
    r[3] = d[3];              // radius
    r[4] = d[4];              // skin
    r[5] = valid ? d[11] : 0u; // layer_mask: 0 asks nothing
    r[6] = 0u;
}

__global__ void __launch_bounds__(kThreads) k_char_move(CharacterParams p)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= p.n) return;
    const uint32_t* d = static_cast<const uint32_t*>(p.desc) + uint64_t(kDescWords) * i;
    const uint32_t* in = static_cast<const uint32_t*>(p.input) + uint64_t(kInputWords) * i;
    const uint32_t* s = static_cast<const uint32_t*>(p.state) + uint64_t(kStateWords) * i;
    const uint32_t* rr = static_cast<const uint32_t*>(p.recover_out) + uint64_t(kRecoverResultWords) * i;
    uint32_t bits = p.scratch[i].y;
    if (rr[6] & BGE_RECOVER_INVALID) bits |= kCharStepInvalid;
    const bool invalid = (bits & kCharStepInvalid) != 0u;
    // Vertical
    const bool was = (s[4] & BGE_CHAR_GROUNDED) != 0u;
    const bool jumped = (bits & kCharStepJumped) != 0u && was;
    const float jump_speed = __uint_as_float(d[9]);
    float vv = __uint_as_float(s[3]);
    float dy = 0.0f;
    bool walking = false;
    if (jumped) {
        vv = jump_speed;
    } else if (was) {
        vv = 0.0f;
        walking = true;
    }
    if (!walking) {
        const float fall_speed = __uint_as_float(d[10]);
        vv = vv - __uint_as_float(d[8]) * p.dt;
        if (vv > jump_speed) vv = jump_speed;
        if (vv < -fall_speed) vv = -fall_speed;
        dy = vv * p.dt;
    }
    bits = (bits & kCharStepInvalid) | (jumped ? kCharStepJumped : 0u);
    p.scratch[i] = make_uint2(__float_as_uint(vv), bits);
    // Move: from the recovered position
    uint32_t* m = static_cast<uint32_t*>(p.step_in) + uint64_t(kStepWords) * i;
    m[0] = rr[0];
    m[1] = rr[1];
    m[2] = rr[2];
    m[3] = in[0];
    m[4] = __float_as_uint(dy);
    m[5] = in[1];
    m[6] = d[3];               // radius
    m[7] = d[4];               // skin
    m[8] = d[7];               // probe_distance
    m[9] = d[6];               // min_ground_ny
    m[10] = invalid ? 0u : d[11];
    m[11] = walking ? d[5] : 0u; // step-up only while walking
}

__global__ void __launch_bounds__(kThreads) k_char_finish(CharacterParams p)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= p.n) return;
    const uint32_t* d = static_cast<const uint32_t*>(p.desc) + uint64_t(kDescWords) * i;
    uint32_t* s = static_cast<uint32_t*>(p.state) + uint64_t(kStateWords) * i;
    const uint32_t* rr = static_cast<const uint32_t*>(p.recover_out) + uint64_t(kRecoverResultWords) * i;
    const uint32_t* mr = static_cast<const uint32_t*>(p.step_out) + uint64_t(kStepResultWords) * i;
    const uint2 sc = p.scratch[i];
    const uint32_t old = s[4];
    const uint32_t steps = s[19] + 1u;
    if ((sc.y & kCharStepInvalid) || (mr[6] & BGE_MOVE_INVALID)) {
        // position, vv and GROUNDED stay as they were before the step
        s[4] = BGE_CHAR_INVALID | (old & BGE_CHAR_GROUNDED);
        s[5] = BGE_RAY_MISS;
        s[6] = BGE_RAY_NO_ENTITY;
        s[7] = s[8] = s[9] = 0u;
        s[10] = BGE_RAY_MISS;
        s[11] = BGE_RAY_NO_ENTITY;
        s[12] = s[13] = s[14] = 0u;
        s[15] = 0u;
        s[16] = s[17] = s[18] = 0u;
        s[19] = steps;
        return;
    }
    const bool was = (old & BGE_CHAR_GROUNDED) != 0u;
    float vv = __uint_as_float(sc.x);
    float qy = __uint_as_float(mr[1]);
    uint32_t flags = 0u;
    if (sc.y & kCharStepJumped) flags |= BGE_CHAR_JUMPED;
    if (rr[6] & BGE_RECOVER_MOVED) flags |= BGE_CHAR_RECOVERED;
    if (rr[6] & BGE_RECOVER_STUCK) flags |= BGE_CHAR_STUCK;
    if (mr[6] & BGE_MOVE_STEPPED) flags |= BGE_CHAR_STEPPED;
    if (mr[6] & BGE_MOVE_OUT_OF_SLIDES) flags |= BGE_CHAR_OUT_OF_SLIDES;
    // Ground
    const bool grounded = (mr[6] & BGE_MOVE_GROUNDED) != 0u && !(vv > 0.0f);
    if (grounded) {
        float e = __uint_as_float(mr[15]) - __uint_as_float(d[4]);
        if (!(e > 0.0f)) e = 0.0f;
        qy = qy - e;
        vv = 0.0f;
        flags |= BGE_CHAR_GROUNDED;
        if (!was) flags |= BGE_CHAR_LANDED;
    }
    // Head
    if (vv > 0.0f && mr[7] >= 1u && __uint_as_float(mr[11]) < 0.0f) {
        vv = 0.0f;
        flags |= BGE_CHAR_HEAD_BUMP;
    }
    s[0] = mr[0];
    s[1] = __float_as_uint(qy);
    s[2] = mr[2];
    s[3] = __float_as_uint(vv);
    s[4] = flags;
    s[5] = mr[13]; // ground_kind, ground_entity, ground_normal: the probe's, or its miss convention
    s[6] = mr[14];
    s[7] = mr[16];
    s[8] = mr[17];
    s[9] = mr[18];
    s[10] = mr[8]; // hit_kind, hit_entity, hit_normal
    s[11] = mr[9];
    s[12] = mr[10];
    s[13] = mr[11];
    s[14] = mr[12];
    s[15] = mr[19]; // step_rise
    s[16] = rr[3];  // recovered = R.pushed
    s[17] = rr[4];
    s[18] = rr[5];
    s[19] = steps;
}

dim3 grid_of(uint32_t n) { return dim3((n + kThreads - 1u) / kThreads); }

} // namespace

hipError_t launch_char_begin(hipStream_t stream, const CharacterParams& p, uint32_t first)
{
    if (p.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_char_begin, grid_of(p.n), dim3(kThreads), 0, stream, p, first);
    return hipGetLastError();
}

hipError_t launch_char_move(hipStream_t stream, const CharacterParams& p)
{
    if (p.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_char_move, grid_of(p.n), dim3(kThreads), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_char_finish(hipStream_t stream, const CharacterParams& p)
{
    if (p.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_char_finish, grid_of(p.n), dim3(kThreads), 0, stream, p);
    return hipGetLastError();
}

} // namespace bge
