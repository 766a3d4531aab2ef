// bge_step.hpp — the kernels between the closest-hit passes of a batch of sphere step moves (bge_step.hip; include/bge_world.h
// "Sphere step moves", bge_world_sphere_step_move*).  Every mover has two lanes that go through the same
// sphere-cast passes (bge_query.hpp launch_query): lane A, the plain slide, whose cast and hit records are at index i, and lane B,
// the step (Up, Forward, Down), whose records are at index n + i.  The host enqueues begin, then per pass the pass and an advance,
// then the probe's pass and finish, and reads nothing in between.
#pragma once

#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>

#include <cstdint>

namespace bge {

// The per-mover state: kStepStatePlanes planes of n float4 each, plane k of mover i at state[k * n + i], so that a wave reads and
// writes 64 consecutive 16-byte words of one plane.  Planes 0-4 are those of bge_move.hpp for lane A, 6-9 the same for lane B.
//   0  A p.xyz, radius          1  A r.xyz, skin           2  d0.xyz, layer mask (bits)
//   3  A previous normal, bits  4  A last hit normal, entity
//   5  probe distance, min ground ny, step height (after the selection: step_rise), u
//   6  B p.xyz, radius          7  B r.xyz, skin           8  B previous normal, bits   9  B last hit normal, entity
// bits as in bge_move.hpp (flags in 0..7, BGE_MOVE_STEP_TRIED and BGE_MOVE_STEPPED among them); lane B's word has the step-failed
// bit 26 in addition.
constexpr uint32_t kStepStatePlanes = 10;
constexpr uint64_t kStepStateBytes = kStepStatePlanes * 16ull;
// advance stages: 1 .. kStepStages - 1 follow passes 1 .. 5 (slide rounds of both lanes), kStepStages follows the Down pass (pass 6)
// and makes the selection
constexpr uint32_t kStepStages = 6;

struct StepParams {
    const void* moves;   // [n] bge_sphere_step_move (device, 4-byte aligned)
    void* results;       // [n] bge_sphere_step_result (device, 4-byte aligned)
    float4* state;       // [kStepStatePlanes][n]
    void* casts;         // [2n] bge_sphere_cast: what the next pass asks; lane A at i, lane B at n + i (layer_mask 0 asks nothing)
    const void* hits;    // [2n] bge_ray_hit: what the last pass answered
    uint32_t n;
};

hipError_t launch_step_begin(hipStream_t stream, const StepParams& p);
// stage = 1 .. kStepStages, after pass `stage`
hipError_t launch_step_advance(hipStream_t stream, const StepParams& p, uint32_t stage);
hipError_t launch_step_finish(hipStream_t stream, const StepParams& p);

} // namespace bge
