// bge_move.hpp — the kernels between the closest-hit passes of a batch of sphere moves (bge_move.hip; include/bge_world.h
// bge_world_sphere_move*).  A move is BGE_MOVE_SLIDES + 1 sphere-cast passes (bge_query.hpp launch_query) over
// cast and hit records in world-owned scratch; the host enqueues begin, then per round a pass and a step, then the probe's pass and
// finish, and reads nothing in between.
#pragma once

#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>

#include <cstdint>

namespace bge {

// The per-mover state: kMoveStatePlanes planes of n float4 each, plane k of mover i at state[k * n + i], so that a wave reads and
// writes 64 consecutive 16-byte words of one plane.
//   0  p.xyz, radius            1  r.xyz, skin             2  d0.xyz, layer mask (bits)
//   3  previous normal, bits    4  last hit normal, entity 5  probe distance, min ground ny, 0, 0
// bits of plane 3: flags in 0..7 (bge_move_flags), n_hits in 8..15, last hit kind in 16..17, has a previous normal 24, finished 25
constexpr uint32_t kMoveStatePlanes = 6;
constexpr uint64_t kMoveStateBytes = kMoveStatePlanes * 16ull;

struct MoveParams {
    const void* moves;   // [n] bge_sphere_move (device, 4-byte aligned)
    void* results;       // [n] bge_sphere_move_result (device, 4-byte aligned)
    float4* state;       // [kMoveStatePlanes][n]
    void* casts;         // [n] bge_sphere_cast: what the next pass asks (a finished or invalid mover: layer_mask 0, hits nothing)
    const void* hits;    // [n] bge_ray_hit: what the last pass answered
    uint32_t n;
};

hipError_t launch_move_begin(hipStream_t stream, const MoveParams& p);
// round = 0 .. BGE_MOVE_SLIDES - 1; the last one writes the probe's cast instead of a next round's
hipError_t launch_move_step(hipStream_t stream, const MoveParams& p, uint32_t round);
hipError_t launch_move_finish(hipStream_t stream, const MoveParams& p);

} // namespace bge
