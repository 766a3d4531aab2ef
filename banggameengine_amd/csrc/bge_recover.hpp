// bge_recover.hpp — the kernels between the penetration passes of a batch of sphere recoveries (bge_recover.hip;
// include/bge_world.h bge_world_sphere_recover*).  A recovery is BGE_RECOVER_ROUNDS + 1 penetration passes
// (bge_query.hpp launch_query, QueryKind::SpherePenetration) over query and hit records in world-owned scratch; the host enqueues
// begin, then per round a pass and a step, then the final check's pass and finish, and reads nothing in between.
#pragma once

#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>

#include <cstdint>

namespace bge {

// The per-sphere state: kRecoverStatePlanes planes of n float4 each, plane k of sphere i at state[k * n + i], so that a wave reads
// and writes 64 consecutive 16-byte words of one plane.
//   0  p.xyz, radius       1  last push: normal, depth       2  skin, layer mask (bits), bits, last push: entity (bits)
// bits of plane 2: flags in 0..7 (bge_recover_flags), n_pushes in 8..15, last push's kind in 16..17, finished 25
constexpr uint32_t kRecoverStatePlanes = 3;
constexpr uint64_t kRecoverStateBytes = kRecoverStatePlanes * 16ull;

struct RecoverParams {
    const void* records; // [n] bge_sphere_recover (device, 4-byte aligned)
    void* results;       // [n] bge_sphere_recover_result (device, 4-byte aligned)
    float4* state;       // [kRecoverStatePlanes][n]
    void* queries;       // [n] bge_sphere: what the next pass asks (a finished or invalid sphere: layer_mask 0, penetrates nothing)
    const void* hits;    // [n] bge_penetration_hit: what the last pass answered
    uint32_t n;
};

hipError_t launch_recover_begin(hipStream_t stream, const RecoverParams& p);
// after each of the BGE_RECOVER_ROUNDS passes; the query it writes after the last one is the final check's
hipError_t launch_recover_step(hipStream_t stream, const RecoverParams& p);
hipError_t launch_recover_finish(hipStream_t stream, const RecoverParams& p);

} // namespace bge
