// bge_character.hpp — the kernels between the recovery and the step move of a batch of sphere characters (bge_character.hip;
// include/bge_world.h "Characters", bge_world_characters_*).  A step of the set is: begin, a batch of sphere
// recoveries (bge_recover.hpp), move, a batch of sphere step moves (bge_step.hpp), finish.  The host enqueues them in that order on
// the world's stream and reads nothing in between; the characters see the world only through the two batches.
#pragma once

#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>

#include <cstdint>

namespace bge {

// scratch[i] of character i within one step: x = vv after Vertical (bits), y = kCharStepInvalid | kCharStepJumped
constexpr uint32_t kCharStepInvalid = 1u;
constexpr uint32_t kCharStepJumped = 2u;

struct CharacterParams {
    const void* desc;    // [n] bge_character_desc (resident, 4-byte aligned as every record below)
    void* input;         // [n] bge_character_input; k_char_begin clears the JUMP edge it consumed
    void* state;         // [n] bge_character_state: read by every kernel, written by k_char_finish alone
    void* recover_in;    // [n] bge_sphere_recover: written by k_char_begin
    const void* recover_out; // [n] bge_sphere_recover_result
    void* step_in;       // [n] bge_sphere_step_move: written by k_char_move
    const void* step_out;    // [n] bge_sphere_step_result
    uint2* scratch;      // [n]
    float dt;
    uint32_t n;
};

// first != 0: this is the first step of an update call, the one that reads and clears the JUMP edge
hipError_t launch_char_begin(hipStream_t stream, const CharacterParams& p, uint32_t first);
hipError_t launch_char_move(hipStream_t stream, const CharacterParams& p);
hipError_t launch_char_finish(hipStream_t stream, const CharacterParams& p);

} // namespace bge
