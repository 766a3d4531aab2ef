// bge_ride.hpp — characters ride moving platforms: the resident ride records of the character set and the three kernels that
// keep them (bge_ride.hip; include/bge_world.h "Character platform riding", bge_world_characters_ride ..).  An
// update call with riding on is: carry, the steps as they are (bge_character.hpp), anchor.  The host enqueues them in that order
// on the world's stream and reads nothing in between.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace bge {

struct RideParams {
    void* state;                    // [n] bge_character_state: k_char_carry writes the position, k_char_anchor only reads
    void* ride;                     // [n] bge_character_ride (resident, 4-byte aligned, moved word by word)
    uint32_t n;                     // characters
    uint32_t dynamic;               // BGE_CHAR_RIDE_DYNAMIC: a Dynamic body is rideable too
    // bodies, as the queries see them (QueryParams names the same arrays)
    uint64_t n_entities, n_slots;
    const uint32_t* flags;          // [n_slots]
    const float* pos;               // [n_slots][3]
    const float* quat;              // [n_slots][4] xyzw
    const uint32_t* slot_of_entity; // [n_entities]
};

// Carry: once per update call, before its first step
hipError_t launch_char_carry(hipStream_t stream, const RideParams& p);
// Anchor: once per update call, after its last step
hipError_t launch_char_anchor(hipStream_t stream, const RideParams& p);
// clears the anchors whose entity lies in [first, first + count); only ride and n of the parameters are read
hipError_t launch_char_ride_forget(hipStream_t stream, void* ride, uint32_t n, uint64_t first, uint64_t count);

} // namespace bge
