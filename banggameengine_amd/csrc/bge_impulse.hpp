// bge_impulse.hpp — impulses on Dynamic bodies and the characters' push (bge_impulse.hip; include/bge_world.h "Impulses",
// "Character push").  One enqueue applies a batch of bge_impulse records that lies in the caller's device memory
// or in the character set's push records: keys, a stable sort, one serial walk per body.  The host enqueues the launches on the
// world's stream and reads nothing in between.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "bge_kernels.hpp"

namespace bge {

struct ImpulseParams {
    const uint32_t* records;        // [n] bge_impulse (4-byte aligned, moved word by word)
    uint32_t* status;               // [n] or NULL
    uint32_t n;
    uint64_t n_entities;
    const uint32_t* slot_of_entity; // [n_entities]
    // key = slot of the record's body (all ones: skipped), value = record index; sorted by key, stable
    uint32_t* keys_in;
    uint32_t* keys_out;
    uint32_t* vals_in;
    uint32_t* vals_out;
    void* sort_tmp;                 // hipcub's temporary storage
    size_t sort_bytes;
};

// Push of one character step: the set's state and the desc in force -> one bge_impulse per character
struct CharPushParams {
    const uint32_t* state;          // [n] bge_character_state
    uint32_t* records;              // [n] bge_impulse
    uint32_t n;
    uint64_t n_entities;
    const uint32_t* slot_of_entity;
    float force, dt, max_normal_y;
    uint32_t body_mask;
};

// hipcub's temporary bytes for the sort of n (key, value) pairs
size_t impulse_sort_bytes(uint32_t n);
hipError_t launch_impulses(hipStream_t stream, const ImpulseParams& p, const WorldView& w);
hipError_t launch_char_push(hipStream_t stream, const CharPushParams& p, const WorldView& w);

} // namespace bge
