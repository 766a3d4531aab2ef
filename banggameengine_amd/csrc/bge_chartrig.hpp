// bge_chartrig.hpp — trigger events for the device's characters: the pair test of every character against every listed trigger
// ghost, the remembered overlap bitmaps and the ordered Enter / Stay / Exit list (bge_chartrig.hip; include/bge_world.h "Character
// trigger events", bge_world_characters_watch_triggers ..).  The host enqueues the passes in order on the world's
// stream and reads nothing in between; order between workgroups comes from the kernel boundaries alone.
#pragma once

#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>

#include <cstdint>

#include "bge_query.hpp"

namespace bge {

constexpr uint32_t kCharTrigChunk = 64;     // ghosts staged in LDS per workgroup of k_ct_test (32 B each)
constexpr uint32_t kCharTrigNoRow = 0xffffffffu;

struct CharTrigParams {
    const void* state;      // [n] bge_character_state: position in its first three words
    const void* desc;       // [n] bge_character_desc: radius in word 3
    const uint32_t* group;  // [n] per character
    const uint32_t* mask;   // [n]
    uint32_t n;             // characters
    uint32_t words;         // ceil(n / 64): 64-bit words of one bitmap row
    const QueryGhost* ghosts; // [n_ghosts] the list the queries see, in the order of the uploaded trigger array
    uint32_t n_ghosts;
    const float* aabb;      // [triggers][6] fed boxes (k_trigger_aabb, or the frozen box)
    const unsigned long long* prev; // [triggers][words] remembered before the call
    unsigned long long* cur;        // [triggers][words] overlapping now (rows of unlisted triggers: carried from prev by the host)
    unsigned long long* counts;     // [n_ghosts][words] per word: low half Enter (+ Stay), high half Exit; scanned in place to offsets
    unsigned long long* row_total;  // [n_ghosts] the same pair of halves summed over the row
    unsigned long long* row_base;   // [n_ghosts] records before the row
    uint2* ghost_rec;       // [n_ghosts] {trigger index, entity} as the call saw them (the list can be made again from these)
    uint32_t* count;        // [1] records of the call (saturates at 2^32 - 1)
    void* events;           // [cap] bge_character_trigger_event
    uint64_t cap;
    uint32_t stay;          // BGE_CHAR_TRIGGER_STAY_EVENTS
};

// test + the three scans + emit, in order, on the stream.  n, n_ghosts >= 1.
hipError_t launch_chartrig(hipStream_t stream, const CharTrigParams& p);
// emit alone: the list again from prev, cur and the offsets the last launch_chartrig left (after the list grew)
hipError_t launch_chartrig_emit(hipStream_t stream, const CharTrigParams& p);
// dst[i][..] = src_row[i] == kCharTrigNoRow ? 0 : src[src_row[i]][..] for i < rows (bge_world_upload_triggers)
hipError_t launch_chartrig_gather(hipStream_t stream, uint32_t rows, uint32_t words, const uint32_t* src_row, const unsigned long long* src,
                                  unsigned long long* dst);

} // namespace bge
