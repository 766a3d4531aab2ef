// bge_impulse_math.hpp — what decides whether an impulse record is looked at, and how much room a batch needs (include/bge_world.h
// "Impulses", "Character push").  Host and device compile these same lines: k_imp_keys (bge_impulse.hip), the host
// checks of bge_world.cpp and the stand-alone sweep tests/cpp/impulse_host.cpp.  The arithmetic of Apply is not here: it uses the
// contact kernels' own functions (bge_contact_device.hpp).
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define BGE_IMP_FN __host__ __device__ inline
#else
#define BGE_IMP_FN inline
#endif

namespace bge {
namespace impulse {

// bge_impulse::flags
constexpr uint32_t kKindMask = 3u;   // BGE_IMPULSE_AT_POINT 0, BGE_IMPULSE_CENTRAL 1, BGE_IMPULSE_TORQUE 2
constexpr uint32_t kAtPoint = 0u, kCentral = 1u, kTorque = 2u;
constexpr uint32_t kWorldPoint = 4u; // BGE_IMPULSE_WORLD_POINT
// status words
constexpr uint32_t kApplied = 1u, kWoke = 2u, kInvalid = 4u, kNoBody = 8u;
constexpr uint32_t kRecordWords = 8u;
// records per call: hipcub's sort counts in int, and the character set's own bound (bge_world_characters_create)
constexpr uint64_t kMaxRecords = 0x3fffffffull;

BGE_IMP_FN bool finite(float v) { return __builtin_isfinite(v); }

// "Valid" as far as the record alone decides it: its flags are known and every float its kind reads is finite
BGE_IMP_FN bool record_ok(uint32_t flags, const float impulse[3], const float point[3])
{
    if (flags & ~(kKindMask | kWorldPoint)) return false;
    const uint32_t kind = flags & kKindMask;
    if (kind > kTorque) return false;
    if ((flags & kWorldPoint) && kind != kAtPoint) return false;
    if (!(finite(impulse[0]) && finite(impulse[1]) && finite(impulse[2]))) return false;
    if (kind == kAtPoint && !(finite(point[0]) && finite(point[1]) && finite(point[2]))) return false;
    return true;
}

BGE_IMP_FN bool count_ok(uint64_t n) { return n <= kMaxRecords; }

// the two key arrays and the two value arrays of a batch (one word per record each), and the staging of the host entry point
BGE_IMP_FN size_t word_array_bytes(uint64_t n) { return static_cast<size_t>(n) * 4u; }
BGE_IMP_FN size_t record_bytes(uint64_t n) { return static_cast<size_t>(n) * kRecordWords * 4u; }

// bge_character_push_desc as bge_world_characters_push takes it: 0 = fine, otherwise which member is wrong (1 flags, 2 force,
// 3 max_normal_y).  max_normal_y < 1 is what makes the level part of a unit normal non-zero.
BGE_IMP_FN int push_desc_error(uint32_t flags, float force, float max_normal_y)
{
    if (flags & ~1u) return 1;
    if (!(finite(force) && force >= 0.0f)) return 2;
    if (!(finite(max_normal_y) && max_normal_y >= 0.0f && max_normal_y < 1.0f)) return 3;
    return 0;
}

} // namespace impulse
} // namespace bge
