// tests/cpp/impulse_host.cpp — stand-alone: the host-side checks and sizes of the impulse entry points (csrc/bge_impulse_math.hpp, the
// very lines k_imp_keys and bge_world.cpp compile) against the rule of include/bge_world.h "Impulses" restated here: which flags are
// known and which floats a kind reads, the record count, the bytes a batch needs, and the push desc.  Built with
// -fsanitize=address,undefined by tests/test_impulses_cpu.py; needs no device.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/bge_world.h"
#include "bge_impulse_math.hpp"

namespace {

int failures = 0;

void expect(bool ok, const char* what, uint64_t a = 0, uint64_t b = 0)
{
    if (ok) return;
    ++failures;
    if (failures <= 20) std::printf("FAIL %s (%llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b);
}

// the header's sentence, on its own words
bool rule_ok(uint32_t flags, const float* impulse, const float* point)
{
    const uint32_t kind = flags & 3u;
    const bool world = (flags & BGE_IMPULSE_WORLD_POINT) != 0;
    if (flags >> 3) return false;
    if (kind == 3u) return false;
    if (world && kind != BGE_IMPULSE_AT_POINT) return false;
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(impulse[a])) return false;
        if (kind == BGE_IMPULSE_AT_POINT && !std::isfinite(point[a])) return false;
    }
    return true;
}

} // namespace

int main()
{
    using namespace bge::impulse;
    static_assert(sizeof(bge_impulse) == kRecordWords * 4, "record words");
    static_assert(kAtPoint == BGE_IMPULSE_AT_POINT && kCentral == BGE_IMPULSE_CENTRAL && kTorque == BGE_IMPULSE_TORQUE && kWorldPoint == BGE_IMPULSE_WORLD_POINT,
                  "flags");
    static_assert(kApplied == BGE_IMPULSE_APPLIED && kWoke == BGE_IMPULSE_WOKE && kInvalid == BGE_IMPULSE_INVALID && kNoBody == BGE_IMPULSE_NO_BODY, "status");

    // every flag word of the low byte and a few high bits, against every place a bad float can sit
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float values[] = {0.0f, -0.0f, 1.5f, -3e38f, std::numeric_limits<float>::denorm_min(), inf, -inf, nan};
    std::vector<uint32_t> flag_words;
    for (uint32_t f = 0; f < 256; ++f) flag_words.push_back(f);
    for (uint32_t bit = 8; bit < 32; ++bit) {
        flag_words.push_back(1u << bit);
        flag_words.push_back((1u << bit) | 1u);
    }
    flag_words.push_back(0xffffffffu);
    uint64_t valid = 0, swept = 0;
    for (uint32_t f : flag_words) {
        for (int slot = 0; slot < 6; ++slot) {
            for (float v : values) {
                float rec[6] = {1.0f, 2.0f, 3.0f, 4.0f, 5.0f, 6.0f};
                rec[slot] = v;
                const bool got = record_ok(f, rec, rec + 3), want = rule_ok(f, rec, rec + 3);
                expect(got == want, "record_ok", f, (uint64_t)slot);
                valid += got ? 1u : 0u;
                ++swept;
            }
        }
    }
    expect(valid > 0 && valid < swept, "the sweep holds valid and invalid records", valid, swept);
    // exactly the five known flag words are valid with finite floats
    {
        const float rec[6] = {1.0f, 2.0f, 3.0f, 4.0f, 5.0f, 6.0f};
        uint32_t known = 0;
        for (uint32_t f : flag_words) known += record_ok(f, rec, rec + 3) ? 1u : 0u;
        expect(known == 4u, "AT_POINT, CENTRAL, TORQUE and AT_POINT | WORLD_POINT are the known flag words", known);
    }

    // the count and the bytes of a batch: no overflow up to the bound, and the bound is what the header states
    expect(kMaxRecords == (1ull << 30) - 1, "n is at most 2^30 - 1");
    expect(count_ok(0) && count_ok(1) && count_ok(kMaxRecords) && !count_ok(kMaxRecords + 1) && !count_ok(~0ull), "count_ok");
    expect(kMaxRecords <= (uint64_t)std::numeric_limits<int>::max(), "the sort counts in int");
    for (uint64_t n : {0ull, 1ull, 63ull, 64ull, 65ull, 257ull, 1000000ull, (unsigned long long)kMaxRecords}) {
        expect(word_array_bytes(n) == n * 4 && word_array_bytes(n) / 4 == n, "word_array_bytes", n);
        expect(record_bytes(n) == n * sizeof(bge_impulse) && record_bytes(n) / sizeof(bge_impulse) == n, "record_bytes", n);
    }
    // a buffer of exactly these sizes holds the last record and the last word (the sanitizer watches the writes)
    for (uint64_t n : {1ull, 65ull, 257ull}) {
        std::vector<unsigned char> records(record_bytes(n)), words(word_array_bytes(n));
        bge_impulse last{};
        last.entity = BGE_RAY_NO_ENTITY;
        const uint32_t word = kApplied | kWoke;
        std::memcpy(records.data() + (n - 1) * sizeof(bge_impulse), &last, sizeof last);
        std::memcpy(words.data() + (n - 1) * 4, &word, 4);
        expect(records.back() == 0 && words[(n - 1) * 4] == 3, "the last record and word are inside", n);
    }

    // the push desc
    expect(push_desc_error(BGE_CHAR_PUSH_ON, 0.0f, 0.0f) == 0 && push_desc_error(BGE_CHAR_PUSH_ON, 250.0f, 0.5f) == 0, "a good desc");
    expect(push_desc_error(BGE_CHAR_PUSH_ON, 1.0f, std::nextafter(1.0f, 0.0f)) == 0, "max_normal_y just below 1");
    expect(push_desc_error(2u, 1.0f, 0.5f) == 1 && push_desc_error(0x80000001u, 1.0f, 0.5f) == 1, "unknown flag bits");
    for (float force : {-1.0f, -std::numeric_limits<float>::denorm_min(), inf, -inf, nan}) expect(push_desc_error(1u, force, 0.5f) == 2, "a bad force");
    for (float ny : {1.0f, 1.5f, -0.25f, inf, -inf, nan}) expect(push_desc_error(1u, 1.0f, ny) == 3, "a bad max_normal_y");
    expect(push_desc_error(1u, -0.0f, -0.0f) == 0, "-0 is 0");

    if (failures) {
        std::printf("impulse_host: %d failures\n", failures);
        return 1;
    }
    std::printf("impulse_host ok\n");
    return 0;
}
