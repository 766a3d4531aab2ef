// fuse_math.cpp — csrc/bge_fuse_math.hpp on the host: the reduced loop (fuse::fuse_ticks) against the exact one, the very
// expressions the kernel runs, with a 64-float array for the wave and an any-lane loop for the ballot.
// Built and run by tests/test_fuse_math_cpu.py (g++ -ffp-contract=off, ASan + UBSan).  Prints "fuse_math ok" when everything held.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "bge_fuse_math.hpp"

namespace {

constexpr int kLanes = 64;

struct Lanes {
    float a[kLanes];
};
struct Mask {
    bool a[kLanes];
};
#define LANEWISE(R, expr)                        \
    R r;                                         \
    for (int i = 0; i < kLanes; ++i) r.a[i] = (expr); \
    return r;
Lanes operator+(const Lanes& p, const Lanes& q) { LANEWISE(Lanes, p.a[i] + q.a[i]) }
Lanes operator+(const Lanes& p, float q) { LANEWISE(Lanes, p.a[i] + q) }
Lanes operator*(const Lanes& p, float q) { LANEWISE(Lanes, p.a[i] * q) }
Mask operator>=(const Lanes& p, float q) { LANEWISE(Mask, p.a[i] >= q) }
Mask operator<=(const Lanes& p, float q) { LANEWISE(Mask, p.a[i] <= q) }
Mask operator&&(const Mask& p, const Mask& q) { LANEWISE(Mask, p.a[i] && q.a[i]) }
Mask operator||(const Mask& p, const Mask& q) { LANEWISE(Mask, p.a[i] || q.a[i]) }
Mask operator!(const Mask& p) { LANEWISE(Mask, !p.a[i]) }

uint32_t bits(float f)
{
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

struct HostWave {
    static bool any(const Mask& m)
    {
        for (int i = 0; i < kLanes; ++i)
            if (m.a[i]) return true;
        return false;
    }
    static Lanes abs(const Lanes& v) { LANEWISE(Lanes, std::fabs(v.a[i])) }
    static Mask same_bits(const Lanes& p, const Lanes& q) { LANEWISE(Mask, bits(p.a[i]) == bits(q.a[i])) }
};

struct L3 {
    Lanes x, y, z;
};

using bge::fuse::Step;

// The loop as the kernel had it before the header existed, a lane at a time and a tick at a time, written out here on its own:
// what fuse_ticks_exact must be.  Returns the 1-based tick whose ballot refused, or 0.
uint32_t plain_loop(const Step& c, uint32_t n, L3& v, L3& x)
{
    for (uint32_t t = 1; t <= n; ++t) {
        bool slow = false;
        for (int i = 0; i < kLanes; ++i) {
            v.x.a[i] = v.x.a[i] + c.cx;
            v.y.a[i] = v.y.a[i] + c.cy;
            v.z.a[i] = v.z.a[i] + c.cz;
            if (!(std::fabs(v.y.a[i]) >= c.sleep_lin)) slow = true;
        }
        if (slow) return t;
        for (int i = 0; i < kLanes; ++i) {
            x.x.a[i] = x.x.a[i] + v.x.a[i] * c.dt;
            x.y.a[i] = x.y.a[i] + v.y.a[i] * c.dt;
            x.z.a[i] = x.z.a[i] + v.z.a[i] * c.dt;
        }
    }
    return 0;
}

bool same(const L3& p, const L3& q) { return std::memcmp(&p, &q, sizeof(L3)) == 0; }

int failures = 0;
void fail(const std::string& what)
{
    if (++failures <= 20) std::printf("FAIL %s\n", what.c_str());
}

struct Wave {
    Step c;
    L3 v, x;
};

// Runs one wave through all three; returns the path the new function took.  refused_at: the plain loop's refusing tick.
uint32_t run(const Wave& w, uint32_t n, const std::string& name, uint32_t* refused_at = nullptr)
{
    L3 ve = w.v, xe = w.x, vp = w.v, xp = w.x, vn = w.v, xn = w.x;
    const bool exact = bge::fuse::fuse_ticks_exact<HostWave>(w.c, n, ve, xe);
    const uint32_t at = plain_loop(w.c, n, vp, xp);
    if (refused_at) *refused_at = at;
    if (exact != (at == 0)) fail(name + ": fuse_ticks_exact and the plain loop disagree on the flag");
    if (exact && !(same(ve, vp) && same(xe, xp))) fail(name + ": fuse_ticks_exact and the plain loop disagree on the bits");
    uint32_t path = 99;
    const bool lean = bge::fuse::fuse_ticks<HostWave>(w.c, n, vn, xn, &path);
    if (lean != exact) fail(name + ": flag differs, n = " + std::to_string(n));
    if (lean && exact && !(same(vn, ve) && same(xn, xe))) fail(name + ": bits differ, n = " + std::to_string(n));
    if (path > bge::fuse::kFirstTick) fail(name + ": no path reported");
    // what a path claims about the flag
    if (path == bge::fuse::kLean && !lean) fail(name + ": lean path returned false");
    if (path == bge::fuse::kExactAccepted && !lean) fail(name + ": accepted path returned false");
    if ((path == bge::fuse::kExactRefused || path == bge::fuse::kFirstTick) && lean) fail(name + ": refused path returned true");
    return path;
}

struct Rng {
    uint64_t s;
    uint32_t next()
    {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return static_cast<uint32_t>(s >> 33);
    }
    float uni(float lo, float hi) { return lo + (hi - lo) * (static_cast<float>(next() & 0xffffffu) / 16777216.0f); }
};

const float kDt = 1.0f / 60.0f;
const float kCy = -9.81f * kDt;

// A wave that falls fast under a y-only gravity: the lean loop's own case.  The others start from it.
Wave falling(Rng& r)
{
    Wave w{};
    w.c = Step{0.0f, kCy, 0.0f, kDt, 0.8f};
    for (int i = 0; i < kLanes; ++i) {
        w.v.x.a[i] = r.uni(-3.0f, 3.0f);
        w.v.y.a[i] = r.uni(-60.0f, -2.0f);
        w.v.z.a[i] = r.uni(-3.0f, 3.0f);
        w.x.x.a[i] = r.uni(-100.0f, 100.0f);
        w.x.y.a[i] = r.uni(0.0f, 500.0f);
        w.x.z.a[i] = r.uni(-100.0f, 100.0f);
    }
    return w;
}

// One lane whose v.y is inside the band after exactly k ticks and outside after every earlier one (s = 0.8, the step kCy).
void enter_band_at(Wave& w, int lane, uint32_t k) { w.v.y.a[lane] = 0.8f + (static_cast<float>(k) - 0.5f) * -kCy; }

void seeded(uint64_t seed, uint32_t per_small_n, uint32_t per_large_n)
{
    Rng r{seed};
    uint64_t count[5] = {0, 0, 0, 0, 0}, total = 0;
    for (uint32_t n : {1u, 2u, 3u, 8u, 64u, 65u, 1024u}) {
        const uint32_t per_n = n <= 65u ? per_small_n : per_large_n;
        for (uint32_t i = 0; i < per_n; ++i) {
            Wave w = falling(r);
            const int lane = static_cast<int>(r.next() % kLanes);
            switch (r.next() % 5u) {
            case 0: // as it is: lean
                break;
            case 1: // a step larger than the band: some lane jumps it at a tick of the group after the first
                w.c.cy = -2.0f;
                w.v.y.a[lane] = r.uni(0.85f, 1.0f) + 2.0f * static_cast<float>(1u + r.next() % (n > 1u ? n - 1u : 1u));
                break;
            case 2: // a lane enters the band at a tick after the first
                enter_band_at(w, lane, 2u + r.next() % (n > 1u ? n - 1u : 1u));
                break;
            case 3: // a sideways gravity that the velocities do not absorb
                w.c.cx = r.uni(0.001f, 0.01f);
                w.c.cz = -w.c.cx;
                break;
            case 4: // rising lanes that stay above the band, and some that may not
                w.v.y.a[lane] = r.uni(0.0f, 400.0f);
                break;
            }
            ++count[run(w, n, "seeded wave " + std::to_string(total))];
            ++total;
        }
    }
    std::printf("seeded: %llu waves; lean %llu, exact accepted %llu, exact refused %llu, not fixed %llu, first tick %llu\n",
                static_cast<unsigned long long>(total), static_cast<unsigned long long>(count[0]), static_cast<unsigned long long>(count[1]),
                static_cast<unsigned long long>(count[2]), static_cast<unsigned long long>(count[3]), static_cast<unsigned long long>(count[4]));
    const char* names[4] = {"lean", "exact accepted", "exact refused", "not fixed"};
    for (int k = 0; k < 4; ++k)
        if (count[k] * 100u < total) fail(std::string("seeded waves: class '") + names[k] + "' holds less than 1 %");
}

void expect(const Wave& w, uint32_t n, uint32_t want, const std::string& name, uint32_t want_refused_at = ~0u)
{
    uint32_t at = 0;
    const uint32_t got = run(w, n, name, &at);
    if (got != want) fail(name + ": path " + std::to_string(got) + ", built for " + std::to_string(want));
    if (want_refused_at != ~0u && at != want_refused_at) fail(name + ": the exact loop refused at tick " + std::to_string(at) + ", built for " + std::to_string(want_refused_at));
}

void constructed()
{
    using namespace bge::fuse;
    Rng r{0x5eedull};
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // one lane entering the band at tick k
    for (uint32_t k = 1; k <= 8; ++k) {
        Wave w = falling(r);
        enter_band_at(w, static_cast<int>(7u * k % kLanes), k);
        expect(w, 8, k == 1 ? kFirstTick : kExactRefused, "enters at tick " + std::to_string(k) + " of 8", k);
    }
    for (uint32_t k : {1u, 2u, 63u, 64u}) {
        Wave w = falling(r);
        enter_band_at(w, 63, k);
        expect(w, 64, k == 1 ? kFirstTick : kExactRefused, "enters at tick " + std::to_string(k) + " of 64", k);
    }
    { // from above +s to below -s inside the group, through the band
        Wave w = falling(r);
        w.v.y.a[5] = 1.2f;
        expect(w, 64, kExactRefused, "crosses the band");
    }
    { // a step larger than 2s: tick 1 leaves the lane at 0.9, tick 2 at -1.1 — never inside, but on both sides
        Wave w = falling(r);
        w.c.cy = -2.0f;
        w.v.y.a[9] = 2.9f;
        expect(w, 8, kExactAccepted, "jumps the band at tick 2", 0);
        w.v.y.a[9] = 0.9f; // the jump is tick 1's own: both ends below
        expect(w, 8, kLean, "jumps the band at tick 1", 0);
    }
    { // v.y exactly on the threshold after tick 1, moving away
        Wave w = falling(r);
        w.c.sleep_lin = 1.0f;
        w.c.cy = 0.5f;
        for (int i = 0; i < kLanes; ++i) w.v.y.a[i] = 0.5f;
        expect(w, 8, kLean, "v.y == +s", 0);
        w.c.cy = -0.5f;
        for (int i = 0; i < kLanes; ++i) w.v.y.a[i] = -0.5f;
        expect(w, 8, kLean, "v.y == -s", 0);
    }
    { // s = 0: every ballot passes; a lane that changes sign is on both sides
        Wave w = falling(r);
        w.c.sleep_lin = 0.0f;
        expect(w, 64, kLean, "s == 0, falling", 0);
        w.v.y.a[1] = 1.0f;
        expect(w, 64, kExactAccepted, "s == 0, through zero", 0);
        w.c.sleep_lin = -0.0f;
        expect(w, 64, kExactAccepted, "s == -0, through zero", 0);
    }
    { // negative s: every ballot passes, and both ends are above s
        Wave w = falling(r);
        w.c.sleep_lin = -1.0f;
        w.v.y.a[2] = 0.5f;
        expect(w, 8, kLean, "s < 0, inside (-|s|, |s|)", 0);
        expect(w, 64, kLean, "s < 0, through zero", 0);
    }
    { // tick 1 changes the sign bit of v.x, tick 2 does not
        Wave w = falling(r);
        w.c.cx = 0.0f;
        for (int i = 0; i < kLanes; i += 3) w.v.x.a[i] = -0.0f;
        w.v.z.a[4] = -0.0f;
        expect(w, 8, kLean, "v.x == -0 with cx == +0", 0);
    }
    { // a sideways gravity absorbed by large velocities, and one that is not
        Wave w = falling(r);
        w.c.cx = 1e-3f;
        w.c.cz = -1e-3f;
        for (int i = 0; i < kLanes; ++i) {
            w.v.x.a[i] = (i & 1) ? 1e8f : -1e8f;
            w.v.z.a[i] = 3e7f;
        }
        expect(w, 64, kLean, "cx absorbed", 0);
        w.v.x.a[17] = 1.0f;
        expect(w, 64, kNotFixed, "cx not absorbed in one lane", 0);
    }
    // NaN and +-inf in each of the six inputs
    for (int comp = 0; comp < 6; ++comp) {
        for (float bad : {nan, inf, -inf}) {
            Wave w = falling(r);
            Lanes* c6[6] = {&w.x.x, &w.x.y, &w.x.z, &w.v.x, &w.v.y, &w.v.z};
            c6[comp]->a[11] = bad;
            const bool nan_vy = comp == 4 && bad != bad;
            expect(w, 8, nan_vy ? kFirstTick : kLean, "component " + std::to_string(comp) + " = " + std::to_string(bad));
            expect(w, 1, nan_vy ? kFirstTick : kLean, "component " + std::to_string(comp) + " = " + std::to_string(bad) + ", n = 1");
        }
    }
    { // a gravity of NaN / inf: v.y turns NaN in tick 1 (NaN) or tick 2 (inf - inf is not reached: inf stays inf, on one side)
        Wave w = falling(r);
        w.c.cy = nan;
        expect(w, 8, kFirstTick, "cy NaN");
        w.c.cy = -inf;
        expect(w, 8, kLean, "cy -inf", 0);
        w.c.cy = kCy;
        w.c.sleep_lin = nan;
        expect(w, 8, kFirstTick, "s NaN");
    }
    { // denormal velocities
        Wave w = falling(r);
        for (int i = 0; i < kLanes; ++i) w.v.x.a[i] = w.v.z.a[i] = (i & 1) ? 1e-40f : -3e-42f;
        expect(w, 64, kLean, "denormal v.x, v.z", 0);
        w.c.sleep_lin = 0.0f;
        w.c.cy = -1e-41f;
        for (int i = 0; i < kLanes; ++i) w.v.y.a[i] = 1e-40f;
        expect(w, 8, kLean, "denormal v.y and step, one side", 0);
        expect(w, 64, kExactAccepted, "denormal v.y and step, through zero", 0);
    }
    // n = 0 stores nothing and accepts, as the exact loop does
    {
        Wave w = falling(r);
        L3 v = w.v, x = w.x;
        if (!bge::fuse::fuse_ticks<HostWave>(w.c, 0, v, x) || !same(v, w.v) || !same(x, w.x)) fail("n == 0");
    }
}

} // namespace

int main()
{
    seeded(0x9e3779b97f4a7c15ull, 400, 60);
    constructed();
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("fuse_math ok\n");
    return 0;
}
