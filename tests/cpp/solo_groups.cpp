// solo_groups.cpp — the host side of solo groups on its own (DESIGN.md §4.1 "Solo groups"): what the tile headers of a pass say about
// the scene's shape (csrc/bge_flatten.hpp TileShape) and which ticks of a call launch, with how many ticks (csrc/bge_epochs.hpp
// SoloPlan on FuseClock's groups).  Built with -fsanitize=address,undefined by tests/test_solo_groups_cpu.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bge_epochs.hpp"
#include "bge_flatten.hpp"

#define CHECK(c)                                                                 \
    do {                                                                         \
        if (!(c)) {                                                              \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                        \
        }                                                                        \
    } while (0)

namespace {

using namespace bge;

constexpr uint32_t hdr(uint32_t bits, uint32_t count = 256, uint32_t max_level = 0) { return bits | (count << kHdrCountShift) | max_level; }

TileShape shape(const std::vector<uint32_t>& h) { return TileShape::of(h.data(), 0, static_cast<uint32_t>(h.size())); }

struct Launch {
    uint32_t tick;   // the tick of the call that launches
    uint32_t n_solo; // TickParams::n_solo
    uint32_t serial, n_left;
};

// the loop of tick_impl for a fusable call: the launches it makes, and how many ticks it counted
std::vector<Launch> call(FuseClock& clock, bool solo, uint32_t ticks, uint32_t T, uint32_t* counted)
{
    std::vector<Launch> out;
    uint32_t first = 0, t0 = 0, n = 0;
    *counted = 0;
    for (uint32_t t = 0; t < ticks; ++t) {
        if (T > 1u && t == t0 + n) {
            t0 = t;
            n = FuseClock::group_size(t, ticks, T);
            bool wrapped = false;
            if (!solo) first = clock.begin_group(n, &wrapped);
        }
        const bool fused = T > 1u && n > 1u && !solo;
        const SoloPlan plan = SoloPlan::plan(solo && T > 1u, t - t0, n);
        if (plan.launch) out.push_back(Launch{t, plan.n_solo, fused ? first + (t - t0) : 0u, fused ? n - (t - t0) : 1u});
        ++*counted; // (physics_updates, the event pair, prof_ticks_pending: every tick, launched or not)
    }
    return out;
}

} // namespace

int main()
{
    const uint32_t flat = kHdrWaveLocal, dyn = kHdrAllDynamic;
    // ---- the tile summary
    {
        const TileShape s = shape({hdr(flat | dyn), hdr(flat | dyn), hdr(flat | dyn, 40)}); // all flat (the last tile partly filled)
        CHECK(s.all_flat && s.any_flat_all_dynamic);
    }
    {
        const TileShape s = shape({hdr(flat | dyn), hdr(0, 256, 3), hdr(flat | dyn)}); // one chain tile (block tile, levels 0..3)
        CHECK(!s.all_flat && s.any_flat_all_dynamic);
    }
    {
        const TileShape s = shape({hdr(flat | dyn), hdr(flat | dyn | kHdrFrozen)}); // one frozen tile
        CHECK(!s.all_flat && s.any_flat_all_dynamic);
        CHECK(!hdr_is_flat(hdr(flat | kHdrFrozen)));
    }
    {
        const TileShape s = shape({hdr(flat | dyn | kHdrExt), hdr(flat | dyn)}); // one tile with an external parent
        CHECK(!s.all_flat && s.any_flat_all_dynamic);
    }
    {
        const TileShape s = shape({}); // no tile: nothing to run alone
        CHECK(!s.all_flat && !s.any_flat_all_dynamic);
        const uint32_t one[1] = {hdr(flat | dyn)};
        const TileShape e = TileShape::of(one, 1, 1);
        CHECK(!e.all_flat && !e.any_flat_all_dynamic);
    }
    {
        const TileShape s = shape({hdr(flat), hdr(flat, 17)}); // no all-Dynamic tile: all flat, and no wave can ever be vouched
        CHECK(s.all_flat && !s.any_flat_all_dynamic);
        const TileShape c = shape({hdr(dyn, 256, 3), hdr(flat)}); // all-Dynamic only where the tile is not flat: the same
        CHECK(!c.all_flat && !c.any_flat_all_dynamic);
    }
    CHECK(hdr_is_flat(hdr(flat)) && hdr_is_flat(hdr(flat | dyn, 1)) && !hdr_is_flat(hdr(0)) && !hdr_is_flat(hdr(flat, 256, 1)));
    // the switch: all three terms
    CHECK(SoloPlan::wanted(true, true, true));
    CHECK(!SoloPlan::wanted(false, true, true) && !SoloPlan::wanted(true, false, true) && !SoloPlan::wanted(true, true, false));

    // ---- the schedule
    const uint32_t Ks[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 17, 1000}, Ts[] = {1, 2, 3, 8, 32};
    for (uint32_t T : Ts) {
        for (uint32_t K : Ks) {
            FuseClock clock;
            uint32_t counted = 0;
            const std::vector<Launch> l = call(clock, true, K, T, &counted);
            CHECK(counted == K);          // every tick does the loop's bookkeeping
            CHECK(clock.next == 1u);      // a solo call hands out no serial
            std::vector<uint32_t> covered(K, 0);
            uint32_t expect_t = 0;
            for (const Launch& a : l) {
                CHECK(a.tick == expect_t);               // the first tick of its group
                CHECK(a.serial == 0u && a.n_left == 1u); // adv is neither read nor written
                const uint32_t n = K - a.tick < T ? K - a.tick : T;
                if (T == 1u || n == 1u) CHECK(a.n_solo == 0u); // a group of one goes out as a plain tick
                else CHECK(a.n_solo == n);
                const uint32_t span = a.n_solo > 1u ? a.n_solo : 1u;
                for (uint32_t i = 0; i < span; ++i) {
                    CHECK(a.tick + i < K);
                    covered[a.tick + i]++;
                }
                expect_t = a.tick + span;
            }
            CHECK(expect_t == K);
            for (uint32_t c : covered) CHECK(c == 1u); // every tick exactly once
            CHECK(l.size() == (T == 1u ? K : (K + T - 1u) / T));

            // switch off: round 9's plan — one launch per tick, serials and n_left as tests/cpp/fuse_clock.cpp has them
            FuseClock clock9;
            const std::vector<Launch> r = call(clock9, false, K, T, &counted);
            CHECK(counted == K && r.size() == K);
            uint32_t t = 0;
            while (t < K) {
                const uint32_t n = K - t < T ? K - t : T;
                for (uint32_t i = 0; i < n; ++i) {
                    CHECK(r[t + i].tick == t + i && r[t + i].n_solo == 0u);
                    if (T == 1u || n == 1u) CHECK(r[t + i].serial == 0u && r[t + i].n_left == 1u);
                    else CHECK(r[t + i].serial == r[t].serial + i && r[t].serial != 0u && r[t + i].n_left == n - i);
                }
                t += n;
            }
        }
    }
    // a tick outside any group (the call is not fusable: no group is ever begun) launches as a plain tick
    CHECK(SoloPlan::plan(false, 0, 0).launch && SoloPlan::plan(false, 5, 0).n_solo == 0u && SoloPlan::plan(false, 3, 8).launch);
    std::printf("solo_groups ok\n");
    return 0;
}
