// fuse_clock.cpp — the host bookkeeping of fused ticks (csrc/bge_epochs.hpp FuseClock) on its own: how the K ticks of a call are
// cut into groups of at most T, which serial and n_left each launch carries, that serials only rise across groups and calls, and
// that the wrap asks for the zeroing and restarts at 1.  Built with -fsanitize=address,undefined by tests/test_fuse_clock_cpu.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bge_epochs.hpp"

#define CHECK(c)                                                                 \
    do {                                                                         \
        if (!(c)) {                                                              \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                        \
        }                                                                        \
    } while (0)

namespace {

struct Launch {
    uint32_t serial, n_left;
    bool zeroed; // the adv array was zeroed before this launch
};

// the loop of tick_impl for a fusable call, launches recorded instead of made
std::vector<Launch> call(bge::FuseClock& clock, uint32_t ticks, uint32_t T)
{
    std::vector<Launch> out;
    uint32_t first = 0, t0 = 0, n = 0;
    for (uint32_t t = 0; t < ticks; ++t) {
        bool wrapped = false;
        if (T > 1u && t == t0 + n) {
            t0 = t;
            n = bge::FuseClock::group_size(t, ticks, T);
            first = clock.begin_group(n, &wrapped);
        }
        const bool fused = T > 1u && n > 1u;
        out.push_back(Launch{fused ? first + (t - t0) : 0u, fused ? n - (t - t0) : 1u, wrapped});
    }
    return out;
}

} // namespace

int main()
{
    const uint32_t Ks[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 17, 1000}, Ts[] = {1, 2, 3, 4, 8};
    for (uint32_t T : Ts) {
        bge::FuseClock clock;
        CHECK(clock.next == 1u);
        uint32_t highest = 0; // the highest serial any earlier group may have written into a word
        for (int round = 0; round < 2; ++round) {
            for (uint32_t K : Ks) {
                const std::vector<Launch> l = call(clock, K, T);
                CHECK(l.size() == K);
                uint32_t t = 0;
                while (t < K) {
                    const uint32_t n = K - t < T ? K - t : T; // the last group takes the remainder
                    if (T == 1u || n == 1u) {
                        // nothing to fuse: the launch goes out as every tick did
                        CHECK(l[t].serial == 0u && l[t].n_left == 1u);
                    } else {
                        const uint32_t s = l[t].serial;
                        CHECK(s > highest && s != 0u);       // above every word an earlier group or call left
                        for (uint32_t i = 0; i < n; ++i) {
                            CHECK(l[t + i].serial == s + i);  // consecutive
                            CHECK(l[t + i].n_left == n - i);  // what is left of the group, this tick included
                            CHECK(l[t + i].serial + l[t + i].n_left - 1u == s + n - 1u); // every launch would write the same adv
                            CHECK(!l[t + i].zeroed);
                        }
                        highest = s + n - 1u;
                    }
                    t += n;
                }
            }
        }
        CHECK(T == 1u ? clock.next == 1u : clock.next > 1u);
    }
    // the wrap: a group that does not fit below 2^32 asks for the zeroing and starts at 1; the next group follows it
    {
        bge::FuseClock clock;
        clock.next = 0xfffffffcu;
        bool wrapped = true;
        CHECK(clock.begin_group(3, &wrapped) == 0xfffffffcu && !wrapped); // serials ..fc, ..fd, ..fe; next = ..ff
        CHECK(clock.next == 0xffffffffu);
        CHECK(clock.begin_group(2, &wrapped) == 1u && wrapped); // ..ff and 0 would be its serials: 0 is "off"
        CHECK(clock.next == 3u);
        CHECK(clock.begin_group(8, &wrapped) == 3u && !wrapped);
        clock.next = 0xfffffff8u;
        CHECK(clock.begin_group(7, &wrapped) == 0xfffffff8u && !wrapped); // last serial ..fe, next = ..ff: still a serial
        CHECK(clock.begin_group(1, &wrapped) == 1u && wrapped);           // (next + n would wrap to 0: restart rather than hand out ..ff)
        // through tick_impl's loop: the launch that begins the wrapping group carries the zeroing, no other does
        clock.next = 0xfffffff0u;
        const std::vector<Launch> l = call(clock, 40, 8);
        int zeroed = 0;
        for (size_t i = 0; i < l.size(); ++i) {
            CHECK(l[i].serial != 0u);
            if (l[i].zeroed) {
                ++zeroed;
                CHECK(i % 8 == 0 && l[i].serial == 1u);
            }
        }
        CHECK(zeroed == 1);
    }
    std::printf("fuse_clock ok\n");
    return 0;
}
