// device_buffer.cpp — the owning buffer (csrc/bge_device_buffer.hpp) on its own, over a stand-in allocator that counts every block
// it hands out and takes back and can be told to fail the k-th allocation.  No HIP: the header is included without a HIP include
// path, so only the template exists.  Built with -fsanitize=address,undefined by tests/test_device_buffer_cpu.py: a block freed
// twice or never is also ASan's finding, not only the stand-in's.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <type_traits>
#include <utility>
#include <vector>

#include "bge_device_buffer.hpp"

#define CHECK(c)                                                                 \
    do {                                                                         \
        if (!(c)) {                                                              \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                        \
        }                                                                        \
    } while (0)

namespace {

struct Counting {
    using error = int;
    static constexpr error ok = 0;
    static inline uint64_t allocs = 0, frees = 0;
    static inline int64_t fail_in = 0; // k > 0: the k-th allocation from now fails
    static inline std::set<void*> live;
    static error alloc(void** p, size_t n)
    {
        if (fail_in > 0 && --fail_in == 0) {
            *p = reinterpret_cast<void*>(0x1); // what a failed call leaves behind must not be kept
            return 2;
        }
        *p = std::malloc(n);
        CHECK(*p && live.insert(*p).second);
        ++allocs;
        return ok;
    }
    static void free(void* p)
    {
        CHECK(live.erase(p) == 1); // a block of ours, freed once
        std::free(p);
        ++frees;
    }
};
using Buf = bge::Buffer<Counting>;

// allocations and frees since the last call
std::pair<uint64_t, uint64_t> delta()
{
    static uint64_t a = 0, f = 0;
    const std::pair<uint64_t, uint64_t> d{Counting::allocs - a, Counting::frees - f};
    a = Counting::allocs;
    f = Counting::frees;
    return d;
}
using P = std::pair<uint64_t, uint64_t>;

void check_live(uint64_t blocks, uint64_t bytes)
{
    CHECK(bge::live_memory().allocations.load() == blocks);
    CHECK(bge::live_memory().bytes.load() == bytes);
    CHECK(Counting::live.size() == blocks);
}

void test_ensure()
{
    {
        Buf b;
        CHECK(b.p == nullptr && b.bytes == 0 && b.as<char>() == nullptr);
        CHECK(b.ensure(0) == Counting::ok && b.p == nullptr); // nothing asked, nothing made
        CHECK(delta() == P(0, 0));
        CHECK(b.ensure(100) == Counting::ok && b.p && b.bytes == 100);
        CHECK(delta() == P(1, 0));
        check_live(1, 100);
        void* const first = b.p;
        CHECK(b.ensure(100) == Counting::ok && b.ensure(40) == Counting::ok && b.ensure(0) == Counting::ok);
        CHECK(b.p == first && b.bytes == 100); // grow-only
        CHECK(delta() == P(0, 0));
        CHECK(b.ensure(101) == Counting::ok && b.bytes == 101);
        CHECK(delta() == P(1, 1)); // exactly one block freed, one made
        check_live(1, 101);
        b.as<char>()[100] = 7; // (ASan: the block has the size it says)
    }
    CHECK(delta() == P(0, 1));
    check_live(0, 0);
}

void test_failed_ensure()
{
    Buf b;
    Counting::fail_in = 1;
    CHECK(b.ensure(64) != Counting::ok);
    CHECK(b.p == nullptr && b.bytes == 0);
    CHECK(delta() == P(0, 0));
    check_live(0, 0);
    CHECK(b.ensure(64) == Counting::ok && b.bytes == 64); // a retry allocates
    // a failed growth: the old block went first and is not kept
    Counting::fail_in = 1;
    CHECK(b.ensure(128) != Counting::ok);
    CHECK(b.p == nullptr && b.bytes == 0);
    CHECK(delta() == P(1, 1));
    check_live(0, 0);
    CHECK(b.ensure(16) == Counting::ok && b.bytes == 16);
    b.release();
    CHECK(delta() == P(1, 1));
    check_live(0, 0);
}

void test_release_then_destructor()
{
    {
        Buf b;
        CHECK(b.ensure(32) == Counting::ok);
        b.release();
        CHECK(b.p == nullptr && b.bytes == 0);
        CHECK(delta() == P(1, 1));
        b.release(); // idempotent
        CHECK(delta() == P(0, 0));
    }
    CHECK(delta() == P(0, 0)); // the destructor had nothing left to free
    check_live(0, 0);
}

void test_moves()
{
    {
        Buf a;
        CHECK(a.ensure(10) == Counting::ok);
        void* const pa = a.p;
        Buf b(std::move(a)); // move construction
        CHECK(a.p == nullptr && a.bytes == 0 && b.p == pa && b.bytes == 10);
        CHECK(delta() == P(1, 0));
        Buf c;
        CHECK(c.ensure(20) == Counting::ok);
        void* const pc = c.p;
        b = std::move(c); // move assignment onto a non-empty buffer: its block goes, once
        CHECK(c.p == nullptr && c.bytes == 0 && b.p == pc && b.bytes == 20);
        CHECK(delta() == P(1, 1));
        check_live(1, 20);
        Buf& same = b;
        b = std::move(same); // onto itself: nothing happens
        CHECK(b.p == pc && b.bytes == 20 && delta() == P(0, 0));
        Buf d;
        CHECK(d.ensure(30) == Counting::ok);
        void* const pd = d.p;
        std::swap(b, d); // as on trig_tab and in EntityBuf::follow_topology
        CHECK(b.p == pd && b.bytes == 30 && d.p == pc && d.bytes == 20);
        CHECK(delta() == P(1, 0));
        Buf e;
        std::swap(e, d); // with an empty one
        CHECK(d.p == nullptr && d.bytes == 0 && e.p == pc && e.bytes == 20);
        CHECK(delta() == P(0, 0));
        check_live(2, 50);
    }
    CHECK(delta() == P(0, 2));
    check_live(0, 0);
}

// a struct that derives from the buffer and adds fields, like SlotBuf and EntityBuf
struct Rows : Buf {
    const uint32_t words;
    explicit Rows(uint32_t words) : words(words) {}
};

void test_derived_and_vector()
{
    struct Carry { // the list of bge_world_set_topology
        Rows* buf;
        Buf tmp;
    };
    {
        Rows r{3};
        CHECK(r.ensure(12) == Counting::ok);
        std::vector<Carry> carries;
        uint64_t want_bytes = 12;
        for (int i = 0; i < 37; ++i) { // grows several times: every element is moved, no block is copied or freed
            carries.push_back(Carry{&r, Buf{}});
            CHECK(carries.back().tmp.ensure(8 + i) == Counting::ok);
            want_bytes += 8 + i;
        }
        CHECK(delta() == P(38, 0));
        check_live(38, want_bytes);
        carries[5].tmp.release(); // freed early on purpose
        CHECK(delta() == P(0, 1));
        carries.erase(carries.begin() + 7); // elements move down by assignment
        CHECK(delta() == P(0, 1));
        Buf grown;
        CHECK(grown.ensure(24) == Counting::ok);
        std::swap<Buf>(r, grown); // the base of a derived buffer takes a new block
        CHECK(r.bytes == 24 && grown.bytes == 12 && r.words == 3);
        CHECK(delta() == P(1, 0));
    }
    CHECK(delta() == P(0, 37)); // 35 left in the vector, r and grown
    check_live(0, 0);
}

// an object that allocates several buffers and fails part-way, like Broadphase::configure: what it made is freed with it
void test_partial_failure()
{
    struct Three {
        Buf a, b, c;
        int make() { return a.ensure(8) || b.ensure(8) || c.ensure(8); }
    };
    {
        Three t;
        Counting::fail_in = 2;
        CHECK(t.make() != 0);
        CHECK(t.a.p && !t.b.p && !t.c.p);
        CHECK(t.make() == 0); // the retry makes what is missing and keeps what is there
        CHECK(delta() == P(3, 0));
    }
    CHECK(delta() == P(0, 3));
    check_live(0, 0);
}

} // namespace

int main()
{
    static_assert(!std::is_copy_constructible<Buf>::value && !std::is_copy_assignable<Buf>::value, "a buffer has one owner");
    static_assert(std::is_nothrow_move_constructible<Buf>::value && std::is_nothrow_move_assignable<Buf>::value, "vectors move it");
    check_live(0, 0);
    test_ensure();
    test_failed_ensure();
    test_release_then_destructor();
    test_moves();
    test_derived_and_vector();
    test_partial_failure();
    check_live(0, 0);
    CHECK(Counting::allocs == Counting::frees && Counting::allocs > 0);
    std::printf("device_buffer ok: %llu blocks made and freed\n", (unsigned long long)Counting::allocs);
    return 0;
}
