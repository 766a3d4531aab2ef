// tests/cpp/qindex_cover.cpp — stand-alone: the arithmetic that decides which cells a query visits (csrc/bge_qindex_math.hpp, the
// lines the kernels compile), swept on the host under ASan + UBSan.  cell() must be monotone in x for every edge, clamp at +-2^20
// (infinities included) and never convert a value an int cannot hold; edge() must keep its floor and FLT_MAX; range() must call far
// what include/bge_world.h "Query index" calls far, and a body inside lo - reach .. hi + reach must lie in the range's cells.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bge_qindex_math.hpp"

using namespace bge::qindex;

static int failures = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            if (++failures < 20) std::printf("line %d: %s\n", __LINE__, #c); \
        }                                                                 \
    } while (0)

int main()
{
    const float inf = INFINITY;
    // the edges: the floor, the default, ordinary ones, huge ones
    const std::vector<float> edges = {kEdgeMin, 1e-6f, 0.01f, 0.5f, 2.0f, 3.7f, 1e6f, 1e30f, FLT_MAX};
    CHECK(edge(0.0f) == kEdgeDefault);
    CHECK(edge(1e-30f) == kEdgeMin && edge(kEdgeMin) == kEdgeMin);
    CHECK(edge(FLT_MAX) == FLT_MAX && edge(inf) == FLT_MAX && edge(2.5f) == 2.5f);
    // coordinates: around zero, around cell boundaries of every edge, around the clamp, the extremes
    std::vector<float> xs = {-inf, -FLT_MAX, -3e9f, -1e5f, -1.0f, -FLT_MIN, -0.0f, 0.0f, FLT_MIN, 1.0f, 1e5f, 3e9f, FLT_MAX, inf};
    for (float h : edges) {
        for (float k : {-1048577.0f, -1048576.0f, -1048575.0f, -3.0f, -1.0f, 0.0f, 1.0f, 2.0f, 1048575.0f, 1048576.0f, 1048577.0f}) {
            float x = k * h;
            if (!std::isfinite(x)) continue;
            float lo = x, hi = x;
            for (int i = 0; i < 3; ++i) {
                lo = std::nextafterf(lo, -inf);
                hi = std::nextafterf(hi, inf);
                xs.push_back(lo);
                xs.push_back(hi);
            }
            xs.push_back(x);
        }
    }
    std::srand(7);
    for (int i = 0; i < 20000; ++i) {
        const float m = std::ldexp(1.0f, std::rand() % 80 - 30);
        xs.push_back((std::rand() / float(RAND_MAX) * 2.0f - 1.0f) * m);
    }
    for (float h : edges) {
        CHECK(cell(inf, h) == 1048576 && cell(-inf, h) == -1048576);
        if (h < 1e30f) CHECK(cell(FLT_MAX, h) == 1048576 && cell(-FLT_MAX, h) == -1048576);
        if (h == FLT_MAX) CHECK(cell(FLT_MAX, h) == 1 && cell(-FLT_MAX, h) == -1);
        // (-FLT_MIN / h may underflow to -0, whose floor is cell 0: still monotone)
        CHECK(cell(0.0f, h) == 0 && cell(-0.0f, h) == 0 && cell(-FLT_MIN, h) <= 0 && cell(-FLT_MIN, h) >= -1 && cell(-h, h) == -1);
        for (size_t i = 0; i < xs.size(); ++i) {
            const int a = cell(xs[i], h);
            CHECK(a >= -1048576 && a <= 1048576);
            // monotone: against the next float up and against a handful of others
            const int b = cell(std::nextafterf(xs[i], inf), h);
            CHECK(b >= a);
            const float y = xs[(i * 7919u + 13u) % xs.size()];
            const int c = cell(y, h);
            CHECK((y <= xs[i] && c <= a) || (y >= xs[i] && c >= a));
        }
        CHECK(wide(NAN, h) && wide(inf, h) && !wide(rb_cap(h), h) && wide(std::nextafterf(rb_cap(h), inf), h));
    }
    // range(): the far classes
    {
        const float lo[3] = {1.0f, 2.0f, 3.0f}, hi[3] = {1.5f, 2.0f, 3.0f};
        Range r = range(lo, hi, 0.1f, 2.0f, 0);
        CHECK(!r.far);
        for (int a = 0; a < 3; ++a) CHECK(r.lo[a] <= cell(lo[a], 2.0f) && r.hi[a] >= cell(hi[a], 2.0f));
        CHECK(range(lo, hi, 0.1f, 2.0f, 1).far);             // more than max_cells
        CHECK(range(lo, hi, NAN, 2.0f, 0).far && range(lo, hi, inf, 2.0f, 0).far && range(lo, hi, 2e18f, 1e19f, 0).far);
        const float nlo[3] = {NAN, 2.0f, 3.0f}, flo[3] = {-FLT_MAX, 0.0f, 0.0f}, fhi[3] = {FLT_MAX, 0.0f, 0.0f};
        CHECK(range(nlo, hi, 0.1f, 2.0f, 0).far);
        CHECK(range(flo, fhi, 1e37f, 2.0f, 0).far);          // lo - reach overflows
        const float wlo[3] = {0.0f, 0.0f, 0.0f}, whi[3] = {3000.0f, 0.0f, 0.0f};
        CHECK(range(wlo, whi, 0.1f, 2.0f, 0xffffffffu).far); // more than 1024 cells on one axis
        CHECK(!range(wlo, whi, 0.1f, 1e6f, 0).far);          // one cell
        CHECK(!range(wlo, wlo, 0.0f, kEdgeMin, 0).far);
        CHECK(range(wlo, wlo, 0.1f, FLT_MAX, 0).far);        // the reach of such an edge is beyond 1e18: every query far
    }
    // a body within the reach of a query lies in the range's cells, whatever the magnitude (monotonicity alone)
    for (float h : edges) {
        for (float m : {1.0f, 1e3f, 1e5f, 3e9f}) {
            for (int i = 0; i < 2000; ++i) {
                const float q = (std::rand() / float(RAND_MAX) * 2.0f - 1.0f) * m, g = std::rand() / float(RAND_MAX) * 2.0f;
                const float lo[3] = {q, q, q}, hi[3] = {q, q, q};
                const Range r = range(lo, hi, g, h, 0xffffffffu);
                const float R = reach(g, h);
                const float t = std::rand() / float(RAND_MAX) * 2.0f - 1.0f;
                const float c = q + t * R; // (rounded: if it left lo - R .. hi + R it is brought back)
                const float cc = c < q - R ? q - R : (c > q + R ? q + R : c);
                if (r.far || !std::isfinite(cc)) continue;
                CHECK(cell(cc, h) >= r.lo[0] && cell(cc, h) <= r.hi[0]);
            }
        }
    }
    if (failures) {
        std::printf("qindex_cover: %d failures\n", failures);
        return 1;
    }
    std::printf("qindex_cover ok\n");
    return 0;
}
