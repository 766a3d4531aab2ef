// bge_qindex_math.hpp — the arithmetic of the query index that decides WHICH bodies a query looks at (include/bge_world.h "Query
// index"): the cell of a coordinate, the wide class of a body, the reach of a query and its far class.  Host and
// device compile these same lines: the kernels (bge_qindex.hip, bge_query.hip k_qindex_search), the host (bge_world.cpp) and the
// stand-alone sweep tests/cpp/qindex_cover.cpp.  Nothing here touches the tests a visited body goes through (Q::cull, Q::exact).
#pragma once

#include <cfloat>
#include <cstdint>

#if defined(__HIPCC__)
#define BGE_QI_FN __host__ __device__ inline
#else
#define BGE_QI_FN inline
#endif

namespace bge {
namespace qindex {

constexpr float kCellMax = 1048576.0f;   // 2^20: cells are clamped here AS FLOATS, before the conversion
constexpr float kEdgeMin = 1e-18f;       // floor of the cell edge
constexpr float kEdgeDefault = 4.0f;     // cell_edge = 0
constexpr uint32_t kMaxCellsDefault = 256u; // max_cells = 0
constexpr int kAxisCells = 1024;         // cells per axis the 10 key bits tell apart
constexpr float kMargin = 1.0625f;       // reach over rb_cap + growth (DESIGN.md 4.24 "The cell hazard")
constexpr float kReachMax = 1e18f;       // beyond it rr * rr may overflow and the cull passes everything: far

BGE_QI_FN bool finite(float v) { return __builtin_isfinite(v); }

// the cell edge used for a requested one (0 = default)
BGE_QI_FN float edge(float requested)
{
    float h = requested == 0.0f ? kEdgeDefault : requested;
    if (!(h >= kEdgeMin)) h = kEdgeMin;
    if (!(h <= FLT_MAX)) h = FLT_MAX;
    return h;
}

// the largest bounding radius a body in a cell may have
BGE_QI_FN float rb_cap(float h) { return 0.5f * h; }
// (NaN and inf are wide)
BGE_QI_FN bool wide(float rb, float h) { return !(rb <= rb_cap(h)); }

// Monotone in x for every h > 0: the division, floor, the clamp and the conversion all are.  x = +-inf gives the clamp; NaN gives
// a cell too (fmax / fmin drop it), which nothing relies on.
BGE_QI_FN int cell(float x, float h)
{
    const float q = __builtin_floorf(x / h);
    return static_cast<int>(__builtin_fminf(__builtin_fmaxf(q, -kCellMax), kCellMax));
}

BGE_QI_FN uint32_t bucket(int x, int y, int z, uint32_t table)
{
    uint32_t h = static_cast<uint32_t>(x) * 73856093u ^ static_cast<uint32_t>(y) * 19349663u ^ static_cast<uint32_t>(z) * 83492791u;
    h ^= h >> 15;
    return h & (table - 1u);
}

// the low 10 bits of the cell per axis
BGE_QI_FN uint32_t key(int x, int y, int z)
{
    return (static_cast<uint32_t>(x) & 1023u) | (static_cast<uint32_t>(y) & 1023u) << 10 | (static_cast<uint32_t>(z) & 1023u) << 20;
}

// how far beyond its extent a query with cull growth `growth` looks
BGE_QI_FN float reach(float growth, float h) { return (rb_cap(h) + growth) * kMargin; }

struct Range {
    int lo[3], hi[3];
    bool far;
};

// The cells of a query whose segment or point has the box lo .. hi and whose cull grows a body's radius by `growth`
BGE_QI_FN Range range(const float lo[3], const float hi[3], float growth, float h, uint32_t max_cells)
{
    Range r{{0, 0, 0}, {0, 0, 0}, false};
    const float R = reach(growth, h);
    if (!(R <= kReachMax)) r.far = true; // (NaN too)
    uint64_t cells = 1;
    for (int a = 0; a < 3; ++a) {
        const float l = lo[a] - R, u = hi[a] + R;
        if (!finite(l) || !finite(u)) {
            r.far = true;
            continue;
        }
        r.lo[a] = cell(l, h);
        r.hi[a] = cell(u, h);
        const int n = r.hi[a] - r.lo[a] + 1; // <= 2^21 + 1
        if (n < 1 || n > kAxisCells) r.far = true;
        else cells *= static_cast<uint64_t>(n); // <= 2^30
    }
    if (cells > (max_cells ? max_cells : kMaxCellsDefault)) r.far = true;
    return r;
}

} // namespace qindex
} // namespace bge
