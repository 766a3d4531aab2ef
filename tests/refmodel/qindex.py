"""The rule of the query index (include/bge_world.h "Query index") in numpy float32, written from the header: which bodies are
members, which are wide, a query's extent, growth, reach and cells, and which queries go far.  The cull of each kind is restated
too (it is what coverage is measured against).  Everything is vectorised over pairs and rounds each operation to float32 once,
as the library does.  `Model` carries the three places a wrong model differs (tests/test_qindex_cpu.py rejects them)."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

F = np.float32
CELL_MAX = F(1048576.0)
EDGE_MIN, EDGE_DEFAULT = F(1e-18), F(4.0)
MAX_CELLS_DEFAULT, AXIS_CELLS = 256, 1024
MARGIN, REACH_MAX = F(1.0625), F(1e18)
FLT_MAX = np.finfo(np.float32).max
KINDS = ("ray", "cast", "overlap", "penetration")


@dataclass(frozen=True)
class Model:
    margin: bool = True          # reach = (cap + growth) * 1.0625; False: cap + growth
    floor_cell: bool = True      # a body's cell by floor; False: by truncation
    position_term: bool = True   # rb carries 1e-5 * |c|_1; False: it does not


RULE = Model()


def f32(a):
    return np.asarray(a, dtype=np.float32)


def abs_sum(v):
    v = f32(v)
    return (np.abs(v[..., 0]) + np.abs(v[..., 1])) + np.abs(v[..., 2])


def edge(requested):
    h = F(requested)
    if h == 0:
        h = EDGE_DEFAULT
    if not h >= EDGE_MIN:
        h = EDGE_MIN
    if not h <= FLT_MAX:
        h = FLT_MAX
    return F(h)


def rb_cap(h):
    return F(0.5) * f32(h)


def body_rad(capsule, dims):
    dims = f32(dims)
    box = np.sqrt((dims[..., 0] * dims[..., 0] + dims[..., 1] * dims[..., 1]) + dims[..., 2] * dims[..., 2])
    return np.where(capsule, dims[..., 0] + dims[..., 1], box).astype(np.float32)


def body_rb(rad, c, model=RULE):
    with np.errstate(all="ignore"):
        pos = F(1e-5) * abs_sum(c) if model.position_term else np.zeros(np.shape(rad), np.float32)
        return (f32(rad) * F(1.0001) + pos) + F(1e-6)


def is_member(body_type, dirty, group, mask):
    """What load_body calls a candidate: a body of any type, not uploaded since the last tick, that some query could see."""
    return (np.asarray(body_type) != 0) & ~np.asarray(dirty, bool) & (np.asarray(group) != 0) & (np.asarray(mask) != 0)


def is_wide(rb, h):
    with np.errstate(all="ignore"):
        return ~(f32(rb) <= rb_cap(h))


def cell(x, h, floor=True):
    with np.errstate(all="ignore"):
        x, h = f32(x), f32(h)
        q = x / (h[..., None] if 0 < h.ndim < x.ndim else h)
        q = np.floor(q) if floor else np.trunc(q)
        return np.fmin(np.fmax(q, -CELL_MAX), CELL_MAX).astype(np.int64)


def bucket(cx, cy, cz, table):
    u = lambda a: np.asarray(a, np.int64).astype(np.uint32)
    with np.errstate(over="ignore"):
        hsh = u(cx) * np.uint32(73856093) ^ u(cy) * np.uint32(19349663) ^ u(cz) * np.uint32(83492791)
    hsh ^= hsh >> np.uint32(15)
    return hsh & np.uint32(table - 1)


def key(cx, cy, cz):
    u = lambda a: np.asarray(a, np.int64).astype(np.uint32) & np.uint32(1023)
    return u(cx) | u(cy) << np.uint32(10) | u(cz) << np.uint32(20)


def table_size(n_slots):
    t = 1024
    while t < 2 * n_slots and t < (1 << 30):
        t <<= 1
    return t


# ---------------------------------------------------------------------------------------------- the queries
def segment(origin, direction, max_distance):
    """delta, the box lo / hi of the segment (a NaN end keeps its NaN)."""
    with np.errstate(all="ignore"):
        o = f32(origin)
        delta = f32(direction) * f32(max_distance)[..., None]
        b = o + delta
        bad = np.isnan(o) | np.isnan(b)
        lo, hi = np.where(bad, F(np.nan), np.fmin(o, b)), np.where(bad, F(np.nan), np.fmax(o, b))
        return delta, lo.astype(np.float32), hi.astype(np.float32)


def growth_of(kind, origin, delta, radius):
    """What the kind's cull adds to rb, and its slack."""
    with np.errstate(all="ignore"):
        if kind == "ray":
            o, d = f32(origin), f32(delta)
            s = ((((np.abs(o[..., 0]) + np.abs(o[..., 1])) + np.abs(o[..., 2])) + np.abs(d[..., 0])) + np.abs(d[..., 1])) + np.abs(d[..., 2])
            slack = F(1e-5) * s
            return slack, slack
        if kind == "cast":
            slack = F(1e-5) * ((abs_sum(origin) + abs_sum(delta)) + f32(radius))
        else:
            slack = F(1e-5) * (abs_sum(origin) + f32(radius))
        return f32(radius) * F(1.0001) + slack, slack


def reach(growth, h, model=RULE):
    with np.errstate(all="ignore"):
        r = rb_cap(h) + f32(growth)
        return r * MARGIN if model.margin else r


def query_range(lo, hi, growth, h, max_cells=0, model=RULE):
    """(lo cells (n, 3), hi cells (n, 3), far (n,))"""
    with np.errstate(all="ignore"):
        R = reach(growth, h, model)
        far = ~(R <= REACH_MAX)
        l, u = f32(lo) - R[..., None], f32(hi) + R[..., None]
        bad = ~np.isfinite(l) | ~np.isfinite(u)
        far = far | bad.any(axis=-1)
        cl, cu = cell(l, h), cell(u, h)
        n = cu - cl + 1
        far = far | (((n < 1) | (n > AXIS_CELLS)) & ~bad).any(axis=-1)
        cells = np.prod(np.where(bad | (n < 1) | (n > AXIS_CELLS), 1, n), axis=-1)
        far = far | (cells > (max_cells if max_cells else MAX_CELLS_DEFAULT))
        return cl, cu, far


def cull_segment(origin, delta, c, rr):
    """segment_near of the library, operation for operation"""
    with np.errstate(all="ignore"):
        a, d, c = f32(origin), f32(delta), f32(c)
        len2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        inv = F(1.0) / len2
        w = c - a
        t = ((w[..., 0] * d[..., 0] + w[..., 1] * d[..., 1]) + w[..., 2] * d[..., 2]) * inv
        t = np.where(t < 0, F(0), np.where(t > 1, F(1), t)).astype(np.float32)
        e = w - d * t[..., None]
        return ((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]) <= f32(rr) * f32(rr)


def cull_point(center, c, rr):
    with np.errstate(all="ignore"):
        e = f32(c) - f32(center)
        return ((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]) <= f32(rr) * f32(rr)


def cull(kind, q, c, rb):
    """Does the kind's cull pass for query records q (dict: origin, direction, max_distance, radius) against bodies (c, rb)"""
    with np.errstate(all="ignore"):
        if kind in ("ray", "cast"):
            delta, _, _ = segment(q["origin"], q["direction"], q["max_distance"])
            _, slack = growth_of(kind, q["origin"], delta, q["radius"])
            rr = f32(rb) + slack if kind == "ray" else (f32(rb) + f32(q["radius"]) * F(1.0001)) + slack
            return cull_segment(q["origin"], delta, c, rr)
        _, slack = growth_of(kind, q["origin"], None, q["radius"])
        return cull_point(q["origin"], c, (f32(rb) + f32(q["radius"]) * F(1.0001)) + slack)


def extent(kind, q):
    """lo, hi, growth of query records"""
    if kind in ("ray", "cast"):
        delta, lo, hi = segment(q["origin"], q["direction"], q["max_distance"])
        return lo, hi, growth_of(kind, q["origin"], delta, q["radius"])[0]
    o = f32(q["origin"])
    return o, o, growth_of(kind, o, None, q["radius"])[0]


def covered(kind, q, c, rad, h, max_cells=0, model=RULE, passes=None):
    """Per pair: (the cull passes, the body is visited: own cell in range, or wide, or the query far).  The cull and the wide
    class are the library's whatever the model says of rb: a wrong model only mis-places the body."""
    rb_true = body_rb(rad, c)
    passes = cull(kind, q, c, rb_true) if passes is None else passes
    lo, hi, growth = extent(kind, q)
    cl, cu, far = query_range(lo, hi, growth, h, max_cells, model)
    wide = is_wide(body_rb(rad, c, model), h)
    bc = cell(c, h, model.floor_cell)
    inside = ((bc >= cl) & (bc <= cu)).all(axis=-1)
    return passes, far | wide | inside


def classify(kind, q, h, max_cells=0):
    """far per query"""
    lo, hi, growth = extent(kind, q)
    return query_range(lo, hi, growth, h, max_cells)[2]
