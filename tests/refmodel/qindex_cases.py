"""Scenes, batches and (query, body) pairs for the query-index tests, each with the class it is meant to exercise
(tests/test_qindex_cpu.py holds the classes as conditions on the model alone; tests/test_gpu_qindex.py runs the same cases on the
device and finds the same numbers in the stats)."""
from __future__ import annotations

import numpy as np

from . import qindex as Q

F = np.float32
ALL = 0xFFFFFFFF
MAGNITUDES = (1.0, 1e3, 1e5, 3e9)

# ---------------------------------------------------------------------------------------------- the grid scene
# 600 bodies on a 25 x 24 grid, 2 units apart, standing on the plane; two ghosts (not indexed).  Five kinds of query in random
# order: down onto a body, up into the sky, at a ghost, down at the plane alone, and level through a row of bodies.
N_BODIES, N_QUERIES = 600, 513
GHOST_POS = np.float32([[6.0, 5.0, 9.0], [31.0, 5.5, 20.0]])
INVALID = (7, 100, 200, 255, 256, 512)
GRID_SEED = 20261020


def grid_scene(rng):
    """type-less arrays of the scene: shape, size, pos (bodies then ghosts), layer"""
    n = N_BODIES + len(GHOST_POS)
    shape = rng.integers(0, 2, n).astype(np.uint8)
    size = rng.uniform(0.2, 0.8, (n, 3)).astype(np.float32)
    ix = np.arange(N_BODIES)
    half = np.where(shape[:N_BODIES] == 1, size[:N_BODIES, 1] + size[:N_BODIES, 0], size[:N_BODIES, 1])
    pos = np.concatenate([np.stack([2.0 * (ix % 25), half, 2.0 * (ix // 25)], 1), GHOST_POS]).astype(np.float32)
    layer = rng.choice(np.uint32([1, 4]), n)
    return dict(shape=shape, size=size, pos=pos, layer=layer, dynamic=rng.integers(0, 2, n).astype(bool))


def grid_queries(rng, pos):
    n = N_QUERIES
    cat = rng.integers(0, 5, n)
    at = pos[rng.integers(0, N_BODIES, n)]
    ghost = GHOST_POS[rng.integers(0, len(GHOST_POS), n)]
    jit = rng.normal(scale=0.15, size=(n, 3))
    o = np.stack([at[:, 0] + jit[:, 0], np.full(n, 7.0), at[:, 2] + jit[:, 2]], 1)
    d = np.tile([0.0, -1.0, 0.0], (n, 1)) + 0.05 * jit
    md = rng.uniform(8.0, 12.0, n)
    mask = np.full(n, ALL, np.uint32)
    d[cat == 1] *= -1.0
    away = rng.normal(size=(n, 3)) * [6.0, 1.0, 6.0] + [0.0, 6.0, 0.0]
    o[cat == 2] = (ghost + away)[cat == 2]
    d[cat == 2] = (ghost + 0.3 * jit - o)[cat == 2]
    md[cat == 2] = 1.5
    mask[cat == 2] = 8
    mask[cat == 3] = rng.choice(np.uint32([2, 10]), n)[cat == 3]
    o[cat == 4] = np.stack([np.full(n, -3.0), rng.uniform(0.2, 0.6, n), at[:, 2] + jit[:, 2]], 1)[cat == 4]
    d[cat == 4] = (np.tile([1.0, 0.0, 0.0], (n, 1)) + 0.02 * jit)[cat == 4]
    md[cat == 4] = 60.0
    radius = np.where(rng.random(n) < 0.2, 0.0, rng.uniform(0.05, 0.6, n))
    c = at + [0.0, 0.3, 0.0] + 2.0 * jit
    c[cat == 1] += [0.0, 50.0, 0.0]
    c[cat == 2] = (ghost + 3.0 * jit)[cat == 2]
    srad = rng.uniform(0.2, 2.5, n)
    smask = np.select([cat == 2, cat == 3, cat == 4], [np.uint32(8), np.uint32(2), np.uint32(1)], np.uint32(ALL)).astype(np.uint32)
    o, d, md, radius, c, srad = (a.astype(np.float32) for a in (o, d, md, radius, c, srad))
    ray_md, cast_radius = md.copy(), radius.copy()
    for k, i in enumerate(INVALID):
        if k % 3 == 0:
            d[i] = 0.0
            srad[i] = -1.0
        elif k % 3 == 1:
            o[i, 1] = np.nan
            c[i, 2] = np.nan
        else:
            ray_md[i] = -md[i]
            cast_radius[i] = -0.25
            srad[i] = -0.5
    return {"raycast": (o, d, ray_md, mask), "raycast_all": (o, d, ray_md, mask), "sphere_cast": (o, d, md, cast_radius, mask),
            "sphere_cast_all": (o, d, md, cast_radius, mask), "overlap_sphere": (c, srad, smask), "sphere_penetration": (c, srad, smask)}


ENTRIES = ("raycast", "raycast_all", "sphere_cast", "sphere_cast_all", "overlap_sphere", "sphere_penetration")
KIND_OF = {"raycast": "ray", "raycast_all": "ray", "sphere_cast": "cast", "sphere_cast_all": "cast", "overlap_sphere": "overlap",
           "sphere_penetration": "penetration"}


def as_records(entry, args):
    """The model's query records of an entry's arguments"""
    if KIND_OF[entry] in ("ray", "cast"):
        o, d, md = args[0], args[1], args[2]
        radius = args[3] if KIND_OF[entry] == "cast" else np.zeros(len(o), np.float32)
        return dict(origin=o, direction=d, max_distance=md, radius=radius)
    return dict(origin=args[0], radius=args[1])


def half_extents(size):
    """The box the library holds for a collider size (margin 0.04 inside, as refmodel.device.Scene.dims)"""
    h = np.maximum(size, F(0.01))
    m0 = F(0.04)
    safe = (F(0.1) * h.min(axis=1))[:, None]
    inner = h - m0
    return np.where(safe < m0, ((inner + m0) - safe) + safe, inner + m0).astype(np.float32)


def body_dims(shape, size):
    h = np.maximum(size, F(0.01))
    cap = np.stack([h[:, 0], np.maximum(size[:, 1], F(0)), h[:, 0]], 1)
    return np.where(shape[:, None] == 1, cap, half_extents(size)).astype(np.float32)


def predicted(entry, args, pos, shape, size, member, cell_edge, max_cells):
    """What the stats of one indexed call of `entry` must say: bodies in cells, bodies wide, queries far (one pass)."""
    h = Q.edge(cell_edge)
    rb = Q.body_rb(Q.body_rad(shape == 1, body_dims(shape, size)), pos)
    wide = Q.is_wide(rb, h) & member
    far = Q.classify(KIND_OF[entry], as_records(entry, args), h, max_cells)
    return dict(bodies_indexed=int((member & ~wide).sum()), bodies_wide=int(wide.sum()), queries_far=int(far.sum()),
                queries_indexed=int((~far).sum()))


# The parameter sweep on the grid scene: (name, cell_edge, max_cells, wide claim, far claim).  The claims are conditions on the model
# alone (tests/test_qindex_cpu.py); the device must then show the model's numbers (tests/test_gpu_qindex.py).
#   wide   "all": every body on the wide list; "none": every body in a cell; "some": both occur
#   far    "all": every valid query; "nan": exactly the queries with a NaN in their extent; "nan (points)": that for overlaps and
#          penetrations, nothing claimed for segments; None: nothing claimed
SWEEP = (("tiny edge", 0.01, 0, "all", None), ("edge 0.5", 0.5, 4096, "all", None), ("edge 2", 2.0, 512, "some", None),
         ("edge 4", 4.0, 512, "none", "nan (points)"), ("one cell", 1e6, 0, "none", "nan"), ("max_cells 1", 2.0, 1, "some", "all"),
         ("max_cells 27", 2.0, 27, "some", None), ("default", 0.0, 0, "none", None))


def check_claims(name, entry, wide_claim, far_claim, n_bodies, n_queries, n_nan, got):
    """got: bodies_wide, queries_far of the model or of the device's stats"""
    wide, far = got["bodies_wide"], got["queries_far"]
    assert {"all": wide == n_bodies, "none": wide == 0, "some": 0 < wide < n_bodies}[wide_claim], (name, entry, wide)
    if far_claim == "all":  # (an invalid record, a negative radius say, may have an extent of one cell: it sees nothing either way)
        assert far >= n_queries - len(INVALID), (name, entry, far)
    if far_claim == "nan" or (far_claim == "nan (points)" and KIND_OF[entry] in ("overlap", "penetration")):
        assert far == n_nan, (name, entry, far, n_nan)


def nan_queries(entry, args):
    q = as_records(entry, args)
    return int(np.isnan(Q.extent(KIND_OF[entry], q)[0]).any(axis=1).sum())


BATCH_SIZES = (1, 63, 64, 65, 257)


# ---------------------------------------------------------------------------------------------- buckets
def coincident_and_colliding(table=1024, h=2.0):
    """257 bodies at one place (one bucket, five strides of a wave), 8 bodies exactly table * h away on x (their cell differs by
    `table` cells), and 8 in the nearest cell that the hash puts into the FIRST group's bucket (searched within 8 cells per axis).
    Returns pos (273, 3) and that cell's offset (3,) in cells."""
    base = np.float32([5.0, 1.0, 5.0])
    cell0 = Q.cell(base, h)
    want = Q.bucket(cell0[0], cell0[1], cell0[2], table)
    r = np.arange(-8, 9)
    off = np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    off = off[np.any(off != 0, axis=1)]
    same = Q.bucket(cell0[0] + off[:, 0], cell0[1] + off[:, 1], cell0[2] + off[:, 2], table) == want
    assert same.any(), "no colliding cell nearby"
    off = off[same]
    off = off[np.argmin((off * off).sum(axis=1))]
    a = np.tile(base, (257, 1))
    b = np.tile(base + np.float32([table * h, 0, 0]), (8, 1))
    c = np.tile(base + (off * h).astype(np.float32), (8, 1))
    return np.concatenate([a, b, c]).astype(np.float32), off


# ---------------------------------------------------------------------------------------------- (query, body) pairs
def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _query_at(kind, rng, origin, n, seg_scale):
    q = dict(origin=origin.astype(np.float32), radius=np.where(rng.random(n) < 0.3, 0.0, rng.uniform(0.0, 1.5, n)).astype(np.float32))
    if kind == "ray":
        q["radius"] = np.zeros(n, np.float32)
    if kind in ("ray", "cast"):
        q["direction"] = _unit(rng, n).astype(np.float32)
        q["max_distance"] = (seg_scale * 10.0 ** rng.uniform(-2, 1, n)).astype(np.float32)
    return q


def random_pairs(kind, rng, n):
    """Bodies at magnitudes 1 .. 3e9 with queries near the edge of what their cull accepts; the cell edge varies per pair."""
    mag = rng.choice(MAGNITUDES, n)
    c = (_unit(rng, n) * mag[:, None] * rng.uniform(0.2, 1.0, (n, 1))).astype(np.float32)
    rad = (10.0 ** rng.uniform(-2, 0.5, n)).astype(np.float32)
    rb = Q.body_rb(rad, c)
    h = np.where(rng.random(n) < 0.5, rng.choice([0.5, 2.0, 8.0], n), rb * rng.uniform(1.5, 4.0, n)).astype(np.float32)
    # the query's origin: the body's centre, off by up to twice what the cull could accept at radius 1.5
    off = _unit(rng, n) * ((rb + 1.5) * rng.uniform(0.0, 2.0, n))[:, None]
    q = _query_at(kind, rng, c.astype(np.float64) + off, n, 1.0)
    if kind in ("ray", "cast"):  # half of the segments END near the body instead of starting there
        flip = rng.random(n) < 0.5
        delta = q["direction"] * q["max_distance"][:, None]
        q["origin"] = np.where(flip[:, None], q["origin"] - delta, q["origin"]).astype(np.float32)
    return q, c, rad, h


def touching_pairs(kind, rng, n, magnitudes=MAGNITUDES, edges=(0.5, 2.0, 8.0)):
    """Per axis and magnitude: the query's point (overlap, penetration) or one end of its segment lies on an axis through the
    body's centre at the distance at which the cull just passes, one float inside and one float outside it.  The cell edge is
    twice the body's rb and a hair more, so that the body is the largest its cell may hold."""
    mag = rng.choice(magnitudes, n)
    axis = rng.integers(0, 3, n)
    sign = rng.choice([-1.0, 1.0], n)
    c = (_unit(rng, n) * mag[:, None] * rng.uniform(0.2, 1.0, (n, 1))).astype(np.float32)
    rad = (10.0 ** rng.uniform(-2, 0.5, n)).astype(np.float32)
    rb = Q.body_rb(rad, c)
    h = np.where(rng.random(n) < 0.5, rb * F(2.0) * F(1.000001), rng.choice(edges, n)).astype(np.float32)
    e = np.zeros((n, 3))
    e[np.arange(n), axis] = sign
    q = _query_at(kind, rng, c.astype(np.float64), n, 1.0)
    if kind in ("ray", "cast"):  # the segment runs along another axis, or along this one away from the body
        other = np.zeros((n, 3))
        other[np.arange(n), (axis + rng.integers(1, 3, n)) % 3] = rng.choice([-1.0, 1.0], n)
        q["direction"] = np.where((rng.random(n) < 0.5)[:, None], other, e).astype(np.float32)
    for _ in range(3):  # the distance depends on the slack, the slack on the origin: settle it
        delta = q["direction"] * q["max_distance"][:, None] if kind in ("ray", "cast") else None
        g = Q.growth_of(kind, q["origin"], delta, q["radius"])[0]
        rr = (rb + g).astype(np.float64)
        q["origin"] = (c.astype(np.float64) + e * rr[:, None]).astype(np.float32)
    step = np.where(rng.random(n) < 0.5, 1.0, -1.0)  # one float further out, or one float in
    k = np.arange(n)
    q["origin"][k, axis] = np.nextafter(q["origin"][k, axis], np.where(sign * step > 0, F(np.inf), F(-np.inf)).astype(np.float32))
    return q, c, rad, h


def _largest_in_cell(c, h):
    """rad of the largest body at c that a cell of edge h still holds: rb <= h / 2, and one float more of rad is wide"""
    cap = Q.rb_cap(h)
    rad = ((cap - F(1e-6) - F(1e-5) * Q.abs_sum(c)) / F(1.0001)).astype(np.float32)
    for _ in range(8):
        rad = np.where(Q.body_rb(rad, c) > cap, np.nextafter(rad, F(0)), rad)
    for _ in range(8):
        up = np.nextafter(rad, F(np.inf))
        rad = np.where(Q.body_rb(up, c) <= cap, up, rad)
    return rad


def _rr(kind, q, rb):
    """The radius the kind's cull compares with, and the growth"""
    delta = q["direction"] * q["max_distance"][:, None] if kind in ("ray", "cast") else None
    g, slack = Q.growth_of(kind, q["origin"], delta, q["radius"])
    return (rb + slack if kind == "ray" else (rb + q["radius"] * F(1.0001)) + slack), g


def boundary_pairs(kind, rng, n, approach):
    """The hazard the margin is there for.  The body is the largest its cell holds and its centre lies ON a cell boundary of one
    axis, so its cell begins at its centre; the query lies below it on that axis at the distance at which the cull just passes
    (and up to two floats either side), so the query's highest cell must reach the boundary exactly.  approach (ray, cast): the
    segment is long and runs TOWARDS the body, its far end at that distance: its origin is of another magnitude than the body, so
    the cull's centre - origin rounds by more than the gap.  Pairs whose body would need rad <= 0 are given rad 0.01 (wide)."""
    h = rng.choice(np.float32([0.5, 2.0, 8.0]), n)
    axis, k = rng.integers(0, 3, n), np.arange(n)
    mag = np.ones(n) if approach else rng.choice([1.0, 1e3, 1e5], n)
    c = (_unit(rng, n) * mag[:, None] * rng.uniform(0.5, 4.0, (n, 1))).astype(np.float32)
    c[k, axis] = (np.round(c[k, axis] / h) * h).astype(np.float32)
    rad = _largest_in_cell(c, h)
    rad = np.where(rad > 0, rad, F(0.01)).astype(np.float32)
    rb = Q.body_rb(rad, c)
    q = _query_at(kind, rng, c.astype(np.float64), n, 1.0)
    e = np.zeros((n, 3), np.float32)
    e[k, axis] = 1.0
    run = np.zeros(n)
    if kind in ("ray", "cast"):
        if approach:
            q["direction"], q["max_distance"] = e, (10.0 ** rng.uniform(1, 4, n)).astype(np.float32)
            run = q["max_distance"].astype(np.float64)
        else:  # along another axis, or along this one away from the body
            other = np.zeros((n, 3), np.float32)
            other[k, (axis + rng.integers(1, 3, n)) % 3] = rng.choice([-1.0, 1.0], n)
            q["direction"] = np.where((rng.random(n) < 0.5)[:, None], other, -e).astype(np.float32)
    for _ in range(4):
        rr, _ = _rr(kind, q, rb)
        o = c.astype(np.float64).copy()
        o[k, axis] = c[k, axis].astype(np.float64) - rr - run
        q["origin"] = o.astype(np.float32)
    st = rng.integers(-2, 3, n)
    for i in (1, 2):
        to = np.where(st >= i, F(np.inf), np.where(st <= -i, F(-np.inf), q["origin"][k, axis])).astype(np.float32)
        q["origin"][k, axis] = np.nextafter(q["origin"][k, axis], to)
    return q, c, rad, h


def pairs(kind, seed, n_random=500_000, n_touching=300_000, n_boundary=200_000, n_approach=300_000):
    """>= 10^6 seeded pairs of a kind: (query records, body centres, body rad, cell edge per pair)"""
    rng = np.random.default_rng(seed)
    parts = [random_pairs(kind, rng, n_random), touching_pairs(kind, rng, n_touching), boundary_pairs(kind, rng, n_boundary, False)]
    parts.append(boundary_pairs(kind, rng, n_approach, True) if kind in ("ray", "cast") else boundary_pairs(kind, rng, n_approach, False))
    q = {k: np.concatenate([p[0][k] for p in parts]) for k in parts[0][0]}
    return (q,) + tuple(np.concatenate([p[i] for p in parts]) for i in (1, 2, 3))
