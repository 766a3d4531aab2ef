"""The island solver's scenes: one per routing class and capacity regime of bge_island.hip, and the classifier that says, from the
oracle's state alone, which solver every island of a tick went to.  Shared by test_island_cases_cpu.py (which proves that every
scene holds the classes it exists for) and test_gpu_island_paths.py (which compares the device with the oracle on them).

Sizes are HALF extents: a unit box is size 0.5 at y = 0.5.  Boxes that should touch are SPACING apart (at exactly 1.0 the manifolds
stay thinner); every scene starts in contact, so a test needs 8 .. 24 ticks."""
from __future__ import annotations

import math

import numpy as np

from banggameengine_amd import synth

# ---- the constants of the routing, stated once.  They mirror banggameengine_amd/csrc/bge_island.hip:
LDS_BODIES, LDS_POINTS = 4, 16        # kIslLdsBodies, kIslLdsPoints (line 541): the LDS column solver
MID_BODIES = 16                       # kIslMidBodies (line 542): the mid launch
BIG_LDS_BYTES = 144 * 1024            # kIslBigLdsBytes (line 1184): the workgroup solver's dynamic LDS
BIG_LAST_LDS = BIG_LDS_BYTES // 4     # kIslBigLastLds = 36 864: last_in_lds (line 1233)
BIG_LDS_BODIES = BIG_LDS_BYTES // 48  # kIslBigLdsBodies = 3 072: bodies_in_lds (line 1341)
WG_THREADS = 256                      # isl_wg_scan's chunk is (depth + 2 + 255) / 256 elements a thread (line 1151)
BIG_WORKGROUPS = 256                  # k_island_solve_big is launched with that many workgroups (lines 1466, 1475)
PRODUCT_BIG_POINTS = 128              # bge_world.cpp isl_big_points; BGE_ISLAND_BIG_POINTS overrides it

SMALL, MID, GLOBAL, BIG = "small", "mid", "global", "big"
SPACING = 0.998
AABB_MARGIN = 0.02                    # k_island_begin feeds the box of the pose grown by Bullet's contact breaking threshold on every side


def route(nb, P, big_points):
    """(class, regime flags) of an island of nb bodies and P contact points, exactly as k_island_solve decides it (lines 962-987);
    the flags (P == 0, walk_in_lds, last_in_lds, bodies_in_lds) only for a big island (k_island_solve_big, lines 1208-1341)."""
    if nb > big_points and nb > LDS_BODIES:
        cls = BIG
    elif nb <= LDS_BODIES and P <= LDS_POINTS:
        cls = SMALL
    elif P > big_points:
        cls = BIG
    elif nb <= MID_BODIES:
        cls = MID
    else:
        cls = GLOBAL
    if cls != BIG:
        return cls, None
    if P == 0:
        return cls, dict(p0=True, walk_in_lds=False, last_in_lds=False, bodies_in_lds=False)   # (the branch leaves before the flags exist)
    return cls, dict(p0=False, walk_in_lds=12 * P + 4 * nb <= BIG_LDS_BYTES, last_in_lds=nb <= BIG_LAST_LDS, bodies_in_lds=nb <= BIG_LDS_BODIES)


def _slack(nb, P, big_points, axis, limit=64):
    """How far nb (axis 0) or P (axis 1) can move either way before route() answers differently: 0 = the next value already does."""
    here = route(nb, P, big_points)
    for d in range(1, limit + 1):
        for s in (-d, d):
            b, p = (nb + s, P) if axis == 0 else (nb, P + s)
            if b < 2 or p < 0:
                continue
            if route(b, p, big_points) != here:
                return d - 1
    return limit


def _find(parent, i):
    while parent[i] != i:
        parent[i] = parent[parent[i]]
        i = parent[i]
    return i


def classify(n, pair_hdr, plane_counts, box_counts, big_points):
    """The islands of a tick and where each went.  pair_hdr: the pair cache (lower entity index, higher entity index, points), every
    pair of it unites its two bodies whether it holds points or not; plane_counts / box_counts: points of every entity's plane
    manifold / of its obstacle manifolds.  One dict per island, ascending by lowest entity: bodies (ascending entity indices), nb, P,
    cls, flags, body_slack / point_slack (how far nb / P are from a value that is routed differently)."""
    pair_hdr = np.asarray(pair_hdr, np.int64).reshape(-1, 3)
    own = np.asarray(plane_counts, np.int64) + np.asarray(box_counts, np.int64)
    parent = list(range(n))
    for a, b, _ in pair_hdr.tolist():
        ra, rb = _find(parent, a), _find(parent, b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    members = np.unique(pair_hdr[:, :2])
    root = np.array([_find(parent, int(e)) for e in members], np.int64)
    pair_root = np.array([_find(parent, int(a)) for a in pair_hdr[:, 0]], np.int64)
    out = []
    for r in np.unique(root):
        bodies = members[root == r]
        nb = len(bodies)
        P = int(own[bodies].sum() + pair_hdr[pair_root == r, 2].sum())
        cls, flags = route(nb, P, big_points)
        out.append(dict(bodies=bodies, nb=nb, P=P, cls=cls, flags=flags, body_slack=_slack(nb, P, big_points, 0), point_slack=_slack(nb, P, big_points, 1)))
    return out


def island_rows(bodies, pair_hdr, plane_counts, box_manifold_counts):
    """The rows of an island in the solver's order (oracle/island_ref.h): bodies ascending by entity; per body its plane points, its
    obstacle manifolds, then its pairs with higher-index boxes.  (P, 2) positions in `bodies`; -1: the fixed solver body.
    box_manifold_counts[e]: the point counts of entity e's obstacle manifolds, in their order (None: no obstacles)."""
    bodies = np.asarray(bodies, np.int64)
    at = {int(e): k for k, e in enumerate(bodies)}
    pair_hdr = np.asarray(pair_hdr, np.int64).reshape(-1, 3)
    pair_hdr = pair_hdr[np.lexsort((pair_hdr[:, 1], pair_hdr[:, 0]))]
    first = np.searchsorted(pair_hdr[:, 0], bodies, "left")
    last = np.searchsorted(pair_hdr[:, 0], bodies, "right")
    rows = []
    for k, e in enumerate(bodies.tolist()):
        own = int(plane_counts[e]) + (sum(int(c) for c in box_manifold_counts[e]) if box_manifold_counts is not None else 0)
        rows += [(k, -1)] * own
        for a, b, c in pair_hdr[first[k]:last[k]].tolist():
            rows += [(k, at[b])] * c
    return np.array(rows, np.int64).reshape(-1, 2)


def level_depth(rows):
    """The number of levels of the workgroup solver's walk: level = 1 + max(last level of A, last level of B) (lines 1258-1269)."""
    rows = np.asarray(rows, np.int64).reshape(-1, 2)
    last = np.zeros(int(rows.max()) + 1 if len(rows) else 0, np.int64)
    depth = 0
    for a, b in rows.tolist():
        l = last[a]
        if b >= 0 and last[b] > l:
            l = last[b]
        l += 1
        last[a] = l
        if b >= 0:
            last[b] = l
        depth = max(depth, int(l))
    return depth


def scan_chunk(depth):
    """Elements a thread of isl_wg_scan sums for an island of that depth."""
    return (depth + 2 + WG_THREADS - 1) // WG_THREADS


# ------------------------------------------------------------------------------------------------------------------ scenes


class Case:
    """A scene: wl (synth.Workload; wl.body_type is what is uploaded), size (half extents), plane on or off, the value of
    BGE_ISLAND_BIG_POINTS, how many ticks to run and the first tick that is compared; groups: name -> entity indices of the islands
    the scene exists for; has_transform: None for a flat world."""

    def __init__(self, name, pos, euler=None, plane=True, big_points=PRODUCT_BIG_POINTS, ticks=16, compare_from=0, groups=None, seed=0x151A):
        pos = np.asarray(pos, np.float32).reshape(-1, 3)
        n = len(pos)
        self.name, self.plane, self.big_points, self.ticks, self.compare_from = name, plane, int(big_points), int(ticks), int(compare_from)
        self.wl = synth.Workload(name, synth.FLAT, n, seed)
        self.wl.pos = pos.copy()
        self.wl.euler = np.zeros((n, 3), np.float32) if euler is None else np.asarray(euler, np.float32).reshape(n, 3).copy()
        self.wl.scale = np.ones((n, 3), np.float32)
        self.wl.body_type = np.ones(n, np.uint8)
        self.size = np.full((n, 3), 0.5, np.float32)
        self.mass = np.ones(n, np.float32)
        self.has_transform = None
        self.groups = groups or {}

    @property
    def n(self):
        return self.wl.n

    @property
    def dyn(self):
        return self.wl.body_type == 1

    @property
    def static(self):
        """The scene holds Static or Kinematic bodies: obstacle manifolds exist and their points count."""
        return bool(np.isin(self.wl.body_type, (0, 2)).any())


def _stack(x, z, count):
    return [(x, 0.5 + SPACING * k, z) for k in range(count)]


def _row(x, z, count, spacing=SPACING, y=0.5):
    return [(x + spacing * k, y, z) for k in range(count)]


BOUNDARY_STACKS = (3, 4, 5, 16, 17, 20)


def boundaries():
    """Both sides of the small | mid and mid | global boundaries under the product's 128 points: stacks of 3 and 4 (small; 4 bodies
    cannot hold more than 4 + 3 x 4 = 16 points), of 5 and 16 (mid, 16 at its body limit), of 17 and 20 (the one-thread solver in
    global memory); rows of 3 at spacing 0.99 and of 4 on the plane (at most 4 bodies, more than 16 points: mid)."""
    pos, groups, at = [], {}, 0
    for k, count in enumerate(BOUNDARY_STACKS):
        pos += _stack(6.0 * k, 0.0, count)
        groups[f"stack{count}"] = np.arange(at, at + count)
        at += count
    pos += _row(0.0, 10.0, 3, spacing=0.99)
    groups["row3"] = np.arange(at, at + 3)
    at += 3
    pos += _row(10.0, 10.0, 4)
    groups["row4"] = np.arange(at, at + 4)
    return Case("boundaries", pos, ticks=16, groups=groups)


def on_a_slab():
    """Plane off, a Static slab (entity 0, top at y = 0) and a row of three boxes on it: 3 bodies whose points are 12 obstacle points
    and the pairs' — what GroundContacts does not see and BoxContacts does.  More than 16 points on 3 bodies: mid."""
    c = Case("on-a-slab", [(0.0, -0.5, 0.0)] + _row(-1.0, 0.0, 3, spacing=0.985), plane=False, ticks=16, groups={"row3": np.arange(1, 4)})
    c.wl.body_type[0] = 0
    c.size[0] = (10.0, 0.5, 10.0)
    return c


BOUNDARY_PAD = 240


def boundaries_embedded():
    """boundaries() as entities 0 .. of a world whose slot order differs from entity order (layout_cases.embedded_topology): island
    keys are root SLOT << 32 | entity.  The pad entities carry no body."""
    from .layout_cases import embedded_topology
    c = boundaries()
    n_own = c.n
    parent, ht = embedded_topology(n_own, BOUNDARY_PAD)
    n = len(parent)
    e = Case("boundaries-embedded", np.concatenate([c.wl.pos, np.zeros((n - n_own, 3), np.float32)]), ticks=c.ticks, groups=c.groups)
    e.wl.parent = parent
    e.wl.body_type[n_own:] = 255
    e.has_transform = ht
    e.n_own = n_own
    return e


N_MANY = 300                                             # more islands than the 256 threads of a 1 200-body mid launch sized by n_bodies / 5


def _grid(k, dx, dz, per_line=20):
    return dx * (k % per_line), dz * (k // per_line)


def rows_of_four():
    """300 rows of four unit boxes on the plane: 4 bodies and more than 16 points each, so 300 entries on the mid list of a world of
    1 200 island bodies."""
    pos, groups = [], {}
    for k in range(N_MANY):
        x, z = _grid(k, 8.0, 3.0)
        pos += _row(x, z, 4)
        groups[f"row{k}"] = np.arange(4 * k, 4 * k + 4)
    return Case("rows-of-four", pos, ticks=10, compare_from=5, groups=groups)


def stacks_of_five(big_points=PRODUCT_BIG_POINTS):
    """300 stacks of five: under 128 the mid list spans several blocks of 64 (every LDS lane column is used); under 0 they are 300
    big islands for the 256 workgroups' ticket loop."""
    pos, groups = [], {}
    for k in range(N_MANY):
        x, z = _grid(k, 3.0, 3.0)
        pos += _stack(x, z, 5)
        groups[f"stack{k}"] = np.arange(5 * k, 5 * k + 5)
    return Case("stacks-of-five", pos, ticks=10, compare_from=5, big_points=big_points, groups=groups)


def free_fall(count=8):
    """Boxes turned 45 degrees about y on a diagonal line, 1.2 apart in x and in z, plane off: the fed AABBs (half width 0.707 + margin)
    overlap, the boxes are 0.7 apart along their own axes and never touch; they fall freely.  One island, P == 0."""
    pos = [(1.2 * k, 5.0, 1.2 * k) for k in range(count)]
    euler = [(math.pi / 4.0, 0.0, 0.0)] * count            # (the body takes rotationEuler[0] as the turn about y: btQuaternion's yaw)
    return Case("free-fall", pos, euler=euler, plane=False, big_points=0, ticks=8, groups={"line": np.arange(count)})


def deep_row(count=40):
    """One row of 40 boxes in index order on the plane: every row of a body waits for the rows of the body before it, so the level
    walk is as deep as the island has rows, and isl_wg_scan sums more than one element a thread."""
    return Case("deep-row", _row(0.0, 0.0, count), ticks=8, compare_from=5, groups={"row": np.arange(count)})


def carpet(side, ticks, compare_from=0, seed=7):
    """side x side unit boxes on the plane, SPACING apart, entity indices shuffled against position with a fixed seed (in index order
    a carpet's depth grows with its length, and one workgroup then spends its time on barriers)."""
    ix, iz = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    pos = np.stack([ix.ravel() * SPACING, np.full(side * side, 0.5), iz.ravel() * SPACING], 1)
    order = np.random.default_rng(seed).permutation(side * side)
    return Case(f"carpet{side}", pos[order], ticks=ticks, compare_from=compare_from, groups={"carpet": np.arange(side * side)})


SPARSE_LINE = 3400


def sparse_line(count=SPARSE_LINE, seed=11):
    """A line of more than 3 072 boxes, plane off, falling freely: links alternate between touching (SPACING: a 4-point manifold) and
    AABB-only (a gap of 0.03: above the contact breaking threshold of 0.02, under the 2 x 0.02 by which the fed AABBs reach).
    About 2 points a body: the level walk fits the LDS (walk_in_lds) while the bodies' delta velocities do not (bodies_in_lds false)."""
    step = np.where(np.arange(count - 1) % 2 == 0, SPACING, 1.0 + 1.5 * AABB_MARGIN)
    x = np.concatenate([[0.0], np.cumsum(step)])
    pos = np.stack([x, np.full(count, 50.0), np.zeros(count)], 1)
    order = np.random.default_rng(seed).permutation(count)
    return Case("sparse-line", pos[order], plane=False, ticks=8, compare_from=2, groups={"line": np.arange(count)})


# the workgroup solver beyond its LDS, one regime each (big_points = 128)
BEYOND_LDS = {
    "carpet45": lambda: carpet(45, 6),        # 2 025 bodies, ~28 k points: the level walk reads the rows from global memory
    "carpet56": lambda: carpet(56, 6),        # 3 136 bodies, ~44 k points: ... and the bodies' delta velocities stay there too
    "sparse-line": sparse_line,               # 3 400 bodies, 6 800 points: the walk in LDS, the bodies not
    "carpet193": lambda: carpet(193, 2),      # 37 249 bodies, ~500 k points: not even the bodies' last levels fit
}


# ------------------------------------------------------------------------------------------------------------------ the oracle side


def oracle_counts(ref, case):
    """(pair header with entity INDICES, plane points per entity, obstacle points per entity, the point counts of every entity's
    obstacle manifolds in their order — None in a case without Static or Kinematic bodies) of the oracle's current state (ref: the
    scene helpers.build_island_oracle made of the case), from DynamicPairs, GroundContacts and BoxContacts."""
    hdr, _ = ref.DynamicPairs()
    hdr = hdr.astype(np.int64)
    hdr[:, :2] -= 1
    plane = np.zeros(case.n, np.int64)
    box = np.zeros(case.n, np.int64)
    manifolds = [()] * case.n if case.static else None
    for e in np.flatnonzero(case.dyn):
        if case.plane:
            plane[e] = ref.GroundContacts(int(e) + 1)[0]
        if case.static:
            manifolds[e] = tuple(len(rows) for _, rows in ref.BoxContacts(int(e) + 1))
            box[e] = sum(manifolds[e])
    return hdr, plane, box, manifolds


def classify_oracle(ref, case):
    """(islands, pair header, plane points per entity, obstacle manifold counts per entity or None)."""
    hdr, plane, box, manifolds = oracle_counts(ref, case)
    return classify(case.n, hdr, plane, box, case.big_points), hdr, plane, manifolds
