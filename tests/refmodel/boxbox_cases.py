"""The box-box narrowphase's cases: pose pairs (A, B) for every detector branch of boxbox::box_box / bb::BoxBox2 and tick
sequences for every branch of the persistent-manifold cache in bp_collide / CollideBoxBox.  Shared by test_boxbox_cases_cpu.py, which
proves on the oracle's TRACE alone that every class meets its floor, and test_gpu_boxbox_paths.py, which runs them on the device.

A class is a tag read off a trace row (tags_of / cache_tags_of) — nothing here decides a class by geometry.  The generators only
PROPOSE: a seeded stream of random poses (it reaches every axis code), a seeded stream of boxes laid face on face with a yaw, a small
tilt and an overhang (clip counts, the cull, the incident-face choice), a handful of constructed ties, and seeded plans of partner
moves for the cache.  Every proposal is settled to a small penetration at its final binary32 position by bisection on the oracle's
detector, then the proposals are walked in order and one is kept where a class it shows is still below its floor.  Every kept pair is
kept a second time with the roles swapped.  Sizes are HALF extents (the collider's size)."""
from __future__ import annotations

import functools
import math

import numpy as np

from oracle import pyoracle as po

from . import boxbox64 as b64
from . import obstacle_cases as oc
from .tolerances import BOXBOX_REL

# ---- the constants the cases rest on; test_boxbox_cases_cpu.py reads them off bge_boxbox_device.hpp / bge_contact_device.hpp
FUDGE_FACTOR, FUDGE2, PARALLEL_D, MAXC, CLIP_EXIT = 1.05, 1.0e-5, 1.0e-4, 4, 8
BREAKING_PER_RADIUS = 0.02          # gContactBreakingThreshold x the shape's bounding radius
PAIR_SPACING = 8.0                  # isolated pairs: centres that far apart (ordinary sizes)
BIG_SPACING = 400.0                 # ... of the pairs with boxes of 50
PAIRS_PER_WORLD = 1000
PEN = 0.01                          # the penetration a pair is settled to (0.002 for the boxes of 0.05)

# ---- floors: tag -> how many pairs must show it
AXIS_FLOOR, FACE_FLOOR, CLIP_FLOOR = 8, 2, 2
AXIS_TAGS = [f"axis:{c}:{i}" for c in range(1, 16) for i in (0, 1)]
FACE_TAGS = [f"face:{ref}:{cn}:{la}:{sg}" for ref in ("A", "B") for cn in range(3) for la in range(3) for sg in ("-", "+")]
# combinations of (reference box, codeN, lanr, sign of nr[lanr]) that geometry forbids: none — the incident box is free to turn any of its
# three axes, either way round, towards any face of the reference box
FACE_EXCLUDED: list[tuple[str, str]] = []
CLIP_TAGS = ([f"clip:{k}" for k in range(3, 9)] + ["early8", "dropped"] + [f"cull:{side}:{c}" for side in ("lt4", "ge4") for c in (5, 6, 7, 8)]
             + ["cull-i0-nonzero"])
TIE_TAGS = ["skips:3:aligned", "skips:3:quarter-turn", "skips:1:yaw-only", "tie:equal-faces", "fudge:edge-loses", "fudge:edge-wins-just", "edge-parallel"]
# classes whose float64 margin is small BY CONSTRUCTION: undecided in the sandwich, checked bit for bit only
# (edge-parallel: the rods must be 30 .. 50 long for the edge axis to win, and at that scale its lead over the faces is below the tolerance)
EXEMPT_FROM_CAP = {"tie:equal-faces", "fudge:edge-wins-just", "edge-parallel"}
FLOORS = {**{t: AXIS_FLOOR for t in AXIS_TAGS}, **{t: FACE_FLOOR for t in FACE_TAGS}, **{t: CLIP_FLOOR for t in CLIP_TAGS}, **{t: 2 for t in TIE_TAGS}}

# Branches no input reaches, each with its argument (DESIGN.md 6b repeats them); the CPU test holds the list's length against the source
# (name, argument, the statement of oracle/boxbox_ref.h that holds the branch — None where the branch is a value, not a statement)
UNREACHABLE = [
    ("clip counts 1 and 2", "a pass of intersectRectQuad2 emits (points inside) + (edges whose ends the SAME predicate puts on different sides); round a "
     "closed polygon the sides change an even number of times, so a pass that keeps a point and drops a point emits at least 1 + 2, and one that "
     "drops none emits what it was given: from the quad's 4 every pass gives 0 or at least 3 - whatever the rounding", None),
    ("more than three edge axes skipped", "an edge axis a_i x b_j is skipped where a_i is parallel to b_j; each a_i is parallel to at most one b_j, so at "
     "most three of the nine are: aligned boxes and quarter turns skip exactly three, a yaw skips one", None),
    ("depth > breaking in addContactPoint", "the detector returns nothing where a face axis has s > 0 or an edge axis s > FLT_EPSILON, so a reported depth is "
     "-dep[j] <= 0 or the winner's s <= FLT_EPSILON / l; the least breaking threshold is 0.02 x the bounding radius of the smallest box "
     "(0.01 x sqrt 3), a thousand times that", "if (depth > m.breaking) {"),
    ("insert < 0 after sortCachedPoints", "maxIndex starts at -1 with maxVal = -1e18, and |res[0]| >= 0 > -1e18 replaces it in the first round (only a NaN "
     "would not, and localA of finite poses is finite)", "if (insert < 0) insert = 0;"),
    ("a = 1e18 in cullPoints2", "needs five or more clipped points whose polygon has an area of no more than 1.2e-7; the incident face is the one most "
     "nearly parallel to the reference face (|nr[lanr]| >= 0.577), so the quad is no sliver, and five points of a sliver-shaped CLIP would have to lie "
     "within 1e-7 of a rectangle side that the strict < already cut them at", "a = 1.0e18f; // BT_LARGE_FLOAT"),
]


# ------------------------------------------------------------------------------------------------------------------ quaternions (x, y, z, w)

def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz])


def qaxis(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    return np.concatenate([a * math.sin(0.5 * angle), [math.cos(0.5 * angle)]])


def qrot(q, v):
    x, y, z, w = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return R @ np.asarray(v, np.float64)


def euler_of(q):
    """The rotationEuler that the oracle reads back from this orientation (what a Transform would hold)."""
    q = np.asarray(q, np.float64)
    return po.transform_euler_from_quat((q / np.linalg.norm(q)).astype(np.float32)).astype(np.float64)


IDENT = np.array([0.0, 0.0, 0.0, 1.0])
E3 = np.eye(3)


def _cube24():
    gens = [qaxis(E3[k], math.pi / 2) for k in range(3)]
    seen, todo = [IDENT], [IDENT]
    while todo:
        q = todo.pop()
        for g in gens:
            r = qmul(g, q)
            if not any(min(np.abs(r - s).max(), np.abs(r + s).max()) < 1e-9 for s in seen):
                seen.append(r)
                todo.append(r)
    return seen


CUBE24 = _cube24()


def _qrandom(rng):
    q = rng.normal(size=4)
    return q / np.linalg.norm(q)


# ------------------------------------------------------------------------------------------------------------------ proposals

KINDS = ("normal", "normal", "normal", "normal", "small", "big", "far1e3", "far1e4")


def _sizes(rng, kind, shape):
    """(hA, hB) for a kind of scale and a shape of pair."""
    s = {"small": 0.1, "big": 100.0}.get(kind, 1.0)
    if shape == "cubes":
        a = b = np.full(3, rng.uniform(0.3, 0.5))
    elif shape == "squares":                                  # equal square faces, any thickness
        w = rng.uniform(0.3, 0.5)
        a, b = np.array([w, rng.uniform(0.2, 0.5), w]), np.array([w, rng.uniform(0.2, 0.5), w])
    elif shape == "a-small":
        a, b = rng.uniform(0.15, 0.3, 3), rng.uniform(0.4, 0.5, 3)
    elif shape == "a-big":
        a, b = rng.uniform(0.4, 0.5, 3), rng.uniform(0.15, 0.3, 3)
    else:                                                     # non-cubic
        a, b = rng.uniform(0.2, 0.5, 3), rng.uniform(0.2, 0.5, 3)
    return a * s, b * s


def _proposal(qa, ha, qb, hb, lat, d, kind, why):
    return dict(qa=qa, ha=ha, qb=qb, hb=hb, lat=np.asarray(lat, np.float64), d=np.asarray(d, np.float64) / np.linalg.norm(d), kind=kind, why=why)


def random_stream(count, seed=0xB0B0):
    """Random orientations, random sizes, a random direction of approach."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        kind = KINDS[i % len(KINDS)]
        ha, hb = _sizes(rng, kind, "free")
        out.append(_proposal(_qrandom(rng), ha, _qrandom(rng), hb, np.zeros(3), rng.normal(size=3), kind, "random"))
    return out


YAWS = (0.0, math.pi / 4, math.radians(5), math.radians(10), math.radians(20), math.radians(30), None)
TILTS = (0.0, 0.0, 0.002, 0.01, 0.05, 0.15)


def stacked_stream(count, seed=0x57AC):
    """A laid on a face of B: any face of B, any of the 24 ways round for A, a yaw about the contact normal (45 degrees, smaller angles, any),
    a small tilt about an axis in the face, an offset along the face up to an overhang."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        kind = KINDS[i % len(KINDS)]
        shape = ("cubes", "squares", "a-small", "a-big", "free")[int(rng.integers(5))]
        ha, hb = _sizes(rng, kind, shape)
        qb = _qrandom(rng) if rng.random() < 0.7 else IDENT
        k, side = (1, 1.0) if shape == "squares" else (int(rng.integers(3)), float(rng.choice([-1.0, 1.0])))
        c = IDENT if shape == "squares" else CUBE24[int(rng.integers(24))]
        yaw = YAWS[int(rng.integers(len(YAWS)))]
        yaw = rng.uniform(0, 2 * math.pi) if yaw is None else yaw
        tilt = TILTS[int(rng.integers(len(TILTS)))]
        in_face = E3[(k + 1) % 3] * math.cos(phi := rng.uniform(0, 2 * math.pi)) + E3[(k + 2) % 3] * math.sin(phi)
        qa = qmul(qb, qmul(qaxis(in_face, tilt), qmul(qaxis(E3[k], yaw), c)))
        over = rng.choice([0.0, 0.0, 0.5, 1.0]) * rng.uniform(0, 1, 2) * (hb[[(k + 1) % 3, (k + 2) % 3]])
        lat = qrot(qb, E3[(k + 1) % 3] * over[0] + E3[(k + 2) % 3] * over[1])
        out.append(_proposal(qa, ha, qb, hb, lat, side * qrot(qb, E3[k]), kind, f"stacked:{shape}"))
    return out


def constructed():
    """The ties and skips, and the crossed ridges that reach the d <= 0.0001 branch with an edge code winning."""
    out = []
    cube = np.full(3, 0.5)
    for k in range(3):                                         # aligned boxes, non-cubic, on each axis: three edge axes skipped
        out.append(_proposal(IDENT, np.array([0.3, 0.4, 0.5]), IDENT, np.array([0.5, 0.3, 0.4]), np.zeros(3), E3[k], "normal", "skips:3:aligned"))
    for k in range(3):                                         # a quarter turn: three again, other ones
        out.append(_proposal(qaxis(E3[k], math.pi / 2), np.array([0.3, 0.4, 0.5]), IDENT, np.array([0.5, 0.3, 0.4]), np.zeros(3), E3[(k + 1) % 3], "normal", "skips:3:quarter-turn"))
    for a in (0.3, 0.7, 1.1):                                  # a yaw alone: one
        out.append(_proposal(qaxis(E3[1], a), np.array([0.3, 0.4, 0.5]), IDENT, cube, np.zeros(3), E3[1], "normal", "skips:1:yaw-only"))
    for d in ((1, 1, 0), (0, 1, 1), (1, 0, 1), (-1, 1, 0)):    # aligned equal cubes approached along a diagonal: two face separations equal
        out.append(_proposal(IDENT, cube, IDENT, cube, np.zeros(3), d, "normal", "tie:equal-faces"))
    rng = np.random.default_rng(0xED6E)
    for i in range(24):                                        # two rods rolled 45 degrees, ridge on ridge, crossing at under 0.01 rad
        # (rods of 30 .. 50: nearly parallel boxes are nearly a problem in the plane, where a face normal always has the least penetration —
        #  only over such a length does the crossing angle cost the face axes more than the factor 1.05 costs the edge axis)
        rod_a, rod_b = np.array([rng.uniform(30.0, 50.0), 0.2, 0.2]), np.array([rng.uniform(30.0, 50.0), 0.25, 0.25])
        cross = rng.uniform(0.002, 0.009) * rng.choice([-1, 1])
        qa = qmul(qaxis(E3[1], cross), qaxis(E3[0], math.pi / 4))
        qb = qaxis(E3[0], math.pi / 4 + rng.uniform(-0.05, 0.05))
        out.append(_proposal(qa, rod_a, qb, rod_b, np.array([rng.uniform(-0.2, 0.2), 0, 0]), E3[1] * rng.choice([-1, 1]), "big", "edge-parallel"))
    return out


def swapped(p):
    return dict(qa=p["qb"], ha=p["hb"], qb=p["qa"], hb=p["ha"], lat=-p["lat"], d=-p["d"], kind=p["kind"], why=p["why"] + ":swapped")


# ------------------------------------------------------------------------------------------------------------------ settling and tags

class PairSet:
    """n pairs at their final poses: pos_a, euler_a, half_a, pos_b, euler_b, half_b (n, 3) float32; kind, why (n,); trace (the detector's
    BoxTraces of these poses), tags (n sets), model (boxbox64.solve of the trace's inputs)."""

    def __init__(self, props, centres):
        n = len(props)
        self.n, self.kind, self.why = n, np.array([p["kind"] for p in props]), np.array([p["why"] for p in props])
        self.half_a = np.array([p["ha"] for p in props], np.float32).reshape(n, 3)
        self.half_b = np.array([p["hb"] for p in props], np.float32).reshape(n, 3)
        self.euler_a = np.array([euler_of(p["qa"]) for p in props], np.float32).reshape(n, 3)
        self.euler_b = np.array([euler_of(p["qb"]) for p in props], np.float32).reshape(n, 3)
        self.pos_b = np.asarray(centres, np.float32).reshape(n, 3)
        lat = np.array([p["lat"] for p in props]).reshape(n, 3)
        d = np.array([p["d"] for p in props]).reshape(n, 3)
        pen = np.where(self.kind == "small", 0.002, PEN)
        base = self.pos_b.astype(np.float64) + lat
        lo = np.zeros(n)
        hi = np.linalg.norm(self.half_a, axis=1) + np.linalg.norm(self.half_b, axis=1) + np.linalg.norm(lat, axis=1) + 1.0
        at = lambda t: (base + d * t[:, None]).astype(np.float32)      # noqa: E731
        for _ in range(44):
            mid = 0.5 * (lo + hi)
            t = self._detect(at(mid))
            too_deep = (t.n_out > 0) & (t.depth.min(1) < -pen)
            lo, hi = np.where(too_deep, mid, lo), np.where(too_deep, hi, mid)
        self.pos_a = at(lo)
        self.trace = self._detect(self.pos_a)
        self.boxes = boxes_of(self.trace)
        self.model = b64.solve(*self.boxes)
        self.tags = tags_of(self.trace, self.model, self.why)

    def _detect(self, pos_a):
        return po.boxbox_detect(pos_a, self.euler_a, self.half_a, self.pos_b, self.euler_b, self.half_b) if self.n else po.boxbox_detect(*[np.zeros((0, 3))] * 6)

    def decided(self, rel=None):
        return self.model["margin"] > (BOXBOX_REL if rel is None else rel) * self.model["scale_local"]


def boxes_of(trace):
    """The detector's inputs of a trace as the model takes them.  The oracle's Mat3 is m[row][col] and its columns are the box's axes."""
    return trace.p1, trace.R1, trace.half1, trace.p2, trace.R2, trace.half2


def answer_of(trace):
    return dict(code=trace.code, n_out=trace.n_out, normal_on_b=trace.normal_on_b, point=trace.point, depth=trace.depth)


def tags_of(trace, model=None, why=None):
    """The classes every row of a trace shows, as a set of tags a row.  model (boxbox64.solve of the same boxes) adds the two classes
    that speak of the factor 1.05; why (the proposals' labels) lets a constructed tie claim its own tag — where the trace bears it out."""
    out = []
    for i in range(len(trace)):
        t = set()
        code, hit = int(trace.code[i]), trace.n_out[i] > 0
        skips = bin(int(trace.skip_mask[i])).count("1")
        if hit:
            t.add(f"axis:{code}:{int(trace.invert_normal[i])}")
            t.add(f"skips:{skips}")
        if hit and code <= 6:
            t.add(f"face:{'A' if code <= 3 else 'B'}:{int(trace.code_n[i])}:{int(trace.lanr[i])}:{'-' if trace.nr_sign[i] < 0 else '+'}")
            t.add(f"clip:{int(trace.n_clip[i])}")
            if trace.early8[i]:
                t.add("early8")
            if trace.cnum[i] < trace.n_clip[i]:
                t.add("dropped")
            if trace.culled[i]:
                t.add(f"cull:{'lt4' if code < 4 else 'ge4'}:{int(trace.cnum[i])}")
                if trace.cull_i0[i] != 0:
                    t.add("cull-i0-nonzero")
        if hit and code > 6 and trace.edge_parallel[i] == 1:
            t.add("edge-parallel")
        label = "" if why is None else str(why[i]).replace(":swapped", "")
        if hit and label.startswith("skips:") and label.split(":")[1] == str(skips):
            t.add(label)
        if model is not None and hit:
            v = model["v"][i]
            face_best, edge_best = np.nanmax(v[:6]), (np.nanmax(v[6:]) if not np.isnan(v[6:]).all() else -np.inf)
            tol = BOXBOX_REL * model["scale_local"][i]
            if label == "tie:equal-faces" and code <= 6 and (np.sort(v[:6])[-1] == np.sort(v[:6])[-2]) and code - 1 == int(np.nanargmax(v[:6])):
                t.add("tie:equal-faces")                      # two (or more) face separations EQUAL in the float64 model too: the first won
            if code <= 6 and edge_best > face_best + tol and edge_best * FUDGE_FACTOR < face_best - tol:
                t.add("fudge:edge-loses")                     # an edge axis has the least penetration and loses by the factor alone
            if code > 6 and 0 < edge_best * FUDGE_FACTOR - face_best < 0.01 * abs(face_best):
                t.add("fudge:edge-wins-just")
        out.append(t)
    return out


# ------------------------------------------------------------------------------------------------------------------ the detector set

def _centres(kinds):
    """Where every pair's B stands: ordinary pairs on a square lattice 8 m apart; the boxes of 50 in a row of their own 400 m apart; the far
    pairs on the same lattice moved out to 1e3 and 1e4."""
    n = len(kinds)
    side = int(math.ceil(math.sqrt(max(n, 1))))
    out = np.zeros((n, 3))
    big = 0
    for i, k in enumerate(kinds):
        if k == "big":
            out[i] = (BIG_SPACING * big, 0.0, -2000.0)
            big += 1
            continue
        out[i] = (PAIR_SPACING * (i % side), 0.0, PAIR_SPACING * (i // side))
        if k == "far1e3":
            out[i] += (1000.0, 0.0, 1000.0)
        if k == "far1e4":
            out[i] += (0.0, 0.0, 10000.0)
    return out


def _pick(props, slack=2):
    """Walk the proposals (settled at the origin first) and keep one where a class it shows is below its floor + slack; decided pairs
    only, except for the classes that are ties by construction."""
    trial = PairSet(props, np.zeros((len(props), 3)))
    also = PairSet([swapped(p) for p in props], np.zeros((len(props), 3)))
    ok, ok2 = trial.decided(4 * BOXBOX_REL), also.decided(4 * BOXBOX_REL)
    have = {t: 0 for t in FLOORS}
    keep = []
    for i in range(len(props)):
        mine = (trial.tags[i] | also.tags[i]) & set(FLOORS)
        exempt = bool(mine & EXEMPT_FROM_CAP)
        if not (trial.trace.n_out[i] > 0 and also.trace.n_out[i] > 0) or not (exempt or (ok[i] and ok2[i])):
            continue
        mine = mine & EXEMPT_FROM_CAP or mine
        if any(have[t] < FLOORS[t] + slack for t in mine):
            keep.append(i)
            for ts in (trial.tags[i], also.tags[i]):
                for t in (ts & EXEMPT_FROM_CAP or ts) & set(FLOORS):
                    have[t] += 1
    return keep


@functools.lru_cache(maxsize=None)
def detector_set():
    """The detector's pairs, every one followed by its swap: PairSet."""
    props = constructed() + random_stream(3000) + stacked_stream(5000)
    keep = _pick(props)
    both = [q for i in keep for q in (props[i], swapped(props[i]))]
    return PairSet(both, _centres([p["kind"] for p in both]))


def tag_counts(tags, decided=None):
    """tag -> (pairs that show it, of them undecided).  A pair that is a tie by construction (a tag of EXEMPT_FROM_CAP) counts for those
    tags alone: it neither fills the floor of an ordinary class nor weighs on its cap."""
    out = {}
    for i, ts in enumerate(tags):
        for t in (ts & EXEMPT_FROM_CAP or ts):
            a, b = out.get(t, (0, 0))
            out[t] = (a + 1, b + (0 if decided is None or decided[i] else 1))
    return out


# ------------------------------------------------------------------------------------------------------------------ worlds

OBSTACLE, ISLAND = "obstacle", "island"


def world_of(ps, path, rows=None, name="boxbox", partner=oc.STATIC):
    """The pairs `rows` of a PairSet as one scene: entity 2 k is A (Dynamic), 2 k + 1 is B — Static (or Kinematic) on the obstacle
    path, Dynamic on the island path; plane off, one tick.  An oc.Case; .rows says which pair every couple of entities is."""
    rows = np.arange(ps.n) if rows is None else np.asarray(rows)
    m = len(rows)
    pos, euler, half = (np.empty((2 * m, 3), np.float32) for _ in range(3))
    pos[0::2], pos[1::2] = ps.pos_a[rows], ps.pos_b[rows]
    euler[0::2], euler[1::2] = ps.euler_a[rows], ps.euler_b[rows]
    half[0::2], half[1::2] = ps.half_a[rows], ps.half_b[rows]
    types = np.full(2 * m, oc.DYNAMIC, np.uint8)
    if path == OBSTACLE:
        types[1::2] = partner
    c = oc.Case(f"{name}-{path}", pos, half, types, euler=euler, plane=False, ticks=1)
    c.static = path == OBSTACLE
    c.path, c.rows = path, rows
    c.dyn = types == oc.DYNAMIC
    return c


def worlds_of(ps, path):
    """As few worlds as the pairs' number allows, PAIRS_PER_WORLD at most in each."""
    parts = -(-ps.n // PAIRS_PER_WORLD)
    return [world_of(ps, path, np.arange(ps.n)[k::parts], name=f"boxbox{k}") for k in range(parts)]


def scene_trace(ref, case, strict=True):
    """The trace of the scene's last tick, one row a pair of the case, in the case's order.  A pair that was not collided (its fed AABBs
    no longer overlap) fails under strict, else it is a row of zeros: ran = 0."""
    t = ref.BoxTrace() if case.path == OBSTACLE else ref.PairTrace()
    at = {(int(a), int(b)): i for i, (a, b) in enumerate(t.key)}
    idx = np.array([at.get((2 * k + 1, 2 * k + 2), -1) for k in range(len(case.rows))], np.int64)
    missing = np.flatnonzero(idx < 0)
    assert not (strict and len(missing)), f"{case.name}: pairs {missing[:8].tolist()} were not collided"
    ints, floats = np.zeros((len(idx), 40), np.int32), np.zeros((len(idx), 50), np.float32)
    ints[idx >= 0], floats[idx >= 0] = t._ints[idx[idx >= 0]], t._floats[idx[idx >= 0]]
    return po.BoxTraces(np.stack([2 * np.arange(len(idx)) + 1, 2 * np.arange(len(idx)) + 2], 1).astype(np.uint32), ints, floats)


# ------------------------------------------------------------------------------------------------------------------ the cache's sequences

SEQ_TICKS = 10
DT = float(np.float32(0.0083333333))
CACHE_TAGS = (["replace-carry"] + [f"append:{n}" for n in (1, 2, 3)] + [f"sort:{i}:{who}" for i in range(4) for who in ("new-deepest", "cached-deepest")]
              + ["remove:distance", "remove:drift", "remove:last", "remove:not-last", "emptied-refilled", "fmin"])
CACHE_FLOORS = {t: (1 if t.startswith("sort:") else 2) for t in CACHE_TAGS}   # (every evicted index x who is deepest: at least once)
MODES = [(path, basis) for path in (OBSTACLE, ISLAND) for basis in (False, True)]


def sequence_proposals(count, seed=0xCAC4E):
    """A on top of B with a yaw and a small tilt, the contact patch set by the smaller face, by both (crossed bars) or by an overhang; then a
    plan: B is moved between ticks — sideways by 0.5 .. 4 breaking thresholds (and a little towards A), away along the normal by 3, back — and A may be given a
    sliding velocity after the first tick (friction: the lateral impulse is not zero) or a spin."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        shape = ("a-big", "a-small", "bars", "overhang")[i % 4]
        u = rng.uniform(0.8, 1.2)
        if shape == "a-big":
            ha, hb = np.array([0.5, 0.3, 0.5]) * u, np.array([0.25, 0.3, 0.2]) * u
        elif shape == "a-small":
            ha, hb = np.array([0.2, 0.3, 0.25]) * u, np.array([0.5, 0.3, 0.5]) * u
        elif shape == "bars":
            ha, hb = np.array([0.15, 0.2, 0.6]) * u, np.array([0.6, 0.25, 0.15]) * u
        else:
            ha, hb = np.array([0.4, 0.3, 0.4]) * u, np.array([0.45, 0.35, 0.45]) * u
        lat = np.array([rng.uniform(0.2, 0.5), 0.0, rng.uniform(-0.3, 0.3)]) if shape == "overhang" else np.array([rng.uniform(-0.05, 0.05), 0.0, rng.uniform(-0.05, 0.05)])
        tilt = float(rng.choice([0.0, 0.004, 0.02]))
        phi = rng.uniform(0, 2 * math.pi)
        qa = qmul(qaxis([math.cos(phi), 0.0, math.sin(phi)], tilt), qaxis(E3[1], rng.uniform(0, math.pi / 2)))
        p = _proposal(qa, ha, IDENT, hb, lat, E3[1], "normal", f"sequence:{shape}")
        b = BREAKING_PER_RADIUS * min(np.linalg.norm(ha), np.linalg.norm(hb))
        moves, total = {}, np.zeros(3)
        for t in sorted(rng.choice(np.arange(2, 8), int(rng.integers(1, 4)), replace=False).tolist()):
            what = rng.choice(["side", "side", "side-up", "side-up", "away", "back"])
            if what in ("side", "side-up"):
                a = rng.uniform(0, 2 * math.pi)
                delta = float(rng.choice([0.5, 1.2, 2.0, 4.0])) * b * np.array([math.cos(a), 0.0, math.sin(a)])
                if what == "side-up":                         # ... and towards A: the new points are deeper than every cached one
                    delta[1] = float(rng.choice([0.15, 0.3, 0.6])) * b
            elif what == "away":
                delta = np.array([0.0, -3.0 * b, 0.0])
            else:
                delta = -total
            if np.abs(delta).max() > 0:
                moves[int(t)] = delta
                total = total + delta
        p["moves"] = moves
        p["slide"] = np.array([rng.uniform(-0.4, 0.4), 0.0, rng.uniform(-0.4, 0.4)]) if rng.random() < 0.5 else None
        p["spin"] = (int(rng.integers(2, 6)), float(rng.uniform(1.0, 3.0))) if rng.random() < 0.3 else None
        out.append(p)
    return out


class SeqSet(PairSet):
    """Pairs with a plan each: moves[k] = {tick: B's displacement before that tick}, slide[k] (A's velocity change after the first tick, or
    None), spin[k] = (tick, yaw rate given to A before that tick) or None.  pen: the settled penetration."""

    def __init__(self, props, centres):
        super().__init__(props, centres)
        self.moves, self.slide, self.spin = [p["moves"] for p in props], [p["slide"] for p in props], [p["spin"] for p in props]


def seq_world(seq, path):
    c = world_of(seq, path, name="boxbox-cache", partner=oc.KINEMATIC)
    c.ticks = SEQ_TICKS
    return c


def seq_edits(seq, case, tick, ref):
    """The edits before a tick, the same for the oracle and the device: ("trs", entity, pos) re-poses a Kinematic B; ("vel", entity, lin, ang)
    sets a velocity — B's pulse on the island path and A's slide and spin are ADDED to what the oracle's body has at that moment, which the
    device's body has too, bit for bit."""
    out = []
    for k in range(len(case.rows)):
        ea, eb = 2 * k, 2 * k + 1
        mv = seq.moves[case.rows[k]]
        if case.path == OBSTACLE:
            if tick in mv:
                total = sum((d for t, d in mv.items() if t <= tick), np.zeros(3))
                out.append(("trs", eb, (seq.pos_b[case.rows[k]].astype(np.float64) + total).astype(np.float32)))
        else:
            pulse = (mv.get(tick, np.zeros(3)) - mv.get(tick - 1, np.zeros(3))) / DT
            if np.abs(pulse).max() > 0:
                body = ref.GetBody(eb + 1)
                out.append(("vel", eb, (body["linvel"].astype(np.float64) + pulse).astype(np.float32), body["angvel"]))
        slide, spin = seq.slide[case.rows[k]], seq.spin[case.rows[k]]
        add_l = slide if (slide is not None and tick == 1) else None
        add_a = np.array([0.0, spin[1], 0.0]) if (spin is not None and tick == spin[0]) else None
        if add_l is not None or add_a is not None:
            body = ref.GetBody(ea + 1)
            lin = body["linvel"] if add_l is None else (body["linvel"].astype(np.float64) + add_l).astype(np.float32)
            ang = body["angvel"] if add_a is None else (body["angvel"].astype(np.float64) + add_a).astype(np.float32)
            out.append(("vel", ea, lin, ang))
    return out


def apply_edits_to_oracle(ref, edits):
    for ed in edits:
        if ed[0] == "trs":
            ref.SetTRS(int(ed[1]) + 1, pos=np.asarray(ed[2], np.float32))
        else:
            ref.SetVelocity(int(ed[1]) + 1, np.asarray(ed[2], np.float32), np.asarray(ed[3], np.float32))


def build_oracle(case, basis):
    """The oracle's scene of a world_of / seq_world case, the trace on."""
    from oracle.pyoracle import ORIENT_BASIS, ORIENT_IDEAL, RefScene
    ref = RefScene()
    ref.SetPhysicsOptions(-9.81, ORIENT_BASIS if basis else ORIENT_IDEAL, False)
    n = case.n
    ref.bulk_build(np.full(n, -1, np.int32), case.wl.pos, case.wl.euler, case.wl.scale, body_type=case.wl.body_type, size=case.size, mass=case.mass)
    ref.SetGroundPlane(False)
    ref.SetStaticContacts(case.path == OBSTACLE)
    ref.SetDynamicContacts(case.path == ISLAND)
    ref.SetBoxTrace(True)
    return ref


def manifolds_of(ref, case):
    """(m, 4, 12) rows and (m,) counts of every pair's manifold, in the case's order."""
    m = len(case.rows)
    rows, cnt = np.zeros((m, 4, 12), np.float32), np.zeros(m, np.int64)
    if case.path == OBSTACLE:
        for k in range(m):
            for other, r in ref.BoxContacts(2 * k + 1):
                if other == 2 * k + 2:
                    rows[k, :len(r)], cnt[k] = r, len(r)
    else:
        hdr, pts = ref.DynamicPairs()
        for (a, b, c), r in zip(hdr.tolist(), pts):
            if b == a + 1 and a % 2 == 1:
                rows[(a - 1) // 2], cnt[(a - 1) // 2] = r, c
    return rows, cnt


def answer_of_manifold(rows, cnt, trace):
    """A manifold after its first tick (the oracle's, or the device's download) as the detector's answer in world coordinates:
    pointInWorld = B's pose applied to localB (float64, on the float32 poses the detector took), the normal of the first point, the
    refreshed distances as depths, the code read off the normal."""
    p2, R2 = trace.p2.astype(np.float64), trace.R2.astype(np.float64)
    point = p2[:, None, :] + np.einsum("nij,nkj->nki", R2, rows[:, :, 3:6].astype(np.float64))
    a = dict(n_out=np.asarray(cnt, np.int64), normal_on_b=rows[:, 0, 6:9].astype(np.float64), point=point, depth=rows[:, :, 9].astype(np.float64))
    a["code"] = b64.infer_code(boxes_of(trace), a["normal_on_b"])
    return a


def cache_tags_of(trace, before_rows, before_cnt):
    """The cache classes every row of a tick's trace shows; before_rows / before_cnt: the manifolds as the tick found them."""
    out = []
    for i in range(len(trace)):
        t = set()
        if not trace.ran[i]:
            out.append(t)
            continue
        R1, p1 = trace.R1[i].astype(np.float64), trace.p1[i].astype(np.float64)
        b_own = BREAKING_PER_RADIUS * np.array([np.linalg.norm(trace.half1[i].astype(np.float64)), np.linalg.norm(trace.half2[i].astype(np.float64))])
        for k in range(int(trace.n_out[i])):
            act, idx = int(trace.action[i, k]), int(trace.index[i, k])
            if act == po.ACT_REPLACED and idx < before_cnt[i] and before_rows[i, idx, 10] != 0 and before_rows[i, idx, 11] != 0:
                t.add("replace-carry")                            # (a row of before the tick, both of its impulses not zero)
            if act == po.ACT_APPENDED:
                t.add(f"append:{idx}")
            if act == po.ACT_SORTED_IN:
                t.add(f"sort:{idx}:{'new-deepest' if trace.max_pen[i, k] == -1 else 'cached-deepest'}")
            if act in (po.ACT_APPENDED, po.ACT_SORTED_IN) and before_cnt[i] and b_own.max() > 1.2 * b_own.min():
                # the smaller of the two thresholds decided: under the larger one this point would have replaced a cached one
                on_a = trace.point[i, k].astype(np.float64) + trace.normal_on_b[i].astype(np.float64) * float(trace.depth[i, k])
                near = np.linalg.norm(before_rows[i, :before_cnt[i], 0:3].astype(np.float64) - R1.T @ (on_a - p1), axis=1).min()
                if 1.05 * b_own.min() < near < 0.95 * b_own.max():
                    t.add("fmin")
        for r in range(int(trace.n_removed[i])):
            t.add("remove:distance" if trace.reason[i, r] == po.REMOVED_BY_DISTANCE else "remove:drift")
            t.add("remove:last" if trace.was_last[i, r] else "remove:not-last")
        out.append(t)
    return out


def run_sequences(seq, path, basis, ticks=SEQ_TICKS):
    """The sequences on the oracle alone: tags[k] = the cache classes pair k shows over the ticks (with "emptied-refilled" where its manifold
    held points, then none, then points again), counts (ticks, m), and what the trace says that must never happen: `never`."""
    case = seq_world(seq, path)
    ref = build_oracle(case, basis)
    m = len(case.rows)
    tags = [set() for _ in range(m)]
    counts = np.zeros((ticks, m), np.int64)
    never = dict(skipped=0, insert_below_zero=0, area_guard=0)
    for tick in range(ticks):
        apply_edits_to_oracle(ref, seq_edits(seq, case, tick, ref))
        rows, cnt = manifolds_of(ref, case)
        ref.PhysicsSystemUpdate(DT)
        ref.TransformSystemUpdate()
        tr = scene_trace(ref, case, strict=False)
        for k, ts in enumerate(cache_tags_of(tr, rows, cnt)):
            tags[k] |= ts
        never["skipped"] += int((tr.action == po.ACT_SKIPPED).sum())
        never["insert_below_zero"] += int(((tr.action == po.ACT_SORTED_IN) & (tr.index < 0)).sum())
        never["area_guard"] += int((tr.culled == 2).sum())
        counts[tick] = manifolds_of(ref, case)[1]
    for k in range(m):
        c = counts[:, k]
        held = np.flatnonzero(c > 0)
        if len(held) and (c[held[0]:held[-1] + 1] == 0).any():
            tags[k].add("emptied-refilled")
    ref.close()
    return tags, counts, never


@functools.lru_cache(maxsize=None)
def sequence_set(proposals=960):
    """The cache's sequences: of the seeded plans, those that bring a class below its floor up on one of the two paths in one of the two
    schemes (MODES) — the floors hold in each of the four.  Every plan keeps the centre it was searched at (isolated pairs do not see
    each other, so the subset behaves as the whole did)."""
    props = sequence_proposals(proposals)
    centres = _centres(["normal"] * len(props))
    trial = SeqSet(props, centres)
    by_mode = [run_sequences(trial, path, basis)[0] for path, basis in MODES]
    have = [{t: 0 for t in CACHE_FLOORS} for _ in MODES]
    keep = []
    for i in range(len(props)):
        if any(have[m][t] < CACHE_FLOORS[t] + 1 for m in range(len(MODES)) for t in by_mode[m][i] & set(CACHE_FLOORS)):
            keep.append(i)
            for m in range(len(MODES)):
                for t in by_mode[m][i] & set(CACHE_FLOORS):
                    have[m][t] += 1
    return SeqSet([props[i] for i in keep], centres[keep])
