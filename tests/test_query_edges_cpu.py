"""Edge geometry of the query kernels without a GPU: a backward-error ("sandwich") checker built on the float64 references of
test_raycast_cpu.py and test_sphere_queries_cpu.py, the input families the GPU tests of test_gpu_query_edges.py ask the device,
and the proof that the checker bites.

The forward checkers (check_against_reference, check_casts) compare the fraction with the float64 fraction.  At grazing incidence
the fraction is ill-conditioned whatever a binary32 kernel does, so they cannot be pointed there.  The sandwich asks instead
whether the answer is the exact answer of a world whose shapes moved by at most

    B_j = N_SCALE * (|from|_1 + |delta|_1 + |origin_j|_1 + bounding radius_j [+ cast radius])

(N_SCALE of test_gpu_raycast.py: "the entry point is known to a few binary32 ulp of the ray's magnitudes").  f_out is the
reference fraction against shape j grown by B_j, f_in against it shrunk by B_j; grown contains true contains shrunk, so
f_out <= f_true <= f_in, and with tau_j = B_j / |delta|:

  closest hit (j, f, point, normal)   j's grown shape is hit (or the query starts inside the grown and outside the shrunk shape:
                                      f_out = 0); f_out - tau <= f <= f_in + tau (no upper side when the shrunk shape is
                                      missed); no other object is certainly earlier; the point lies within B_j of j's surface
                                      (a cast: the centre from + delta f within B_j of distance radius from it, too); the normal
                                      is within N_ABS + N_SCALE (...) / min_dim of the float64 outward normal at the reported
                                      point, unless that point lies within B_j of an edge, a corner or a capsule seam
  miss                                no object is certainly hit (shrunk shape hit from outside the grown shape)
  all hits                            every certain object is listed, every listed object is possible with f in its interval,
                                      the list ascends in (f, code), offsets are consistent, its head is the closest hit
  the plane                           takes part with B = N_SCALE * (|from.y| + |delta.y| + radius)

A query is UNDECIDED when the sandwich does not force the answer (closest: the winner; all hits: the set).  Per family and kind
at most 10 % may be, at least 100 must be certain hits and 30 certain misses: asserted here on the reference alone, so a GPU
failure cannot hide behind them.  Overlaps and penetrations are well conditioned (distance is 1-Lipschitz): they go through the
existing check_overlaps and the penetration comparison of test_gpu_sphere_recover.py (check_penetrations below is that
comparison, its tolerances imported); only the inputs are new.

Every tolerance here is imported from the existing test modules or exact by construction.  The families' clearances (depth inside
a corner, offset from a face) are max(1e-2 x size, 30 x B)."""
from __future__ import annotations

import collections
import copy
import functools
import math

import numpy as np
import pytest

from banggameengine_amd import world as W

from test_gpu_raycast import N_ABS, N_SCALE, P_REL
from test_raycast_cpu import (CODE_GHOST, CODE_PLANE, NO_ENTITY, RAY_BODY, RAY_GROUND, RAY_MISS, RAY_TRIGGER, World64, box_half_extents,
                              capsule_dims, quat_from_euler)
from test_sphere_queries_cpu import EPS_CLEAR, SphereRef
from test_sphere_recover_cpu import classify

ALL = 0xFFFFFFFF
N_BODIES, N_QUERIES, N_GHOSTS, N_DYNAMIC = 300, 600, 4, 6  # a full workgroup of bodies and a partial one; two LDS chunks of queries and a partial one
SKIN = 0.01
CLEAR = 30.0  # clearances of the families in units of B
MAX_UNDECIDED, MIN_HITS, MIN_MISSES = 0.10, 100, 30
KINDS = ("ray", "ray_all", "cast", "cast_all", "overlap", "penetration")

# ------------------------------------------------------------------------------------------------ the sandwich


def bounding_radius(w):
    return np.where(w.capsule, w.dims[:, 0] + w.dims[:, 1], np.linalg.norm(w.dims, axis=1))


def shifted(w, bv, sign):
    """The World64 with object j's shape grown (sign +1) or shrunk (-1) by bv[j]: a box on every half extent, a capsule on its
    radius.  An object shrunk to nothing can no longer be hit (its mask word is 0)."""
    c = copy.copy(w)
    g = sign * bv
    dims = w.dims.copy()
    dims[:, 0] += g
    dims[:, 2] += g
    dims[:, 1] += np.where(w.capsule, 0.0, g)
    gone = np.where(w.capsule, dims[:, 0], dims.min(axis=1)) <= 0
    c.dims = np.where(gone[:, None], 1.0, dims)
    c.omask = np.where(gone, 0, w.omask)
    c._derive()
    return c


def distances(w, p):
    """Distance from the point p to every object of the World64 (0 inside)."""
    q = np.einsum("nji,nj->ni", w.basis, p - w.origin)
    h = w.dims
    db = np.linalg.norm(q - np.clip(q, -h, h), axis=1)
    s = np.zeros_like(q)
    s[:, 1] = np.clip(q[:, 1], -h[:, 1], h[:, 1])
    dc = np.maximum(0.0, np.linalg.norm(q - s, axis=1) - h[:, 0])
    return np.where(w.capsule, dc, db)


def plane_interval(fy, ty, r, bp):
    """(f_out, f_in or None, certain) of the plane y = 0 for a centre moving from fy to ty with radius r, or None: never hit."""
    if fy < 0:
        fy, ty = -fy, -ty
    if fy > r + bp:
        if not ty < r + bp:
            return None
        hi = (fy - (r - bp)) / (fy - ty) if ty < r - bp else None
        return (fy - (r + bp)) / (fy - ty), hi, hi is not None
    if fy < r - bp:
        return None  # starts within the radius of it for certain
    return (0.0, None, False) if ty < r + bp else None


def code_of(kind, entity):
    return int(entity) if kind == RAY_BODY else (CODE_GHOST | int(entity) if kind == RAY_TRIGGER else CODE_PLANE)


Iv = collections.namedtuple("Iv", "lo hi tau b certain")
Query = collections.namedtuple("Query", "frm delta r md mag iv true")


class Sandwich:
    """The intervals of every query of a batch against a World64; cast = the queries are sphere casts (o, d, md, rad, mask)."""

    def __init__(self, w64, queries, cast):
        self.w, self.cast = w64, cast
        self.index = {int(c): i for i, c in enumerate(w64.code)}
        self.brad = bounding_radius(w64)
        self.o1 = np.abs(w64.origin).sum(axis=1)
        self.q = [self._one(*(a[i] for a in queries)) for i in range(len(queries[0]))]

    def only(self, i):
        """The sandwich of query i alone."""
        one = copy.copy(self)
        one.q = [self.q[i]]
        return one

    def _lists(self, w, o, d, md, r, mask):
        hits = SphereRef(w).sweep_all(o, d, md, r, mask) if self.cast else w.cast_all(o, d, md, mask)
        return [h for h in hits if h[1] != CODE_PLANE]

    def _one(self, o, d, md, *rest):
        r, mask = (float(np.float32(rest[0])), rest[1]) if self.cast else (0.0, rest[0])
        w = self.w
        frm = np.asarray(o, np.float32).astype(np.float64)
        delta = (np.asarray(d, np.float32) * np.float32(md)).astype(np.float64)
        mag = float(np.abs(frm).sum() + np.abs(delta).sum() + r)
        length = float(np.linalg.norm(delta))
        bv = N_SCALE * (mag + self.o1 + self.brad)
        wg, ws = shifted(w, bv, 1.0), shifted(w, bv, -1.0)
        true = (SphereRef(w).sweep_all(o, d, md, r, mask) if self.cast else w.cast_all(o, d, md, mask))
        f_out = {h[1]: h[0] for h in self._lists(wg, o, d, md, r, mask)}
        f_in = {h[1]: h[0] for h in self._lists(ws, o, d, md, r, mask)}
        iv = {}
        for code, lo in f_out.items():
            b = bv[self.index[code]]
            iv[code] = Iv(lo, f_in.get(code), b / length, b, code in f_in)
        # starts inside the grown shape and outside the shrunk one: it may be hit from f = 0 on, or not at all
        seen = ((w.group & int(mask)) != 0) & (w.omask != 0)
        band = seen & (distances(wg, frm) <= r) & ~((ws.omask != 0) & (distances(ws, frm) <= r))
        for k in np.nonzero(band)[0]:
            code = int(w.code[k])
            iv[code] = Iv(0.0, f_in.get(code), bv[k] / length, bv[k], False)
        if w.plane and (int(mask) & 2):
            bp = N_SCALE * (abs(frm[1]) + abs(delta[1]) + r)
            pi = plane_interval(frm[1], frm[1] + delta[1], r, bp)
            if pi is not None:
                iv[CODE_PLANE] = Iv(pi[0], pi[1], bp / length, bp, pi[2])
        return Query(frm, delta, r, float(np.float32(md)), mag, iv, true)

    # -- what the sandwich forces
    def status_closest(self, i):
        """'hit': the reference's winner is certain and everything else possible is certainly later; 'miss': nothing is possible."""
        q = self.q[i]
        if not q.iv:
            return "miss"
        if not q.true or q.true[0][1] not in q.iv:
            return "undecided"
        j = q.true[0][1]
        a = q.iv[j]
        if not a.certain:
            return "undecided"
        return "hit" if all(k == j or b.lo - b.tau > a.hi + a.tau for k, b in q.iv.items()) else "undecided"

    def status_all(self, i):
        q = self.q[i]
        if not q.iv:
            return "miss"
        return "hit" if all(a.certain for a in q.iv.values()) else "undecided"

    def counts(self, all_hits):
        c = collections.Counter((self.status_all if all_hits else self.status_closest)(i) for i in range(len(self.q)))
        return c["hit"], c["miss"], c["undecided"]

    # -- the surface of one object
    def _surface(self, q, code, f, point, normal):
        """Errors of a record's point (in units of B) and normal (as a share of its tolerance, None where the float64 normal is
        discontinuous within B of the point)."""
        a = q.iv[code]
        centre = q.frm + q.delta * f
        p = np.asarray(point, np.float64)
        if code == CODE_PLANE:
            assert (p[1] == 0.0) if self.cast else (abs(p[1]) <= a.b), f"point {p} off the plane"
            err = abs(abs(centre[1]) - q.r) / a.b if a.b > 0 else 0.0
            assert np.array_equal(normal, [0.0, 1.0 if q.frm[1] > 0 else -1.0, 0.0]), normal
            return err, 0.0
        k = self.index[code]
        w = self.w
        basis, h, cap = w.basis[k], w.dims[k], bool(w.capsule[k])

        def signed(x):
            if cap:
                s = np.array([0.0, min(max(x[1], -h[1]), h[1]), 0.0])
                return float(np.linalg.norm(x - s)) - h[0]
            e = x - np.clip(x, -h, h)
            return float(np.linalg.norm(e)) if (np.abs(x) > h).any() else -float((h - np.abs(x)).min())

        pl, cl = basis.T @ (p - w.origin[k]), basis.T @ (centre - w.origin[k])
        err = abs(signed(pl)) / a.b
        if self.cast:
            err = max(err, abs(signed(cl) - q.r) / a.b)
        x = cl if self.cast else pl
        small = w.min_dim(code)
        if cap:
            if abs(abs(x[1]) - h[1]) <= a.b:
                return err, None
            e = x - np.array([0.0, min(max(x[1], -h[1]), h[1]), 0.0])
            n = e / np.linalg.norm(e)
        else:
            gaps = np.abs(x) - h
            if self.cast and q.r > 0:
                if (np.abs(gaps) <= a.b).any():
                    return err, None
                out = gaps > 0
                assert out.any(), f"the centre {x} lies inside the box {h}"
                if out.sum() == 1:
                    n = np.where(out, np.sign(x), 0.0)
                else:
                    e = x - np.clip(x, -h, h)
                    n = e / np.linalg.norm(e)
                    small = min(small, q.r)
            else:
                order = np.argsort(gaps)
                if gaps[order[1]] >= -a.b:
                    return err, None
                n = np.zeros(3)
                n[order[2]] = 1.0 if x[order[2]] > 0 else -1.0
        n_tol = N_ABS + N_SCALE * q.mag / small
        return err, float(np.max(np.abs(np.asarray(normal, np.float64) - basis @ n))) / n_tol

    def _interval(self, q, code, f, what):
        assert code in q.iv, f"{what}: object {code:#x} is reported, its grown shape is not hit"
        a = q.iv[code]
        assert 0.0 <= f <= 1.0 and a.lo - a.tau <= f and (a.hi is None or f <= a.hi + a.tau), f"{what}: f {f} outside [{a.lo}, {a.hi}] -+ {a.tau}"
        span = max(a.lo - f, 0.0 if a.hi is None else f - a.hi, 0.0)
        return span / a.tau if a.tau > 0 else 0.0

    # -- the checks
    def check_closest(self, got):
        """The closest-hit answers of the batch; returns the worst errors (f: outside its interval, in units of tau = B / |delta|;
        forward: |f - f_true| in the same units, not asserted; point in B; normal as a share of its tolerance) and the counts."""
        ef = ep = en = fw = 0.0
        skipped = 0
        for i, q in enumerate(self.q):
            what = f"query {i}"
            kind = int(got["kind"][i])
            if kind == RAY_MISS:
                sure = [hex(k) for k, a in q.iv.items() if a.certain]
                assert not sure and got["entity"][i] == NO_ENTITY, f"{what}: a miss, {sure} are certainly hit"
                continue
            code = code_of(kind, got["entity"][i])
            f = float(got["fraction"][i])
            ef = max(ef, self._interval(q, code, f, what))
            a = q.iv[code]
            if q.true and q.true[0][1] == code:  # (reported, not asserted: the forward error of f, which grazing incidence inflates)
                fw = max(fw, abs(f - q.true[0][0]) / a.tau)
            for k, b in q.iv.items():
                assert k == code or not b.certain or not (b.hi + b.tau < a.lo - a.tau), f"{what}: {code:#x} at {f}, {k:#x} is certainly earlier ({b.hi})"
            assert got["distance"][i] == np.float32(got["fraction"][i] * np.float32(q.md)), what
            e, s = self._surface(q, code, f, got["point"][i], got["normal"][i])
            assert e <= 1.0, f"{what}: the point {got['point'][i]} is {e:.2f} B off the surface of {code:#x}"
            assert s is None or s <= 1.0, f"{what}: normal {got['normal'][i]} is {s:.2f} of its tolerance off"
            ep, en, skipped = max(ep, e), max(en, s or 0.0), skipped + (s is None)
        return dict(f=ef, forward=fw, point=ep, normal=en, normals_skipped=skipped, counts=self.counts(False))

    def check_all(self, allh, got=None):
        """The all-hits answers; got: the closest-hit answers of the same batch (the head of every list, byte for byte)."""
        off = allh["offsets"].astype(np.int64)
        assert off[0] == 0 and np.all(np.diff(off) >= 0) and off[-1] == len(allh["kind"]) and len(off) == len(self.q) + 1
        ef = 0.0
        for i, q in enumerate(self.q):
            what = f"query {i}"
            seg = slice(off[i], off[i + 1])
            codes = [code_of(k, e) for k, e in zip(allh["kind"][seg].tolist(), allh["entity"][seg].tolist())]
            fr = allh["fraction"][seg]
            assert len(set(codes)) == len(codes), f"{what}: an object listed twice"
            for k, a in q.iv.items():
                assert not a.certain or k in codes, f"{what}: {k:#x} is certainly hit and not listed"
            for code, f in zip(codes, fr.tolist()):
                ef = max(ef, self._interval(q, code, f, what))
            keys = list(zip(fr.tolist(), codes))
            assert keys == sorted(keys), f"{what}: not ascending in (f, code): {keys}"
            if got is not None:
                if off[i + 1] > off[i]:
                    for k in ("kind", "entity", "fraction", "distance"):
                        assert allh[k][off[i]] == got[k][i], (i, k)
                    assert np.array_equal(allh["point"][off[i]], got["point"][i]) and np.array_equal(allh["normal"][off[i]], got["normal"][i]), what
                else:
                    assert got["kind"][i] == RAY_MISS, what
        return dict(f=ef, counts=self.counts(True))

    # -- answers in the device's format from per-query hit lists (the reference's own: self.q[i].true)
    def answers(self, lists=None):
        lists = [q.true for q in self.q] if lists is None else lists
        n = len(lists)
        total = sum(len(h) for h in lists)
        got = dict(kind=np.zeros(n, np.uint32), entity=np.full(n, NO_ENTITY, np.uint32), fraction=np.zeros(n, np.float32),
                   distance=np.zeros(n, np.float32), point=np.zeros((n, 3), np.float32), normal=np.zeros((n, 3), np.float32))
        allh = dict(kind=np.zeros(total, np.uint32), entity=np.zeros(total, np.uint32), fraction=np.zeros(total, np.float32),
                    distance=np.zeros(total, np.float32), point=np.zeros((total, 3), np.float32), normal=np.zeros((total, 3), np.float32),
                    offsets=np.zeros(n + 1, np.uint64))
        at = 0
        for i, (q, hits) in enumerate(zip(self.q, lists)):
            for m, h in enumerate(hits):
                f = np.float32(h[0])
                p = h[5] if self.cast else q.frm + q.delta * h[0]
                for dst, k in ((allh, at),) + (((got, i),) if m == 0 else ()):
                    dst["kind"][k], dst["entity"][k], dst["fraction"][k] = h[2], h[3], f
                    dst["distance"][k] = np.float32(f * np.float32(q.md))
                    dst["point"][k], dst["normal"][k] = p, h[4]
                at += 1
            allh["offsets"][i + 1] = at
        return got, allh


def check_penetrations(w64, recs, pen):
    """The comparison of test_gpu_sphere_recover.py::test_penetration_against_the_float64_reference on any spheres (records with
    position, radius, layer_mask) and PENETRATION_HIT_DTYPE answers; returns (hits compared, misses, set aside, worst shares)."""
    n_hit = n_miss = n_aside = 0
    share_d = share_p = share_n = 0.0
    for i, (m, got) in enumerate(zip(recs, pen)):
        cands, winner_clear, normal_clear = classify(w64, m)
        if not cands:
            assert got["kind"] == RAY_MISS, f"sphere {i}: hit where the reference finds nothing near"
            n_miss += 1
            continue
        if cands[0].depth < 0 or not winner_clear:
            n_aside += 1
            continue
        h = cands[0]
        n_hit += 1
        assert (got["kind"], got["entity"]) == (h.kind, h.entity), f"sphere {i}: {got['kind']}/{got['entity']} != {h.kind}/{h.entity}"
        c = m["position"].astype(np.float64)
        tol = P_REL * (1.0 + float(np.abs(c).max()))
        ed = abs(float(got["depth"]) - h.depth) / tol
        assert ed <= 1.0, f"sphere {i}: depth {got['depth']} vs {h.depth}"
        share_d = max(share_d, ed)
        if not normal_clear:
            continue
        ep = float(np.max(np.abs(got["point"] - h.point))) / tol
        n_tol = N_ABS + N_SCALE * float(np.abs(c).sum() + m["radius"]) / min(w64.min_dim(h.code), h.cond)
        en = float(np.max(np.abs(got["normal"] - h.normal))) / n_tol
        assert ep <= 1.0 and en <= 1.0, f"sphere {i}: point {got['point']} vs {h.point}, normal {got['normal']} vs {h.normal}; shares {ep:.2f} {en:.2f}"
        share_p, share_n = max(share_p, ep), max(share_n, en)
    return dict(counts=(n_hit, n_miss, n_aside), depth=share_d, point=share_p, normal=share_n)


def check_caps(what, counts):
    hits, misses, undecided = counts
    total = hits + misses + undecided
    print(f"{what}: {hits} certain hits, {misses} certain misses, {undecided} of {total} undecided ({undecided / total:.1%})")
    assert undecided <= MAX_UNDECIDED * total and hits >= MIN_HITS and misses >= MIN_MISSES, (what, counts)


# ------------------------------------------------------------------------------------------------ the worlds of the families

# sizes log-uniform in [lo, hi] per axis on a jittered 7 x 7 x 7 grid of the given pitch, translated by offset.
#
# The far worlds ("supported range"; include/bge_world.h, "Range").  B is about 4e-6 x |origin|_1 for a query
# from nearby: 0.005 at 1e3, 0.09 at 2e4, 1.3 at 3e5, where one binary32 spacing is already 0.03.  A body thinner than B has no
# shrunk shape, so the sandwich forces nothing about it, and the clearance of 30 B the families keep (36 units at 3e5) does not
# fit inside the sizes 0.01 .. 20 there.  So every second body of a far world has the sizes 0.01 .. 20 of the shell family and
# the others the sizes `big`; the spheres (overlaps, penetrations: forward checks that scale with |centre|) are put at all of
# them, the rays and casts at the bodies IN RANGE: smallest half extent or radius >= 30 B (in_range below).  That is about a
# third of the bodies of 0.01 .. 20 at 1e3, a few of them at 1e4 and none at 1e5.  The cast and sphere radii are those of the
# shell family in every world: 0, 1e-3, 0.3, 5 and 0.05, 0.3, 1, 5.
FAMILIES = dict(
    shell=dict(seed=101, lo=0.01, hi=20.0, pitch=25.0, offset=(0.0, 0.0, 0.0), plane=True),
    far3=dict(seed=102, lo=0.01, hi=20.0, big=(1.0, 20.0), pitch=60.0, offset=(1e3, 0.0, 0.0), plane=True),
    far4=dict(seed=103, lo=0.01, hi=20.0, big=(10.0, 200.0), pitch=600.0, offset=(1e4, 0.0, 1e4), plane=True),
    far5=dict(seed=104, lo=0.01, hi=20.0, big=(100.0, 2000.0), pitch=6000.0, offset=(1e5, 1e5, 1e5), plane=False),
    scale=dict(seed=105, plane=False),
    grazing=dict(seed=106, lo=0.3, hi=1.2, pitch=4.0, offset=(0.0, 0.0, 0.0), plane=True),
)
FAR = ("far3", "far4", "far5")
N_GIANTS = 40


class Spec:
    """What is uploaded for a family: poses, body types (Static and Kinematic, a few Dynamic), shapes, sizes, the trigger
    entities, the plane.  Every body is on layer 1 with mask ALL; every query sees every layer."""

    def __init__(self, name):
        p = FAMILIES[name]
        rng = np.random.default_rng(p["seed"])
        n = N_BODIES
        self.name, self.plane = name, p["plane"]
        cells = rng.choice(343, n, replace=False)
        ijk = np.stack([cells // 49, (cells // 7) % 7, cells % 7], 1) - 3.0
        euler = rng.uniform(-math.pi, math.pi, (n, 3))
        shape = rng.integers(0, 2, n)
        if name == "scale":  # sizes 0.01 .. 0.05 about the origin, sizes 300 and 500 some thousands of units away
            pos = (ijk + rng.uniform(-0.2, 0.2, (n, 3))) * 0.4
            size = rng.choice([0.01, 0.02, 0.05], (n, 3))
            giants = rng.choice(n, N_GIANTS, replace=False)
            v = rng.normal(size=(N_GIANTS, 3))
            pos[giants] = v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(3000.0, 6000.0, (N_GIANTS, 1))
            size[giants] = rng.choice([300.0, 500.0], (N_GIANTS, 3))
        else:
            pos = (ijk + rng.uniform(-0.2, 0.2, (n, 3))) * p["pitch"] + np.asarray(p["offset"])
            size = np.exp(rng.uniform(math.log(p["lo"]), math.log(p["hi"]), (n, 3)))
        if "big" in p:
            big = rng.random(n) < 0.5
            size[big] = np.exp(rng.uniform(math.log(p["big"][0]), math.log(p["big"][1]), (int(big.sum()), 3)))
        if name == "grazing":  # most boxes unrotated, at poses and sizes whose sums are representable
            ident = (shape == 0) & (rng.random(n) < 0.6)
            euler[ident] = 0.0
            pos[ident] = np.round(pos[ident] * 64.0) / 64.0
            size[ident] = np.maximum(np.round(size[ident] * 8.0) / 8.0, 0.5)
        self.type = rng.choice([W.BODY_STATIC, W.BODY_KINEMATIC], n).astype(np.uint8)
        special = rng.choice(n, N_DYNAMIC + N_GHOSTS, replace=False)
        self.type[special[:N_DYNAMIC]] = W.BODY_DYNAMIC
        self.trig = np.sort(special[N_DYNAMIC:])
        self.type[self.trig] = W.BODY_NONE
        self.pos, self.euler = pos.astype(np.float32), euler.astype(np.float32)
        self.shape, self.size = shape.astype(np.uint8), size.astype(np.float32)
        self.layer, self.mask = np.full(n, 1, np.uint32), np.full(n, ALL, np.uint32)

    def dims(self):
        return np.array([capsule_dims(s) if c else box_half_extents(s) for c, s in zip(self.shape, self.size)])

    def world64(self):
        """The reference's world at the uploaded poses (the GPU tests take the device's poses after one tick)."""
        kind = np.full(N_BODIES, RAY_BODY)
        kind[self.trig] = RAY_TRIGGER
        quat = np.array([quat_from_euler(e.astype(np.float64)) for e in self.euler])
        return World64.from_arrays(kind, np.arange(N_BODIES), self.layer, self.mask, self.shape == 1, self.dims(), self.pos, quat, self.plane)


# ------------------------------------------------------------------------------------------------ the queries of the families


def _unit(v):
    return v / np.linalg.norm(v)


def _perp(rng, u):
    v = rng.normal(size=3)
    return _unit(v - u * (v @ u))


def _logu(rng, lo, hi):
    return lo if hi <= lo else float(np.exp(rng.uniform(math.log(lo), math.log(hi))))


def _axes(a, va, vb, vc):
    """The vector with component a = va and the two following axes vb, vc."""
    v = np.zeros(3)
    v[a], v[(a + 1) % 3], v[(a + 2) % 3] = va, vb, vc
    return v


class Batch:
    """Segments and spheres given in the frame of a body, collected in world coordinates."""

    def __init__(self, w):
        self.w = w
        self.brad = bounding_radius(w)
        self.o1 = np.abs(w.origin).sum(axis=1)
        self.segs, self.sph, self.tags = [], [], []

    def b(self, j, r, reach):
        """An upper bound of B_j for a query of radius r that stays within reach (2-norm) of the body's origin."""
        return N_SCALE * (2.0 * self.o1[j] + 2.0 * math.sqrt(3.0) * reach + self.brad[j] + r)

    def seg(self, j, a, t, length, r=0.0, tag=None):
        w = self.w
        self.segs.append((w.origin[j] + w.basis[j] @ a, w.basis[j] @ t, length, r))
        self.tags.append((tag, int(w.code[j])))

    def sphere(self, j, c, r):
        self.sph.append((self.w.origin[j] + self.w.basis[j] @ c, r))

    def rays(self):
        o, d, md, _ = (np.array(x) for x in zip(*self.segs))
        return o.astype(np.float32), d.astype(np.float32), md.astype(np.float32), np.full(len(o), ALL, np.uint32)

    def casts(self):
        o, d, md, r = (np.array(x) for x in zip(*self.segs))
        return o.astype(np.float32), d.astype(np.float32), md.astype(np.float32), r.astype(np.float32), np.full(len(o), ALL, np.uint32)

    def spheres(self):
        c, r = (np.array(x) for x in zip(*self.sph))
        return c.astype(np.float32), r.astype(np.float32), np.full(len(c), ALL, np.uint32)


def _overlap_clear(bt, j, r):
    """The band in which check_overlaps and classify set a sphere aside, three times over."""
    return 3.0 * EPS_CLEAR * (1.0 + float(np.abs(bt.w.origin[j]).max()) + bt.brad[j] + r)


def shell_case(bt, rng, j, r, hit, extra=0.0):
    """A line tangential to the outer shell of body j's bounding sphere (grown by r), through a corner of the box or the tip of
    the capsule (hit) or just outside it: (a point of closest approach P, direction t, lengths before and after P)."""
    w = bt.w
    h = w.dims[j]
    if w.capsule[j]:
        c = np.array([0.0, rng.choice([-1.0, 1.0]) * (h[0] + h[1]), 0.0])
        s, feat = np.sign(c), np.full(3, h[0])
    else:
        s = rng.choice([-1.0, 1.0], 3)
        c, feat = s * h, h
    brad = bt.brad[j]
    u = c / brad
    b = bt.b(j, r, 6.5 * (brad + r))
    d = np.maximum(np.maximum(0.01 * feat, CLEAR * b), extra)
    if hit:
        inner = c - min(d[0], h[0]) * u if w.capsule[j] else s * np.maximum(h - d, 0.0)
        dr = max(0.01 * min(r, brad), CLEAR * b, extra)
        p = c + (r - dr) * u if r > 2.0 * dr else inner
    else:
        p = c + (r + max(0.005 * brad, CLEAR * b, extra)) * u
    t = _perp(rng, _unit(p) if np.linalg.norm(p) > 0 else u)
    l1, l2 = rng.uniform(1.0, 2.0, 2) * (brad + r)
    return p, t, l1, l2


def aimed_case(bt, rng, j, r, far):
    """A segment aimed at a point in and about body j from 1.5 .. 4 bounding radii away, or from 1e3 further."""
    w = bt.w
    h = w.dims[j]
    box = np.array([h[0], h[0] + h[1], h[0]]) if w.capsule[j] else h
    target = rng.uniform(-1.2, 1.2, 3) * box
    back = _unit(rng.normal(size=3))
    dist = rng.uniform(1.5, 4.0) * (bt.brad[j] + r) + (1e3 if far else 0.0)
    return target + back * dist, -back, dist * rng.uniform(0.7, 1.5)


def in_range(bt, r):
    """The bodies whose smallest half extent or radius is at least 30 B for a query of radius r from within the reach of the
    shell recipe: the clearance of the families fits inside them (the supported range of include/bge_world.h)."""
    w = bt.w
    small = np.where(w.capsule, w.dims[:, 0], w.dims.min(axis=1))
    return np.array([small[j] >= CLEAR * bt.b(j, r, 6.5 * (bt.brad[j] + r)) for j in range(len(small))])


def shell_queries(w, rng, aimed_share):
    """Shell recipe; with aimed_share = 2 (the far worlds) every second query is of the aimed recipe instead (every fourth of
    those from 1e3 away), and the rays and casts go to the bodies in range only."""
    radii = np.array([0.0, 1e-3, 0.3, 5.0])
    sphere_radii = np.array([0.05, 0.3, 1.0, 5.0])
    live = w.omask != 0
    out = {}
    for kind in ("ray", "cast", "sphere"):
        bt = Batch(w)
        pool = np.nonzero(live & in_range(bt, float(radii.max())) if aimed_share and kind != "sphere" else live)[0]
        assert len(pool) >= 50, (kind, len(pool))
        order = rng.permutation(pool)
        for i in range(N_QUERIES):
            j = int(order[i % len(order)])
            r = 0.0 if kind == "ray" else float(radii[i % 4])
            if kind == "sphere":  # (a sphere smaller than the band in which check_overlaps sets it aside says nothing)
                r = max(float(sphere_radii[i % 4]), 4.0 * _overlap_clear(bt, j, float(sphere_radii[i % 4])))
            hit = (i // len(order)) % 2 == 0
            if aimed_share and i % aimed_share == 1:
                if kind == "sphere":
                    box = np.array([w.dims[j][0], w.dims[j][0] + w.dims[j][1], w.dims[j][0]]) if w.capsule[j] else w.dims[j]
                    bt.sphere(j, rng.uniform(-1.5, 1.5, 3) * box, max(rng.uniform(0.0, 0.5) * bt.brad[j], r))
                else:
                    bt.seg(j, *aimed_case(bt, rng, j, r, i % (4 * aimed_share) == 1), r)
                continue
            p, t, l1, l2 = shell_case(bt, rng, j, r, hit, _overlap_clear(bt, j, r) if kind == "sphere" else 0.0)
            if kind == "sphere":
                bt.sphere(j, p, r)
            else:
                bt.seg(j, p - t * l1, t, l1 + l2, r)
        out[kind] = bt.spheres() if kind == "sphere" else (bt.rays() if kind == "ray" else bt.casts())
    return out


def scale_queries(w, rng):
    """Sizes 0.01 and 500 in one world, max_distance 1e-3 .. 1e6, origins max(1e-4, 30 B) outside a surface; the casts are the
    rays with radius 0."""
    big = np.nonzero((w.omask != 0) & (bounding_radius(w) > 100.0))[0]
    small = np.nonzero((w.omask != 0) & (bounding_radius(w) < 1.0))[0]
    bt, sp = Batch(w), Batch(w)
    for i in range(N_QUERIES):
        giant = i % 3 == 2
        j = int((big if giant else small)[rng.integers(0, len(big if giant else small))])
        h = w.dims[j]
        a, sa = int(rng.integers(0, 3)), float(rng.choice([-1.0, 1.0]))
        if w.capsule[j]:
            a, half = 1, np.array([0.0, h[0] + h[1], 0.0])
        else:
            half = h
        inward = _unit(_axes(a, -sa, *rng.uniform(-0.5, 0.5, 2)))
        at = _axes(a, sa * half[a], *(rng.uniform(-0.5, 0.5, 2) * np.array([half[(a + 1) % 3], half[(a + 2) % 3]])))
        if giant:  # from 1e3 .. 3e5 before the face, max_distance up to 1e6; every fourth stops at half the way
            dist = _logu(rng, 1e3, 3e5)
            md = 0.5 * dist if i % 4 == 0 else _logu(rng, 2.0 * dist, 1e6)
            bt.seg(j, at - inward * dist, inward, md)
            sp.sphere(j, at + _axes(a, sa * rng.uniform(-200.0, 200.0), 0.0, 0.0), rng.uniform(50.0, 150.0))
        else:  # from just outside the surface inwards over 1e-3 .. 1; every fourth heads away from it
            gap = max(1e-4, CLEAR * bt.b(j, 0.0, 2.0))
            md = _logu(rng, max(1e-3, 4.0 * gap), 1.0)
            bt.seg(j, at - inward * (gap / abs(inward[a])), -inward if i % 4 == 0 else inward, md)
            r = rng.uniform(0.005, 0.05)
            off = max(0.3 * r, _overlap_clear(sp, j, r))
            sp.sphere(j, at + _axes(a, sa * (r + (off if i % 4 == 0 else -off)), 0.0, 0.0), r)
    o, d, md, mask = bt.rays()
    return dict(ray=(o, d, md, mask), cast=(o, d, md, np.zeros(len(o), np.float32), mask), sphere=sp.spheres())


def grazing_queries(w, rng):
    """Rays and casts along faces and sides at offsets of 30 B .. 1e-2 x size, tilted in by 1e-3 .. 3e-2, the move's own pattern
    (the centre at radius + skin from a face, cast along it), the seams of the rounded box, and exactly zero direction
    components against unrotated boxes, inside the slab and exactly on |o| == h."""
    live = w.omask != 0
    boxes, caps = np.nonzero(live & ~w.capsule)[0], np.nonzero(live & w.capsule)[0]
    ident = np.array([k for k in boxes if np.array_equal(w.basis[k], np.eye(3))])
    rays, casts, sph = Batch(w), Batch(w), Batch(w)
    n_exact = 0

    def pick(pool):
        return int(pool[rng.integers(0, len(pool))])

    def face(j):
        a, sa = int(rng.integers(0, 3)), float(rng.choice([-1.0, 1.0]))
        h = w.dims[j]
        return a, sa, h[a], h[(a + 1) % 3], h[(a + 2) % 3]

    def delta_of(bt, j, r, size):
        b = bt.b(j, r, 4.0 * bt.brad[j] + 12.0)
        return b, _logu(rng, CLEAR * b, 0.01 * size)

    for i in range(N_QUERIES):
        # ---- rays
        kind = i % 8
        if kind < 3:  # along a box face: outside it, inside it, tilted into it
            j = pick(boxes)
            a, sa, ha, hb, hc = face(j)
            b, dl = delta_of(rays, j, 0.0, min(ha, hb, hc))
            cc = rng.uniform(-0.8, 0.8) * hc
            if kind < 2:
                l1, l2 = rng.uniform(0.2, 1.0, 2) * hb
                rays.seg(j, _axes(a, sa * (ha + (dl if kind == 0 else -dl)), -hb - l1, cc), _axes(a, 0.0, 1.0, 0.0), 2.0 * hb + l1 + l2)
            else:
                tilt = max(_logu(rng, 1e-3, 3e-2), dl / (1.5 * hb))
                run = (dl + max(dl, CLEAR * b)) / tilt * 1.2
                rays.seg(j, _axes(a, sa * (ha + dl), -0.9 * hb, cc), _unit(_axes(a, -sa * tilt, 1.0, 0.0)), run * math.sqrt(1.0 + tilt * tilt))
        elif kind < 6:  # the same along a capsule's side
            j = pick(caps)
            rad, hh = w.dims[j][0], w.dims[j][1]
            b, dl = delta_of(rays, j, 0.0, rad)
            e = _perp(rng, np.array([0.0, 1.0, 0.0]))
            up = np.array([0.0, 1.0, 0.0])
            if kind < 5:
                l1, l2 = rng.uniform(0.2, 1.0, 2) * (hh + rad)
                rays.seg(j, e * (rad + (dl if kind == 3 else -dl)) - up * (hh + rad + l1), up, 2.0 * (hh + rad) + l1 + l2)
            else:
                tilt = max(_logu(rng, 1e-3, 3e-2), dl / (1.5 * hh))
                run = (dl + max(dl, CLEAR * b)) / tilt * 1.2
                rays.seg(j, e * (rad + dl) - up * 0.9 * hh, _unit(up - e * tilt), run * math.sqrt(1.0 + tilt * tilt))
        else:  # exactly zero direction components against an unrotated box: two zeros, or one
            j = pick(ident)
            a, sa, ha, hb, hc = face(j)
            ac, cc = rng.uniform(-0.8, 0.8) * ha, rng.uniform(-0.8, 0.8) * hc
            if kind == 6:
                bx = (a + 2) % 3
                on = np.float32(np.float32(w.origin[j][bx]) + np.float32(hc))
                if i % 32 == 6 and np.float32(on - np.float32(w.origin[j][bx])) == np.float32(hc):
                    cc, n_exact = hc, n_exact + 1  # the ray lies in the face's plane: |o| == h to the bit
                rays.seg(j, _axes(a, ac, -sa * (hb + rng.uniform(0.5, 2.0)), cc), _axes(a, 0.0, sa, 0.0), 2.0 * hb + 3.0)
            else:
                t = _unit(_axes(a, 0.0, 1.0, sa))
                rays.seg(j, _axes(a, ac, rng.uniform(-0.5, 0.5) * hb, rng.uniform(-0.5, 0.5) * hc) - t * 2.0 * rays.brad[j], t, 4.0 * rays.brad[j])
        # ---- casts
        kind = i % 8
        flip = (i // 8) % 2 == 0
        if kind in (0, 1, 2, 3, 4, 5):
            j = pick(boxes if kind != 4 or not len(ident) else (ident if flip else boxes))
            a, sa, ha, hb, hc = face(j)
        if kind == 0:  # the move's pattern: at radius + skin from the face, along it
            r = float(rng.choice([0.1, 0.3, 0.5]))
            casts.seg(j, _axes(a, sa * (ha + r + SKIN), rng.uniform(-0.9, -0.2) * hb, rng.uniform(-0.6, 0.6) * hc), _axes(a, 0.0, 1.0, 0.0),
                      _logu(rng, 0.1, 10.0), r, "along")
        elif kind == 1:  # the same, tilted so that it closes more than skin + 30 B
            r = float(rng.choice([0.1, 0.3, 0.5]))
            b = casts.b(j, r, 4.0 * casts.brad[j] + 12.0)
            run = rng.uniform(0.4, 1.2) * hb
            tilt = (SKIN + max(2.0 * CLEAR * b, 0.5 * SKIN)) / (0.7 * run)
            casts.seg(j, _axes(a, sa * (ha + r + SKIN), -0.9 * hb, rng.uniform(-0.6, 0.6) * hc), _unit(_axes(a, -sa * tilt, 1.0, 0.0)),
                      run * math.sqrt(1.0 + tilt * tilt), r, "closing")
        elif kind == 2:  # a small sphere along the face, outside by delta or inside by delta
            r = float(rng.choice([1e-3, 0.05]))
            b, dl = delta_of(casts, j, r, min(ha, hb, hc))
            l1, l2 = rng.uniform(0.2, 1.0, 2) * hb
            at = ha + r + dl if flip else (ha + r - dl if r > 2.0 * dl else ha - dl)
            casts.seg(j, _axes(a, sa * at, -hb - r - l1, rng.uniform(-0.8, 0.8) * hc), _axes(a, 0.0, 1.0, 0.0), 2.0 * (hb + r) + l1 + l2, r)
        elif kind == 3:  # beside an edge: through a point delta inside the edge's cylinder, from outside
            r = float(rng.choice([0.05, 0.3]))
            b, dl = delta_of(casts, j, r, min(ha, hb, hc))
            sc = float(rng.choice([-1.0, 1.0]))
            phi, psi = rng.uniform(math.radians(10), math.radians(80), 2)
            pm = _axes(a, sa * (ha + (r - dl) * math.cos(phi)), rng.uniform(-0.7, 0.7) * hb, sc * (hc + (r - dl) * math.sin(phi)))
            t = -_unit(_axes(a, sa * math.cos(psi), rng.uniform(-0.5, 0.5), sc * math.sin(psi)))
            dist = rng.uniform(1.0, 3.0) * casts.brad[j]
            casts.seg(j, pm - t * dist, t, dist + 0.5, r)
        elif kind == 4:  # radius 0 and radii below delta at an edge: delta inside the face, or delta past the edge
            r = float(rng.choice([0.0, 1e-4, 1e-3]))
            b, dl = delta_of(casts, j, r, min(ha, hb, hc))
            dl = max(dl, 2.0 * r)
            sc = float(rng.choice([-1.0, 1.0]))
            dist = rng.uniform(1.0, 3.0) * casts.brad[j]
            if (i // 16) % 2 == 0:
                t = _unit(_axes(a, -sa, *rng.uniform(-0.6, 0.6, 2)))
                casts.seg(j, _axes(a, sa * ha, rng.uniform(-0.7, 0.7) * hb, sc * (hc - dl)) - t * dist, t, 2.0 * dist, r)
            else:
                t = _unit(_axes(a, -sa, rng.uniform(-0.6, 0.6), 0.0))
                casts.seg(j, _axes(a, sa * ha, rng.uniform(-0.7, 0.7) * hb, sc * (hc + r + dl)) - t * dist, t, 2.0 * dist, r)
        elif kind == 5:  # starting inside the grown box beside an edge, outside the rounded box
            r = float(rng.choice([0.1, 0.3]))
            b, dl = delta_of(casts, j, r, min(ha, hb, hc))
            sc = float(rng.choice([-1.0, 1.0]))
            rho = r + dl + rng.uniform(0.0, 1.0) * max(r * (math.sqrt(2.0) - 1.0) - 2.0 * dl, 0.0)
            start = _axes(a, sa * (ha + rho / math.sqrt(2.0)), rng.uniform(-0.5, 0.5) * hb, sc * (hc + rho / math.sqrt(2.0)))
            target = _axes(a, 0.0, start[(a + 1) % 3] + rng.uniform(-0.3, 0.3) * hb, 0.0)
            casts.seg(j, start, _unit(target - start), 1.5 * float(np.linalg.norm(target - start)), r)
        elif kind == 6:  # exactly along an axis of an unrotated box: onto a face, or along it through the rounded edge
            j = pick(ident)
            a, sa, ha, hb, hc = face(j)
            r = 0.3
            ac = rng.uniform(-0.8, 0.8) * ha if flip else sa * (ha + 0.5 * r)
            casts.seg(j, _axes(a, ac, -sa * (hb + r + rng.uniform(0.5, 2.0)), rng.uniform(-0.8, 0.8) * hc), _axes(a, 0.0, sa, 0.0), 2.0 * hb + 4.0, r)
        else:  # the move's pattern along a capsule's side, straight and tilted
            j = pick(caps)
            rad, hh = w.dims[j][0], w.dims[j][1]
            r = float(rng.choice([0.1, 0.3]))
            b = casts.b(j, r, 4.0 * casts.brad[j] + 12.0)
            e, up = _perp(rng, np.array([0.0, 1.0, 0.0])), np.array([0.0, 1.0, 0.0])
            run = rng.uniform(0.4, 1.2) * hh
            tilt = 0.0 if flip else (SKIN + max(2.0 * CLEAR * b, 0.5 * SKIN)) / (0.7 * run)
            casts.seg(j, e * (rad + r + SKIN) - up * 0.9 * hh, _unit(up - e * tilt), run * math.sqrt(1.0 + tilt * tilt), r,
                      "along" if flip else "closing")
        # ---- spheres: at radius -+ delta from a face or a side
        r = float(rng.choice([0.05, 0.3, 0.5]))
        j = pick(boxes if i % 2 == 0 else caps)
        dl = max(delta_of(sph, j, r, w.dims[j].min() if i % 2 == 0 else w.dims[j][0])[1], _overlap_clear(sph, j, r))
        off = r + (dl if (i // 2) % 2 == 0 else -dl)
        if i % 2 == 0:
            a, sa, ha, hb, hc = face(j)
            sph.sphere(j, _axes(a, sa * (ha + off), rng.uniform(-0.7, 0.7) * hb, rng.uniform(-0.7, 0.7) * hc), r)
        else:
            e = _perp(rng, np.array([0.0, 1.0, 0.0]))
            sph.sphere(j, e * (w.dims[j][0] + off) + np.array([0.0, rng.uniform(-0.7, 0.7) * w.dims[j][1], 0.0]), r)
    assert n_exact >= 5, n_exact
    return dict(ray=rays.rays(), cast=casts.casts(), sphere=sph.spheres(), cast_tags=casts.tags)


def family_queries(name, w64):
    """The 600 rays, 600 casts and 600 spheres of a family: a pure function of the World64's poses."""
    rng = np.random.default_rng(FAMILIES[name]["seed"] + 1000)
    if name == "scale":
        return scale_queries(w64, rng)
    if name == "grazing":
        return grazing_queries(w64, rng)
    return shell_queries(w64, rng, 2 if name in FAR else 0)


def sphere_records(spheres):
    """The spheres as records with position, radius, layer_mask: what classify() and check_penetrations() read."""
    c, r, mask = spheres
    return W.make_sphere_recovers(c, r, SKIN, mask)


def overlap_counts(ref, spheres):
    c, r, mask = spheres
    got = [ref.overlap(c[i], r[i], mask[i]) for i in range(len(c))]
    hits = sum(1 for lst, clear in got if clear and lst)
    misses = sum(1 for lst, clear in got if clear and not lst)
    return hits, misses, len(c) - hits - misses


def penetration_answers(w64, recs):
    """The float64 reference's own penetration records (signed_ref's winner)."""
    from test_sphere_recover_cpu import signed_ref
    pen = np.zeros(len(recs), W.PENETRATION_HIT_DTYPE)
    pen["entity"] = NO_ENTITY
    for i, m in enumerate(recs):
        got = signed_ref(w64, m["position"], m["radius"], m["layer_mask"])
        if got:
            h = got[0]
            pen[i] = (h.kind, h.entity, h.depth, h.point, h.normal, 0)
    return pen


# ------------------------------------------------------------------------------------------------ the reference alone


@functools.lru_cache(maxsize=None)
def reference(name):
    """(World64 at the uploaded poses, the family's queries)."""
    w64 = Spec(name).world64()
    return w64, family_queries(name, w64)


@functools.lru_cache(maxsize=None)
def sandwich(name, cast):
    w64, qs = reference(name)
    return Sandwich(w64, qs["cast" if cast else "ray"], cast)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(FAMILIES))
def test_reference_passes_its_own_checker_inside_the_caps(name, kind):
    w64, qs = reference(name)
    if kind == "overlap":
        check_caps(f"{name} {kind}", overlap_counts(SphereRef(w64), qs["sphere"]))
    elif kind == "penetration":
        recs = sphere_records(qs["sphere"])
        check_caps(f"{name} {kind}", check_penetrations(w64, recs, penetration_answers(w64, recs))["counts"])
    else:
        sw = sandwich(name, kind.startswith("cast"))
        got, allh = sw.answers()
        res = sw.check_all(allh, got) if kind.endswith("_all") else sw.check_closest(got)
        print({k: v for k, v in res.items() if k != "counts"})
        check_caps(f"{name} {kind}", res["counts"])


def test_radius_zero_casts_of_the_scale_family_are_its_rays():
    rays, casts = sandwich("scale", False), sandwich("scale", True)
    assert not reference("scale")[1]["cast"][3].any()
    n = 0
    for a, b in zip(rays.q, casts.q):
        assert [h[1] for h in a.true] == [h[1] for h in b.true]
        assert set(a.iv) == set(b.iv) and [k for k, v in a.iv.items() if v.certain] == [k for k, v in b.iv.items() if v.certain]
        n += bool(a.true)
    assert n >= MIN_HITS


def test_the_sandwich_decides_the_moves_own_pattern():
    """A sphere at radius + skin from a face or a side, cast along it, cannot have touched that body; with a tilt that closes
    more than skin + 30 B it certainly has.  So check_closest and check_all reject a device that reports the first or drops
    the second."""
    sw = sandwich("grazing", True)
    tags = reference("grazing")[1]["cast_tags"]
    along = [i for i, (tag, _) in enumerate(tags) if tag == "along"]
    closing = [i for i, (tag, _) in enumerate(tags) if tag == "closing"]
    assert len(along) >= 100 and len(closing) >= 100
    assert all(tags[i][1] not in sw.q[i].iv for i in along)
    assert all(sw.q[i].iv[tags[i][1]].certain for i in closing)


# ------------------------------------------------------------------------------------------------ the checker bites


CLOSEST_LOST = "are certainly hit|is certainly earlier"  # what check_closest says of a miss, and of a later object, in place of a certain winner
NOT_LISTED, NOT_ASCENDING = "is certainly hit and not listed", "not ascending"
OFF = r"outside \[|off the surface"  # a fraction that leaves its interval, a point that leaves the surface


def _closest_rejected(sw, i, hits, match):
    """check_closest rejects query i, asked alone, answered with these hits, and says why."""
    one = sw.only(i)
    got, _ = one.answers([hits])
    with pytest.raises(AssertionError, match=match):
        one.check_closest(got)


def _list_rejected(sw, i, hits, match):
    one = sw.only(i)
    with pytest.raises(AssertionError, match=match):
        one.check_all(one.answers([hits])[1])


def _drops_rejected(sw, lists):
    """Lists with hits dropped, one query at a time: wherever a dropped object is certain check_all misses it, wherever the
    dropped object is the certain winner check_closest does; returns how many of each."""
    n_closest = n_listed = 0
    for i, (q, hits) in enumerate(zip(sw.q, lists)):
        if len(hits) == len(q.true):
            continue
        kept = {h[1] for h in hits}
        if any(q.iv[h[1]].certain for h in q.true if h[1] not in kept and h[1] in q.iv):
            _list_rejected(sw, i, hits, NOT_LISTED)
            n_listed += 1
        if sw.status_closest(i) == "hit" and q.true[0][1] not in kept:
            _closest_rejected(sw, i, hits, CLOSEST_LOST)
            n_closest += 1
    return n_closest, n_listed


def _approach(sw, q, code):
    """Closest approach of the query's segment to the object's centre, as a share of its bounding radius grown by the radius."""
    k = sw.index[code]
    wv = sw.w.origin[k] - q.frm
    t = min(max(float(wv @ q.delta) / float(q.delta @ q.delta), 0.0), 1.0)
    return float(np.linalg.norm(wv - t * q.delta)) / (sw.brad[k] + q.r)


@pytest.mark.parametrize("cast", [False, True], ids=["rays", "casts"])
@pytest.mark.parametrize("name", ["shell"])
def test_a_cull_one_percent_tight_is_rejected(name, cast):
    """(a) hits dropped where the closest approach to the body's centre exceeds 0.99 of the bounding radius; every dropped
    certain hit is missed by name.  (In the far worlds 30 B is more than 1 % of the sizes, so no certain hit lies in that
    shell: (b) is the mutation that applies there.)"""
    sw = sandwich(name, cast)
    lists = [[h for h in q.true if h[1] == CODE_PLANE or _approach(sw, q, h[1]) <= 0.99] for q in sw.q]
    dropped = sum(len(q.true) - len(x) for q, x in zip(sw.q, lists))
    n_closest, n_listed = _drops_rejected(sw, lists)
    print(f"{name}: {dropped} hits dropped, rejected as winners {n_closest} times and as list entries {n_listed} times")
    assert dropped >= 20 and n_closest >= 20 and n_listed >= 20


@pytest.mark.parametrize("cast", [False, True], ids=["rays", "casts"])
@pytest.mark.parametrize("name", FAR + ("scale",))
def test_a_forgotten_slack_term_is_rejected(name, cast):
    """(b) hits dropped for bodies with |origin|_1 > 1e3."""
    sw = sandwich(name, cast)
    lists = [[h for h in q.true if h[1] == CODE_PLANE or sw.o1[sw.index[h[1]]] <= 1e3] for q in sw.q]
    n_closest, n_listed = _drops_rejected(sw, lists)
    print(f"{name}: rejected as winners {n_closest} times and as list entries {n_listed} times")
    assert n_closest >= 20 and n_listed >= 20


@pytest.mark.parametrize("cast", [False, True], ids=["rays", "casts"])
@pytest.mark.parametrize("name", list(FAMILIES))
def test_a_point_ten_b_off_the_surface_is_rejected(name, cast):
    """(c) the winner's fraction moved so that its point leaves the surface by 10 B; one query at a time, every one rejected."""
    sw = sandwich(name, cast)
    tried = 0
    for i, q in enumerate(sw.q):
        if sw.status_closest(i) != "hit":
            continue
        h = q.true[0]
        closing = abs(float(h[4] @ q.delta))
        if closing == 0.0:
            continue
        f = h[0] - 10.0 * q.iv[h[1]].b / closing
        if f < 0.0:
            f = h[0] + 10.0 * q.iv[h[1]].b / closing
        if f > 1.0:
            continue
        moved = (f,) + tuple(h[1:5]) + ((q.frm + q.delta * f - q.r * h[4],) if sw.cast else ())
        _closest_rejected(sw, i, [moved] + list(q.true[1:]), OFF)
        tried += 1
    assert tried >= MIN_HITS, tried


@pytest.mark.parametrize("cast", [False, True], ids=["rays", "casts"])
@pytest.mark.parametrize("name", list(FAMILIES))
def test_the_second_closest_object_and_broken_lists_are_rejected(name, cast):
    """(e) the second-closest object reported where the first is certain (a miss where there is no second); (f) an entry of an
    all-hits list omitted, and two entries swapped.  One query at a time, every one rejected for that reason."""
    sw = sandwich(name, cast)
    sw.check_all(sw.answers()[1])
    sure = [i for i in range(len(sw.q)) if sw.status_closest(i) == "hit"]
    assert len(sure) >= MIN_HITS
    for i in sure:
        _closest_rejected(sw, i, sw.q[i].true[1:], CLOSEST_LOST)
    sure_all = [i for i in range(len(sw.q)) if sw.status_all(i) == "hit"]
    assert len(sure_all) >= MIN_HITS
    for i in sure_all:
        _list_rejected(sw, i, sw.q[i].true[:-1], NOT_LISTED)
    two = [i for i, q in enumerate(sw.q) if len(q.true) >= 2 and np.float32(q.true[0][0]) != np.float32(q.true[1][0])]
    if name not in ("scale", "far5"):  # (their rays meet one body each: short ones, and bodies 6,000 units apart)
        assert two
    for i in two:
        q = sw.q[i]
        _list_rejected(sw, i, [q.true[1], q.true[0]] + list(q.true[2:]), NOT_ASCENDING)


# ------------------------------------------------------------------------------------------------ exact ties

# (name, bodies [(size, position)], (origin, direction, max distance), radius, expected f): unrotated Static boxes whose half
# extents are their sizes (1 and 0.5 pass the margin arithmetic unchanged) at representable poses, entered at a representable f.
# Entities 1 and 3 share one pose; entities 2 and 4 differ in size and pose and have their top faces in one plane.
TIE_BODIES = [((1.0, 1.0, 1.0), (8.0, 2.0, 0.0)), ((1.0, 1.0, 1.0), (0.0, 2.0, 0.0)), ((0.5, 0.5, 0.5), (-8.0, 2.5, 0.0)),
              ((1.0, 1.0, 1.0), (0.0, 2.0, 0.0)), ((0.5, 1.0, 0.5), (-8.0, 2.0, 0.125))]
TIE_SPHERE = ((0.0, 3.25, 0.0), 0.5, 1)  # a penetration sphere over the shared pose: centre, radius, the entity that wins
# (origin, direction, max distance, radius, the entities hit at the first fraction in code order, that fraction)
TIE_QUERIES = [
    ((0.0, 7.0, 0.0), (0.0, -1.0, 0.0), 16.0, 0.0, [1, 3], 0.25),        # the shared pose from above: y = 3 at 4 of 16
    ((0.0, 7.0, 0.25), (0.0, -1.0, 0.0), 8.0, 0.5, [1, 3], 0.4375),      # the same with a sphere: centre stops at 3.5
    ((-8.0, 7.0, 0.125), (0.0, -1.0, 0.0), 16.0, 0.0, [2, 4], 0.25),     # two boxes of different size, both tops at y = 3
    ((-8.0, 7.0, 0.125), (0.0, -1.0, 0.0), 8.0, 0.5, [2, 4], 0.4375),    # the same with a sphere
    ((-4.0, 2.0, 0.0), (1.0, 0.0, 0.0), 8.0, 0.0, [1, 3], 0.375),        # the shared pose from the side
]


def tie_world64():
    objs_kind = np.full(len(TIE_BODIES), RAY_BODY)
    dims = np.array([box_half_extents(s) for s, _ in TIE_BODIES])
    quat = np.tile([0.0, 0.0, 0.0, 1.0], (len(TIE_BODIES), 1))
    n = len(TIE_BODIES)
    return World64.from_arrays(objs_kind, np.arange(n), np.full(n, 1), np.full(n, ALL), np.zeros(n, bool), dims,
                               np.array([p for _, p in TIE_BODIES], np.float64), quat, False)


def check_ties(closest_of, all_of):
    """closest_of(query) -> (entity, fraction as float32); all_of(query) -> [(entity, fraction)] in the list's order."""
    for q in TIE_QUERIES:
        want, f = q[4], np.float32(q[5])
        ent, gf = closest_of(q)
        assert ent == want[0] and np.float32(gf).tobytes() == f.tobytes(), (q, ent, gf)
        head = all_of(q)[:len(want)]
        assert [e for e, _ in head] == want and all(np.float32(x).tobytes() == f.tobytes() for _, x in head), (q, head)


def test_exact_ties_on_the_reference_and_the_checker_rejects_the_higher_entity():
    """(d) the tie rule: the lower object code wins; the lists hold both at identical fraction bits in code order."""
    w64 = tie_world64()
    assert np.array_equal(w64.dims, [[1, 1, 1], [1, 1, 1], [0.5, 0.5, 0.5], [1, 1, 1], [0.5, 1, 0.5]])
    from test_sphere_recover_cpu import signed_ref
    cands = signed_ref(w64, TIE_SPHERE[0], TIE_SPHERE[1], ALL)
    assert [c.entity for c in cands[:2]] == [1, 3] and cands[0].depth == cands[1].depth == 0.25

    def hits(q):
        o, d, md, r = q[:4]
        return SphereRef(w64).sweep_all(o, d, md, r, ALL) if r else w64.cast_all(o, d, md, ALL)

    check_ties(lambda q: (hits(q)[0][3], hits(q)[0][0]), lambda q: [(h[3], h[0]) for h in hits(q)])
    with pytest.raises(AssertionError):  # the higher entity on the tie
        check_ties(lambda q: (hits(q)[1][3], hits(q)[1][0]), lambda q: [(h[3], h[0]) for h in hits(q)])
    with pytest.raises(AssertionError):  # the list out of code order
        check_ties(lambda q: (hits(q)[0][3], hits(q)[0][0]), lambda q: [(h[3], h[0]) for h in hits(q)][1::-1])
