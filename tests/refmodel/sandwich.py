"""The backward-error ("sandwich") checker of the edge-geometry tests: an answer is accepted iff it is the exact
float64 answer of a world whose shapes and poses are within the stated binary32 bounds of the one given."""
from __future__ import annotations

import collections
import copy

import numpy as np

from .tolerances import N_ABS, N_SCALE, P_REL
from .rays import CODE_GHOST, CODE_PLANE, NO_ENTITY, RAY_BODY, RAY_MISS, RAY_TRIGGER
from .spheres import SphereRef
from .recover import classify

SKIN = 0.01
CLEAR = 30.0  # clearances of the families in units of B
MAX_UNDECIDED, MIN_HITS, MIN_MISSES = 0.10, 100, 30


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
