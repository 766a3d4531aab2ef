"""The reference of the sphere moves (include/bge_world.h "Sphere moves"): move_ref, the header's rule in numpy float32 scalars
(written from the header, not from the kernel) over a caster handed in, and the casters it is run on."""
from __future__ import annotations

import numpy as np

from .records import (MOVE_GROUNDED, MOVE_INVALID, MOVE_OUT_OF_SLIDES, MOVE_PROBE_HIT, MOVE_SLIDES, RAY_HIT_DTYPE, SPHERE_CAST_DTYPE,
                      SPHERE_MOVE_RESULT_DTYPE)
from .rays import NO_ENTITY, RAY_BODY, RAY_MISS

F = np.float32
REST_SQ, MIN_APPROACH = F(1e-12), F(0.0625)


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def mover_valid(m):
    floats = [*m["position"], *m["displacement"], m["radius"], m["skin"], m["probe_distance"], m["min_ground_ny"]]
    return bool(all(np.isfinite(v) for v in floats) and m["radius"] >= 0 and m["skin"] > 0 and m["probe_distance"] >= 0 and m["layer_mask"] != 0)


def move_ref(cast_fn, moves, trace=None):
    """The header's rule.  cast_fn(casts: SPHERE_CAST_DTYPE[n]) -> RAY_HIT_DTYPE[n] answers one pass (a cast with layer_mask 0
    stands for a mover that asks nothing); it is called MOVE_SLIDES + 1 times.  trace, if a dict, gets "crease": per mover,
    whether a round took the crease branch."""
    n = len(moves)
    out = np.zeros(n, SPHERE_MOVE_RESULT_DTYPE)
    zero = [F(0), F(0), F(0)]
    p = [[F(v) for v in m["position"]] for m in moves]
    r = [[F(v) for v in m["displacement"]] for m in moves]
    d0 = [list(v) for v in r]
    prev = [None] * n
    valid = [mover_valid(m) for m in moves]
    done = [not v for v in valid]
    crease = np.zeros(n, bool)
    out["hit_entity"] = NO_ENTITY
    out["ground_entity"] = NO_ENTITY
    with np.errstate(all="ignore"):
        for i in range(n):
            if not valid[i]:
                r[i] = list(zero)
        for _ in range(MOVE_SLIDES):
            casts = np.zeros(n, SPHERE_CAST_DTYPE)
            L2 = [None] * n
            for i in range(n):
                if done[i]:
                    continue
                L2[i] = _dot(r[i], r[i])
                if not L2[i] > REST_SQ:  # step 1
                    r[i], done[i] = list(zero), True
                    continue
                casts[i] = (p[i], r[i], 1.0, moves["radius"][i], moves["layer_mask"][i], 0)
            hits = cast_fn(casts)
            for i in range(n):
                if done[i]:
                    continue
                h = hits[i]
                if h["kind"] == RAY_MISS:  # step 2
                    p[i] = [p[i][j] + r[i][j] for j in range(3)]
                    r[i], done[i] = list(zero), True
                    continue
                f, nrm, skin = F(h["fraction"]), [F(v) for v in h["normal"]], F(moves["skin"][i])
                L = np.sqrt(L2[i])  # step 3
                a = -(_dot(r[i], nrm) / L)
                if not a >= MIN_APPROACH:
                    a = MIN_APPROACH
                g = f - skin / (a * L)
                if not g > 0:
                    g = F(0)
                p[i] = [p[i][j] + r[i][j] * g for j in range(3)]
                out["n_hits"][i] += 1
                out["hit_kind"][i], out["hit_entity"][i], out["hit_normal"][i] = h["kind"], h["entity"], nrm
                w = F(1) - f  # step 4
                lft = [r[i][j] * w for j in range(3)]
                dn = _dot(lft, nrm)
                s = [lft[j] - nrm[j] * dn for j in range(3)]
                m = prev[i]
                if m is not None and _dot(s, m) < 0:  # step 5
                    crease[i] = True
                    c = [m[1] * nrm[2] - m[2] * nrm[1], m[2] * nrm[0] - m[0] * nrm[2], m[0] * nrm[1] - m[1] * nrm[0]]
                    cc = _dot(c, c)
                    if not cc > REST_SQ:
                        s = list(zero)
                    else:
                        t = _dot(lft, c) / cc
                        s = [c[j] * t for j in range(3)]
                if not _dot(s, d0[i]) > 0:  # step 6
                    s = list(zero)
                r[i], prev[i] = s, nrm  # step 7
        casts = np.zeros(n, SPHERE_CAST_DTYPE)
        for i in range(n):
            if not valid[i]:
                out["flags"][i] = MOVE_INVALID
                out["position"][i] = moves["position"][i]
                continue
            if _dot(r[i], r[i]) > REST_SQ:
                out["flags"][i] |= MOVE_OUT_OF_SLIDES
                out["remaining"][i] = r[i]
            out["position"][i] = p[i]
            if moves["probe_distance"][i] > 0:
                casts[i] = (p[i], (0.0, -1.0, 0.0), moves["probe_distance"][i], moves["radius"][i], moves["layer_mask"][i], 0)
        hits = cast_fn(casts)
        for i in range(n):
            h = hits[i]
            if valid[i] and moves["probe_distance"][i] > 0 and h["kind"] != RAY_MISS:
                out["flags"][i] |= MOVE_PROBE_HIT
                out["ground_kind"][i], out["ground_entity"][i], out["ground_distance"][i] = h["kind"], h["entity"], h["distance"]
                out["ground_normal"][i] = h["normal"]
                if F(h["normal"][1]) >= F(moves["min_ground_ny"][i]):
                    out["flags"][i] |= MOVE_GROUNDED
    if trace is not None:
        trace["crease"] = crease
    return out


def _miss(hits, i):
    hits[i] = (RAY_MISS, NO_ENTITY, 0, 0, (0, 0, 0), (0, 0, 0))


def _asks(c):
    vals = [*c["origin"], *c["direction"], c["max_distance"], c["radius"]]
    return bool(c["layer_mask"] != 0 and all(np.isfinite(v) for v in vals) and c["max_distance"] > 0 and c["radius"] >= 0 and np.any(c["direction"] != 0))


class HalfSpaces:
    """An analytic caster: solids {x: n.x <= c}, given as (unit normal, a point of the surface, kind, entity).  The sphere's
    centre touches one where n.x - c = radius; a sphere that starts within the radius does not hit it (the cast's start rule);
    ties go to the earlier entry.  float64, rounded to the binary32 record."""

    def __init__(self, walls):
        self.walls = [(np.asarray(n, np.float64), float(np.dot(n, pt)), kind, ent) for n, pt, kind, ent in walls]

    def __call__(self, casts):
        hits = np.zeros(len(casts), RAY_HIT_DTYPE)
        for i, c in enumerate(casts):
            _miss(hits, i)
            if not _asks(c):
                continue
            o = c["origin"].astype(np.float64)
            d = c["direction"].astype(np.float64) * float(c["max_distance"])
            rad, best = float(c["radius"]), None
            for n, off, kind, ent in self.walls:
                d0, d1 = float(n @ o) - off, float(n @ (o + d)) - off
                if d0 > rad and d1 < rad:
                    f = (d0 - rad) / (d0 - d1)
                    if best is None or f < best[0]:
                        best = (f, n, kind, ent)
            if best is not None:
                f, n, kind, ent = best
                cc = o + d * f
                hits[i] = (kind, ent, f, F(f) * c["max_distance"], cc - rad * n, n)
        return hits


def caster_of(sweep):
    """A caster from sweep(origin, direction, max_distance, radius, mask) -> sorted touches (f, code, kind, entity, normal,
    point) of the float64 shape reference."""
    def cast_fn(casts):
        hits = np.zeros(len(casts), RAY_HIT_DTYPE)
        for i, c in enumerate(casts):
            _miss(hits, i)
            if c["layer_mask"] == 0:
                continue
            got = sweep(c["origin"], c["direction"], c["max_distance"], c["radius"], c["layer_mask"])
            if got:
                f, _, kind, ent, n, pt = got[0]
                hits[i] = (kind, ent, f, F(f) * c["max_distance"], pt, n)
        return hits
    return cast_fn


def scripted(rounds):
    """A caster that answers pass k with rounds[k] = (f, normal) for every cast that asks, and misses after the list."""
    state = {"k": 0}

    def cast_fn(casts):
        hits = np.zeros(len(casts), RAY_HIT_DTYPE)
        k = state["k"]
        state["k"] += 1
        for i, c in enumerate(casts):
            _miss(hits, i)
            if _asks(c) and k < len(rounds):
                f, n = rounds[k]
                hits[i] = (RAY_BODY, k, f, F(f) * c["max_distance"], (0, 0, 0), n)
        return hits
    return cast_fn
