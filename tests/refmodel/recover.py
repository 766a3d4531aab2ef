"""The reference of sphere penetration and recovery (include/bge_world.h "Sphere penetration and recovery"): signed_ref, the
signed-distance rule in float64 on a World64; recover_ref, the Recover rule in numpy float32 scalars (written from the header, not
from the kernel) over a penetration function handed in; classify, what a comparison with signed_ref may rely on."""
from __future__ import annotations

import collections
import math

import numpy as np

from .records import PENETRATION_HIT_DTYPE, RECOVER_INVALID, RECOVER_MOVED, RECOVER_ROUNDS, RECOVER_STUCK, SPHERE_DTYPE, SPHERE_RECOVER_RESULT_DTYPE
from .rays import CODE_PLANE, NO_ENTITY, RAY_GROUND, RAY_MISS
from .spheres import EPS_CLEAR, sphere_valid
from .moves import F

# One candidate of a sphere: depth = radius - sd; gap = inside a box, how much further the runner-up face is than the nearest
# (inf elsewhere); cond = the length the normal was divided by (outside a box: sd; a capsule: the distance to its segment; inf for
# an axis normal and the plane)
Cand = collections.namedtuple("Cand", "depth code kind entity sd normal point gap cond")


def signed_ref(w64, center, radius, mask, slack=0.0):
    """The header's signed distance and outward direction of every candidate of the World64 with sd <= radius + slack, in the
    order of the penetration query: largest depth first, ties to the lowest object code.  center and radius are rounded to
    binary32 first (they are the record's), everything after is float64."""
    if not sphere_valid(center, radius, mask):
        return []
    w = w64
    c, r = np.asarray(center, np.float32).astype(np.float64), float(np.float32(radius))
    out = []
    near = ((w.origin - c) ** 2).sum(axis=1) <= (w.radius + r + slack) ** 2
    sel = np.nonzero(near & ((w.group & int(mask)) != 0) & (w.omask != 0))[0]
    if len(sel):
        B = w.basis[sel]
        q = np.einsum("nji,nj->ni", B, c - w.origin[sel])
        h, cap, rows = w.dims[sel], w.capsule[sel], np.arange(len(sel))
        with np.errstate(all="ignore"):
            # box: outside, the distance to the closest point and the direction from it; inside, the nearest face
            a = np.abs(q)
            outside = (a > h).any(axis=1)
            e = q - np.clip(q, -h, h)
            dist = np.linalg.norm(e, axis=1)
            m = h - a
            j = np.argmin(m, axis=1)  # (the first minimum: ties to the lowest axis)
            axis_n = np.zeros_like(q)
            axis_n[rows, j] = np.where(q[rows, j] < 0, -1.0, 1.0)
            ms = np.sort(m, axis=1)
            sd_box = np.where(outside, dist, -m[rows, j])
            n_box = np.where(outside[:, None], e / dist[:, None], axis_n)
            gap_box = np.where(outside, np.inf, ms[:, 1] - ms[:, 0])
            cond_box = np.where(outside, dist, np.inf)
            # capsule: the distance to the segment less the radius; on the segment itself out along the local +x
            s = np.zeros_like(q)
            s[:, 1] = np.clip(q[:, 1], -h[:, 1], h[:, 1])
            ec = q - s
            al = np.linalg.norm(ec, axis=1)
            n_cap = np.where((al > 0)[:, None], ec / al[:, None], np.array([1.0, 0.0, 0.0]))
        sd = np.where(cap, al - h[:, 0], sd_box)
        nl = np.where(cap[:, None], n_cap, n_box)
        gap = np.where(cap, np.inf, gap_box)
        cond = np.where(cap, al, cond_box)
        nw = np.einsum("nij,nj->ni", B, nl)
        for k in np.nonzero(sd <= r + slack)[0]:
            i = sel[k]
            out.append(Cand(r - sd[k], int(w.code[i]), int(w.kind[i]), int(w.entity[i]), float(sd[k]), nw[k], c - nw[k] * sd[k], float(gap[k]),
                            float(cond[k])))
    if w.plane and (int(mask) & 2) and abs(c[1]) <= r + slack:
        n = np.array([0.0, 1.0 if c[1] >= 0 else -1.0, 0.0])
        out.append(Cand(r - abs(c[1]), CODE_PLANE, RAY_GROUND, NO_ENTITY, abs(c[1]), n, c - n * abs(c[1]), math.inf, math.inf))
    out.sort(key=lambda h: (-h.depth, h.code))
    return out


def _miss(hits, i):
    hits[i] = (RAY_MISS, NO_ENTITY, 0, (0, 0, 0), (0, 0, 0), 0)


def pen_of(w64):
    """The penetration function of a World64: signed_ref's winner, rounded to the binary32 record."""
    def pen_fn(spheres):
        hits = np.zeros(len(spheres), PENETRATION_HIT_DTYPE)
        for i, s in enumerate(spheres):
            _miss(hits, i)
            got = signed_ref(w64, s["center"], s["radius"], s["layer_mask"])
            if got:
                h = got[0]
                hits[i] = (h.kind, h.entity, h.depth, h.point, h.normal, 0)
        return hits
    return pen_fn


class HalfSpacesPen:
    """An analytic penetration function: solids {x: n.x <= c}, given as (unit normal, a point of the surface, kind, entity).
    sd = n.x - c, negative inside; the deepest wins, ties to the earlier entry.  float64, rounded to the binary32 record."""

    def __init__(self, walls):
        self.walls = [(np.asarray(n, np.float64), float(np.dot(n, pt)), kind, ent) for n, pt, kind, ent in walls]

    def __call__(self, spheres):
        hits = np.zeros(len(spheres), PENETRATION_HIT_DTYPE)
        for i, s in enumerate(spheres):
            _miss(hits, i)
            if not sphere_valid(s["center"], s["radius"], s["layer_mask"]):
                continue
            c, r, best = s["center"].astype(np.float64), float(s["radius"]), None
            for n, off, kind, ent in self.walls:
                sd = float(n @ c) - off
                if sd <= r and (best is None or r - sd > best[0]):
                    best = (r - sd, sd, n, kind, ent)
            if best is not None:
                depth, sd, n, kind, ent = best
                hits[i] = (kind, ent, depth, c - n * sd, n, 0)
        return hits


def record_valid(m):
    floats = [*m["position"], m["radius"], m["skin"]]
    return bool(all(np.isfinite(v) for v in floats) and m["radius"] >= 0 and m["skin"] > 0 and m["layer_mask"] != 0)


def recover_ref(pen_fn, records):
    """The header's rule.  pen_fn(spheres: SPHERE_DTYPE[n]) -> PENETRATION_HIT_DTYPE[n] answers one pass (a sphere with layer_mask
    0 stands for one that asks nothing); it is called RECOVER_ROUNDS + 1 times."""
    n = len(records)
    out = np.zeros(n, SPHERE_RECOVER_RESULT_DTYPE)
    out["hit_entity"] = NO_ENTITY
    p = [[F(v) for v in m["position"]] for m in records]
    valid = [record_valid(m) for m in records]
    done = [not v for v in valid]

    def ask():
        spheres = np.zeros(n, SPHERE_DTYPE)
        for i in range(n):
            if not done[i]:
                spheres[i] = (p[i], records["radius"][i], records["layer_mask"][i])
        return pen_fn(spheres)

    with np.errstate(all="ignore"):
        for _ in range(RECOVER_ROUNDS):
            hits = ask()  # step 1
            for i in range(n):
                if done[i]:
                    continue
                h = hits[i]
                if h["kind"] == RAY_MISS:  # step 2
                    done[i] = True
                    continue
                e, nrm = F(h["depth"]), [F(v) for v in h["normal"]]  # step 3
                t = e + F(records["skin"][i])
                p[i] = [p[i][j] + nrm[j] * t for j in range(3)]
                out["n_pushes"][i] += 1
                out["hit_kind"][i], out["hit_entity"][i], out["hit_normal"][i], out["hit_depth"][i] = h["kind"], h["entity"], nrm, e
        hits = ask()  # after
        for i in range(n):
            if not valid[i]:
                out["flags"][i] = RECOVER_INVALID
                out["position"][i] = records["position"][i]
                continue
            if not done[i] and hits[i]["kind"] != RAY_MISS:
                out["flags"][i] |= RECOVER_STUCK
                out["remaining_depth"][i] = hits[i]["depth"]
            if out["n_pushes"][i] > 0:
                out["flags"][i] |= RECOVER_MOVED
            out["pushed"][i] = [p[i][j] - F(records["position"][i][j]) for j in range(3)]
            out["position"][i] = p[i]
    return out


DEPTH_CLEAR = 1e-4  # the runner-up object (inside a box: the runner-up face) must be further behind than this
MIN_COND = 1e-3     # a normal divided by a length below this is not compared: its error is the rounding of the centre over that length


def classify(w64, m):
    """What the comparison with the float64 reference may rely on for the sphere m of a batch (conditions on the reference alone):
    (candidates in order, winner_clear, normal_clear).  winner_clear: the deepest candidate is at least DEPTH_CLEAR inside the
    sphere and the runner-up — among everything within the overlap's band EPS_CLEAR x (1 + |centre|_inf) of the radius — is more
    than DEPTH_CLEAR behind.  normal_clear: additionally the winner's normal is well defined: inside a box the runner-up face is
    more than DEPTH_CLEAR further, elsewhere the length it is divided by is at least MIN_COND."""
    c = np.asarray(m["position"], np.float32).astype(np.float64)
    band = EPS_CLEAR * (1.0 + float(np.abs(c).max())) if np.isfinite(c).all() else 0.0
    cands = signed_ref(w64, m["position"], m["radius"], m["layer_mask"], slack=band)
    if not cands:
        return cands, True, True
    winner_clear = cands[0].depth > DEPTH_CLEAR and (len(cands) == 1 or cands[0].depth - cands[1].depth > DEPTH_CLEAR)
    return cands, winner_clear, winner_clear and cands[0].gap > DEPTH_CLEAR and cands[0].cond >= MIN_COND
