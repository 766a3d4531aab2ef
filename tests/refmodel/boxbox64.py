"""The box-box narrowphase as geometry, in float64: what the 15-axis separating-axis test of Bullet's dBoxBox2 must answer
for two boxes given as data, and a checker that holds an answer (normal, points, depths) against it as a sandwich.  numpy alone:
nothing of the product, nothing of the oracle.  The device was ported from the oracle's restatement, so device == oracle cannot see
an error the two share; this model shares none of their expressions' order, only Bullet's RULE for the winner:

    faces 1 .. 6 in order, a later one wins by strict >;  edge axes 7 .. 15 (a_i x b_j, code 7 + 3 i + j) normalised, skipped where
    the cross product is no longer than FLT_EPSILON, with 1e-5 added to every |R_ij| of their extents, winning where
    s * 1.05 > the best so far.

A box is (p, R, h): the float32 origin, the basis whose COLUMNS are the box's axes, the half extents with margin.  Everything takes
batches: p (n, 3), R (n, 3, 3), h (n, 3).

Scales.  Every check is relative, and a tolerance is a fraction (tolerances.BOXBOX_REL) of one of two scales of a pair.  The detector
works on p2 - p1, which binary32 forms exactly for boxes that touch, and on the half extents: `scale_local` = the largest of |p2 - p1|
and the half extents holds the DECISIONS (the winner's margin) and the depths.  Its points leave it in world coordinates: `scale` =
the largest coordinate magnitude, origins included, holds every check of a point's place.  The closest points of two edge lines are
conditioned by 1 / d, d = 1 - (ua . ub)^2 (the detector divides by it): their allowance is tol / d; at d <= 0.0001 the detector takes
alpha = beta = 0 and reports an END of box 2's supporting edge, which is what the checker then asks for."""
from __future__ import annotations

import numpy as np

FUDGE_FACTOR, FUDGE2, EPSILON = 1.05, 1.0e-5, 1.1920928955078125e-7   # dBoxBox2's fudge_factor and fudge2; SIMD_EPSILON = FLT_EPSILON
PARALLEL_D = 1.0e-4                                                   # dLineClosestApproach: alpha = beta = 0 where d <= 0.0001


def _f64(*a):
    return tuple(np.asarray(x, np.float64) for x in a)


def scale_of(p1, h1, p2, h2):
    p1, h1, p2, h2 = _f64(p1, h1, p2, h2)
    return np.maximum(np.maximum(np.abs(p1).max(-1), np.abs(p2).max(-1)), np.maximum(h1.max(-1), h2.max(-1)))


def scale_local_of(p1, h1, p2, h2):
    p1, h1, p2, h2 = _f64(p1, h1, p2, h2)
    return np.maximum(np.abs(p2 - p1).max(-1), np.maximum(h1.max(-1), h2.max(-1)))


def separations(p1, R1, h1, p2, R2, h2):
    """The 15 candidate axes.  v (n, 15): the signed separation along each (negative: overlap), edge axes normalised — NaN where the
    axis is skipped; raw (n, 15): the same before the normalisation (what the separation tests see); axis (n, 15, 3): the unit axis
    in the world, pointing from box 1 to box 2."""
    p1, R1, h1, p2, R2, h2 = _f64(p1, R1, h1, p2, R2, h2)
    n = len(p1)
    p = p2 - p1
    pp = np.einsum("nij,ni->nj", R1, p)                     # p in box 1's frame
    R = np.einsum("nki,nkj->nij", R1, R2)                   # R_ij = a_i . b_j
    Q = np.abs(R)
    v, raw, axis = np.full((n, 15), np.nan), np.zeros((n, 15)), np.zeros((n, 15, 3))
    for i in range(3):
        e = pp[:, i]
        raw[:, i] = np.abs(e) - (h1[:, i] + (h2 * Q[:, i, :]).sum(1))
        axis[:, i] = R1[:, :, i] * np.where(e < 0, -1.0, 1.0)[:, None]
    for j in range(3):
        e = np.einsum("ni,ni->n", R2[:, :, j], p)
        raw[:, 3 + j] = np.abs(e) - ((h1 * Q[:, :, j]).sum(1) + h2[:, j])
        axis[:, 3 + j] = R2[:, :, j] * np.where(e < 0, -1.0, 1.0)[:, None]
    v[:, :6] = raw[:, :6]
    Qf = Q + FUDGE2
    for i in range(3):
        i1, i2 = (i + 1) % 3, (i + 2) % 3
        for j in range(3):
            j1, j2 = (j + 1) % 3, (j + 2) % 3
            k = 6 + 3 * i + j
            e = pp[:, i2] * R[:, i1, j] - pp[:, i1] * R[:, i2, j]
            ext = h1[:, i1] * Qf[:, i2, j] + h1[:, i2] * Qf[:, i1, j] + h2[:, j1] * Qf[:, i, j2] + h2[:, j2] * Qf[:, i, j1]
            raw[:, k] = np.abs(e) - ext
            c = np.cross(R1[:, :, i], R2[:, :, j])         # a_i x b_j in the world
            l = np.linalg.norm(c, axis=1)
            ok = l > EPSILON
            ls = np.where(ok, l, 1.0)
            v[:, k] = np.where(ok, raw[:, k] / ls, np.nan)
            sign = np.where(np.einsum("ni,ni->n", c, p) < 0, -1.0, 1.0)
            axis[:, k] = c / ls[:, None] * sign[:, None]
    return v, raw, axis


def _winner(v, bump=None):
    """Bullet's sequential rule on the separations v (n, 15); bump (n, 15) is added first.  Returns the winning column."""
    if bump is not None:
        v = v + bump
    best = np.full(len(v), -np.inf)
    win = np.full(len(v), -1, np.int64)
    for k in range(15):
        x = v[:, k]
        with np.errstate(invalid="ignore"):
            better = (x > best) if k < 6 else (x * FUDGE_FACTOR > best)
        better &= ~np.isnan(x)
        best = np.where(better, x, best)
        win = np.where(better, k, win)
    return win


def twins_of(v, axis, win):
    """(n, 15) bool: the axes that are the winner's own direction with the winner's own separation (itself included)."""
    rows = np.arange(len(v))
    along = np.abs(np.einsum("nki,ni->nk", axis, axis[rows, win]))
    with np.errstate(invalid="ignore"):
        return (along > 1.0 - 1e-9) & (np.abs(v - v[rows, win][:, None]) <= 1e-9 * np.abs(v[rows, win])[:, None] + 1e-300) & ~np.isnan(v)


def edge_fudge(code, R1, h1, R2, h2):
    """By how much fudge2 on the four |R_ij| of an edge axis' extents deepens that axis' reported depth (0 for a face code)."""
    rows = np.arange(len(code))
    e = np.clip(code - 7, 0, 8)
    ia, jb = e // 3, e % 3
    i1, i2, j1, j2 = (ia + 1) % 3, (ia + 2) % 3, (jb + 1) % 3, (jb + 2) % 3
    l = np.linalg.norm(np.cross(R1[rows, :, ia], R2[rows, :, jb]), axis=1)
    return np.where(code > 6, FUDGE2 * (h1[rows, i1] + h1[rows, i2] + h2[rows, j1] + h2[rows, j2]) / np.maximum(l, 1e-300), 0.0)


def solve(p1, R1, h1, p2, R2, h2):
    """The model's answer: dict of
      separated (n,)  some axis separates the boxes (the detector reports nothing)
      code (n,)       1 .. 15 of the winner (0 where separated)
      twin (n, 15)    the axes that are the same answer as the winner (twins_of)
      runner (n,)     the code that wins when the winner is taken out
      margin (n,)     the largest d such that the winner still wins with its own separation lowered by d and every other raised by d,
                      and no axis comes within d of separating; absolute (same unit as the boxes); hold it against scale_local
      depth (n,)      the winner's separation (negative)
      normal_on_b (n, 3)  unit, from box 2 to box 1
      v, raw, axis    of separations()
      edge: ua, ub (n, 3) the two edge directions, pa, pb (n, 3) the closest points of the two edge LINES, d (n,) = 1 - (ua . ub)^2
            (valid where code > 6)."""
    p1, R1, h1, p2, R2, h2 = _f64(p1, R1, h1, p2, R2, h2)
    v, raw, axis = separations(p1, R1, h1, p2, R2, h2)
    n = len(v)
    sep_test = raw.copy()                                   # (an edge axis runs its separation test before it may be skipped)
    sep_test[:, 6:] -= EPSILON
    separated = (sep_test > 0).any(1)
    win = _winner(v)
    rows = np.arange(n)
    without = v.copy()
    without[rows, win] = np.nan
    runner = _winner(without)
    # the margin, by bisection on d (40 halvings of the boxes' scale)
    lo, hi = np.zeros(n), np.abs(v[rows, win]) + scale_of(p1, h1, p2, h2)
    # (an axis PARALLEL to the winner's — the facing faces of two boxes laid flat on each other, codes k and 3 + k' — with the same
    #  separation is the same answer under another code: such twins move with the winner and either may win)
    twin = twins_of(v, axis, win)
    up = np.where(twin, -1.0, 1.0)
    for _ in range(48):
        mid = 0.5 * (lo + hi)
        same = twin[rows, _winner(v, up * mid[:, None])]
        lo, hi = np.where(same, mid, lo), np.where(same, hi, mid)
    margin = np.minimum(lo, -sep_test.max(1))
    normal = axis[rows, win]
    # the edge winner's lines: the supporting edge of box 1 towards box 2 and of box 2 towards box 1
    e = np.clip(win - 6, 0, 8)
    ia, jb = e // 3, e % 3
    ua, ub = R1[rows, :, ia], R2[rows, :, jb]
    ca, cb = p1.copy(), p2.copy()
    for k in range(3):
        sa = np.where(np.einsum("ni,ni->n", normal, R1[:, :, k]) > 0, 1.0, -1.0)
        sb = np.where(np.einsum("ni,ni->n", normal, R2[:, :, k]) > 0, -1.0, 1.0)
        ca += (sa * h1[:, k] * (ia != k))[:, None] * R1[:, :, k]          # (the edge's own axis left out: any point of the line will do)
        cb += (sb * h2[:, k] * (jb != k))[:, None] * R2[:, :, k]
    uaub = np.einsum("ni,ni->n", ua, ub)
    d = 1.0 - uaub * uaub
    fudge_depth = edge_fudge(win + 1, R1, h1, R2, h2)
    w = cb - ca
    q1, q2 = np.einsum("ni,ni->n", ua, w), -np.einsum("ni,ni->n", ub, w)
    ds = np.where(d > 0, d, 1.0)
    alpha, beta = (q1 + uaub * q2) / ds, (uaub * q1 + q2) / ds
    return dict(separated=separated, code=np.where(separated, 0, win + 1), runner=runner + 1, margin=margin, depth=v[rows, win], normal_on_b=-normal,
                v=v, raw=raw, axis=axis, twin=twin, ua=ua, ub=ub, pa=ca + ua * alpha[:, None], pb=cb + ub * beta[:, None], d=d, fudge_depth=fudge_depth,
                edge_ends=np.stack([cb - ub * h2[rows, jb][:, None], cb + ub * h2[rows, jb][:, None]], 1),
                scale=scale_of(p1, h1, p2, h2), scale_local=scale_local_of(p1, h1, p2, h2))


def _outside(x, p, R, h, free=None):
    """How far the points x (n, 3) lie outside the box (p, R, h): the largest excess over a face, 0 inside.  free (n,): a box axis
    along which the point may lie anywhere (-1: none)."""
    loc = np.einsum("nki,nk->ni", R, x - p)
    out = np.maximum(np.abs(loc) - h, 0.0)
    if free is not None:
        out = np.where(np.arange(3)[None, :] == free[:, None], 0.0, out)
    return out.max(1)


def deviations(boxes, answer, model=None, refreshed=False):
    """How far an answer is from the model, per pair, every figure divided by the pair's scale (depth: by scale_local) except `normal`
    and `unit` (already relative).
    boxes: (p1, R1, h1, p2, R2, h2); answer: dict code (n,), n_out (n,), normal_on_b (n, 3), point (n, 4, 3) = pointInWorld,
    depth (n, 4).  Returns dict of (n,) arrays — NaN where a figure does not apply:
      normal      |normalOnB - model's| (inf norm) where the codes agree
      unit        | |normalOnB| - 1 |
      depth       edge answers: |depth - model depth|; face answers: how far the deepest point goes BEYOND the model depth, or any
                  point above zero
      on_b, on_a  how far pointInWorld lies outside box 2 / pointInWorld + normalOnB * depth outside box 1 (worst point); an edge
                  answer's points are free along their own edge, its on_a allows for fudge2 and is not held at d <= 0.0001
      plane       face answers: how far the point on the reference box lies off the reference face's plane (worst point)
      rect        face answers: how far it lies outside the reference face's rectangle (worst point)
      edge        edge answers: |pointInWorld - model's closest point on box 2's edge line| * d  (d = 1 - (ua . ub)^2); where
                  d <= 0.0001: the distance to the nearer END of that edge (within 1e-6 of the threshold: not held)
    and code_ok (n,) bool: the answer's code is the model's.  refreshed: the depths are a manifold's distances after
    refreshContactPoints — (worldA - worldB) . normal recomputed from the two local points through the two poses, which rounds at the
    size of the world coordinates: the depth is then taken relative to `scale` like the points, not to scale_local."""
    p1, R1, h1, p2, R2, h2 = _f64(*boxes)
    m = solve(p1, R1, h1, p2, R2, h2) if model is None else model
    n = len(p1)
    sc = m["scale"]
    code = np.asarray(answer["code"], np.int64)
    nout = np.asarray(answer["n_out"], np.int64)
    nb, pt, dep = _f64(answer["normal_on_b"], answer["point"], answer["depth"])
    out = {k: np.full(n, np.nan) for k in ("normal", "unit", "depth", "on_b", "on_a", "plane", "rect", "edge")}
    has = nout > 0
    code_ok = (code == m["code"]) | (m["twin"][np.arange(n), np.clip(code - 1, 0, 14)] & (code > 0))   # (a twin of the winner: the same answer)
    out["unit"] = np.where(has, np.abs(np.linalg.norm(nb, axis=1) - 1.0), np.nan)
    out["normal"] = np.where(has & code_ok, np.abs(nb - m["normal_on_b"]).max(1), np.nan)
    face, edge = has & (code <= 6), has & (code > 6)
    k4 = np.arange(4)[None, :] < nout[:, None]
    worst = lambda a: np.where(k4, a, 0.0).max(1)            # noqa: E731
    on_a_pt = pt + nb[:, None, :] * dep[:, :, None]
    # Two documented deviations of an EDGE answer from "a point of each box" (Bullet's published dBoxBox2, which the oracle restates):
    # dLineClosestApproach works on the infinite edge LINES, so the point may lie beyond the ends of its edge — it is held to the box
    # in the two directions across the edge only; and the edge axes' extents carry fudge2 = 1e-5 on every |R_ij|, so the reported
    # depth exceeds the geometric one by m["fudge_depth"] — the point on box 1 may lie that far outside it.
    e = np.clip(code - 7, 0, 8)
    free_a, free_b = np.where(edge_code := code > 6, e // 3, -1), np.where(edge_code, e % 3, -1)
    out["on_b"] = np.where(has, worst(np.stack([_outside(pt[:, k], p2, R2, h2, free_b) for k in range(4)], 1)) / sc, np.nan)
    on_a = worst(np.stack([_outside(on_a_pt[:, k], p1, R1, h1, free_a) for k in range(4)], 1))
    # A third: at d <= 0.0001 the point is an END of box 2's edge, up to the edge's whole length from where the lines pass each other, and
    # "that end moved by the depth along the normal" is no point of box 1 (the lines have parted by the crossing angle x that length):
    # there the point on box 1 is not held at all.
    rows = np.arange(n)
    uaub = np.einsum("ni,ni->n", R1[rows, :, e // 3], R2[rows, :, e % 3])
    parallel = edge_code & (1.0 - uaub * uaub <= PARALLEL_D + 1e-6)
    out["on_a"] = np.where(has & ~parallel, np.maximum(on_a - edge_fudge(code, R1, h1, R2, h2), 0.0) / sc, np.nan)
    deepest = np.where(k4, dep, np.inf).min(1)
    highest = np.where(k4, dep, -np.inf).max(1)
    out["depth"] = np.where(edge, np.abs(dep[:, 0] - m["depth"]), np.where(face, np.maximum(np.maximum(m["depth"] - deepest, highest), 0.0), np.nan)) / (sc if refreshed else m["scale_local"])
    # the reference face of a face answer: of box 1 for codes 1 .. 3 (the point on it is pointInWorld + normalOnB * depth), of box 2
    # for 4 .. 6 (pointInWorld itself); its axis is code - 1 or code - 4, its side the one that faces the other box
    c0 = np.clip(code - 1, 0, 5)
    ref1 = c0 < 3
    ax = np.where(ref1, c0, c0 - 3)
    rp, rR, rh = np.where(ref1[:, None], p1, p2), np.where(ref1[:, None, None], R1, R2), np.where(ref1[:, None], h1, h2)
    ref_pt = np.where(ref1[:, None, None], on_a_pt, pt)
    loc = np.einsum("nki,njk->nji", rR, ref_pt - rp[:, None, :])                      # (n, 4, 3) in the reference box's frame
    rows = np.arange(n)
    side = np.sign(np.einsum("nk,nk->n", rR[rows, :, ax], np.where(ref1[:, None], p2 - p1, p1 - p2)))
    off_plane = np.abs(loc[rows, :, ax] - (side * rh[rows, ax])[:, None])
    others = np.stack([(ax + 1) % 3, (ax + 2) % 3], 1)
    off_rect = np.maximum(np.abs(loc[rows[:, None], :, others]) - rh[rows[:, None], others][:, :, None], 0.0).max(1)   # (n, 4)
    out["plane"] = np.where(face, worst(off_plane) / sc, np.nan)
    out["rect"] = np.where(face, worst(off_rect) / sc, np.nan)
    general = np.abs(pt[:, 0] - m["pb"]).max(1) * m["d"]
    at_end = np.abs(pt[:, 0, None, :] - m["edge_ends"]).max(2).min(1)
    held = edge & code_ok & (np.abs(m["d"] - PARALLEL_D) > 1e-6)
    out["edge"] = np.where(held, np.where(m["d"] <= PARALLEL_D, at_end, general) / sc, np.nan)
    out["code_ok"] = code_ok
    return out


FIGURES = ("normal", "unit", "depth", "on_b", "on_a", "plane", "rect", "edge")


def check(boxes, answer, rel, model=None, refreshed=False):
    """The sandwich.  rel: the tolerance as a fraction of a pair's scale (tolerances.BOXBOX_REL).  Returns (failures, undecided):
    failures is a list of (pair, what, figure); undecided (n,) marks the pairs whose winner's margin does not exceed the tolerance —
    there the code and the normal are not held against the model (every other check still is).  A pair the model calls separated
    must have no points; a pair with points must not be separated by more than the tolerance."""
    p1, R1, h1, p2, R2, h2 = _f64(*boxes)
    m = solve(p1, R1, h1, p2, R2, h2) if model is None else model
    dev = deviations(boxes, answer, m, refreshed)
    undecided = ~(m["margin"] > rel * m["scale_local"])
    nout = np.asarray(answer["n_out"], np.int64)
    fails = []
    for i in np.flatnonzero(~undecided & (nout > 0) & ~dev["code_ok"]):
        fails.append((int(i), "code", (int(answer["code"][i]), int(m["code"][i]))))
    for i in np.flatnonzero(~undecided & (nout == 0) & ~m["separated"]):
        fails.append((int(i), "no points", float(m["depth"][i])))
    for k in FIGURES:
        x = dev[k]
        bad = (x > rel) & (~undecided if k in ("normal", "edge") else True)   # (every figure is already divided by its scale)
        for i in np.flatnonzero(bad & ~np.isnan(x)):
            fails.append((int(i), k, float(x[i])))
    return fails, undecided


def infer_code(boxes, normal_on_b, model=None):
    """The code of an answer that reports only its normal (the device's manifolds): the axis of the model that the normal lies along;
    the model's own winner where several axes coincide with it (aligned boxes)."""
    p1, R1, h1, p2, R2, h2 = _f64(*boxes)
    m = solve(p1, R1, h1, p2, R2, h2) if model is None else model
    nb = np.asarray(normal_on_b, np.float64)
    dist = np.abs(nb[:, None, :] + m["axis"]).max(2)                  # axis points from box 1 to box 2, normalOnB the other way
    dist = np.where(np.isnan(m["v"]), np.inf, dist)
    best = dist.argmin(1)
    rows = np.arange(len(nb))
    win = m["code"] - 1
    same = np.where(win >= 0, dist[rows, np.maximum(win, 0)] <= dist[rows, best] + 1e-6, False)
    return np.where(same, win, best) + 1
