"""The reference of crowd separation (include/bge_world.h "Crowd separation"): crowd_ref, the rule in numpy float32 scalars over
all pairs (written from the header, not from the kernels), and separate_ref, the stage Separate of a character step over a
STATE_DTYPE array.  The character reference of a step with the crowd on is char_ref(..., separate_ref(state)[0] ...)."""
from __future__ import annotations

import numpy as np

from .characters import STATE_DTYPE  # noqa: F401  (what separate_ref takes and returns)
from .moves import F
from .rays import NO_ENTITY

INVALID, PUSHED, CLAMPED = 1, 2, 4
SPHERE_DTYPE = np.dtype([("center", "<f4", (3,)), ("radius", "<f4"), ("group", "<u4"), ("mask", "<u4")])
HIT_DTYPE = np.dtype([("flags", "<u4"), ("other", "<u4"), ("n_overlaps", "<u4"), ("depth", "<f4"), ("push", "<f4", (3,)), ("reserved", "<u4")])
assert SPHERE_DTYPE.itemsize == 24 and HIT_DTYPE.itemsize == 32


def make_spheres(centers, radius=0.5, group=1, mask=0xFFFFFFFF):
    c = np.asarray(centers, np.float32).reshape(-1, 3)
    s = np.zeros(len(c), SPHERE_DTYPE)
    s["center"] = c
    s["radius"] = np.broadcast_to(np.asarray(radius, np.float32), (len(c),))
    s["group"] = np.broadcast_to(np.asarray(group, np.uint64).astype(np.uint32), (len(c),))
    s["mask"] = np.broadcast_to(np.asarray(mask, np.uint64).astype(np.uint32), (len(c),))
    return s


def valid_of(spheres):
    with np.errstate(all="ignore"):
        return np.isfinite(spheres["center"]).all(axis=1) & np.isfinite(spheres["radius"]) & (spheres["radius"] >= 0)


def pair_depths(spheres, i, cand):
    """depth of the rule for sphere i against the spheres cand (an index array): float32 array, one rounding per operation."""
    c, r = spheres["center"], spheres["radius"]
    with np.errstate(all="ignore"):
        d = (c[i][None, :] - c[cand]).astype(np.float32)
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        return (r[i] + r[cand]) - np.sqrt(d2)


def crowd_ref(spheres, max_push=0.0):
    """HIT_DTYPE[n]: the rule for every sphere, all pairs.  (The per-pair arithmetic runs on float32 arrays: elementwise numpy
    float32 operations round once each, like the scalars.)"""
    n = len(spheres)
    hits = np.zeros(n, HIT_DTYPE)
    hits["other"] = NO_ENTITY
    max_push = F(max_push)
    valid = valid_of(spheres)
    index = np.arange(n)
    group, mask = spheres["group"], spheres["mask"]
    for i in range(n):
        if not valid[i]:
            hits["flags"][i] = INVALID
            continue
        cand = index[valid & (index != i) & ((group[i] & mask) != 0) & ((group & mask[i]) != 0)]
        if len(cand) == 0:
            continue
        depth = pair_depths(spheres, i, cand)
        with np.errstate(all="ignore"):
            over = depth > 0
        if not over.any():
            continue
        cand, depth = cand[over], depth[over]
        k = int(np.flatnonzero(depth == depth.max())[0])  # cand ascends: the lowest j of the largest depth
        other = int(cand[k])
        h = hits[i]
        h["n_overlaps"], h["other"], h["depth"] = len(cand), other, depth[k]
        # Push
        with np.errstate(all="ignore"):
            dx = F(spheres["center"][i][0]) - F(spheres["center"][other][0])
            dz = F(spheres["center"][i][2]) - F(spheres["center"][other][2])
            hl2 = dx * dx + dz * dz
            if hl2 > F(1e-12):
                hl = np.sqrt(hl2)
                mx, mz = dx / hl, dz / hl
            else:
                mx, mz = F(1 if i < other else -1), F(0)
            t = F(depth[k]) * F(0.5)
            flags = PUSHED
            if max_push > 0 and t > max_push:
                t = max_push
                flags |= CLAMPED
            h["push"] = (mx * t, F(0), mz * t)
        h["flags"] = flags
    return hits


def separate_ref(descs, state, group=None, mask=None, max_push=0.0):
    """The stage Separate: (the new STATE_DTYPE array, the HIT_DTYPE records).  Only x and z of a PUSHED character change."""
    n = len(descs)
    spheres = make_spheres(state["position"], descs["radius"], 1 if group is None else group, 0xFFFFFFFF if mask is None else mask)
    hits = crowd_ref(spheres, max_push)
    out = state.copy()
    with np.errstate(all="ignore"):
        for i in range(n):
            if hits["flags"][i] & PUSHED:
                out["position"][i][0] = F(state["position"][i][0]) + F(hits["push"][i][0])
                out["position"][i][2] = F(state["position"][i][2]) + F(hits["push"][i][2])
    return out, hits
