"""The references of frustum culling (include/bge_world.h bge_world_visible*): the rule restated in numpy binary32 operation for
operation, a float64 geometric reference (box corners through the matrix against normalised planes) and bge_frustum_planes."""
from __future__ import annotations

import numpy as np

F = np.float32
AMBIGUOUS_REL = 1e-4  # within this x (1 + |cw|_inf + |h * scale|_inf) of a plane the float64 reference does not decide
IDENTITY = np.eye(4, dtype=F).reshape(1, 16)


def renderable(center, half):
    center, half = np.asarray(center, F).reshape(-1, 3), np.asarray(half, F).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        return np.all(np.isfinite(half) & (half >= 0), axis=1) & np.all(np.isfinite(center), axis=1)


def visible_ref32(world, center, half, planes, eligible=None):
    """The header's rule in binary32, one numpy operation per rounding, left to right.  world (n, 16), center / half (n, 3),
    planes (k, 4); eligible: owns a Transform and is not dirty (default: all).  Returns the visible mask."""
    m = np.asarray(world, F).reshape(-1, 16)
    c, h = np.asarray(center, F).reshape(-1, 3), np.asarray(half, F).reshape(-1, 3)
    planes = np.zeros((0, 4), F) if planes is None else np.asarray(planes, F).reshape(-1, 4)
    vis = renderable(c, h)
    if eligible is not None:
        vis &= np.asarray(eligible, bool)
    with np.errstate(invalid="ignore", over="ignore"):
        cw = [((c[:, 0] * m[:, j] + c[:, 1] * m[:, 4 + j]) + c[:, 2] * m[:, 8 + j]) + m[:, 12 + j] for j in range(3)]
        for a, b, c4, d in planes:
            e = [(a * m[:, 4 * i] + b * m[:, 4 * i + 1]) + c4 * m[:, 4 * i + 2] for i in range(3)]
            r = (np.abs(e[0]) * h[:, 0] + np.abs(e[1]) * h[:, 1]) + np.abs(e[2]) * h[:, 2]
            sd = ((a * cw[0] + b * cw[1]) + c4 * cw[2]) + d
            assert r.dtype == F and sd.dtype == F
            vis &= sd >= -r  # False for a NaN on either side
    return vis


CORNERS = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64)


def visible_ref64(world, center, half, planes):
    """Geometry in float64: the 8 corners of the box through the matrix; inside a plane iff some corner is on its inner side.
    Returns (visible, ambiguous): ambiguous where the deciding corner lies within AMBIGUOUS_REL x (1 + |cw|_inf + |h * scale|_inf)
    of some plane (in units of the normalised plane)."""
    m = np.asarray(world, np.float64).reshape(-1, 4, 4)
    c, h = np.asarray(center, np.float64).reshape(-1, 3), np.asarray(half, np.float64).reshape(-1, 3)
    planes = np.asarray(planes, np.float64).reshape(-1, 4)
    local = c[:, None, :] + CORNERS[None] * h[:, None, :]                       # (n, 8, 3)
    pts = np.einsum("nki,nij->nkj", local, m[:, :3, :3]) + m[:, None, 3, :3]    # row vectors: p * M
    cw = np.einsum("ni,nij->nj", c, m[:, :3, :3]) + m[:, 3, :3]
    extent = np.abs(h[:, :, None] * m[:, :3, :3]).sum(axis=1)                   # half extents scaled by the matrix rows
    scale = 1.0 + np.abs(cw).max(axis=1) + extent.max(axis=1)
    vis = np.ones(len(m), bool)
    amb = np.zeros(len(m), bool)
    for p in planes:
        nrm = np.linalg.norm(p[:3])
        dist = ((pts @ p[:3]) + p[3]).max(axis=1) / nrm                         # the innermost corner
        vis &= dist >= 0
        amb |= np.abs(dist) <= AMBIGUOUS_REL * scale
    return vis, amb


def frustum_planes_ref(vp, homogeneous_depth):
    m = np.asarray(vp, F).reshape(4, 4)
    x, y, z, w = m[:, 0], m[:, 1], m[:, 2], m[:, 3]
    return np.stack([w + x, w - x, w + y, w - y, (w + z) if homogeneous_depth else z, w - z]).astype(F)
