"""Sphere casts and sphere overlaps (include/bge_world.h bge_world_sphere_cast*, bge_world_overlap_sphere) without a GPU: the float64
reference the GPU tests compare against, checked on hand-worked cases; the exported symbols; the C99 view of the records; the
adapter's SphereCast / SphereCastAll / OverlapSphere on the reference's types (C++20, -Werror).

The reference does not follow the kernel's method (entry region of the grown box, then at most three edge capsules): it takes the
rounded box as the UNION of three boxes (the sharp box grown by r along one axis each) and the twelve edge capsules of radius r,
and the first touch as the minimum over those fifteen parts, each part tested by the ray reference of test_raycast_cpu.py."""
from __future__ import annotations

import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from test_raycast_cpu import (CODE_GHOST, CODE_PLANE, NO_ENTITY, RAY_BODY, RAY_GROUND, RAY_TRIGGER, Obj, World64, box_half_extents,
                              capsule_dims, cast_all, clear_decision, quat_from_euler, quat_to_mat, random_objects, ray_box, ray_capsule,
                              ray_valid)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
LIBDIR = os.path.join(ROOT, "banggameengine_amd")
EPS_CLEAR = 1e-4

# ------------------------------------------------------------------------------------------------ float64 reference, one object


def box_closest(p, h):
    return np.clip(p, -h, h)


def box_dist(p, h):
    return float(np.linalg.norm(p - box_closest(p, h)))


def capsule_axis_point(p, hh):
    return np.array([0.0, min(max(p[1], -hh), hh), 0.0])


def capsule_dist(p, r, hh):
    return max(0.0, float(np.linalg.norm(p - capsule_axis_point(p, hh))) - r)


def sweep_box(o, d, h, r):
    """Sphere of radius r, centre o + d f, against the sharp box h: (f, local normal, local contact point) or None."""
    if box_dist(o, h) <= r:
        return None
    best, face_n = math.inf, None
    for a in range(3):  # the box grown along one axis: the face slabs
        g = h.copy()
        g[a] += r
        hit = ray_box(o, d, g)
        if hit is not None and hit[0] < best:
            best, face_n = hit[0], hit[1]
    for a in range(3):  # the twelve edges: capsules of radius r along axis a, taken to ray_capsule's Y axis
        b, c = (a + 1) % 3, (a + 2) % 3
        for sb in (-1.0, 1.0):
            for sc in (-1.0, 1.0):
                oo = np.array([o[b] - sb * h[b], o[a], o[c] - sc * h[c]])
                hit = ray_capsule(oo, np.array([d[b], d[a], d[c]]), r, h[a]) if r > 0 else None
                if hit is not None and hit[0] < best:
                    best, face_n = hit[0], None
    if not best <= 1.0:
        return None
    cc = o + d * best
    q = box_closest(cc, h)
    n = face_n if face_n is not None else (cc - q) / np.linalg.norm(cc - q)
    return best, n, q


def sweep_capsule(o, d, R, hh, r):
    hit = ray_capsule(o, d, R + r, hh)
    if hit is None:
        return None
    cc = o + d * hit[0]
    return hit[0], hit[1], cc - r * hit[1]


def sweep_plane(from_y, to_y, r):
    if from_y > r and to_y < r:
        return (from_y - r) / (from_y - to_y), np.array([0.0, 1.0, 0.0])
    if from_y < -r and to_y > -r:
        return (from_y + r) / (from_y - to_y), np.array([0.0, -1.0, 0.0])
    return None


def obj_sweep(ob, frm, delta, r, grow=0.0):
    """(f, world normal, world contact point) of the sphere cast against Obj ob, or None."""
    o, d = ob.basis.T @ (frm - ob.origin), ob.basis.T @ delta
    hit = sweep_capsule(o, d, ob.dims[0] + grow, ob.dims[1], r) if ob.capsule else sweep_box(o, d, ob.dims + grow, r)
    return None if hit is None else (hit[0], ob.basis @ hit[1], ob.origin + ob.basis @ hit[2])


def obj_dist(ob, c):
    p = ob.basis.T @ (c - ob.origin)
    return capsule_dist(p, ob.dims[0], ob.dims[1]) if ob.capsule else box_dist(p, ob.dims)


def cast_valid(origin, direction, max_distance, radius, mask):
    r = np.float32(radius)
    return ray_valid(origin, direction, max_distance, mask) and bool(np.isfinite(r) and r >= 0)


def sweep_all(objs, origin, direction, max_distance, radius, mask, plane, grow=0.0):
    """Every touch of one cast: sorted list of (f, code, kind, entity, normal, point)."""
    if not cast_valid(origin, direction, max_distance, radius, mask):
        return []
    frm = np.asarray(origin, np.float32).astype(np.float64)
    delta = (np.asarray(direction, np.float32) * np.float32(max_distance)).astype(np.float64)
    r = float(np.float32(radius))
    out = []
    for ob in objs:
        if (ob.group & int(mask)) == 0 or ob.mask == 0:
            continue
        hit = obj_sweep(ob, frm, delta, r, grow)
        if hit is not None:
            out.append((hit[0], ob.code, ob.kind, ob.entity, hit[1], hit[2]))
    if plane and (int(mask) & 2):
        hit = sweep_plane(frm[1], frm[1] + delta[1], r)
        if hit is not None:
            cc = frm + delta * hit[0]
            out.append((hit[0], CODE_PLANE, RAY_GROUND, NO_ENTITY, hit[1], np.array([cc[0], 0.0, cc[2]])))
    out.sort(key=lambda h: (h[0], h[1]))
    return out


def sphere_valid(center, radius, mask):
    c, r = np.asarray(center, np.float32), np.float32(radius)
    return bool(np.isfinite(c).all() and np.isfinite(r) and r >= 0 and int(mask) != 0)


def overlap_all(objs, center, radius, mask, plane):
    """Brute force: (list of (code, kind, entity, distance) in ascending code, clear) — clear is False when some candidate's
    distance lies within 1e-4 * (1 + |center|_inf) of the radius."""
    if not sphere_valid(center, radius, mask):
        return [], True
    c, r = np.asarray(center, np.float32).astype(np.float64), float(np.float32(radius))
    tol = EPS_CLEAR * (1.0 + float(np.abs(c).max()))
    out, clear = [], True
    for ob in objs:
        if (ob.group & int(mask)) == 0 or ob.mask == 0:
            continue
        dist = obj_dist(ob, c)
        clear &= abs(dist - r) > tol
        if dist <= r:
            out.append((ob.code, ob.kind, ob.entity, dist))
    if plane and (int(mask) & 2):
        clear &= abs(abs(c[1]) - r) > tol
        if abs(c[1]) <= r:
            out.append((CODE_PLANE, RAY_GROUND, NO_ENTITY, abs(c[1])))
    out.sort(key=lambda h: h[0])
    return out, clear


# ------------------------------------------------------------------------------------------------ the same, vectorised over objects


def _ray_box_v(o, d, h):
    """ray_box over rows: (f or inf, entry axis, sign of the face normal)."""
    rows = np.arange(len(o))
    with np.errstate(all="ignore"):
        inside = (np.abs(o) <= h).all(axis=1)
        par = d == 0
        bad = (par & (np.abs(o) > h)).any(axis=1)
        t1, t2 = (-h - o) / d, (h - o) / d
        near = np.where(par, -np.inf, np.minimum(t1, t2))
        far = np.where(par, np.inf, np.maximum(t1, t2))
        ax = np.argmax(near, axis=1)
        tn, tf = near[rows, ax], far.min(axis=1)
        hit = ~inside & ~bad & (tn > -np.inf) & (tn <= tf) & (tn >= 0) & (tn <= 1)
    return np.where(hit, tn, np.inf), ax, np.where(d[rows, ax] > 0, -1.0, 1.0)


def _ray_capsule_v(o, d, r, hh):
    """ray_capsule over rows (Y-axis capsules): f or inf."""
    with np.errstate(all="ignore"):
        cy = np.clip(o[:, 1], -hh, hh)
        cin = o[:, 0] ** 2 + (o[:, 1] - cy) ** 2 + o[:, 2] ** 2 <= r * r
        a = d[:, 0] ** 2 + d[:, 2] ** 2
        b = o[:, 0] * d[:, 0] + o[:, 2] * d[:, 2]
        disc = b * b - a * (o[:, 0] ** 2 + o[:, 2] ** 2 - r * r)
        t = (-b - np.sqrt(disc)) / a
        side = (a > 0) & (disc >= 0) & (t >= 0) & (t <= 1) & (np.abs(o[:, 1] + d[:, 1] * t) <= hh)
        best = np.where(side, t, np.inf)
        aa = (d * d).sum(axis=1)
        for c0 in (-1.0, 1.0):
            m = o.copy()
            m[:, 1] -= c0 * hh
            bb = (m * d).sum(axis=1)
            ds = bb * bb - aa * ((m * m).sum(axis=1) - r * r)
            ts = (-bb - np.sqrt(ds)) / aa
            ok = (ds >= 0) & (ts >= 0) & (ts <= 1) & (ts < best)
            best = np.where(ok, ts, best)
    return np.where(cin, np.inf, best)


class SphereRef:
    """sweep_all / overlap_all on a World64 (test_raycast_cpu.py), vectorised over the objects a bounding-sphere cull leaves."""

    def __init__(self, w64):
        self.w = w64

    def _sweep_sel(self, sel, frm, delta, r, grow):
        w = self.w
        B = w.basis[sel]
        o = np.einsum("nji,nj->ni", B, frm - w.origin[sel])
        d = np.einsum("nji,j->ni", B, delta)
        cap = w.capsule[sel]
        h = w.dims[sel] + grow
        rr = np.full(len(sel), r)
        # capsules: the ray against radius R + r
        f = np.where(cap, _ray_capsule_v(o, d, h[:, 0] + r, w.dims[sel][:, 1]), np.inf)
        # boxes: three grown boxes and twelve edge capsules
        q0 = np.clip(o, -h, h)
        start = ((o - q0) ** 2).sum(axis=1) <= r * r
        fb = np.full(len(sel), np.inf)
        face = np.zeros(len(sel), bool)
        fn = np.zeros((len(sel), 3))
        rows = np.arange(len(sel))
        for a in range(3):
            g = h.copy()
            g[:, a] += r
            t, ax, sg = _ray_box_v(o, d, g)
            better = t < fb
            fb = np.where(better, t, fb)
            face |= better
            nb = np.zeros((len(sel), 3))
            nb[rows, ax] = sg
            fn = np.where(better[:, None], nb, fn)
        if r > 0:
            for a in range(3):
                b, c = (a + 1) % 3, (a + 2) % 3
                dd = np.stack([d[:, b], d[:, a], d[:, c]], 1)
                for sb in (-1.0, 1.0):
                    for sc in (-1.0, 1.0):
                        oo = np.stack([o[:, b] - sb * h[:, b], o[:, a], o[:, c] - sc * h[:, c]], 1)
                        t = _ray_capsule_v(oo, dd, rr, h[:, a])
                        better = t < fb
                        fb = np.where(better, t, fb)
                        face &= ~better
        fb = np.where(start, np.inf, fb)
        f = np.where(cap, f, fb)
        hit = np.nonzero(np.isfinite(f))[0]
        out = []
        for k in hit:
            cc = o[k] + d[k] * f[k]
            if cap[k]:
                s = capsule_axis_point(cc, w.dims[sel[k]][1])
                n = (cc - s) / np.linalg.norm(cc - s)
                q = cc - r * n
            else:
                q = np.clip(cc, -h[k], h[k])
                n = fn[k] if face[k] else (cc - q) / np.linalg.norm(cc - q)
            i = sel[k]
            out.append((float(f[k]), int(w.code[i]), int(w.kind[i]), int(w.entity[i]), B[k] @ n, w.origin[i] + B[k] @ q))
        return out

    def _prep(self, origin, direction, max_distance, radius, mask):
        frm = np.asarray(origin, np.float32).astype(np.float64)
        delta = (np.asarray(direction, np.float32) * np.float32(max_distance)).astype(np.float64)
        r = float(np.float32(radius))
        w = self.w
        wv = w.origin - frm
        t = np.clip((wv @ delta) / float(delta @ delta), 0.0, 1.0)
        e = wv - t[:, None] * delta
        near = (e * e).sum(axis=1) <= (w.radius + r) ** 2
        return frm, delta, r, np.nonzero(near & ((w.group & int(mask)) != 0) & (w.omask != 0))[0]

    def sweep_all(self, origin, direction, max_distance, radius, mask, grow=0.0, _prep=None):
        if not cast_valid(origin, direction, max_distance, radius, mask):
            return []
        frm, delta, r, sel = _prep or self._prep(origin, direction, max_distance, radius, mask)
        out = self._sweep_sel(sel, frm, delta, r, grow) if len(sel) else []
        if self.w.plane and (int(mask) & 2):
            hit = sweep_plane(frm[1], frm[1] + delta[1], r)
            if hit is not None:
                cc = frm + delta * hit[0]
                out.append((hit[0], CODE_PLANE, RAY_GROUND, NO_ENTITY, hit[1], np.array([cc[0], 0.0, cc[2]])))
        out.sort(key=lambda h: (h[0], h[1]))
        return out

    def sweep_clear(self, origin, direction, max_distance, radius, mask, eps=EPS_CLEAR):
        """(all touches, clear): clear = the ray tests' rule on the swept sphere — the runner-up more than eps behind in f, and
        growing or shrinking every shape by eps changes no hit set."""
        if not cast_valid(origin, direction, max_distance, radius, mask):
            return [], True
        prep = self._prep(origin, direction, max_distance, radius, mask)
        base = self.sweep_all(origin, direction, max_distance, radius, mask, _prep=prep)
        if len(base) > 1 and base[1][0] - base[0][0] <= eps:
            return base, False
        codes = [h[1] for h in base]
        ok = all([h[1] for h in self.sweep_all(origin, direction, max_distance, radius, mask, grow=g, _prep=prep)] == codes for g in (eps, -eps))
        return base, ok

    def overlap(self, center, radius, mask):
        """overlap_all on this world."""
        if not sphere_valid(center, radius, mask):
            return [], True
        w = self.w
        c, r = np.asarray(center, np.float32).astype(np.float64), float(np.float32(radius))
        tol = EPS_CLEAR * (1.0 + float(np.abs(c).max()))
        near = ((w.origin - c) ** 2).sum(axis=1) <= (w.radius + r + tol) ** 2
        sel = np.nonzero(near & ((w.group & int(mask)) != 0) & (w.omask != 0))[0]
        p = np.einsum("nji,nj->ni", w.basis[sel], c - w.origin[sel])
        h = w.dims[sel]
        db = np.linalg.norm(p - np.clip(p, -h, h), axis=1)
        s = np.zeros_like(p)
        s[:, 1] = np.clip(p[:, 1], -h[:, 1], h[:, 1])
        dc = np.maximum(0.0, np.linalg.norm(p - s, axis=1) - h[:, 0])
        dist = np.where(w.capsule[sel], dc, db)
        clear = bool((np.abs(dist - r) > tol).all())
        out = [(int(w.code[i]), int(w.kind[i]), int(w.entity[i]), float(dd)) for i, dd in zip(sel, dist) if dd <= r]
        if w.plane and (int(mask) & 2):
            clear &= abs(abs(c[1]) - r) > tol
            if abs(c[1]) <= r:
                out.append((CODE_PLANE, RAY_GROUND, NO_ENTITY, abs(c[1])))
        out.sort(key=lambda hh: hh[0])
        return out, clear


# ------------------------------------------------------------------------------------------------ generators shared with the GPU tests


def random_casts(rng, n, scene_pos, spread=30.0):
    """Casts aimed mostly at bodies, radii from [0, 2] with every tenth exactly 0: origin, direction, max distance, radius, mask."""
    o = np.stack([rng.uniform(-spread, spread, n), rng.uniform(-2.0, 12.0, n), rng.uniform(-spread, spread, n)], 1)
    d = rng.normal(size=(n, 3))
    aim = rng.random(n) < 0.6
    tgt = scene_pos[rng.integers(0, len(scene_pos), n)] + rng.normal(scale=0.3, size=(n, 3))
    d[aim] = tgt[aim] - o[aim]
    d *= rng.uniform(0.5, 2.0, (n, 1))
    md = rng.uniform(0.5, 1.5, n) * np.where(aim, 1.0, 20.0)
    rad = rng.uniform(0.0, 2.0, n)
    rad[::10] = 0.0
    mask = rng.choice(np.array([1, 2, 4, 8, 3, 6, 0xFFFFFFFF], np.uint32), n)
    return o.astype(np.float32), d.astype(np.float32), md.astype(np.float32), rad.astype(np.float32), mask


def random_spheres(rng, n, scene_pos, spread=30.0, max_radius=3.0):
    """Overlap spheres, most centred near a body: centre, radius from [0, max_radius], mask."""
    c = np.stack([rng.uniform(-spread, spread, n), rng.uniform(-2.0, 8.0, n), rng.uniform(-spread, spread, n)], 1)
    near = rng.random(n) < 0.6
    tgt = scene_pos[rng.integers(0, len(scene_pos), n)] + rng.normal(scale=1.0, size=(n, 3))
    c[near] = tgt[near]
    rad = rng.uniform(0.0, max_radius, n)
    mask = rng.choice(np.array([1, 2, 4, 8, 3, 6, 0xFFFFFFFF], np.uint32), n)
    return c.astype(np.float32), rad.astype(np.float32), mask


def scene_world64(n, rng, n_triggers=12, spread=30.0):
    """The World64 of test_gpu_raycast.Scene(n, rng, n_triggers) before its first tick: the same draws in the same order."""
    pos = np.stack([rng.uniform(-spread, spread, n), rng.uniform(0.3, 6.0, n), rng.uniform(-spread, spread, n)], 1).astype(np.float32)
    euler = rng.uniform(-math.pi, math.pi, (n, 3)).astype(np.float32)
    btype = rng.choice([1, 2, 3], n, p=[0.3, 0.5, 0.2])
    trig = rng.choice(n, n_triggers, replace=False)
    shape = rng.integers(0, 2, n)
    size = rng.uniform(0.1, 1.5, (n, 3)).astype(np.float32)
    layer = 1 << rng.integers(0, 4, n)
    mask = rng.choice(np.array([0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0x3, 0], np.uint32), n)
    del btype
    kind = np.full(n, RAY_BODY)
    kind[trig] = RAY_TRIGGER
    dims = np.array([capsule_dims(size[i]) if shape[i] else box_half_extents(size[i]) for i in range(n)])
    quat = np.array([quat_from_euler(e.astype(np.float64)) for e in euler])
    return World64.from_arrays(kind, np.arange(n), layer, mask, shape == 1, dims, pos, quat, True), pos


def reference_coverage(ref, casts, spheres):
    """What the caps of the GPU comparison see on the reference alone: (casts compared, of them hits, spheres compared)."""
    o, d, md, rad, mask = casts
    clear = hits = 0
    for i in range(len(o)):
        base, ok = ref.sweep_clear(o[i], d[i], md[i], rad[i], mask[i])
        clear += ok
        hits += bool(ok and base)
    c, srad, smask = spheres
    compared = sum(ref.overlap(c[i], srad[i], smask[i])[1] for i in range(len(c)))
    return clear, hits, compared


# ------------------------------------------------------------------------------------------------ hand-worked cases

IDQ = (0.0, 0.0, 0.0, 1.0)
S2, S3 = math.sqrt(2.0), math.sqrt(3.0)
ALL = 0xFFFFFFFF
# (name, bodies [(capsule, size, position)], plane, (origin, direction, max distance, radius, mask),
#  expected (entity or NO_ENTITY for the plane, f, point, normal) or None).  Sizes of 1 and 0.5 keep the library's half extents
# at the sizes themselves; every body is at rest with the identity rotation.  The GPU tests run the same list on the device.
HAND_CASES = [
    # face: box (1, 2, 3) at x = 10, its face x = 9; the centre stops at 9 - 0.5
    ("box face", [(False, (1, 2, 3), (10, 0, 0))], False, ((0, 0, 0), (1, 0, 0), 20.0, 0.5, 1), (0, 8.5 / 20, (9, 0, 0), (-1, 0, 0))),
    # edge: unit cube, approach along the diagonal of the xy plane onto the edge (1, 1, z): the centre stops 0.5 from the edge
    ("box edge at 45 degrees", [(False, (1, 1, 1), (0, 0, 0))], False, ((5, 5, 0.25), (-1, -1, 0), 10.0, 0.5, 1),
     (0, (4 - 0.5 / S2) / 10, (1, 1, 0.25), (1 / S2, 1 / S2, 0))),
    # corner: along the space diagonal onto (1, 1, 1)
    ("box corner", [(False, (1, 1, 1), (0, 0, 0))], False, ((5, 5, 5), (-1, -1, -1), 10.0, 0.5, 1),
     (0, (4 - 0.5 / S3) / 10, (1, 1, 1), (1 / S3, 1 / S3, 1 / S3))),
    # capsule radius 0.5, half height 1: the side x = -0.5, the top cap y = 1.5
    ("capsule side", [(True, (0.5, 1.0, 0.5), (0, 0, 0))], False, ((-10, 0.3, 0), (1, 0, 0), 20.0, 0.25, 1),
     (0, 9.25 / 20, (-0.5, 0.3, 0), (-1, 0, 0))),
    ("capsule cap", [(True, (0.5, 1.0, 0.5), (0, 0, 0))], False, ((0, 10, 0), (0, -1, 0), 20.0, 0.25, 1), (0, 8.25 / 20, (0, 1.5, 0), (0, 1, 0))),
    # cap, off axis: the cap sphere at y = 1 grown to 0.75; from x = 0.45 straight down it is met at y = 1 + 0.6
    ("capsule cap off axis", [(True, (0.5, 1.0, 0.5), (0, 0, 0))], False, ((0.45, 10, 0), (0, -1, 0), 20.0, 0.25, 1),
     (0, 8.4 / 20, (0.3, 1.4, 0), (0.6, 0.8, 0))),
    ("plane from above", [], True, ((100, 5, 0), (0, -1, 0), 10.0, 1.0, 2), (NO_ENTITY, 0.4, (100, 0, 0), (0, 1, 0))),
    ("plane from below", [], True, ((100, -5, 3), (0, 1, 0), 10.0, 1.0, 2), (NO_ENTITY, 0.4, (100, 0, 3), (0, -1, 0))),
    ("plane, starting within the radius", [], True, ((100, 0.5, 0), (0, -1, 0), 10.0, 1.0, 2), None),
    ("plane, stopping short", [], True, ((100, 5, 0), (0, -1, 0), 3.9, 1.0, 2), None),
    # start rule: overlapping the cube (0.4 from its face), exactly touching it, and the capsule behind is still hit
    ("starts overlapping", [(False, (1, 1, 1), (0, 0, 0))], False, ((1.4, 0, 0), (-1, 0, 0), 10.0, 0.5, 1), None),
    ("starts touching", [(False, (1, 1, 1), (0, 0, 0))], False, ((1.5, 0, 0), (-1, 0, 0), 10.0, 0.5, 1), None),
    ("starts touching, moving away", [(False, (1, 1, 1), (0, 0, 0))], False, ((1.5, 0, 0), (1, 0, 0), 10.0, 0.5, 1), None),
    ("starts overlapping a capsule", [(True, (0.5, 1.0, 0.5), (0, 0, 0))], False, ((0.7, 0, 0), (-1, 0, 0), 10.0, 0.25, 1), None),
    ("starts in the cube, hits the capsule behind", [(False, (1, 1, 1), (0, 0, 0)), (True, (0.5, 1.0, 0.5), (5, 0, 0))], False,
     ((0, 0, 0), (1, 0, 0), 20.0, 0.5, 1), (1, 4.0 / 20, (4.5, 0, 0), (-1, 0, 0))),
    # past the rounded edge: 0.5 from both faces is inside the grown box but 0.707 from the edge
    ("passes the rounded edge", [(False, (1, 1, 1), (0, 0, 0))], False, ((1.5, 5, 0), (0, -1, 0), 3.55, 0.5, 1), None),
]


def hand_objects(bodies):
    return [Obj(RAY_BODY, i, 1, ALL, cap, capsule_dims(size) if cap else box_half_extents(size), pos, IDQ) for i, (cap, size, pos) in enumerate(bodies)]


def check_hand_case(name, got, want, tol=1e-5):
    """got: (entity, f, point, normal) or None."""
    if want is None:
        assert got is None, f"{name}: hit {got}"
        return
    assert got is not None, f"{name}: no hit"
    assert got[0] == want[0], f"{name}: entity {got[0]}"
    assert abs(got[1] - want[1]) <= tol, f"{name}: f {got[1]} vs {want[1]}"
    assert np.allclose(got[2], want[2], atol=10 * tol), f"{name}: point {got[2]} vs {want[2]}"
    assert np.allclose(got[3], want[3], atol=10 * tol), f"{name}: normal {got[3]} vs {want[3]}"


@pytest.mark.parametrize("case", HAND_CASES, ids=[c[0] for c in HAND_CASES])
def test_reference_hand_worked(case):
    name, bodies, plane, (o, d, md, r, mask), want = case
    objs = hand_objects(bodies)
    for hits in (sweep_all(objs, o, d, md, r, mask, plane), SphereRef(World64(objs, plane)).sweep_all(o, d, md, r, mask)):
        got = None if not hits else (hits[0][3], hits[0][0], hits[0][5], hits[0][4])
        check_hand_case(name, got, want, tol=1e-7)


def test_reference_rotated_box_and_distance_definition():
    # 45 degrees about y: the cube's vertical edge at distance sqrt(2) points down the x axis; a sphere of 0.5 from -10 stops there
    q45 = (0.0, math.sin(math.pi / 8), 0.0, math.cos(math.pi / 8))
    cube = Obj(RAY_BODY, 0, 1, 1, False, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), q45)
    h = sweep_all([cube], (-10, 0.5, 0), (1, 0, 0), 20.0, 0.5, 1, False)[0]
    assert h[0] * 20 == pytest.approx(10 - S2 - 0.5) and np.allclose(h[5], (-S2, 0.5, 0)) and np.allclose(h[4], (-1, 0, 0))
    # distance = f * max_distance with a direction that is not normalised
    h2 = sweep_all([cube], (-10, 0.5, 0), (2, 0, 0), 10.0, 0.5, 1, False)[0]
    assert h2[0] == pytest.approx(h[0])


def test_reference_tie_order_and_all_hits():
    a = Obj(RAY_BODY, 9, 1, 1, False, (1, 1, 1), (0, 0, 0), IDQ)
    b = Obj(RAY_BODY, 8, 1, 1, False, (1, 1, 1), (0, 0, 0), IDQ)
    g = Obj(RAY_TRIGGER, 2, 1, 1, False, (1, 1, 1), (0, 0, 0), IDQ)
    far = Obj(RAY_BODY, 1, 1, 1, True, (0.5, 1.0, 0.5), (0, -6, 0), IDQ)
    for hits in (sweep_all([a, g, far, b], (0, 5, 0), (0, -1, 0), 20.0, 0.5, 1, False),
                 SphereRef(World64([a, g, far, b], False)).sweep_all((0, 5, 0), (0, -1, 0), 20.0, 0.5, 1)):
        assert [h[1] for h in hits] == [8, 9, CODE_GHOST | 2, 1]
        assert hits[0][0] == hits[2][0] == pytest.approx(3.5 / 20) and hits[3][0] == pytest.approx(9.0 / 20)
    # the plane after a body at the same fraction; an object mask of 0 and a foreign layer are not candidates
    slab = Obj(RAY_BODY, 3, 2, ALL, False, (5, 1, 5), (0, -1, 0), IDQ)
    hits = sweep_all([slab, Obj(RAY_BODY, 4, 2, 0, False, (1, 1, 1), (0, 3, 0), IDQ), Obj(RAY_BODY, 5, 4, ALL, False, (1, 1, 1), (0, 3, 0), IDQ)],
                     (0, 10, 0), (0, -1, 0), 20.0, 1.0, 2, True)
    assert [h[1] for h in hits] == [3, CODE_PLANE] and hits[0][0] == hits[1][0] == pytest.approx(9.0 / 20)


def test_reference_no_hit_inputs():
    box = Obj(RAY_BODY, 1, 1, 1, False, (1, 1, 1), (0, 0, 0), IDQ)
    ref = SphereRef(World64([box], True))
    nan, inf = float("nan"), float("inf")
    good = ((0, 5, 0), (0, -1, 0), 10.0, 0.5, 1)
    assert len(sweep_all([box], *good, True)) == 1 and len(ref.sweep_all(*good)) == 1
    for o, d, md, r, m in [((0, 5, 0), (0, -1, 0), 0.0, 0.5, 1), ((0, 5, 0), (0, -1, 0), -1.0, 0.5, 1), ((0, 5, 0), (0, -1, 0), 10.0, 0.5, 0),
                           ((0, 5, 0), (0, 0, 0), 10.0, 0.5, 1), ((0, 5, nan), (0, -1, 0), 10.0, 0.5, 1), ((0, 5, 0), (0, nan, 0), 10.0, 0.5, 1),
                           ((0, 5, 0), (0, -1, 0), nan, 0.5, 1), ((0, 5, 0), (0, -1, 0), inf, 0.5, 1), ((0, 5, 0), (0, -1, 0), 10.0, -0.5, 1),
                           ((0, 5, 0), (0, -1, 0), 10.0, nan, 1), ((0, 5, 0), (0, -1, 0), 10.0, inf, 1)]:
        assert sweep_all([box], o, d, md, r, m, True) == [] and ref.sweep_all(o, d, md, r, m) == []
    for c, r, m in [((0, 0, nan), 1.0, 1), ((0, 0, 0), -1.0, 1), ((0, 0, 0), nan, 1), ((0, 0, 0), inf, 1), ((0, 0, 0), 1.0, 0)]:
        assert overlap_all([box], c, r, m, True)[0] == [] and ref.overlap(c, r, m)[0] == []


def test_reference_overlap_hand_worked():
    box = Obj(RAY_BODY, 4, 1, ALL, False, (1, 2, 3), (0, 0, 0), IDQ)
    cap = Obj(RAY_TRIGGER, 2, 1, ALL, True, (0.5, 1.0, 0.5), (10, 0, 0), IDQ)
    objs = [box, cap]
    # inside the box: distance 0; 0.5 outside a face; sqrt(2) / 2 from an edge; capsule: beside it and above its cap
    assert overlap_all(objs, (0.5, 0.5, 0.5), 0.0, 1, False)[0] == [(4, RAY_BODY, 4, 0.0)]
    assert overlap_all(objs, (1.5, 0, 0), 0.6, 1, False)[0][0][3] == pytest.approx(0.5)
    assert overlap_all(objs, (1.5, 0, 0), 0.4, 1, False)[0] == []
    assert overlap_all(objs, (1.5, 2.5, 0), 0.8, 1, False)[0][0][3] == pytest.approx(S2 / 2)
    assert overlap_all(objs, (1.5, 2.5, 0), 0.7, 1, False)[0] == []
    got = overlap_all(objs, (11, 0.5, 0), 0.6, 1, False)[0]
    assert got[0][:3] == (CODE_GHOST | 2, RAY_TRIGGER, 2) and got[0][3] == pytest.approx(0.5)
    assert overlap_all(objs, (10, 2.0, 0), 0.6, 1, False)[0][0][3] == pytest.approx(0.5)
    # the plane: |y| <= radius, mask 2 only; order: bodies, ghosts, the plane
    both = [Obj(RAY_BODY, 4, 3, ALL, False, (1, 2, 3), (0, 0, 0), IDQ), Obj(RAY_TRIGGER, 2, 3, ALL, True, (0.5, 1.0, 0.5), (3, 0, 0), IDQ)]
    got = overlap_all(both, (2, -0.5, 0), 2.0, 2, True)[0]
    assert [h[0] for h in got] == [4, CODE_GHOST | 2, CODE_PLANE] and got[2][3] == pytest.approx(0.5)
    assert overlap_all(both, (2, -0.5, 0), 2.0, 1, True)[0][-1][0] == CODE_GHOST | 2
    # the clear flag: a candidate within 1e-4 * (1 + |centre|) of the radius
    assert not overlap_all(objs, (1.5, 0, 0), 0.50001, 1, False)[1] and overlap_all(objs, (1.5, 0, 0), 0.6, 1, False)[1]


def test_radius_zero_equals_the_ray_reference_on_clear_rays():
    rng = np.random.default_rng(21)
    objs = random_objects(rng, 60)
    ref = SphereRef(World64(objs, True))
    n_clear = n_hits = 0
    for _ in range(300):
        o, d = rng.uniform(-9, 9, 3), rng.normal(size=3)
        md, mask = float(rng.uniform(1, 30)), int(rng.choice([1, 2, 3, 4, ALL]))
        if not clear_decision(objs, o, d, md, mask, True):
            continue
        n_clear += 1
        want = cast_all(objs, o, d, md, mask, True)
        for got in (sweep_all(objs, o, d, md, 0.0, mask, True), ref.sweep_all(o, d, md, 0.0, mask)):
            assert [h[1] for h in got] == [h[1] for h in want]
            for x, y in zip(got, want):
                assert abs(x[0] - y[0]) < 1e-12 and np.allclose(x[4], y[4], atol=1e-9)
                assert np.allclose(x[5], np.asarray(o, np.float32) + (np.asarray(d, np.float32) * np.float32(md)).astype(np.float64) * y[0], atol=1e-9)
        n_hits += len(want)
    assert n_clear > 150 and n_hits > 100


def test_vectorised_reference_equals_scalar_and_overlap_brute_force():
    rng = np.random.default_rng(9)
    objs = random_objects(rng, 100)
    ref = SphereRef(World64(objs, True))
    pos = np.array([ob.origin for ob in objs])
    o, d, md, rad, mask = random_casts(rng, 250, pos, spread=8.0)
    n_hits = 0
    for i in range(len(o)):
        a = sweep_all(objs, o[i], d[i], md[i], rad[i], mask[i], True)
        b = ref.sweep_all(o[i], d[i], md[i], rad[i], mask[i])
        assert [h[1] for h in a] == [h[1] for h in b], i
        for x, y in zip(a, b):
            assert abs(x[0] - y[0]) < 1e-12 and np.allclose(x[4], y[4], atol=1e-8) and np.allclose(x[5], y[5], atol=1e-8)
        n_hits += len(a)
    assert n_hits > 200
    # overlap lists against brute force on the 100-object scene
    c, srad, smask = random_spheres(rng, 400, pos, spread=8.0)
    n_found = 0
    for i in range(len(c)):
        a, ca = overlap_all(objs, c[i], srad[i], smask[i], True)
        b, cb = ref.overlap(c[i], srad[i], smask[i])
        assert [h[:3] for h in a] == [h[:3] for h in b] and ca == cb, i
        assert all(abs(x[3] - y[3]) < 1e-12 for x, y in zip(a, b))
        n_found += len(a)
    assert n_found > 400


def test_touch_is_where_the_distance_equals_the_radius():
    """The union of parts against the definition: at the touch dist(c(f), S) = radius, before it the distance is larger."""
    rng = np.random.default_rng(33)
    objs = random_objects(rng, 40)
    pos = np.array([ob.origin for ob in objs])
    by_code = {ob.code: ob for ob in objs}
    o, d, md, rad, mask = random_casts(rng, 200, pos, spread=8.0)
    n = 0
    for i in range(len(o)):
        frm, delta = o[i].astype(np.float64), (d[i] * md[i]).astype(np.float64)
        for f, code, _, _, normal, point in sweep_all(objs, o[i], d[i], md[i], rad[i], mask[i], False):
            ob = by_code[code]
            assert abs(obj_dist(ob, frm + delta * f) - float(rad[i])) < 1e-9
            assert all(obj_dist(ob, frm + delta * f * s) > float(rad[i]) for s in (0.0, 0.25, 0.5, 0.75, 0.999))
            assert obj_dist(ob, point) < 1e-9 and np.allclose(frm + delta * f - float(rad[i]) * normal, point, atol=1e-9)
            n += 1
    assert n > 100


@pytest.mark.parametrize("n,seed,n_casts", [(2000, 1, 3000), (20000, 2, 3000)])
def test_reference_alone_stays_inside_the_caps_of_the_gpu_comparison(n, seed, n_casts):
    """The GPU tests compare a cast only where it is clear and an overlap sphere only where no object grazes its surface; they
    require half of the casts compared with 50 hits among them, and 90 % of the spheres.  The same generators and seeds on the
    reference alone (the scene before its first tick) must clear those caps, so a GPU failure cannot hide behind them.  A
    sample of the casts and spheres stands for the batch here (the GPU tests take all of them)."""
    rng = np.random.default_rng(seed)
    w64, pos = scene_world64(n, rng)
    casts = random_casts(rng, n_casts, pos)
    spheres = random_spheres(rng, n_casts, pos)
    k = 400
    clear, hits, compared = reference_coverage(SphereRef(w64), tuple(a[:k] for a in casts), tuple(a[:k] for a in spheres))
    print(f"n = {n}: {clear} of {k} casts clear, {hits} of them hits; {compared} of {k} spheres compared")
    assert clear >= 0.5 * k and hits >= 50 and compared >= 0.9 * k


# ------------------------------------------------------------------------------------------------ the ABI


def test_sphere_query_symbols_exported():
    from banggameengine_amd import _capi
    lib = _capi.lib()
    for name in ("bge_world_sphere_cast", "bge_world_sphere_cast_all", "bge_world_sphere_cast_device", "bge_world_overlap_sphere"):
        assert name in _capi.SYMBOLS
        assert getattr(lib, name) is not None
    from banggameengine_amd.world import OVERLAP_HIT_DTYPE, SPHERE_CAST_DTYPE, SPHERE_DTYPE, World, make_sphere_casts, make_spheres
    assert SPHERE_CAST_DTYPE.itemsize == 40 and SPHERE_DTYPE.itemsize == 20 and OVERLAP_HIT_DTYPE.itemsize == 12
    c = make_sphere_casts([[0, 1, 0], [1, 2, 3]], [[0, -1, 0], [1, 0, 0]], [5.0, 6.0], 0.5, 3)
    assert c["max_distance"].tolist() == [5.0, 6.0] and c["radius"].tolist() == [0.5, 0.5] and c["layer_mask"].tolist() == [3, 3]
    assert not c["reserved"].any()
    s = make_spheres([[0, 1, 0]], 2.0)
    assert s["radius"].tolist() == [2.0] and s["layer_mask"].tolist() == [0xFFFFFFFF]
    for name in ("sphere_cast", "sphere_cast_all", "sphere_cast_device", "overlap_sphere"):
        assert callable(getattr(World, name))


def test_sphere_queries_reject_null_world_and_zero_count():
    from banggameengine_amd import _capi
    lib = _capi.lib()
    total = C.c_uint64(5)
    assert lib.bge_world_sphere_cast(None, 1, None, None) == -1
    assert lib.bge_world_sphere_cast(None, 0, None, None) == -1
    assert lib.bge_world_sphere_cast_all(None, 0, None, None, 0, None, C.byref(total)) == -1
    assert lib.bge_world_sphere_cast_device(None, 0, None, None) == -1
    assert lib.bge_world_overlap_sphere(None, 0, None, None, 0, None, C.byref(total)) == -1
    assert lib.bge_last_error()


def test_abi_c99_sphere_records(tmp_path):
    exe = str(tmp_path / "abi_check_sphere")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(CPP, "abi_check_sphere.c"),
                           f"-L{LIBDIR}", "-lbge_world", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sphere abi ok" in r.stdout


def test_adapter_sphere_queries_compile_on_reference_shapes(tmp_path):
    subprocess.check_call(["g++", "-std=c++20", "-O0", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-c",
                           os.path.join(CPP, "sphere_reference_shapes.cpp"), "-o", str(tmp_path / "sphere_reference_shapes.o")])
