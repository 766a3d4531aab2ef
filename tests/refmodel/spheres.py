"""The float64 reference of the sphere casts and sphere overlaps (include/bge_world.h bge_world_sphere_cast*,
bge_world_overlap_sphere) on the objects of rays.py: the scalar rule and SphereRef, the same rule vectorised over a World64."""
from __future__ import annotations

import math

import numpy as np

from .rays import CODE_PLANE, NO_ENTITY, RAY_GROUND, ray_box, ray_capsule, ray_valid

EPS_CLEAR = 1e-4


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
    """sweep_all / overlap_all on a World64 (rays.py), vectorised over the objects a bounding-sphere cull leaves."""

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
