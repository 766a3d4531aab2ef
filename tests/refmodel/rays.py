"""The float64 reference of the ray queries (include/bge_world.h bge_world_raycast*): the shapes and their poses as the library
holds them, the scalar rule object by object, and World64, the same rule vectorised over the objects.  numpy and math only."""
from __future__ import annotations

import math

import numpy as np

RAY_MISS, RAY_BODY, RAY_TRIGGER, RAY_GROUND = 0, 1, 2, 3
NO_ENTITY = 0xFFFFFFFF
CODE_GHOST, CODE_PLANE = 1 << 30, (2 << 30) | ((1 << 30) - 1)


def quat_to_mat(q):
    """btMatrix3x3::setRotation in float64 (s = 2 / |q|^2)."""
    x, y, z, w = (float(v) for v in q)
    s = 2.0 / (x * x + y * y + z * z + w * w)
    xs, ys, zs = x * s, y * s, z * s
    wx, wy, wz = w * xs, w * ys, w * zs
    xx, xy, xz = x * xs, x * ys, x * zs
    yy, yz, zz = y * ys, y * zs, z * zs
    return np.array([[1 - (yy + zz), xy - wz, xz + wy], [xy + wz, 1 - (xx + zz), yz - wx], [xz - wy, yz + wx, 1 - (xx + yy)]])


def quat_from_euler(e):
    """ToBtQuaternion(euler) = setEulerZYX(yaw = e.y, pitch = e.x, roll = e.z), float64."""
    hy, hp, hr = e[1] * 0.5, e[0] * 0.5, e[2] * 0.5
    cy, sy, cp, sp, cr, sr = math.cos(hy), math.sin(hy), math.cos(hp), math.sin(hp), math.cos(hr), math.sin(hr)
    return np.array([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy])


def box_half_extents(size):
    """collider_half_extents for a box, in binary32 as the library computes it (btBoxShape: implicit = he - 0.04, safe margin)."""
    h = np.maximum(np.asarray(size, np.float32), np.float32(0.01))
    m0 = np.float32(0.04)
    inner = (h - m0).astype(np.float32)
    safe = np.float32(0.1) * h.min()
    if safe < m0:
        return (((inner + m0).astype(np.float32) - safe).astype(np.float32) + safe).astype(np.float32)
    return (inner + m0).astype(np.float32)


def capsule_dims(size):
    r = max(np.float32(size[0]), np.float32(0.01))
    return np.array([r, max(np.float32(size[1]), np.float32(0.0)), r], np.float32)


def ray_box(o, d, h):
    """Sharp box: (f, local normal) of the first entry, None on a miss or when o is inside / on the box."""
    if all(abs(o[a]) <= h[a] for a in range(3)):
        return None
    tn, tf, ax = -math.inf, math.inf, -1
    for a in range(3):
        if d[a] == 0.0:
            if abs(o[a]) > h[a]:
                return None
            continue
        t1, t2 = (-h[a] - o[a]) / d[a], (h[a] - o[a]) / d[a]
        near, far = min(t1, t2), max(t1, t2)
        if near > tn:
            tn, ax = near, a
        tf = min(tf, far)
    if ax < 0 or not (tn <= tf) or not (0.0 <= tn <= 1.0):
        return None
    n = np.zeros(3)
    n[ax] = -1.0 if d[ax] > 0 else 1.0
    return tn, n


def ray_capsule(o, d, r, hh):
    """Y-axis capsule (radius r, half height hh): (f, local normal) or None (miss, or o inside / on it)."""
    cy = min(max(o[1], -hh), hh)
    if o[0] ** 2 + (o[1] - cy) ** 2 + o[2] ** 2 <= r * r:
        return None
    best, bn = math.inf, None
    a = d[0] ** 2 + d[2] ** 2
    if a > 0:
        b = o[0] * d[0] + o[2] * d[2]
        c = o[0] ** 2 + o[2] ** 2 - r * r
        disc = b * b - a * c
        if disc >= 0:
            t = (-b - math.sqrt(disc)) / a
            y = o[1] + d[1] * t
            if 0 <= t <= 1 and abs(y) <= hh:
                best, bn = t, np.array([o[0] + d[0] * t, 0.0, o[2] + d[2] * t])
    aa = float(np.dot(d, d))
    for c0 in (-hh, hh):
        m = np.array([o[0], o[1] - c0, o[2]])
        bb, cc = float(np.dot(m, d)), float(np.dot(m, m)) - r * r
        disc = bb * bb - aa * cc
        if disc >= 0:
            t = (-bb - math.sqrt(disc)) / aa
            if 0 <= t <= 1 and t < best:
                best, bn = t, m + d * t
    if bn is None:
        return None
    return best, bn / np.linalg.norm(bn)


def ray_plane(from_y, to_y):
    """y = 0 from either side (btTriangleRaycastCallback, no back-face filter): ends strictly on opposite sides."""
    if not ((from_y > 0 and to_y < 0) or (from_y < 0 and to_y > 0)):
        return None
    return from_y / (from_y - to_y), np.array([0.0, 1.0 if from_y > 0 else -1.0, 0.0])


class Obj:
    """A collision object of the query's world: kind RAY_BODY / RAY_TRIGGER, entity, filter words, shape, pose."""

    def __init__(self, kind, entity, group, mask, capsule, dims, origin, quat):
        self.kind, self.entity, self.group, self.mask = kind, int(entity), int(group), int(mask)
        self.capsule, self.dims = bool(capsule), np.asarray(dims, np.float64)
        self.origin, self.basis = np.asarray(origin, np.float64), quat_to_mat(quat)

    @property
    def code(self):
        return self.entity if self.kind == RAY_BODY else CODE_GHOST | self.entity

    def cast(self, frm, delta, grow=0.0):
        o = self.basis.T @ (frm - self.origin)
        d = self.basis.T @ delta
        if self.capsule:
            r = ray_capsule(o, d, self.dims[0] + grow, self.dims[1])
        else:
            r = ray_box(o, d, self.dims + grow)
        return None if r is None else (r[0], self.basis @ r[1])


def ray_valid(origin, direction, max_distance, mask):
    o, d = np.asarray(origin, np.float32), np.asarray(direction, np.float32)
    md = np.float32(max_distance)
    with np.errstate(all="ignore"):
        delta = d * md
        ok = (np.isfinite(o).all() and np.isfinite(d).all() and np.isfinite(md) and md > 0 and int(mask) != 0 and (d != 0).any()
              and np.isfinite(delta).all() and np.isfinite(np.float32(np.dot(delta, delta))))
    return bool(ok)


def cast_all(objs, origin, direction, max_distance, mask, plane, grow=0.0):
    """Every hit of one ray: sorted list of (f, code, kind, entity, normal)."""
    if not ray_valid(origin, direction, max_distance, mask):
        return []
    frm = np.asarray(origin, np.float32).astype(np.float64)
    delta = (np.asarray(direction, np.float32) * np.float32(max_distance)).astype(np.float64)
    out = []
    for ob in objs:
        if (ob.group & int(mask)) == 0 or ob.mask == 0:
            continue
        r = ob.cast(frm, delta, grow)
        if r is not None:
            out.append((r[0], ob.code, ob.kind, ob.entity, r[1]))
    if plane and (int(mask) & 2):
        r = ray_plane(frm[1], frm[1] + delta[1])
        if r is not None:
            out.append((r[0], CODE_PLANE, RAY_GROUND, NO_ENTITY, r[1]))
    out.sort(key=lambda h: (h[0], h[1]))
    return out


def cast_closest(objs, origin, direction, max_distance, mask, plane):
    hits = cast_all(objs, origin, direction, max_distance, mask, plane)
    return hits[0] if hits else None


def clear_decision(objs, origin, direction, max_distance, mask, plane, eps=1e-4):
    """The closest object is well defined: the runner-up is more than eps further along in f, and growing or shrinking every
    shape by eps (a ray grazing an edge, a near miss, an origin near a surface) does not change which objects are hit."""
    base = cast_all(objs, origin, direction, max_distance, mask, plane)
    if len(base) > 1 and base[1][0] - base[0][0] <= eps:
        return False
    codes = [h[1] for h in base]
    for g in (eps, -eps):
        if [h[1] for h in cast_all(objs, origin, direction, max_distance, mask, plane, grow=g)] != codes:
            return False
    return True


class World64:
    """The same reference, vectorised over the objects (the GPU tests cast thousands of rays at thousands of objects)."""

    def __init__(self, objs, plane):
        self.plane = bool(plane)
        n = len(objs)
        self.kind = np.array([o.kind for o in objs], np.int64).reshape(n)
        self.entity = np.array([o.entity for o in objs], np.int64).reshape(n)
        self.group = np.array([o.group for o in objs], np.int64).reshape(n)
        self.omask = np.array([o.mask for o in objs], np.int64).reshape(n)
        self.capsule = np.array([o.capsule for o in objs], bool).reshape(n)
        self.dims = np.array([o.dims for o in objs], np.float64).reshape(n, 3)
        self.origin = np.array([o.origin for o in objs], np.float64).reshape(n, 3)
        self.basis = np.array([o.basis for o in objs], np.float64).reshape(n, 3, 3)
        self._derive()

    @classmethod
    def from_arrays(cls, kind, entity, group, mask, capsule, dims, origin, quat, plane):
        """Same world from per-object arrays (quat (n, 4) xyzw) without a Python object per body."""
        w = cls([], plane)
        w.kind, w.entity = np.asarray(kind, np.int64), np.asarray(entity, np.int64)
        w.group, w.omask = np.asarray(group, np.int64), np.asarray(mask, np.int64)
        w.capsule, w.dims, w.origin = np.asarray(capsule, bool), np.asarray(dims, np.float64), np.asarray(origin, np.float64)
        q = np.asarray(quat, np.float64)
        x, y, z, ww = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        s = 2.0 / (x * x + y * y + z * z + ww * ww)
        xs, ys, zs = x * s, y * s, z * s
        wx, wy, wz, xx, xy, xz, yy, yz, zz = ww * xs, ww * ys, ww * zs, x * xs, x * ys, x * zs, y * ys, y * zs, z * zs
        w.basis = np.stack([np.stack([1 - (yy + zz), xy - wz, xz + wy], 1), np.stack([xy + wz, 1 - (xx + zz), yz - wx], 1),
                            np.stack([xz - wy, yz + wx, 1 - (xx + yy)], 1)], 1)
        w._derive()
        return w

    def _derive(self):
        self.code = np.where(self.kind == RAY_BODY, self.entity, CODE_GHOST | self.entity)
        # bounding spheres: a cull before the exact tests (shapes grown by at most 1e-3 stay inside).  sandwich.py
        # edits dims and calls this again, so the cull radius must stay a function of dims alone.
        self.radius = np.where(self.capsule, self.dims[:, 0] + self.dims[:, 1], np.linalg.norm(self.dims, axis=1)) + 2e-3
        self._min_dim = None

    def min_dim(self, code):
        """Smallest half extent (box) or radius (capsule) of the object with this code; 1 for the plane."""
        if self._min_dim is None:
            small = np.where(self.capsule, self.dims[:, 0], self.dims.min(axis=1))
            self._min_dim = dict(zip(self.code.tolist(), small.tolist()))
        return self._min_dim.get(int(code), 1.0)

    def cast_all(self, origin, direction, max_distance, mask, grow=0.0):
        if not ray_valid(origin, direction, max_distance, mask):
            return []
        frm = np.asarray(origin, np.float32).astype(np.float64)
        delta = (np.asarray(direction, np.float32) * np.float32(max_distance)).astype(np.float64)
        w = self.origin - frm
        t = np.clip((w @ delta) / float(delta @ delta), 0.0, 1.0)
        e = w - t[:, None] * delta
        near = (e * e).sum(axis=1) <= self.radius ** 2
        sel = np.nonzero(near & ((self.group & int(mask)) != 0) & (self.omask != 0))[0]
        out = []
        if len(sel):
            B = self.basis[sel]
            o = np.einsum("nji,nj->ni", B, frm - self.origin[sel])
            d = np.einsum("nji,j->ni", B, delta)
            h = self.dims[sel] + grow
            cap = self.capsule[sel]
            f = np.full(len(sel), np.inf)
            nl = np.zeros((len(sel), 3))
            with np.errstate(all="ignore"):
                # boxes
                inside = (np.abs(o) <= h).all(axis=1)
                par = d == 0
                bad = (par & (np.abs(o) > h)).any(axis=1)
                t1, t2 = (-h - o) / d, (h - o) / d
                near = np.where(par, -np.inf, np.minimum(t1, t2))
                far = np.where(par, np.inf, np.maximum(t1, t2))
                ax = np.argmax(near, axis=1)
                tn = near[np.arange(len(sel)), ax]
                tf = far.min(axis=1)
                hit = ~cap & ~inside & ~bad & (tn > -np.inf) & (tn <= tf) & (tn >= 0) & (tn <= 1)
                f = np.where(hit, tn, f)
                sgn = np.where(d[np.arange(len(sel)), ax] > 0, -1.0, 1.0)
                nb = np.zeros((len(sel), 3))
                nb[np.arange(len(sel)), ax] = sgn
                nl = np.where(hit[:, None], nb, nl)
                # capsules: side, then the two cap spheres
                r, hh = h[:, 0], self.dims[sel][:, 1]
                cy = np.clip(o[:, 1], -hh, hh)
                cin = o[:, 0] ** 2 + (o[:, 1] - cy) ** 2 + o[:, 2] ** 2 <= r * r
                a = d[:, 0] ** 2 + d[:, 2] ** 2
                b = o[:, 0] * d[:, 0] + o[:, 2] * d[:, 2]
                c = o[:, 0] ** 2 + o[:, 2] ** 2 - r * r
                disc = b * b - a * c
                t = (-b - np.sqrt(disc)) / a
                y = o[:, 1] + d[:, 1] * t
                side = cap & ~cin & (a > 0) & (disc >= 0) & (t >= 0) & (t <= 1) & (np.abs(y) <= hh)
                best = np.where(side, t, np.inf)
                bn = np.where(side[:, None], np.stack([o[:, 0] + d[:, 0] * t, np.zeros_like(t), o[:, 2] + d[:, 2] * t], 1), 0.0)
                aa = (d * d).sum(axis=1)
                for c0 in (-1.0, 1.0):
                    m = o - np.stack([np.zeros_like(hh), c0 * hh, np.zeros_like(hh)], 1)
                    bb, cc = (m * d).sum(axis=1), (m * m).sum(axis=1) - r * r
                    ds = bb * bb - aa * cc
                    ts = (-bb - np.sqrt(ds)) / aa
                    ok = cap & ~cin & (ds >= 0) & (ts >= 0) & (ts <= 1) & (ts < best)
                    best = np.where(ok, ts, best)
                    bn = np.where(ok[:, None], m + d * ts[:, None], bn)
                bn = bn / np.linalg.norm(bn, axis=1, keepdims=True)
                f = np.where(cap, best, f)
                nl = np.where(cap[:, None], bn, nl)
            for k in np.nonzero(np.isfinite(f))[0]:
                i = sel[k]
                out.append((float(f[k]), int(self.code[i]), int(self.kind[i]), int(self.entity[i]), B[k] @ nl[k]))
        if self.plane and (int(mask) & 2):
            r = ray_plane(frm[1], frm[1] + delta[1])
            if r is not None:
                out.append((r[0], CODE_PLANE, RAY_GROUND, NO_ENTITY, r[1]))
        out.sort(key=lambda hit: (hit[0], hit[1]))
        return out

    def clear(self, origin, direction, max_distance, mask, eps=1e-4):
        """clear_decision() on this world."""
        base = self.cast_all(origin, direction, max_distance, mask)
        if len(base) > 1 and base[1][0] - base[0][0] <= eps:
            return False
        codes = [h[1] for h in base]
        return all([h[1] for h in self.cast_all(origin, direction, max_distance, mask, grow=g)] == codes for g in (eps, -eps))


ALL = 0xFFFFFFFF
