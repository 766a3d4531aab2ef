"""The reference of the debug overlay (include/bge_world.h bge_world_debug_lines*): the lines of every shape and contact in
float64, in the order the header states."""
from __future__ import annotations

import numpy as np

COL_STATIC, COL_DYNAMIC, COL_TRIGGER, COL_CONTACT = 0xFF7F7F7F, 0xFF00FFFF, 0xFFFF00FF, 0xFF0000FF
STATIC, DYNAMIC, KINEMATIC, GHOST = "static", "dynamic", "kinematic", "ghost"
SHAPES, CONTACTS, ALL = 1, 2, 3
LINE64 = np.dtype([("from", "<f8", (3,)), ("to", "<f8", (3,)), ("abgr", "<u4")])

BOX_EDGES = np.array([[0, 1], [1, 2], [2, 3], [3, 0], [4, 5], [5, 6], [6, 7], [7, 4], [0, 4], [1, 5], [2, 6], [3, 7]])
BOX_SIGNS = np.array([[-1, -1, -1], [1, -1, -1], [1, 1, -1], [-1, 1, -1], [-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]], np.float64)

# the drawer's angles are formed in binary32: (i / 24) * SIMD_2_PI and (i / 12) * SIMD_HALF_PI, SIMD_HALF_PI = SIMD_2_PI * 0.25
_F = np.float32
_TWO_PI = _F(6.283185307179586232)
_HALF_PI = _F(_TWO_PI * _F(0.25))
RING = np.array([np.float64(_F(_F(i) / _F(24)) * _TWO_PI) for i in range(25)])
HEMI = np.array([np.float64(_F(_F(i) / _F(12)) * _HALF_PI) for i in range(13)])


class Obj:
    """One collision object: kind (STATIC / DYNAMIC / KINEMATIC / GHOST), pose, capsule or box, dims (box: half extents with
    margin; capsule: radius, half height)."""

    def __init__(self, kind, origin, quat=(0, 0, 0, 1), capsule=False, dims=(0.5, 0.5, 0.5)):
        self.kind, self.capsule = kind, bool(capsule)
        self.origin = np.asarray(origin, np.float64)
        self.quat = np.asarray(quat, np.float64)
        self.dims = np.asarray(dims, np.float64)

    def colour(self):
        # CF_NO_CONTACT_RESPONSE first; isStaticObject() holds for Static bodies only (a Kinematic body loses CF_STATIC_OBJECT)
        return COL_TRIGGER if self.kind == GHOST else (COL_STATIC if self.kind == STATIC else COL_DYNAMIC)

    def n_lines(self):
        return 120 if self.capsule else 12


def basis_of(q):
    """btMatrix3x3::setRotation."""
    x, y, z, w = q
    s = 2.0 / (x * x + y * y + z * z + w * w)
    xs, ys, zs = x * s, y * s, z * s
    wx, wy, wz, xx, xy, xz, yy, yz, zz = w * xs, w * ys, w * zs, x * xs, x * ys, x * zs, y * ys, y * zs, z * zs
    return np.array([[1 - (yy + zz), xy - wz, xz + wy], [xy + wz, 1 - (xx + zz), yz - wx], [xz - wy, yz + wx, 1 - (xx + yy)]])


def box_lines(o):
    corners = (BOX_SIGNS * o.dims) @ basis_of(o.quat).T + o.origin
    return corners[BOX_EDGES]  # (12, 2, 3)


def capsule_lines(o):
    r = basis_of(o.quat)
    unit = lambda v: v / np.linalg.norm(v)
    # up axis 1: "axisY" = column 1, "axisX" = column (1 + 1) % 3 = 2, "axisZ" = column (1 + 2) % 3 = 0
    ay, ax, az = unit(r[:, 1]), unit(r[:, 2]), unit(r[:, 0])
    radius, hh = o.dims[0], o.dims[1]
    top, bottom = o.origin + ay * hh, o.origin - ay * hh
    out = []
    for i in range(24):
        d0 = ax * np.cos(RING[i]) + az * np.sin(RING[i])
        d1 = ax * np.cos(RING[i + 1]) + az * np.sin(RING[i + 1])
        t0, t1, b0, b1 = top + d0 * radius, top + d1 * radius, bottom + d0 * radius, bottom + d1 * radius
        out += [(t0, t1), (b0, b1), (t0, b0)]
    for i in range(12):
        s0, c0, s1, c1 = np.sin(HEMI[i]), np.cos(HEMI[i]), np.sin(HEMI[i + 1]), np.cos(HEMI[i + 1])
        u0, u1 = ay * (s0 * radius), ay * (s1 * radius)
        for side in (ax, az):
            f0, f1 = side * (c0 * radius), side * (c1 * radius)
            out += [(top + f0 + u0, top + f1 + u1), (bottom - f0 - u0, bottom - f1 - u1)]
    return np.array(out)  # (120, 2, 3)


def plane_lines():
    """The plane ((0, 1, 0), 0): u = (-1, 0, 0), v = (0, 0, 1), extent 25."""
    u, v = np.array([-1.0, 0, 0]), np.array([0, 0, 1.0])
    c = [(u + v) * 25, (u - v) * 25, (-u - v) * 25, (-u + v) * 25]
    out = [(c[i], c[(i + 1) % 4]) for i in range(4)]
    lerp = lambda a, b, t: a + (b - a) * t
    for i in range(1, 5):
        t = np.float64(_F(i) / _F(5))
        out += [(lerp(c[0], c[3], t), lerp(c[1], c[2], t)), (lerp(c[0], c[1], t), lerp(c[3], c[2], t))]
    return np.array(out)


def in_region(region, p):
    if region is None:
        return True
    mn, mx = (np.asarray(r, np.float32) for r in region)
    p = np.asarray(p, np.float32)
    return bool(np.all(mn <= p) and np.all(p <= mx))  # a NaN or min > max admits nothing


def contact_line(point, normal):
    n = np.asarray(normal, np.float64)
    if n @ n < float(np.finfo(np.float32).eps):
        n = np.array([0.0, 1.0, 0.0])
    n = n / np.linalg.norm(n)
    p = np.asarray(point, np.float64)
    return p, p + n * 0.25


def debug_lines_ref(objects, plane, contacts=(), flags=ALL, region=None):
    """objects: Obj in the order of the specification (bodies by entity index, then ghosts by trigger order); plane: bool;
    contacts: (pointOnB, normalWorldOnB) pairs.  Returns LINE64 records: the shapes section, then the contact section."""
    parts, colours = [np.zeros((0, 2, 3))], [np.zeros(0, np.uint32)]

    def add(lines, colour):
        parts.append(np.asarray(lines, np.float64).reshape(-1, 2, 3))
        colours.append(np.full(len(parts[-1]), colour, np.uint32))

    if flags & SHAPES:
        if plane:
            add(plane_lines(), COL_STATIC)
        for o in objects:
            if in_region(region, o.origin):
                add(capsule_lines(o) if o.capsule else box_lines(o), o.colour())
    if flags & CONTACTS:
        for point, normal in contacts:
            if in_region(region, point):
                add([contact_line(point, normal)], COL_CONTACT)
    lines = np.concatenate(parts)
    out = np.zeros(len(lines), LINE64)
    out["from"], out["to"], out["abgr"] = lines[:, 0], lines[:, 1], np.concatenate(colours)
    return out
