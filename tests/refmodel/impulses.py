"""The reference of impulses and of the characters' push (include/bge_world.h "Impulses", "Character push"): apply_ref — Valid,
Apply, Wake and Status in numpy float32 scalars, one rounding per operation, written from the header and not from the kernels —
over a Bodies image of what the device holds, and push_ref, the stage Push of a character step over a STATE_DTYPE array.

`variant` of apply_ref names three WRONG models (the impulses of a body summed before one application, the records of a body in
descending order, no wake): tests/test_impulses_cpu.py shows that the cases tell each of them from the rule."""
from __future__ import annotations

import numpy as np

from .moves import F
from .rays import NO_ENTITY

AT_POINT, CENTRAL, TORQUE, WORLD_POINT = 0, 1, 2, 4
APPLIED, WOKE, INVALID, NO_BODY = 1, 2, 4, 8
# bge_activation
ACT_NONE, ACTIVE_TAG, ISLAND_SLEEPING, WANTS_DEACTIVATION, DISABLE_DEACTIVATION = 0, 1, 2, 3, 4
BODY_STATIC, BODY_DYNAMIC, BODY_KINEMATIC, BODY_NONE = 0, 1, 2, 255
RAY_BODY = 1
CHAR_INVALID = 1
IMPULSE_DTYPE = np.dtype([("entity", "<u4"), ("flags", "<u4"), ("impulse", "<f4", (3,)), ("point", "<f4", (3,))])
assert IMPULSE_DTYPE.itemsize == 32
MAX_RECORDS = (1 << 30) - 1


def make_impulses(entity, impulse, point=None, flags=CENTRAL):
    e = np.atleast_1d(np.asarray(entity, np.uint64)).astype(np.uint32)
    r = np.zeros(len(e), IMPULSE_DTYPE)
    r["entity"] = e
    r["impulse"] = np.asarray(impulse, np.float32).reshape(-1, 3)
    if point is not None:
        r["point"] = np.asarray(point, np.float32).reshape(-1, 3)
    r["flags"] = np.broadcast_to(np.asarray(flags, np.uint32), (len(e),))
    return r


# ------------------------------------------------------------------------------------------------ Inertia


def half_extents(size):
    """A box collider's half extents with margin (btBoxShape with setSafeMargin), float32 as the library computes them."""
    h = [max(F(s), F(0.01)) for s in size]
    m0 = F(0.04)
    i = [c - m0 for c in h]
    safe = F(0.1) * min(h)
    margin = m0
    if safe < margin:
        i = [(c + m0) - safe for c in i]
        margin = safe
    return [c + margin for c in i]


def shape_dims(capsule, size):
    """What the inertia is taken of: a box's half extents with margin, a capsule's (radius, half height, radius)."""
    if capsule:
        r = max(F(size[0]), F(0.01))
        return [r, F(0.5) * (max(F(size[1]), F(0.0)) * F(2.0)), r]
    return half_extents(size)


def local_inertia(capsule, dims, mass):
    mass = F(mass)
    if capsule:
        h = [dims[0], dims[0] + dims[1], dims[0]]
        scaled = mass * F(0.08333333)
    else:
        h = dims
        scaled = mass * F(0.0833333358168602)
    lx, ly, lz = (F(2.0) * c for c in h)
    x2, y2, z2 = lx * lx, ly * ly, lz * lz
    return [scaled * (y2 + z2), scaled * (x2 + z2), scaled * (x2 + y2)]


def mat_from_quat(q):
    x, y, z, w = (F(c) for c in q)
    d = ((x * x + y * y) + z * z) + w * w
    s = F(2.0) / d
    xs, ys, zs = x * s, y * s, z * s
    wx, wy, wz = w * xs, w * ys, w * zs
    xx, xy, xz = x * xs, x * ys, x * zs
    yy, yz, zz = y * ys, y * zs, z * zs
    one = F(1.0)
    return [[one - (yy + zz), xy - wz, xz + wy], [xy + wz, one - (xx + zz), yz - wx], [xz - wy, yz + wx, one - (xx + yy)]]


def inv_inertia_world(capsule, dims, mass, quat):
    il = [F(1.0) / c if c != 0 else F(0.0) for c in local_inertia(capsule, dims, mass)]
    b = mat_from_quat(quat)
    return [[((b[r][0] * il[0]) * b[c][0] + (b[r][1] * il[1]) * b[c][1]) + (b[r][2] * il[2]) * b[c][2] for c in range(3)] for r in range(3)]


def cross3(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def mat_vec(m, v):
    return [(m[r][0] * v[0] + m[r][1] * v[1]) + m[r][2] * v[2] for r in range(3)]


# ------------------------------------------------------------------------------------------------ the bodies


class Bodies:
    """What the rule reads and writes, per ENTITY: body type (BODY_NONE where there is none or the entity has no slot), the
    collider and mass as uploaded, collision group; origin, quaternion, both velocities, the activation state and timer."""

    def __init__(self, types, pos, quat=None, linvel=None, angvel=None, state=None, time=None, capsule=None, size=None, mass=None, group=None):
        n = len(types)
        self.n = n
        self.types = np.asarray(types, np.uint8).copy()
        self.pos = np.asarray(pos, np.float32).reshape(n, 3).copy()
        self.quat = np.tile(np.float32([0, 0, 0, 1]), (n, 1)) if quat is None else np.asarray(quat, np.float32).reshape(n, 4).copy()
        self.linvel = np.zeros((n, 3), np.float32) if linvel is None else np.asarray(linvel, np.float32).reshape(n, 3).copy()
        self.angvel = np.zeros((n, 3), np.float32) if angvel is None else np.asarray(angvel, np.float32).reshape(n, 3).copy()
        self.state = np.where(self.types == BODY_DYNAMIC, ACTIVE_TAG, ACT_NONE).astype(np.uint8) if state is None else np.asarray(state, np.uint8).copy()
        self.time = np.zeros(n, np.float32) if time is None else np.asarray(time, np.float32).copy()
        self.capsule = np.zeros(n, bool) if capsule is None else np.asarray(capsule, bool).copy()
        self.size = np.full((n, 3), 0.5, np.float32) if size is None else np.asarray(size, np.float32).reshape(n, 3).copy()
        self.mass = np.ones(n, np.float32) if mass is None else np.asarray(mass, np.float32).copy()
        self.group = np.ones(n, np.uint32) if group is None else np.asarray(group, np.uint32).copy()

    def copy(self):
        return Bodies(self.types, self.pos, self.quat, self.linvel, self.angvel, self.state, self.time, self.capsule, self.size, self.mass, self.group)

    def dynamic(self, entity):
        return entity < self.n and self.types[entity] == BODY_DYNAMIC

    def mass_of(self, e):
        return max(F(self.mass[e]), F(0.01))


# ------------------------------------------------------------------------------------------------ Valid / Apply / Wake / Status


def record_ok(rec):
    """Valid as far as the record alone decides it: known flags, and every float its kind reads finite."""
    flags = int(rec["flags"])
    if flags & ~(3 | WORLD_POINT):
        return False
    kind = flags & 3
    if kind == 3 or ((flags & WORLD_POINT) and kind != AT_POINT):
        return False
    if not np.isfinite(rec["impulse"]).all():
        return False
    return kind != AT_POINT or bool(np.isfinite(rec["point"]).all())


def apply_one(rec, v, w, inv_mass, inv_i, origin):
    """One record on (v, w): lists of three float32 scalars, changed in place."""
    flags = int(rec["flags"])
    kind = flags & 3
    imp = [F(c) for c in rec["impulse"]]
    if kind != TORQUE:
        for k in range(3):
            v[k] = v[k] + imp[k] * inv_mass
    if kind != CENTRAL:
        t = imp
        if kind == AT_POINT:
            r = [F(c) for c in rec["point"]]
            if flags & WORLD_POINT:
                r = [r[k] - origin[k] for k in range(3)]
            t = cross3(r, imp)
        u = mat_vec(inv_i, t)
        for k in range(3):
            w[k] = w[k] + u[k]


def apply_ref(records, bodies, variant=None):
    """(the Bodies after the call, the status words).  variant: None = the rule; "summed", "reversed", "no wake" = wrong models."""
    out = bodies.copy()
    n = len(records)
    status = np.zeros(n, np.uint32)
    runs = {}  # entity -> the indices of its valid records, ascending
    for i in range(n):
        rec = records[i]
        if not record_ok(rec):
            status[i] = INVALID
        elif not bodies.dynamic(int(rec["entity"])):
            status[i] = NO_BODY
        else:
            runs.setdefault(int(rec["entity"]), []).append(i)
    with np.errstate(all="ignore"):
        for e, idx in runs.items():
            mass = bodies.mass_of(e)
            inv_mass = F(1.0) / mass
            origin = [F(c) for c in bodies.pos[e]]
            inv_i = inv_inertia_world(bool(bodies.capsule[e]), shape_dims(bool(bodies.capsule[e]), bodies.size[e]), mass, bodies.quat[e])
            v = [F(c) for c in bodies.linvel[e]]
            w = [F(c) for c in bodies.angvel[e]]
            if variant == "summed":
                # one application of the summed impulse and the summed torque
                dv, dt = [F(0)] * 3, [F(0)] * 3
                zero_v, zero_w = [F(0)] * 3, [F(0)] * 3
                for i in idx:
                    a, b = list(zero_v), list(zero_w)
                    apply_one(records[i], a, b, F(1.0), [[F(r == c) for c in range(3)] for r in range(3)], origin)
                    dv = [dv[k] + a[k] for k in range(3)]
                    dt = [dt[k] + b[k] for k in range(3)]
                u = mat_vec(inv_i, dt)
                v = [v[k] + dv[k] * inv_mass for k in range(3)]
                w = [w[k] + u[k] for k in range(3)]
            else:
                for i in (reversed(idx) if variant == "reversed" else idx):
                    apply_one(records[i], v, w, inv_mass, inv_i, origin)
            out.linvel[e], out.angvel[e] = v, w
            was_awake = bodies.state[e] == ACTIVE_TAG and bodies.time[e] == 0
            for i in idx:
                status[i] = APPLIED
            if not was_awake:
                status[idx[0]] |= WOKE
            if variant != "no wake":
                out.state[e], out.time[e] = ACTIVE_TAG, 0.0
    return out, status


# ------------------------------------------------------------------------------------------------ Push


def push_ref(state, bodies, dt, force, max_normal_y, body_mask=0xFFFFFFFF):
    """The stage Push over the states a step left: one IMPULSE_DTYPE record per character."""
    n = len(state)
    out = np.zeros(n, IMPULSE_DTYPE)
    out["entity"] = NO_ENTITY
    force, dt, max_normal_y = F(force), F(dt), F(max_normal_y)
    with np.errstate(all="ignore"):
        for i in range(n):
            s = state[i]
            if int(s["flags"]) & CHAR_INVALID or int(s["hit_kind"]) != RAY_BODY:
                continue
            e = int(s["hit_entity"])
            if not bodies.dynamic(e) or (int(bodies.group[e]) & int(body_mask)) == 0:
                continue
            nx, ny, nz = (F(c) for c in s["hit_normal"])
            if not abs(ny) <= max_normal_y:
                continue
            h = np.sqrt(nx * nx + nz * nz)
            m = force * dt
            d = (-nx / h, F(0.0), -nz / h)
            out[i] = (e, CENTRAL, (d[0] * m, d[1] * m, d[2] * m), (0, 0, 0))
    return out
