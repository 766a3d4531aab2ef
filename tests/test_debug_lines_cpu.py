"""The debug overlay's specification (include/bge_world.h bge_world_debug_lines*) as a float64 reference, with hand-worked cases,
plus the C99 view of the record and the C++20 compile of the adapter's overlay members.

debug_lines_ref() is written from the description of the reference's drawer (BulletDebugDrawer: DrawBox, DrawCapsule,
DrawStaticPlane, drawContactPoint; PhysicsSystem::CollectDebugLines for the colours): the GPU tests compare the device's lines
with it."""
from __future__ import annotations

import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

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


# ---------------------------------------------------------------- hand-worked cases

def test_unit_box_at_the_origin():
    got = debug_lines_ref([Obj(DYNAMIC, (0, 0, 0), dims=(1, 1, 1))], plane=False)
    c = [(-1, -1, -1), (1, -1, -1), (1, 1, -1), (-1, 1, -1), (-1, -1, 1), (1, -1, 1), (1, 1, 1), (-1, 1, 1)]
    want = [(c[a], c[b]) for a, b in [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)]]
    assert len(got) == 12
    assert np.array_equal(got["from"], np.array([w[0] for w in want], np.float64))
    assert np.array_equal(got["to"], np.array([w[1] for w in want], np.float64))
    assert set(got["abgr"].tolist()) == {COL_DYNAMIC}


def test_box_rotated_a_quarter_turn_about_y():
    h = np.sqrt(0.5)
    got = debug_lines_ref([Obj(STATIC, (10, 0, 0), quat=(0, h, 0, h), dims=(2, 1, 0.5))], plane=False)
    # +90 degrees about y takes local x to world -z and local z to world x: corner 0 (-2, -1, -0.5) -> (-0.5, -1, 2)
    assert np.allclose(got["from"][0], (10 - 0.5, -1, 2), atol=1e-12)
    assert np.allclose(got["to"][0], (10 - 0.5, -1, -2), atol=1e-12)      # corner 1 (2, -1, -0.5)
    assert np.allclose(got["to"][8], (10 + 0.5, -1, 2), atol=1e-12)       # edge 0-4: corner 4 (-2, -1, 0.5)
    assert set(got["abgr"].tolist()) == {COL_STATIC}


def test_upright_capsule():
    got = debug_lines_ref([Obj(KINEMATIC, (0, 0, 0), capsule=True, dims=(0.5, 1.0, 0.5))], plane=False)
    assert len(got) == 120
    ring = got[:72]
    for k in range(24):
        top, bottom, side = ring[3 * k], ring[3 * k + 1], ring[3 * k + 2]
        for rec, y in ((top, 1.0), (bottom, -1.0)):
            for p in (rec["from"], rec["to"]):
                assert abs(p[1] - y) < 1e-12 and abs(np.hypot(p[0], p[2]) - 0.5) < 1e-7
        assert np.array_equal(side["from"], top["from"]) and np.array_equal(side["to"], bottom["from"])
        assert np.allclose(top["to"], ring[3 * ((k + 1) % 24)]["from"], atol=1e-6)  # the ring closes
    # the ring starts on the basis' Z column and turns towards its X column
    assert np.allclose(ring[0]["from"], (0, 1, 0.5), atol=1e-12) and np.allclose(ring[3 * 6]["from"], (0.5, 1, 0), atol=1e-7)
    hemi = got[72:]
    assert np.allclose(hemi[0]["from"], (0, 1, 0.5), atol=1e-12)   # top, Z-column plane
    assert np.allclose(hemi[1]["from"], (0, -1, -0.5), atol=1e-12)  # bottom, mirrored
    assert np.allclose(hemi[2]["from"], (0.5, 1, 0), atol=1e-12)   # top, X-column plane
    for k in range(4):
        assert np.allclose(hemi[44 + k]["to"], (0, 1.5 if k % 2 == 0 else -1.5, 0), atol=1e-7)
    assert set(got["abgr"].tolist()) == {COL_DYNAMIC}  # Kinematic is NOT static-coloured


def test_plane_constants():
    got = debug_lines_ref([], plane=True)
    assert len(got) == 12 and set(got["abgr"].tolist()) == {COL_STATIC}
    c = [(-25, 0, 25), (-25, 0, -25), (25, 0, -25), (25, 0, 25)]
    for i in range(4):
        assert np.array_equal(got["from"][i], c[i]) and np.array_equal(got["to"][i], c[(i + 1) % 4])
    assert np.allclose(got["from"][4], (-15, 0, 25), atol=1e-5) and np.allclose(got["to"][4], (-15, 0, -25), atol=1e-5)
    assert np.allclose(got["from"][5], (-25, 0, 15), atol=1e-5) and np.allclose(got["to"][5], (25, 0, 15), atol=1e-5)
    assert np.allclose(got["from"][10], (15, 0, 25), atol=1e-5) and np.allclose(got["from"][11], (-25, 0, -15), atol=1e-5)


def test_colours_and_contact_lines():
    objs = [Obj(STATIC, (0, 0, 0)), Obj(DYNAMIC, (2, 0, 0)), Obj(KINEMATIC, (4, 0, 0)), Obj(GHOST, (6, 0, 0))]
    contacts = [((1, 0, 1), (0, 2, 0)), ((0, 1, 0), (0, 0, 0)), ((0, 0, 0), (3, 0, 4))]
    got = debug_lines_ref(objs, True, contacts)
    assert len(got) == 12 + 48 + 3
    assert [int(got["abgr"][12 * k]) for k in range(5)] == [COL_STATIC, COL_STATIC, COL_DYNAMIC, COL_DYNAMIC, COL_TRIGGER]
    tail = got[60:]
    assert set(tail["abgr"].tolist()) == {COL_CONTACT}
    assert np.allclose(tail["to"][0], (1, 0.25, 1)) and np.allclose(tail["to"][1], (0, 1.25, 0))  # normalised; degenerate -> +y
    assert np.allclose(tail["to"][2], (0.15, 0, 0.2))
    # the two flags are the two halves
    assert np.array_equal(debug_lines_ref(objs, True, contacts, SHAPES), got[:60])
    assert np.array_equal(debug_lines_ref(objs, True, contacts, CONTACTS), got[60:])


def test_region_rule():
    objs = [Obj(DYNAMIC, (1, 2, 3)), Obj(DYNAMIC, (1.5, 2, 3)), Obj(GHOST, (0, 0, 0), capsule=True)]
    contacts = [((1, 0, 3), (0, 1, 0)), ((9, 0, 9), (0, 1, 0))]
    got = debug_lines_ref(objs, True, contacts, region=((0, 0, 0), (1, 2, 3)))  # origin exactly on region_max is in
    assert len(got) == 12 + 12 + 120 + 1
    assert np.array_equal(got[12:24], debug_lines_ref(objs[:1], False))
    nan = float("nan")
    for bad in (((nan, 0, 0), (5, 5, 5)), ((0, 0, 0), (5, nan, 5)), ((2, 0, 0), (1, 5, 5))):
        got = debug_lines_ref(objs, True, contacts, region=bad)
        assert len(got) == 12 and np.array_equal(got, debug_lines_ref([], True))  # only the plane


# ---------------------------------------------------------------- the C and C++ views

def test_c99_record_layout(tmp_path):
    exe = str(tmp_path / "abi_check_debug")
    lib = os.path.join(ROOT, "banggameengine_amd")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "abi_check_debug.c"), f"-L{lib}", "-lbge_world", f"-Wl,-rpath,{lib}",
                           "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "debug abi ok" in r.stdout


def test_adapter_overlay_members_compile_against_reference_shapes(tmp_path):
    subprocess.check_call(["g++", "-std=c++20", "-O0", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-c",
                           os.path.join(ROOT, "tests", "cpp", "debug_reference_shapes.cpp"), "-o", str(tmp_path / "debug_reference_shapes.o")])
