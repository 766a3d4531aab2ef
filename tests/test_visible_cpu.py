"""Frustum culling (include/bge_world.h bge_world_visible*): the rule restated in numpy binary32 operation for operation, a float64
geometric reference (box corners through the matrix against normalised planes), hand-worked cases, bge_frustum_planes, the
exported symbols, the C99 view of the header and the C++20 compile of the adapter's members.

The GPU tests (test_gpu_visible.py) compare the device's list with visible_ref32() exactly and with visible_ref64() wherever the
latter is not ambiguous; the conditions that make that comparison meaningful for the seeded scene are asserted here."""
from __future__ import annotations

import math
import os
import subprocess

import numpy as np

import banggameengine_amd as B
from banggameengine_amd import world as W
from oracle import np_oracle as npo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
AMBIGUOUS_REL = 1e-4  # within this x (1 + |cw|_inf + |h * scale|_inf) of a plane the float64 reference does not decide
IDENTITY = np.eye(4, dtype=F).reshape(1, 16)


# ---------------------------------------------------------------- the two references

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


# ---------------------------------------------------------------- the seeded scene and its views

def make_scene(seed=7, n=4000):
    """Flat scene: positions uniform in +-50, euler +-3, scale 0.25..4, centres +-1, half extents 0.05..2."""
    rng = np.random.default_rng(seed)
    return dict(pos=rng.uniform(-50, 50, (n, 3)).astype(F), euler=rng.uniform(-3, 3, (n, 3)).astype(F),
                scale=rng.uniform(0.25, 4, (n, 3)).astype(F), center=rng.uniform(-1, 1, (n, 3)).astype(F),
                half=rng.uniform(0.05, 2, (n, 3)).astype(F))


def view_proj(eye=(0.0, 10.0, -80.0), fov_deg=60.0, aspect=16.0 / 9.0, near=0.1, far=150.0, homogeneous_depth=False):
    """Looking down +z from eye (left-handed, as bx::mtxProj): view = translate(-eye), row-vector convention."""
    view = np.eye(4, dtype=np.float64)
    view[3, :3] = -np.asarray(eye, np.float64)
    h = 1.0 / math.tan(math.radians(fov_deg) * 0.5)
    proj = np.zeros((4, 4), np.float64)
    proj[0, 0], proj[1, 1], proj[2, 3] = h / aspect, h, 1.0
    if homogeneous_depth:
        proj[2, 2], proj[3, 2] = (far + near) / (far - near), -2.0 * far * near / (far - near)
    else:
        proj[2, 2], proj[3, 2] = far / (far - near), -near * far / (far - near)
    return (view @ proj).astype(F).reshape(16)


def wide_view():
    return W.frustum_planes(view_proj(), False)


def narrow_view():
    return W.frustum_planes(view_proj(fov_deg=12.0), False)


# ---------------------------------------------------------------- hand-worked cases

def _one(world, center, half, planes):
    return bool(visible_ref32(np.asarray(world, F).reshape(1, 16), [center], [half], planes)[0])


def test_unit_box_touching_a_plane_is_visible_and_one_ulp_beyond_is_not():
    # identity matrix, centre 0, half 1, plane x + d >= 0: e = (1, 0, 0), r = 1, sd = d
    assert _one(IDENTITY, (0, 0, 0), (1, 1, 1), [(1, 0, 0, -1.0)])
    assert not _one(IDENTITY, (0, 0, 0), (1, 1, 1), [(1, 0, 0, np.nextafter(F(-1), F(-2)))])
    assert _one(IDENTITY, (0, 0, 0), (1, 1, 1), [(1, 0, 0, np.nextafter(F(-1), F(0)))])
    # an unnormalised plane scales both sides: 4x + d >= 0 touches at d = -4
    assert _one(IDENTITY, (0, 0, 0), (1, 1, 1), [(4, 0, 0, -4.0)])
    assert not _one(IDENTITY, (0, 0, 0), (1, 1, 1), [(4, 0, 0, np.nextafter(F(-4), F(-5)))])
    # the float64 geometry agrees away from the boundary
    vis, amb = visible_ref64(IDENTITY, [(0, 0, 0)], [(1, 1, 1)], [(1, 0, 0, -0.5)])
    assert vis[0] and not amb[0]
    vis, amb = visible_ref64(IDENTITY, [(0, 0, 0)], [(1, 1, 1)], [(1, 0, 0, -1.5)])
    assert not vis[0] and not amb[0]


def test_rotated_and_non_uniformly_scaled_box():
    # scale (2, 3, 4), then a quarter turn that takes local x to world y and local y to world -x, then translate to (10, 0, 0)
    m = np.array([0, 2, 0, 0, -3, 0, 0, 0, 0, 0, 4, 0, 10, 0, 0, 1], F)
    h = (1, 1, 1)
    # plane x + d: e = (0, -3, 0), r = 3, sd = 10 + d: the box spans x in [7, 13]
    assert _one(m, (0, 0, 0), h, [(1, 0, 0, -13.0)])
    assert not _one(m, (0, 0, 0), h, [(1, 0, 0, np.nextafter(F(-13), F(-14)))])
    # plane y + d: e = (2, 0, 0), r = 2, sd = d: y in [-2, 2]
    assert _one(m, (0, 0, 0), h, [(0, 1, 0, -2.0)]) and not _one(m, (0, 0, 0), h, [(0, 1, 0, -2.0000002)])
    # plane -z + d: r = 4: z in [-4, 4]
    assert _one(m, (0, 0, 0), h, [(0, 0, -1, -4.0)]) and not _one(m, (0, 0, 0), h, [(0, 0, -1, -4.000001)])
    # a centre offset goes through the matrix: c = (1, 0, 0) -> cw = (10, 2, 0); y now spans [0, 4]
    assert _one(m, (1, 0, 0), h, [(0, 1, 0, -4.0)]) and not _one(m, (1, 0, 0), h, [(0, 1, 0, -4.000001)])
    # all planes must hold
    assert not _one(m, (0, 0, 0), h, [(1, 0, 0, -13.0), (0, 1, 0, -3.0)])
    vis, amb = visible_ref64(m.reshape(1, 16), [(1, 0, 0)], [h], [(0, 1, 0, -3.9), (1, 0, 0, -12.9)])
    assert vis[0] and not amb[0]
    vis, _ = visible_ref64(m.reshape(1, 16), [(1, 0, 0)], [h], [(0, 1, 0, -4.1)])
    assert not vis[0]


def test_nan_culls_and_no_planes_lists_everything_renderable():
    nan = float("nan")
    assert not _one(IDENTITY, (0, 0, 0), (1, 1, 1), [(nan, 0, 0, 5.0)])
    assert not _one(IDENTITY, (0, 0, 0), (1, 1, 1), [(1, 0, 0, 5.0), (0, 1, 0, nan)])
    assert _one(IDENTITY, (0, 0, 0), (1, 1, 1), [(1, 0, 0, 5.0)])
    m = IDENTITY.copy()
    m[0, 13] = nan  # a NaN in the matrix
    assert not _one(m, (0, 0, 0), (1, 1, 1), [(0, 1, 0, 5.0)])
    assert _one(IDENTITY, (0, 0, 0), (1, 1, 1), None) and _one(IDENTITY, (0, 0, 0), (0, 0, 0), None)
    for c, h in (((0, 0, 0), (1, -1, 1)), ((0, 0, 0), (1, nan, 1)), ((0, 0, 0), (float("inf"), 1, 1)), ((nan, 0, 0), (1, 1, 1)),
                 ((0, float("inf"), 0), (1, 1, 1))):
        assert not _one(IDENTITY, c, h, None), (c, h)
    assert not bool(visible_ref32(IDENTITY, [(0, 0, 0)], [(1, 1, 1)], None, eligible=[False])[0])


# ---------------------------------------------------------------- bge_frustum_planes

def test_frustum_planes_are_single_adds_of_matrix_columns():
    rng = np.random.default_rng(3)
    for homogeneous in (False, True):
        for vp in (view_proj(homogeneous_depth=homogeneous), rng.uniform(-2, 2, 16).astype(F)):
            got = W.frustum_planes(vp, homogeneous)
            assert got.shape == (6, 4) and got.dtype == F
            assert np.array_equal(got.view(np.uint32), frustum_planes_ref(vp, homogeneous).view(np.uint32))


def test_frustum_planes_of_a_hand_built_view_projection():
    near, far, fov, aspect, eye = 0.1, 150.0, 60.0, 16.0 / 9.0, np.array([0.0, 10.0, -80.0])
    ty = math.tan(math.radians(fov) * 0.5)
    tx = ty * aspect
    for homogeneous in (False, True):
        pl = W.frustum_planes(view_proj(homogeneous_depth=homogeneous), homogeneous).astype(np.float64)
        inside = lambda p: bool(np.all(pl[:, :3] @ p + pl[:, 3] >= 0))
        which = lambda p: set(np.nonzero(pl[:, :3] @ p + pl[:, 3] < 0)[0].tolist())
        z = 40.0
        assert inside(eye + (0, 0, z))
        eps = 1e-3
        # a point just inside / outside each plane, in view space: w+x (left), w-x (right), w+y (bottom), w-y (top), near, far
        cases = [((-tx * z, 0, z), 0), ((tx * z, 0, z), 1), ((0, -ty * z, z), 2), ((0, ty * z, z), 3)]
        for (x, y, zz), k in cases:
            assert inside(eye + (x * (1 - eps), y * (1 - eps), zz)), (homogeneous, k)
            assert which(eye + (x * (1 + eps), y * (1 + eps), zz)) == {k}, (homogeneous, k)
        assert inside(eye + (0, 0, near * (1 + eps))) and which(eye + (0, 0, near * (1 - eps))) == {4}
        assert inside(eye + (0, 0, far * (1 - eps))) and which(eye + (0, 0, far * (1 + eps))) == {5}
        # the planes point inwards and classify a box through the rule as well
        ident = IDENTITY.copy()
        ident[0, 12:15] = eye + (0, 0, z)
        assert _one(ident, (0, 0, 0), (1, 1, 1), pl.astype(F))
        ident[0, 12:15] = eye + (0, 0, -5.0)
        assert not _one(ident, (0, 0, 0), (1, 1, 1), pl.astype(F))


# ---------------------------------------------------------------- the conditions the GPU test relies on

def test_seeded_scene_is_a_meaningful_case():
    sc = make_scene()
    world = npo.mtx_srt(sc["scale"], sc["euler"], sc["pos"])
    n = len(world)
    vis64, amb = visible_ref64(world, sc["center"], sc["half"], wide_view())
    share = vis64.mean()
    print(f"wide view: {int(vis64.sum())} of {n} visible, {int(amb.sum())} ambiguous")
    assert 0.10 <= share <= 0.90
    assert amb.sum() < 0.02 * n
    vis32 = visible_ref32(world, sc["center"], sc["half"], wide_view())
    assert np.array_equal(vis32[~amb], vis64[~amb])  # the two references agree wherever the geometry decides
    nv64, namb = visible_ref64(world, sc["center"], sc["half"], narrow_view())
    print(f"narrow view: {int(nv64.sum())} of {n} visible, {int(namb.sum())} ambiguous")
    assert 0 < nv64.mean() < 0.20 and namb.sum() < 0.02 * n
    nv32 = visible_ref32(world, sc["center"], sc["half"], narrow_view())
    assert np.array_equal(nv32[~namb], nv64[~namb])


# ---------------------------------------------------------------- the library, the C and the C++ views

def test_exported_symbols_are_present():
    lib = B.lib()
    for name in ("bge_world_upload_bounds", "bge_world_upload_bounds_indexed", "bge_world_visible", "bge_world_visible_device",
                 "bge_frustum_planes"):
        assert getattr(lib, name) is not None
    for name in ("upload_bounds", "visible", "visible_device", "visible_count"):
        assert callable(getattr(B.World, name))
    assert callable(W.frustum_planes)


def test_c99_view_of_the_header(tmp_path):
    exe = str(tmp_path / "abi_check_visible")
    lib = os.path.join(ROOT, "banggameengine_amd")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "abi_check_visible.c"), f"-L{lib}", "-lbge_world", f"-Wl,-rpath,{lib}",
                           "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "visible abi ok" in r.stdout


def test_adapter_members_compile_against_reference_shapes(tmp_path):
    subprocess.check_call(["g++", "-std=c++20", "-O0", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-c",
                           os.path.join(ROOT, "tests", "cpp", "visible_reference_shapes.cpp"), "-o", str(tmp_path / "visible_reference_shapes.o")])
