"""Seeded casts, spheres and scenes, the hand-worked cases of the sphere queries and their checker: shared by
test_sphere_queries_cpu.py and the GPU suites."""
from __future__ import annotations

import math

import numpy as np

from .rays import ALL, NO_ENTITY, RAY_BODY, RAY_TRIGGER, Obj, World64, box_half_extents, capsule_dims, quat_from_euler
from .ray_cases import IDQ

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
    """The World64 of device.Scene(n, rng, n_triggers) before its first tick: the same draws in the same order."""
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


S2, S3 = math.sqrt(2.0), math.sqrt(3.0)

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
