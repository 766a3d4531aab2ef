"""Sphere casts and sphere overlaps (include/bge_world.h bge_world_sphere_cast*, bge_world_overlap_sphere) without a GPU: the float64
reference the GPU tests compare against (refmodel/spheres.py), checked on hand-worked cases; the exported symbols; the C99 view of the records; the
adapter's SphereCast / SphereCastAll / OverlapSphere on the reference's types (C++20, -Werror).

The reference does not follow the kernel's method (entry region of the grown box, then at most three edge capsules): it takes the
rounded box as the UNION of three boxes (the sharp box grown by r along one axis each) and the twelve edge capsules of radius r,
and the first touch as the minimum over those fifteen parts, each part tested by the ray reference of refmodel/rays.py."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import pytest

from abi import assert_exported, build_and_run_c99, compile_reference_shapes
from refmodel.rays import ALL, CODE_GHOST, CODE_PLANE, RAY_BODY, RAY_TRIGGER, Obj, World64, cast_all, clear_decision
from refmodel.spheres import SphereRef, obj_dist, overlap_all, sweep_all
from refmodel.ray_cases import IDQ, random_objects
from refmodel.sphere_cases import HAND_CASES, S2, check_hand_case, hand_objects, random_casts, random_spheres, reference_coverage, scene_world64

# ------------------------------------------------------------------------------------------------ hand-worked cases


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
    assert_exported(("bge_world_sphere_cast", "bge_world_sphere_cast_all", "bge_world_sphere_cast_device", "bge_world_overlap_sphere"))
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
    build_and_run_c99(tmp_path, "abi_check_sphere.c", "sphere abi ok")


def test_adapter_sphere_queries_compile_on_reference_shapes(tmp_path):
    compile_reference_shapes(tmp_path, "sphere_reference_shapes.cpp")
