"""Sphere penetration and recovery (include/bge_world.h "Sphere penetration and recovery", bge_world_sphere_penetration*,
bge_world_sphere_recover*) without a GPU: the references of refmodel/recover.py (signed_ref, the signed-distance rule in float64 on a World64;
recover_ref, the Recover rule in numpy float32 scalars over a penetration function handed in) on the hand-worked cases of
refmodel/recover_cases.py, through an analytic penetration function of half-spaces and through the float64 shapes; the batch and the
caps the GPU comparison relies on; the exported symbols, the C99 view of the records and the adapter's SpherePenetration /
RecoverSphere / RecoverSpheres on the reference's types.

recover_ref(pen_fn, records) is the reference of the GPU tests: there pen_fn is World.sphere_penetration on the same world, and the
device's result must equal it byte for byte."""
from __future__ import annotations

import collections

import numpy as np
import pytest

from banggameengine_amd.world import (PENETRATION_HIT_DTYPE, RECOVER_INVALID, RECOVER_MOVED, RECOVER_ROUNDS, RECOVER_STUCK, SPHERE_RECOVER_DTYPE,
                                      SPHERE_RECOVER_RESULT_DTYPE, make_sphere_recovers, make_spheres)

from abi import assert_exported, build_and_run_c99, compile_reference_shapes
from refmodel.rays import ALL, CODE_PLANE, RAY_BODY, RAY_GROUND, RAY_TRIGGER, Obj, World64
from refmodel.spheres import SphereRef
from refmodel.moves import F
from refmodel.recover import HalfSpacesPen, classify, pen_of, record_valid, recover_ref, signed_ref
from refmodel.sphere_cases import scene_world64
from refmodel.move_cases import BATCHES, SCENE_N, SCENE_SEED, ghost_positions
from refmodel.recover_cases import (DOWN, EAST, HAND_RECOVERS, PLANE, S2, SKIN, SPHERE_SEED, UP, check_caps, check_hand_recover, check_invalid,
                                    hand_objects, hand_record, invalid_records, sphere_batch)

# ------------------------------------------------------------------------------------------------ hand-worked cases


@pytest.mark.parametrize("case", HAND_RECOVERS, ids=[c[0] for c in HAND_RECOVERS])
def test_hand_worked_recoveries(case):
    name, walls, bodies, plane, _, want = case
    fns = [pen_of(World64(hand_objects(bodies), plane))]
    if walls is not None:
        fns.append(HalfSpacesPen(walls))
    for pen_fn in fns:
        check_hand_recover(name, recover_ref(pen_fn, hand_record(case))[0], want)


def test_after_one_push_the_gap_to_a_flat_surface_is_skin():
    for skin in (0.002, 0.01, 0.05):
        got = recover_ref(HalfSpacesPen([PLANE]), make_sphere_recovers([(1, 0.1, 2)], 0.4, skin, ALL))[0]
        assert got["n_pushes"] == 1 and abs(float(got["position"][1]) - 0.4 - skin) < 1e-6


def test_signed_distance_hand_worked():
    box = Obj(RAY_BODY, 4, 1, ALL, False, (1, 2, 3), (0, 0, 0), (0.0, 0.0, 0.0, 1.0))
    cap = Obj(RAY_TRIGGER, 2, 1, ALL, True, (0.5, 1.0, 0.5), (10, 0, 0), (0.0, 0.0, 0.0, 1.0))
    w = World64([box, cap], True)
    # outside a face, an edge: the overlap's distance, the direction from the closest point
    h = signed_ref(w, (1.5, 0, 0), 0.6, 1)[0]
    assert h.sd == pytest.approx(0.5) and h.depth == pytest.approx(0.1) and np.allclose(h.normal, EAST) and np.allclose(h.point, (1, 0, 0))
    h = signed_ref(w, (1.5, 2.5, 0), 0.8, 1)[0]
    assert h.sd == pytest.approx(S2 / 2) and np.allclose(h.normal, (1 / S2, 1 / S2, 0)) and np.allclose(h.point, (1, 2, 0))
    assert h.sd == pytest.approx(SphereRef(w).overlap((1.5, 2.5, 0), 0.8, 1)[0][0][3], abs=1e-15)
    assert signed_ref(w, (1.5, 0, 0), 0.4, 1) == []
    # inside: minus the distance to the nearest face, on the surface -0 counts as inside; q.y == -0 counts as +
    h = signed_ref(w, (0.5, -1.9, 0.5), 0.0, 1)[0]
    assert h.sd == pytest.approx(-0.1) and np.allclose(h.normal, DOWN) and np.allclose(h.point, (0.5, -2, 0.5)) and h.gap == pytest.approx(0.4)
    assert signed_ref(w, (1.0, 0, 0), 0.0, 1)[0].sd == 0 and np.allclose(signed_ref(w, (1.0, 0, 0), 0.0, 1)[0].normal, EAST)
    thin = World64([Obj(RAY_BODY, 0, 1, ALL, False, (3, 1, 3), (0, 0, 0), (0.0, 0.0, 0.0, 1.0))], False)
    assert np.allclose(signed_ref(thin, (0.5, -0.0, 0.5), 0.0, 1)[0].normal, UP)
    # the capsule: beside it, above its cap, inside, and on its axis
    h = signed_ref(w, (11, 0.5, 0), 0.6, 1)[0]
    assert h.kind == RAY_TRIGGER and h.sd == pytest.approx(0.5) and np.allclose(h.normal, EAST) and np.allclose(h.point, (10.5, 0.5, 0))
    h = signed_ref(w, (10, 2.0, 0), 0.6, 1)[0]
    assert h.sd == pytest.approx(0.5) and np.allclose(h.normal, UP)
    h = signed_ref(w, (10, 0.2, 0.3), 0.0, 1)[0]
    assert h.sd == pytest.approx(-0.2) and np.allclose(h.normal, (0, 0, 1)) and np.allclose(h.point, (10, 0.2, 0.5))
    h = signed_ref(w, (10, 0.7, 0), 0.0, 1)[0]
    assert h.sd == -0.5 and np.allclose(h.normal, EAST)
    # the plane: two-sided, -0 goes up, only through layer 2; largest depth first, then the object code
    assert np.allclose(signed_ref(w, (50, -0.0, 0), 0.1, 2)[0].normal, UP) and np.allclose(signed_ref(w, (50, -0.05, 0), 0.1, 2)[0].normal, DOWN)
    assert signed_ref(w, (50, 0.05, 0), 0.1, 1) == []
    got = signed_ref(w, (0.9, 0.5, 0), 1.0, 3)
    assert [h.code for h in got] == [4, CODE_PLANE] and got[0].depth == pytest.approx(1.1) and got[1].depth == pytest.approx(0.5)
    # the no-hit inputs of the overlap
    for c, r, m in [((0, 0, float("nan")), 1.0, 1), ((0, 0, 0), -1.0, 1), ((0, 0, 0), float("nan"), 1), ((0, 0, 0), float("inf"), 1), ((0, 0, 0), 1.0, 0)]:
        assert signed_ref(w, c, r, m) == []


def test_signed_reference_agrees_with_the_overlap_reference():
    """Penetrating iff overlapping, and the overlap's distance is max(sd, 0): on a random scene through both references."""
    w64, pos = scene_world64(300, np.random.default_rng(3), n_triggers=6, spread=8.0)
    ref = SphereRef(w64)
    recs = sphere_batch(np.random.default_rng(4), 200, pos, ghost_positions(w64), spread=8.0)
    n = 0
    for m in recs:
        want, _ = ref.overlap(m["position"], m["radius"], m["layer_mask"])
        got = sorted(signed_ref(w64, m["position"], m["radius"], m["layer_mask"]), key=lambda h: h.code)
        assert [h.code for h in got] == [h[0] for h in want]
        assert all(abs(max(g.sd, 0.0) - h[3]) < 1e-12 for g, h in zip(got, want))
        assert all(abs(np.linalg.norm(g.normal) - 1) < 1e-12 for g in got)
        n += len(got)
    assert n > 200


def test_invalid_records_echo_the_position():
    recs = invalid_records()
    check_invalid(recs, recover_ref(HalfSpacesPen([PLANE]), recs))
    # radius 0 is valid: a point on the plane touches it (sd = 0 <= 0, depth 0) and is lifted by the skin
    got = recover_ref(HalfSpacesPen([PLANE]), make_sphere_recovers([(0, 0.0, 0)], 0.0, SKIN, ALL))[0]
    assert got["flags"] == RECOVER_MOVED and got["n_pushes"] == 1 and got["position"].tolist() == [0, F(SKIN), 0]


# ------------------------------------------------------------------------------------------------ the batch of the GPU comparison


def test_reference_alone_stays_inside_the_caps_of_the_gpu_comparison():
    """The GPU test compares the device's penetration hits with signed_ref on the ticked scene; it sets a sphere aside where
    classify() says the reference's own answer is ambiguous, and requires that at least half of the valid spheres start in
    penetration, that all three kinds win at least once, that at most half of the penetrating spheres are set aside and that 20
    axis normals inside boxes are compared.  The same
    scene (before its first tick) and the same spheres on the reference alone must stay inside those caps, so a GPU failure cannot
    hide behind them.  And the recoveries the byte-for-byte comparison sees must not all be of one sort."""
    w64, pos = scene_world64(SCENE_N, np.random.default_rng(SCENE_SEED))
    recs = sphere_batch(np.random.default_rng(SPHERE_SEED), max(BATCHES), pos, ghost_positions(w64))
    n_valid = n_pen = n_skipped = n_axis = 0
    kinds = collections.Counter()
    for m in recs:
        if not record_valid(m):
            continue
        n_valid += 1
        cands, winner_clear, normal_clear = classify(w64, m)
        if cands and cands[0].depth >= 0:
            n_pen += 1
            n_skipped += not normal_clear
            if winner_clear:
                kinds[cands[0].kind] += 1
            n_axis += normal_clear and cands[0].kind != RAY_GROUND and np.isfinite(cands[0].gap)
    check_caps(n_valid, n_pen, n_skipped, kinds, n_axis)
    assert n_valid == len(recs) - len(range(36, len(recs), 37))
    got = recover_ref(pen_of(w64), recs)
    ok = (got["flags"] & RECOVER_INVALID) == 0
    cov = dict(clear=int((ok & (got["flags"] == 0)).sum()), one=int((got["n_pushes"] == 1).sum()), more=int((got["n_pushes"] >= 2).sum()),
               stuck=int(((got["flags"] & RECOVER_STUCK) != 0).sum()))
    print("recoveries:", cov)
    assert cov["clear"] >= 20 and cov["one"] >= 20 and cov["more"] >= 20 and cov["stuck"] >= 1, cov


# ------------------------------------------------------------------------------------------------ the ABI


def test_recover_symbols_exported():
    import banggameengine_amd as B
    assert_exported(("bge_world_sphere_penetration", "bge_world_sphere_penetration_device", "bge_world_sphere_recover",
                     "bge_world_sphere_recover_device"))
    from banggameengine_amd.world import World
    assert PENETRATION_HIT_DTYPE.itemsize == 40 and SPHERE_RECOVER_DTYPE.itemsize == 28 and SPHERE_RECOVER_RESULT_DTYPE.itemsize == 64
    assert PENETRATION_HIT_DTYPE.fields["normal"][1] == 24 and SPHERE_RECOVER_DTYPE.fields["layer_mask"][1] == 20
    assert SPHERE_RECOVER_RESULT_DTYPE.fields["hit_normal"][1] == 40 and SPHERE_RECOVER_RESULT_DTYPE.fields["remaining_depth"][1] == 56
    assert (RECOVER_ROUNDS, RECOVER_INVALID, RECOVER_MOVED, RECOVER_STUCK) == (4, 1, 2, 4)
    m = make_sphere_recovers([[0, 1, 0], [1, 2, 3]], [0.5, 0.25], 0.02, 3)
    assert m["radius"].tolist() == [0.5, 0.25] and m["skin"].tolist() == [F(0.02)] * 2 and m["layer_mask"].tolist() == [3, 3] and not m["reserved"].any()
    assert make_spheres([[0, 1, 0]], 2.0)["layer_mask"].tolist() == [ALL]
    for name in ("sphere_penetration", "sphere_penetration_device", "sphere_recover", "sphere_recover_device"):
        assert callable(getattr(World, name))
    for name in ("PENETRATION_HIT_DTYPE", "SPHERE_RECOVER_DTYPE", "SPHERE_RECOVER_RESULT_DTYPE", "RECOVER_ROUNDS", "RECOVER_INVALID", "RECOVER_MOVED",
                 "RECOVER_STUCK", "make_sphere_recovers"):
        assert hasattr(B, name), name


def test_recover_entry_points_reject_null_world_and_zero_count():
    from banggameengine_amd import _capi
    lib = _capi.lib()
    for fn in (lib.bge_world_sphere_penetration, lib.bge_world_sphere_penetration_device, lib.bge_world_sphere_recover,
               lib.bge_world_sphere_recover_device):
        assert fn(None, 1, None, None) == -1
        assert fn(None, 0, None, None) == -1
    assert lib.bge_last_error()


def test_abi_c99_recover_records(tmp_path):
    build_and_run_c99(tmp_path, "abi_check_recover.c", "recover abi ok")


def test_adapter_recovery_compiles_on_reference_shapes(tmp_path):
    compile_reference_shapes(tmp_path, "recover_reference_shapes.cpp")
