"""Sphere step moves (include/bge_world.h "Sphere step moves", bge_world_sphere_step_move*) without a GPU: step_ref of
refmodel/step_moves.py, the rule of the header in numpy float32 scalars over a caster handed in, on the hand-worked cases of
refmodel/step_cases.py, through the float64 shape reference of refmodel/spheres.py and, where half-spaces can express the scene,
through the analytic caster; the two byte equalities the header promises and the coverage the GPU comparison relies on, on the
seeded step field; the exported symbols, the C99 view of the records and the adapter's StepMoveSphere / StepMoveSpheres on the
reference's types.

step_ref(cast_fn, moves) is the reference of the GPU tests: there cast_fn is World.sphere_cast on the same world, and the device's
result must equal it byte for byte."""
from __future__ import annotations

import numpy as np
import pytest

from banggameengine_amd.world import (MOVE_GROUNDED, MOVE_INVALID, MOVE_PROBE_HIT, MOVE_STEP_TRIED, MOVE_STEPPED, SPHERE_MOVE_DTYPE,
                                      SPHERE_MOVE_RESULT_DTYPE, SPHERE_STEP_MOVE_DTYPE, SPHERE_STEP_RESULT_DTYPE, make_sphere_step_moves)

from abi import assert_exported, build_and_run_c99, compile_reference_shapes
from refmodel.rays import ALL
from refmodel.spheres import SphereRef, sweep_all
from refmodel.moves import F, HalfSpaces, caster_of, move_ref
from refmodel.move_cases import PLANE, R, SKIN, hand_objects
from refmodel import step_moves
from refmodel.step_moves import compose_ref, plain_of, step_ref
from refmodel.step_cases import (BATCHES, FIELD_SEED, HAND_STEPS, STEPPER_SEED, StepField, check_hand_step, check_invalid_steps, check_step_coverage,
                                 hand_stepper, invalid_steppers, step_coverage, stepper_batch)

# ------------------------------------------------------------------------------------------------ hand-worked cases


@pytest.mark.parametrize("case", HAND_STEPS, ids=[c[0] for c in HAND_STEPS])
def test_hand_worked_steps(case):
    name, walls, bodies, ghosts, plane, _, want = case
    objs = hand_objects(bodies, ghosts)
    shapes = caster_of(lambda o, d, md, r, mask: sweep_all(objs, o, d, md, r, mask, plane))
    moves = hand_stepper(case)
    for cast_fn in ([HalfSpaces(walls)] if walls is not None else []) + [shapes]:
        got = step_ref(cast_fn, moves)[0]
        check_hand_step(name, got, want)
        if not got["flags"] & MOVE_STEPPED:  # "plain bytes": the plain move of the same record, and STEP_TRIED
            plain = move_ref(cast_fn, plain_of(moves))[0]
            masked = got.copy()
            masked["flags"] &= ~np.uint32(MOVE_STEP_TRIED)
            assert masked.tobytes() == plain.tobytes(), name
        assert compose_ref(cast_fn, moves, np.array([got]))[0].tobytes() == got.tobytes(), name


def test_invalid_steppers_echo_the_position():
    moves = invalid_steppers()
    assert len(moves) == 16
    check_invalid_steps(moves, step_ref(HalfSpaces([PLANE]), moves))
    # and a zero displacement is valid: it stays, tries nothing, and still probes
    got = step_ref(HalfSpaces([PLANE]), make_sphere_step_moves([(0, 0.55, 0)], [(0, 0, 0)], R, SKIN, 0.1, 0.7, ALL, 0.5))[0]
    assert got["flags"] == MOVE_GROUNDED | MOVE_PROBE_HIT and got["n_hits"] == 0 and got["position"].tolist() == [0, F(0.55), 0] and got["step_rise"] == 0


def test_a_vertical_displacement_tries_nothing():
    # straight down onto a slope too steep to stand on: it is hit, it is no ground, but there is no level way to go: the gate is shut
    steep = ((0.8, 0.6, 0.0), (0, 0, 0), 1, 0)
    moves = make_sphere_step_moves([(0, 1.5, 0)], [(0, -1, 0)], R, SKIN, 0.5, 0.7071, ALL, 0.5)
    got = step_ref(HalfSpaces([steep]), moves)[0]
    assert got["n_hits"] >= 1 and not got["flags"] & (MOVE_STEP_TRIED | MOVE_STEPPED)
    assert got.tobytes() == move_ref(HalfSpaces([steep]), plain_of(moves))[0].tobytes()


# ------------------------------------------------------------------------------------------------ the batch of the GPU comparison


@pytest.fixture(scope="module")
def seeded():
    field = StepField(np.random.default_rng(FIELD_SEED))
    moves = stepper_batch(np.random.default_rng(STEPPER_SEED), max(BATCHES), field)
    cast_fn = caster_of(SphereRef(field.world64()).sweep_all)
    trace = {}
    return field, moves, cast_fn, step_ref(cast_fn, moves, trace), trace


def test_the_step_field_is_what_the_issue_asks(seeded):
    field, moves, _, _, _ = seeded
    assert 450 <= field.n <= 550 and np.abs(field.pos[:, [0, 2]]).max() <= 32 and 4 <= len(field.ghosts) <= 12
    boxes = ~field.capsule
    assert (boxes & (field.euler[:, 0] == 0) & (field.euler[:, 2] == 0)).sum() > field.n / 2  # most are boxes turned about y alone
    made = np.ones(len(moves), bool)
    made[36::37] = False  # (the invalid ones had a field overwritten)
    assert np.array_equal(moves["position"][made, 1], (moves["radius"] + moves["skin"])[made])
    assert set(np.unique(moves["step_height"][np.isfinite(moves["step_height"])]).tolist()) <= {F(0), F(0.3), F(0.5), F(0.8), F(-0.5)}
    assert (moves["displacement"] == 0).all(axis=1).sum() == len(range(40, len(moves), 41))


def test_reference_alone_clears_the_floors_of_the_gpu_comparison(seeded):
    """The GPU test compares World.sphere_step_move with step_ref over World.sphere_cast on the ticked field and asserts these
    floors on what it saw.  The same field and the same movers through the float64 shape reference must clear them too, so the
    comparison cannot pass by missing everything."""
    _, moves, _, got, trace = seeded
    check_step_coverage(step_coverage(got, trace))
    assert ((got["flags"] & MOVE_INVALID) != 0).sum() == len(range(36, len(moves), 37))


def test_not_stepped_is_the_plain_move_byte_for_byte(seeded):
    _, moves, cast_fn, got, _ = seeded
    plain = move_ref(cast_fn, plain_of(moves))
    rest = np.nonzero((got["flags"] & MOVE_STEPPED) == 0)[0]
    assert len(rest) > 300
    for i in rest:
        if not step_moves.step_mover_valid(moves[i]) and not plain["flags"][i] & MOVE_INVALID:
            continue  # a step_height that is no height: invalid here, and the plain move does not look at that word
        masked = got[i].copy()
        masked["flags"] &= ~np.uint32(MOVE_STEP_TRIED)
        assert masked.tobytes() == plain[i].tobytes(), (i, got[i], plain[i])


def test_stepped_is_the_composition_of_public_calls_byte_for_byte(seeded):
    _, moves, cast_fn, got, _ = seeded
    want = compose_ref(cast_fn, moves, got)
    bad = [i for i in range(len(moves)) if want[i].tobytes() != got[i].tobytes()]
    assert not bad, (bad[0], got[bad[0]], want[bad[0]])
    assert ((got["flags"] & MOVE_STEPPED) != 0).sum() >= 30


# ------------------------------------------------------------------------------------------------ the ABI


def test_sphere_step_move_symbols_exported():
    assert_exported(("bge_world_sphere_step_move", "bge_world_sphere_step_move_device"))
    from banggameengine_amd.world import World
    assert SPHERE_STEP_MOVE_DTYPE.itemsize == 48 and SPHERE_STEP_RESULT_DTYPE.itemsize == 80 and (MOVE_STEP_TRIED, MOVE_STEPPED) == (16, 32)
    assert SPHERE_STEP_MOVE_DTYPE.fields["step_height"][1] == 44 and SPHERE_STEP_RESULT_DTYPE.fields["step_rise"][1] == 76
    for step, plain in ((SPHERE_STEP_MOVE_DTYPE, SPHERE_MOVE_DTYPE), (SPHERE_STEP_RESULT_DTYPE, SPHERE_MOVE_RESULT_DTYPE)):
        for name in plain.names[:-1]:  # every field but the reserved word is the plain record's, at its offset
            assert step.fields[name] == plain.fields[name], name
    assert step_moves.STEP_MOVE_DTYPE == SPHERE_STEP_MOVE_DTYPE and step_moves.STEP_RESULT_DTYPE == SPHERE_STEP_RESULT_DTYPE
    assert (step_moves.STEP_TRIED, step_moves.STEPPED) == (MOVE_STEP_TRIED, MOVE_STEPPED) and step_moves.PLAIN_MOVE_DTYPE == SPHERE_MOVE_DTYPE
    m = make_sphere_step_moves([[0, 1, 0], [1, 2, 3]], [[0, -1, 0], [1, 0, 0]], [0.5, 0.25], 0.02, 0.3, 0.5, 3, [0.3, 0.0])
    assert m["radius"].tolist() == [0.5, 0.25] and m["skin"].tolist() == [F(0.02)] * 2 and m["layer_mask"].tolist() == [3, 3]
    assert m["probe_distance"].tolist() == [F(0.3)] * 2 and m["step_height"].tolist() == [F(0.3), 0]
    for name in ("sphere_step_move", "sphere_step_move_device"):
        assert callable(getattr(World, name))


def test_sphere_step_moves_reject_null_world_and_zero_count():
    from banggameengine_amd import _capi
    lib = _capi.lib()
    for fn in (lib.bge_world_sphere_step_move, lib.bge_world_sphere_step_move_device):
        assert fn(None, 1, None, None) == -1
        assert fn(None, 0, None, None) == -1
    assert lib.bge_last_error()


def test_abi_c99_step_records(tmp_path):
    build_and_run_c99(tmp_path, "abi_check_step.c", "step abi ok")


def test_adapter_sphere_step_moves_compile_on_reference_shapes(tmp_path):
    compile_reference_shapes(tmp_path, "step_reference_shapes.cpp")
