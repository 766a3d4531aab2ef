"""Character platform riding (include/bge_world.h "Character platform riding", bge_world_characters_ride ..) without a GPU:
ride_run_ref of refmodel/rides.py — Carry, the steps of char_ref, Anchor, in numpy float32 scalars — over the float64 shape
reference, on the hand-worked platforms of the header and on the seeded platform field of the GPU comparison with its coverage
floors; the exported symbols, the C99 view of the record and the adapter's riding members on the reference's types.

ride_run_ref is the reference of the GPU tests: there the caster is World.sphere_cast, the penetration function
World.sphere_penetration and the poses are the device's, and the states and the 64-byte ride records must equal it byte for byte."""
from __future__ import annotations

import math

import numpy as np

from banggameengine_amd import world as W
from banggameengine_amd.world import CHAR_GROUNDED, CHAR_JUMPED, CHAR_LANDED, CHAR_RECOVERED, CHARACTER_RIDE_DTYPE

from abi import assert_exported, build_and_run_c99, compile_reference_shapes
from refmodel import rides
from refmodel.rays import NO_ENTITY, RAY_BODY, RAY_GROUND, quat_to_mat
from refmodel.rides import BODY_DYNAMIC, BODY_NONE, BODY_STATIC, CARRIED, LOST, carry_ref, fresh_rides
from refmodel.character_cases import REST_Y, hand_character, inputs_of
from refmodel.layout_cases import acyclic, layout_numbers
from refmodel.ride_cases import (N_CALLS, N_CHARS, N_PLATFORMS, SHUFFLE_PAD, STEPS_PER_CALL, YAW, Platforms, RideRun, check_ride_coverage, field_case,
                                 ride_coverage, shuffled_topology)

TOP = 1.0  # the hand platform: half extents (2, 0.5, 2), its top at y = 1
STAND_Y = TOP + REST_Y  # radius 0.5 + skin 0.01 above it


def table(body_type=BODY_STATIC):
    return Platforms([body_type], [(2.0, 0.5, 2.0)], [(0.0, 0.5, 0.0)], [(0.0, 0.0, 0.0)])


def standing(riding, x=0.0, body_type=BODY_STATIC, dynamic=False):
    """The hand character settled on the table by one call: GROUNDED on body 0, and with riding on anchored to it."""
    p = table(body_type)
    run = RideRun(p, hand_character((x, STAND_Y + 0.01, 0.0)), riding, dynamic)
    s = run.update(2)[0]
    assert s["flags"] == CHAR_GROUNDED and s["ground_kind"] == RAY_BODY and s["ground_entity"] == 0 and abs(s["position"][1] - STAND_Y) <= 1e-6
    assert run.history[0]["flags"][0] == CHAR_GROUNDED | CHAR_LANDED
    run.history.clear()
    return p, run


# ------------------------------------------------------------------------------------------------ the four hand cases


def test_a_platform_that_moves_along_carries_the_character():
    # +0.25 in x before every call.  Riding off: the character stays at x = 0; the trailing edge (x = 0.25 k - 2) passes under it,
    # and in the 10th call, 0.5 behind it, the probe finds no walkable ground: it drops off.
    p, run = standing(False)
    lost = None
    for k in range(1, 11):
        p.move(dpos=(0.25, 0, 0))
        s = run.update(2)[0]
        assert s["position"][0] == 0 and s["position"][2] == 0
        if lost is None and not s["flags"] & CHAR_GROUNDED:
            lost = k
    assert lost == 10 and s["position"][1] < STAND_Y - 0.05
    # Riding on: x = 0.25 k after call k, GROUNDED throughout
    p, run = standing(True)
    for k in range(1, 13):
        p.move(dpos=(0.25, 0, 0))
        s = run.update(2)[0]
        assert abs(s["position"][0] - 0.25 * k) <= 1e-6 and abs(s["position"][1] - STAND_Y) <= 1e-6 and s["position"][2] == 0, (k, s)
        r = run.rides[0]
        assert r["flags"] == CARRIED and np.allclose(r["carried"], (0.25, 0, 0), atol=1e-6, rtol=0) and r["turn"].tolist() == [0, 0, 0, 1]
        assert r["entity"] == 0 and np.allclose(r["anchor_position"], (0.25 * k, 0.5, 0), atol=1e-6, rtol=0)
    assert all(h["flags"][0] == CHAR_GROUNDED for h in run.history) and len(run.history) == 24


def test_a_platform_that_descends_takes_the_character_down():
    # -0.25 in y before every call: more than probe_distance 0.1.  Riding off: the first step after the platform sank walks level,
    # its probe finds nothing within 0.1 and GROUNDED is lost: no call from the 2nd on is GROUNDED (with the platform moved before
    # the 1st call, as in the translation case, the 1st is not either) and the character free-falls after the platform.
    p, run = standing(False)
    grounded = []
    for k in range(1, 4):
        p.move(dpos=(0, -0.25, 0))
        s = run.update(2)[0]
        grounded.append(bool(s["flags"] & CHAR_GROUNDED))
    assert not any(grounded[1:]) and s["vertical_velocity"] < -0.8 and s["position"][1] > p.pos[0][1] + 0.5 + 0.51 + 0.2
    # Riding on: GROUNDED in every call, y = top + 0.51
    p, run = standing(True)
    for k in range(1, 5):
        p.move(dpos=(0, -0.25, 0))
        s = run.update(2)[0]
        assert s["flags"] == CHAR_GROUNDED and abs(s["position"][1] - (TOP - 0.25 * k + 0.51)) <= 1e-6 and s["vertical_velocity"] == 0, (k, s)
    assert all(h["flags"][0] == CHAR_GROUNDED for h in run.history)


def test_a_platform_that_rises_is_a_lift_not_a_collision():
    # +0.25 in y, one step per call.  Riding off: Recover pushes the character out: RECOVERED with recovered = (0, 0.25, 0) every call.
    p, run = standing(False)
    for k in range(1, 4):
        p.move(dpos=(0, 0.25, 0))
        s = run.update(1)[0]
        assert s["flags"] & CHAR_RECOVERED and abs(s["recovered"][1] - 0.25) <= 1e-6 and s["recovered"][0] == 0 and s["recovered"][2] == 0, (k, s)
    # Riding on: GROUNDED alone, recovered 0
    p, run = standing(True)
    for k in range(1, 4):
        p.move(dpos=(0, 0.25, 0))
        s = run.update(1)[0]
        assert s["flags"] == CHAR_GROUNDED and not s["recovered"].any() and abs(s["position"][1] - (STAND_Y + 0.25 * k)) <= 1e-6, (k, s)


def test_a_platform_that_turns_takes_the_character_round():
    # pi / 8 about the vertical through its centre, the character at (1, ., 0).  Riding off: it does not move.
    p, run = standing(False, x=1.0)
    for k in range(1, 4):
        p.move(deuler=np.eye(3)[YAW] * (math.pi / 8))
        s = run.update(2)[0]
        assert s["flags"] == CHAR_GROUNDED and s["position"][0] == 1 and s["position"][2] == 0
    # Riding on: (1, 0) -> (0.92388, -0.38268) -> (0.70711, -0.70711) -> .. at radius 1 +- 3e-7
    p, run = standing(True, x=1.0)
    for k in range(1, 5):  # (each carry rounds anew: the radius wanders by a few ulps of 1 per call)
        p.move(deuler=np.eye(3)[YAW] * (math.pi / 8))
        s = run.update(2)[0]
        x, z = float(s["position"][0]), float(s["position"][2])
        assert s["flags"] == CHAR_GROUNDED and abs(math.hypot(x, z) - 1.0) <= 3e-7 and abs(s["position"][1] - STAND_Y) <= 1e-6, (k, s)
        assert abs(x - math.cos(k * math.pi / 8)) <= 1e-6 and abs(z + math.sin(k * math.pi / 8)) <= 1e-6, (k, x, z)
        assert np.allclose(run.rides["turn"][0], (0, math.sin(math.pi / 16), 0, math.cos(math.pi / 16)), atol=1e-6, rtol=0)
    first = run.history[1]["position"][0]
    assert np.allclose(first, (0.92388, STAND_Y, -0.38268), atol=1e-5, rtol=0)


# ------------------------------------------------------------------------------------------------ the rule's other clauses


def test_translation_turn_and_walk_together():
    """The platform moves by (0.25, 0.125, 0) and turns by pi / 8 per call while the character walks 0.1 in +x per step: it stays
    GROUNDED on the platform, and its position in the platform's frame changes only by the walk."""
    p, run = standing(True)
    local = np.array([0.0, STAND_Y - 0.5, 0.0])
    for k in range(1, 6):
        p.move(dpos=(0.25, 0.125, 0), deuler=np.eye(3)[YAW] * (math.pi / 8))
        s = run.update(2, inputs_of(walk_x=0.1))[0]
        assert s["flags"] == CHAR_GROUNDED and s["ground_entity"] == 0 and run.rides["flags"][0] == CARRIED, (k, s)
        basis = quat_to_mat(p.quat()[0].astype(np.float64))
        local = local + basis.T @ np.array([0.2, 0.0, 0.0])  # two steps of the walk, seen from the platform as it stands now
        got = basis.T @ (s["position"].astype(np.float64) - p.pos[0].astype(np.float64))
        assert np.abs(got - local).max() <= 1e-5, (k, got, local)


def test_a_world_that_does_not_move_is_untouched_by_riding():
    field, _, descs, inputs = field_case()
    some = np.r_[0:48, 192:200]
    on, off = RideRun(field, descs[some], True), RideRun(field, descs[some], False)
    for k in range(3):
        a, b = on.update(STEPS_PER_CALL, inputs[k][some]), off.update(STEPS_PER_CALL, inputs[k][some])
        assert a.tobytes() == b.tobytes()
        assert not (on.rides["flags"] & (CARRIED | LOST)).any() and not on.rides["carried"].any() and (on.rides["turn"] == (0, 0, 0, 1)).all()
    assert (on.rides["entity"][:48] != NO_ENTITY).sum() >= 24 and (on.rides["entity"][48:] == NO_ENTITY).all()


def test_a_character_that_jumped_is_left_behind():
    p, run = standing(True)
    p.move(dpos=(0.25, 0, 0))
    s = run.update(2, inputs_of(jump=True))[0]  # carried, then it jumps
    assert run.rides["flags"][0] == CARRIED and run.history[0]["flags"][0] == CHAR_JUMPED and not s["flags"] & CHAR_GROUNDED
    assert abs(s["position"][0] - 0.25) <= 1e-6 and run.rides["entity"][0] == NO_ENTITY and not run.rides["anchor_position"][0].any()
    for k in range(4):  # airborne: the platform leaves without it
        p.move(dpos=(0.25, 0, 0))
        s = run.update(2)[0]
        assert not s["flags"] & CHAR_GROUNDED and abs(s["position"][0] - 0.25) <= 1e-6 and run.rides["flags"][0] == 0 and not run.rides["carried"][0].any()


def test_a_warped_character_is_not_carried():
    p, run = standing(True)
    run.warp(0, (0.5, STAND_Y + 0.01, 0.5))
    p.move(dpos=(0.25, 0, 0))
    assert run.rides["entity"][0] == 0  # (the anchor is still there: it is GROUNDED that a warp clears)
    s = run.update(2)[0]
    assert run.rides["flags"][0] == 0 and not run.rides["carried"][0].any() and s["position"][0] == 0.5 and s["position"][2] == 0.5
    assert s["flags"] & CHAR_GROUNDED and run.rides["entity"][0] == 0  # it landed again: the next call carries it
    p.move(dpos=(0.25, 0, 0))
    assert abs(run.update(2)[0]["position"][0] - 0.75) <= 1e-6 and run.rides["flags"][0] == CARRIED


def test_an_anchor_body_that_left_the_world_is_lost():
    p, run = standing(True)
    p.type[0] = BODY_NONE
    p.move(dpos=(0.25, 0, 0))
    before = run.state.copy()
    carried, records = carry_ref(run.state, run.rides, p.poses())
    assert records["flags"][0] == LOST and carried.tobytes() == before.tobytes() and not records["carried"][0].any()
    s = run.update(2)[0]
    assert run.rides["flags"][0] == LOST and s["position"][0] == 0 and run.rides["entity"][0] == NO_ENTITY
    assert not s["flags"] & CHAR_GROUNDED  # (nothing under it any more: it falls towards the plane)
    run.update(2)
    assert run.rides["flags"][0] == 0
    # a pose that is not finite: LOST, position untouched
    p, run = standing(True)
    p.pos[0, 0] = np.inf
    carried, records = carry_ref(run.state, run.rides, p.poses())
    assert records["flags"][0] == LOST and carried.tobytes() == run.state.tobytes() and records["turn"][0].tolist() == [0, 0, 0, 1]


def test_a_dynamic_body_is_ridden_only_with_the_flag():
    p, run = standing(True, body_type=BODY_DYNAMIC)
    assert run.rides["entity"][0] == NO_ENTITY
    p.move(dpos=(0.25, 0, 0))
    s = run.update(2)[0]
    assert run.rides["flags"][0] == 0 and s["position"][0] == 0
    p, run = standing(True, body_type=BODY_DYNAMIC, dynamic=True)
    assert run.rides["entity"][0] == 0
    p.move(dpos=(0.25, 0, 0))
    s = run.update(2)[0]
    assert run.rides["flags"][0] == CARRIED and abs(s["position"][0] - 0.25) <= 1e-6
    run.dynamic = False  # the flag is dropped while the anchor is there: the body is no longer rideable
    p.move(dpos=(0.25, 0, 0))
    s = run.update(2)[0]
    assert run.rides["flags"][0] == LOST and abs(s["position"][0] - 0.25) <= 1e-6 and run.rides["entity"][0] == NO_ENTITY


def test_the_plane_is_never_an_anchor():
    p = Platforms([BODY_NONE], [(1, 1, 1)], [(0, 0, 0)], [(0, 0, 0)])
    run = RideRun(p, hand_character((0.0, REST_Y + 0.01, 0.0)), True)
    s = run.update(2)[0]
    assert s["flags"] == CHAR_GROUNDED and s["ground_kind"] == RAY_GROUND and run.rides["entity"][0] == NO_ENTITY
    assert run.rides[0].tobytes() == fresh_rides(1)[0].tobytes()


# ------------------------------------------------------------------------------------------------ the field of the GPU comparison


def test_reference_alone_clears_the_floors_of_the_gpu_comparison():
    """The GPU test compares the device with ride_run_ref over the device's own queries and poses and asserts these floors on what
    it saw.  The same field, characters and scripts through the float64 shape reference must clear them too."""
    field, moves, descs, inputs = field_case()
    assert len(field) == N_PLATFORMS == 64 and len(descs) == N_CHARS == 257 and len(moves) == len(inputs) == N_CALLS == 6
    assert all(np.abs(dp).max() <= 0.3 and np.abs(de).max() <= 0.2 and not de[0::2].any() for dp, de in moves)
    assert all(np.hypot(i["walk_x"], i["walk_z"]).max() <= 0.1 for i in inputs)
    run = RideRun(field, descs, True)
    calls = []
    for (dpos, deuler), inp in zip(moves, inputs):
        field.move(dpos, deuler)
        before = run.rides
        state = run.update(STEPS_PER_CALL, inp)
        calls.append((before, run.rides, state))
    check_ride_coverage(ride_coverage(calls))
    assert (run.state["steps"] == N_CALLS * STEPS_PER_CALL).all() and not (run.state["flags"] & W.CHAR_INVALID).any()
    assert not any((after["flags"] & LOST).any() for _, after, _ in calls)


def test_the_shuffled_world_of_the_gpu_comparison_has_no_entity_at_its_slot():
    parent, has_transform = shuffled_topology()
    assert acyclic(parent) and len(parent) == N_PLATFORMS + SHUFFLE_PAD
    numbers, slots = layout_numbers(parent, has_transform, N_PLATFORMS)
    print(numbers)
    assert numbers["off"] == N_PLATFORMS and numbers["far"] >= 16 and len(set(slots.tolist())) == N_PLATFORMS


# ------------------------------------------------------------------------------------------------ the ABI


def test_ride_symbols_exported():
    assert_exported(("bge_world_characters_ride", "bge_world_characters_rides", "bge_world_characters_rides_device"))
    assert CHARACTER_RIDE_DTYPE.itemsize == 64 and rides.RIDE_DTYPE == CHARACTER_RIDE_DTYPE
    assert (W.CHAR_RIDE_ON, W.CHAR_RIDE_DYNAMIC, W.CHAR_RIDE_CARRIED, W.CHAR_RIDE_LOST) == (1, 2, 1, 2)
    assert (rides.RIDE_ON, rides.RIDE_DYNAMIC, rides.CARRIED, rides.LOST) == (1, 2, 1, 2)
    assert (rides.BODY_STATIC, rides.BODY_DYNAMIC, rides.BODY_KINEMATIC, rides.BODY_NONE) == (W.BODY_STATIC, W.BODY_DYNAMIC, W.BODY_KINEMATIC, W.BODY_NONE)
    assert [CHARACTER_RIDE_DTYPE.fields[k][1] for k in ("flags", "entity", "anchor_position", "anchor_rotation", "carried", "turn")] == [0, 4, 8, 20, 36, 48]
    for name in ("characters_ride", "characters_rides", "characters_rides_device"):
        assert callable(getattr(W.World, name))


def test_ride_calls_reject_a_null_world():
    from banggameengine_amd import _capi
    lib = _capi.lib()
    assert lib.bge_world_characters_ride(None, 1) == -1
    assert lib.bge_world_characters_rides(None, 0, 0, None) == -1
    assert lib.bge_world_characters_rides_device(None, None, None) == -1
    assert lib.bge_last_error()


def test_abi_c99_ride_record(tmp_path):
    build_and_run_c99(tmp_path, "abi_check_ride.c", "ride abi ok")


def test_adapter_riding_compiles_on_reference_shapes(tmp_path):
    compile_reference_shapes(tmp_path, "ride_reference_shapes.cpp")
