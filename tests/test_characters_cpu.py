"""Characters (include/bge_world.h "Characters", bge_world_characters_*) without a GPU: char_ref of refmodel/characters.py, the
header's rule in numpy float32 scalars composed from recover_ref and step_ref, on the hand-worked cases of
refmodel/character_cases.py — through the analytic half-space caster and penetration function where half-spaces can express the
scene, through the float64 shape reference otherwise — the seeded walk of the GPU comparison on the shape reference alone with its
coverage floors, the exported symbols, the C99 view of the records and the adapter's character members on the reference's types.

char_ref is the reference of the GPU tests: there the caster is World.sphere_cast and the penetration function
World.sphere_penetration on the same world, and the device's 80-byte states must equal it byte for byte."""
from __future__ import annotations

import numpy as np
import pytest

from banggameengine_amd import world as W
from banggameengine_amd.world import (CHAR_GROUNDED, CHAR_HEAD_BUMP, CHAR_INVALID, CHAR_JUMPED, CHAR_LANDED, CHAR_RECOVERED, CHAR_STEPPED,
                                      CHARACTER_DESC_DTYPE, CHARACTER_INPUT_DTYPE, CHARACTER_STATE_DTYPE)

from abi import assert_exported, build_and_run_c99, compile_reference_shapes
from refmodel import characters
from refmodel.characters import fresh_state, run_ref
from refmodel.rays import NO_ENTITY, RAY_BODY, RAY_GROUND, RAY_MISS, World64
from refmodel.spheres import SphereRef
from refmodel.moves import F, HalfSpaces, caster_of
from refmodel.move_cases import hand_objects
from refmodel.recover import HalfSpacesPen, pen_of
from refmodel.step_cases import FIELD_SEED, StepField
from refmodel.character_cases import (CHAR_SEED, DT, HEAD_BUMP_STEP, HEAD_BUMP_Y, INPUT_SEED, INTRUDER_PUSH, JUMP_HEIGHTS, JUMP_LANDS_IN_STEP, N_CHARS,
                                      N_OVERLAPPING, N_STEPS, REST_Y, SCENES, SKIN, character_batch, character_coverage, check_character_coverage,
                                      hand_character, input_script, inputs_of)


def views(scene):
    """[(caster, penetration function)] of a scene: the analytic one where half-spaces say it, the shape reference where it has bodies
    (or nothing but the plane)."""
    walls, bodies, plane = SCENES[scene]
    out = []
    if walls is not None:
        out.append((HalfSpaces(walls), HalfSpacesPen(walls)))
    if bodies is not None:
        w64 = World64(hand_objects(bodies, ()), plane)
        out.append((caster_of(SphereRef(w64).sweep_all), pen_of(w64)))
    return out


class Run:
    """A character set of one over a view: update(steps, ...) as the device's calls go, with every step's state kept."""

    def __init__(self, view, descs):
        self.view, self.descs = view, descs
        self.state = fresh_state(descs)
        self.inputs = np.zeros(len(descs), CHARACTER_INPUT_DTYPE)
        self.history = []

    def update(self, steps=1, **inp):
        if inp:
            self.inputs = inputs_of(**inp)
        self.state = run_ref(self.view[0], self.view[1], self.descs, self.inputs, self.state, DT, steps, self.history)
        return self.state[0]

    def flags(self):
        return [int(s["flags"][0]) for s in self.history]

    def ys(self):
        return [float(s["position"][0][1]) for s in self.history]


def settled(view, x=0.0, **kw):
    run = Run(view, hand_character((x, REST_Y + 0.01, 0.0), **kw))
    s = run.update()
    assert s["flags"] == CHAR_GROUNDED | CHAR_LANDED and abs(s["position"][1] - REST_Y) <= 1e-6 and s["vertical_velocity"] == 0, s  # SETTLE
    assert s["ground_kind"] == RAY_GROUND and s["steps"] == 1
    run.history.clear()
    return run


# ------------------------------------------------------------------------------------------------ hand-worked cases


@pytest.mark.parametrize("view", views("plane"), ids=["half-spaces", "shapes"])
def test_at_rest_on_the_plane(view):
    run = settled(view)
    run.update(10)
    assert run.flags() == [CHAR_GROUNDED] * 10
    assert all(s["vertical_velocity"][0] == 0 for s in run.history)
    assert max(abs(y - REST_Y) for y in run.ys()) <= 1e-6 and run.state["steps"][0] == 11
    assert not run.state["position"][0][[0, 2]].any()


@pytest.mark.parametrize("view", views("plane"), ids=["half-spaces", "shapes"])
def test_jump_arc(view):
    run = settled(view)
    run.update(JUMP_LANDS_IN_STEP + 10, jump=True)
    fl, ys = run.flags(), run.ys()
    assert fl[0] == CHAR_JUMPED and sum(1 for f in fl if f & CHAR_JUMPED) == 1
    assert np.allclose(ys[:3], JUMP_HEIGHTS, atol=1e-5, rtol=0), ys[:3]
    vv = [float(s["vertical_velocity"][0]) for s in run.history[:3]]
    assert np.allclose(vv, [4.8365, 4.673, 4.5095], atol=1e-5, rtol=0), vv
    landed = [k + 1 for k, f in enumerate(fl) if f & CHAR_LANDED]
    assert landed == [JUMP_LANDS_IN_STEP], landed
    assert not any(f & CHAR_GROUNDED for f in fl[:JUMP_LANDS_IN_STEP - 1]) and all(f == CHAR_GROUNDED for f in fl[JUMP_LANDS_IN_STEP:])
    assert abs(ys[-1] - REST_Y) <= 1e-4 and run.state["vertical_velocity"][0] == 0
    assert max(ys) == pytest.approx(REST_Y + DT * (5 * 30 - 9.81 * DT * 30 * 31 / 2), abs=1e-4)  # the apex, after 30 steps
    assert run.inputs["buttons"][0] == 0


def test_jump_in_the_air_is_ignored_and_consumed():
    view = views("plane")[0]
    run = Run(view, hand_character((0.0, 3.0, 0.0)))
    s = run.update(jump=True)
    # not grounded: no jump; vv = -g dt, y = 3 - g dt dt; the edge is gone
    assert s["flags"] == 0 and s["vertical_velocity"] == pytest.approx(-0.1635, abs=1e-6) and s["position"][1] == pytest.approx(3 - 0.002725, abs=1e-6)
    assert run.inputs["buttons"][0] == 0
    run.update(59)  # 2.49 of fall take sqrt(2 * 2.49 / 9.81) = 0.7125 s = 43 steps
    fl = run.flags()
    assert not any(f & CHAR_JUMPED for f in fl) and sum(1 for f in fl if f & CHAR_LANDED) == 1 and fl[-1] == CHAR_GROUNDED
    assert abs(run.ys()[-1] - REST_Y) <= 1e-4
    # several steps in one call: the first consumes the edge on the ground, the others do not jump again
    run2 = settled(view)
    run2.update(3, jump=True)
    assert [f & CHAR_JUMPED for f in run2.flags()] == [CHAR_JUMPED, 0, 0]


def test_a_fall_is_clamped_at_the_fall_speed():
    # nothing to meet.  fall_speed 2: vv = -k g dt for k <= 12 (1.962), then -2 for good; a step then moves by 2 dt
    run = Run(views("nothing")[0], hand_character((0.0, 50.0, 0.0), fall_speed=2.0))
    run.update(20)
    vv = [float(s["vertical_velocity"][0]) for s in run.history]
    assert np.allclose(vv[:12], [-0.1635 * k for k in range(1, 13)], atol=1e-5, rtol=0) and vv[12:] == [-2.0] * 8
    ys = run.ys()
    assert np.allclose(np.diff(ys[12:]), -2.0 * DT, atol=1e-5, rtol=0) and run.flags() == [0] * 20
    assert run.state["ground_kind"][0] == RAY_MISS and run.state["ground_entity"][0] == NO_ENTITY


@pytest.mark.parametrize("view", views("ceiling"), ids=["half-spaces", "shapes"])
def test_head_bump_under_a_ceiling(view):
    run = settled(view)
    run.update(HEAD_BUMP_STEP, jump=True)
    fl, ys = run.flags(), run.ys()
    assert fl == [CHAR_JUMPED, 0, CHAR_HEAD_BUMP]
    assert np.allclose(ys, JUMP_HEIGHTS[:2] + (HEAD_BUMP_Y,), atol=1e-5, rtol=0), ys
    s = run.state[0]
    assert s["vertical_velocity"] == 0 and s["hit_kind"] == RAY_BODY and s["hit_entity"] == 0 and np.allclose(s["hit_normal"], (0, -1, 0), atol=1e-6)
    run.update(30)  # and down again: 0.18 of fall
    assert sum(1 for f in run.flags() if f & CHAR_LANDED) == 1 and abs(run.ys()[-1] - REST_Y) <= 1e-4


def test_stairs_are_climbed_with_enough_step_height_and_block_without():
    # Treads 1 deep and 0.3 high from x = 1.  The character has radius 0.25, below a riser's height, so it meets a riser's face head-on
    # (a sphere of radius 0.5 meets the upper edge instead and rolls over it without a step).  Walking 0.1 a step from x = 0, 60 steps
    # ask 6 of way.  The plain move rests at the face with the skin: x = 1 - 0.25 - 0.01 = 0.74.  With step_height 0.35 the raised
    # sphere's underside (0.01 + 0.35) clears the riser, goes 0.1 forward to x = 0.84 and comes down on the riser's upper edge 0.16
    # away: normal.y = sqrt(0.0625 - 0.0256) / 0.25 = 0.768 >= cos 45: STEPPED, once per riser, step_rise 0.35.  It ends on the top tread;
    # a step lands on an edge, where the vertical back-off keeps a gap of skin * normal.y, and the level walk from there slides onto
    # the tread at that height: the gap to the tread is within (0, skin], the height within (0.9 + 0.25, 0.9 + 0.26].  With step_height
    # 0.2 the raised sphere (underside 0.21) meets the same face at the same place: nothing gained, it stays at x = 0.74 on the plane.
    view = views("stairs")[0]
    kw = dict(radius=0.25)

    def walker(step_height):
        run = Run(view, hand_character((0.0, 0.25 + SKIN + 0.01, 0.0), step_height=step_height, **kw))
        assert run.update()["flags"] == CHAR_GROUNDED | CHAR_LANDED
        run.history.clear()
        run.update(60, walk_x=0.1)
        return run

    climb = walker(0.35)
    s = climb.state[0]
    assert s["flags"] & CHAR_GROUNDED and 0.9 + 0.25 < s["position"][1] <= 0.9 + 0.26 + 1e-5 and s["position"][0] > 3.5, s
    assert s["ground_kind"] == RAY_BODY and s["ground_entity"] == 2
    assert sum(1 for f in climb.flags() if f & CHAR_STEPPED) == 3 and all(f & CHAR_GROUNDED for f in climb.flags())
    rises = sorted({round(float(h["step_rise"][0]), 4) for h in climb.history if h["flags"][0] & CHAR_STEPPED})
    assert rises == [0.35], rises
    block = walker(0.2)
    s = block.state[0]
    assert abs(s["position"][0] - 0.74) <= 1e-5 and abs(s["position"][1] - 0.26) <= 1e-5 and s["flags"] == CHAR_GROUNDED, s
    assert not any(f & CHAR_STEPPED for f in block.flags()) and s["hit_kind"] == RAY_BODY and s["hit_entity"] == 0


def test_walking_off_an_edge_falls_and_lands():
    # The table's top is at y = 1, its edge at x = 2.  From x = 1.5 on the top, 0.1 a step: once the centre is past the edge the probe
    # finds the edge at a normal that leans out; beyond normal.y < cos 45 (0.354 out) it is no ground: GROUNDED goes without JUMPED,
    # the character falls 1 (0.45 s = 27 steps) and lands on the plane.
    view = views("table")[0]
    run = Run(view, hand_character((1.5, 1.0 + REST_Y + 0.01, 0.0)))
    assert run.update()["flags"] == CHAR_GROUNDED | CHAR_LANDED and run.state["ground_kind"][0] == RAY_BODY
    run.history.clear()
    run.update(50, walk_x=0.1)
    fl = run.flags()
    lost = next(k for k, f in enumerate(fl) if not f & CHAR_GROUNDED)
    assert 5 <= lost <= 12 and not any(f & CHAR_JUMPED for f in fl), (lost, fl)
    assert run.history[lost]["position"][0][0] > 2.3
    landed = [k for k, f in enumerate(fl) if f & CHAR_LANDED]
    assert len(landed) == 1 and landed[0] > lost + 15 and run.history[landed[0]]["ground_kind"][0] == RAY_GROUND
    assert abs(run.ys()[-1] - REST_Y) <= 1e-4 and fl[-1] == CHAR_GROUNDED


def test_a_downward_ramp_needs_a_probe_that_covers_the_drop():
    # 30 degrees down: a level step of 0.1 opens a drop of 0.1 tan 30 = 0.0577 under the sphere, on top of the gap it keeps
    # (skin * normal.y along the vertical after a snap).  probe_distance 0.1 covers that: GROUNDED every step, and the height follows the
    # ramp: -0.0577 a step.  probe_distance 0.001 covers neither: the character leaves the ground.
    view = views("ramp")[0]
    n = np.array([0.5, np.cos(np.pi / 6), 0.0])
    start = np.array([0.0, 2.0, 0.0]) + n * (0.5 + 0.02)
    run = Run(view, hand_character(tuple(start), probe_distance=0.1))
    run.update(3)
    assert run.flags()[-1] == CHAR_GROUNDED
    run.history.clear()
    run.update(30, walk_x=0.1)
    assert run.flags() == [CHAR_GROUNDED] * 30
    assert np.allclose(np.diff(run.ys()), -0.1 * np.tan(np.pi / 6), atol=1e-4, rtol=0)
    assert np.allclose(run.state["ground_normal"][0], n, atol=1e-6)
    short = Run(view, hand_character(tuple(start), probe_distance=0.001))
    short.update(30, walk_x=0.1)
    assert sum(1 for f in short.flags() if f & CHAR_GROUNDED) < 30 and not any(f & CHAR_JUMPED for f in short.flags())
    never = Run(view, hand_character(tuple(start), probe_distance=0.0))  # probe_distance = 0 never grounds
    never.update(30, walk_x=0.1)
    assert not any(f & CHAR_GROUNDED for f in never.flags())


def test_a_box_placed_over_a_standing_character_is_recovered_from():
    run = settled(views("plane")[1])
    run.view = views("intruder")[0]  # the world changed under the character
    s = run.update()
    assert s["flags"] == CHAR_GROUNDED | CHAR_RECOVERED, s
    assert np.allclose(s["recovered"], INTRUDER_PUSH, atol=1e-5, rtol=0) and np.allclose(s["position"], (-0.21, REST_Y, 0), atol=1e-5, rtol=0)
    assert run.update()["flags"] == CHAR_GROUNDED and not run.state["recovered"][0].any()


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_a_walk_that_is_not_finite_is_invalid_and_keeps_the_state(bad):
    run = settled(views("plane")[0])
    run.update(2, walk_x=0.1)
    before = run.state.copy()
    s = run.update(walk_z=bad, jump=True)
    assert s["flags"] == CHAR_INVALID | CHAR_GROUNDED and s["steps"] == before["steps"][0] + 1
    assert s["position"].tobytes() == before["position"][0].tobytes() and s["vertical_velocity"] == before["vertical_velocity"][0]
    assert s["ground_kind"] == RAY_MISS and s["ground_entity"] == NO_ENTITY and s["hit_entity"] == NO_ENTITY and not s["recovered"].any()
    assert run.inputs["buttons"][0] == 0  # the edge is consumed all the same
    assert run.update(walk_x=0.1)["flags"] == CHAR_GROUNDED  # and the next valid step goes on from there
    air = Run(views("plane")[0], hand_character((0.0, 3.0, 0.0)))
    air.update(3)
    before = air.state.copy()
    s = air.update(walk_x=bad)
    assert s["flags"] == CHAR_INVALID and s["position"].tobytes() == before["position"][0].tobytes()
    assert s["vertical_velocity"] == before["vertical_velocity"][0]


# ------------------------------------------------------------------------------------------------ the walk of the GPU comparison


def test_reference_alone_clears_the_floors_of_the_gpu_comparison():
    """The GPU test compares the device's states with char_ref over the device's own queries on the ticked step field and asserts
    these floors on what it saw.  The same field, characters and inputs through the float64 shape reference must clear them too, so
    that the comparison cannot pass by seeing nothing happen."""
    field = StepField(np.random.default_rng(FIELD_SEED))
    descs, heading = character_batch(np.random.default_rng(CHAR_SEED), N_CHARS, field)
    script = input_script(np.random.default_rng(INPUT_SEED), heading, N_STEPS)
    assert len(descs) == 257 and len(script) == 8 and all(np.hypot(s["walk_x"], s["walk_z"]).max() <= 0.3 for s in script)
    w64 = field.world64()
    cast_fn, pen_fn = caster_of(SphereRef(w64).sweep_all), pen_of(w64)
    initial = fresh_state(descs)
    state, history = initial, []
    for inp in script:
        state = run_ref(cast_fn, pen_fn, descs, inp.copy(), state, DT, 1, history)
    cov = character_coverage(initial, history)
    check_character_coverage(cov)
    assert (history[0]["flags"][:N_OVERLAPPING] & CHAR_RECOVERED).all()  # the deliberately overlapping ones
    assert not (state["flags"] & CHAR_INVALID).any() and (state["steps"] == 8).all()


# ------------------------------------------------------------------------------------------------ the ABI


def test_character_symbols_exported():
    assert_exported(("bge_world_characters_create", "bge_world_characters_set_input", "bge_world_characters_set_input_device",
                     "bge_world_characters_warp", "bge_world_characters_update", "bge_world_characters_download",
                     "bge_world_characters_state_device"))
    assert (CHARACTER_DESC_DTYPE.itemsize, CHARACTER_INPUT_DTYPE.itemsize, CHARACTER_STATE_DTYPE.itemsize) == (48, 16, 80)
    assert characters.DESC_DTYPE == CHARACTER_DESC_DTYPE and characters.INPUT_DTYPE == CHARACTER_INPUT_DTYPE and characters.STATE_DTYPE == CHARACTER_STATE_DTYPE
    assert characters.RECOVER_DTYPE == W.SPHERE_RECOVER_DTYPE
    names = ("INVALID", "GROUNDED", "JUMPED", "LANDED", "HEAD_BUMP", "RECOVERED", "STUCK", "STEPPED", "OUT_OF_SLIDES")
    assert [getattr(W, "CHAR_" + k) for k in names] == [1 << k for k in range(9)]
    assert [getattr(characters, k if k != "STEPPED" else "CHAR_STEPPED") for k in names] == [1 << k for k in range(9)]
    assert W.CHAR_BUTTON_JUMP == characters.BUTTON_JUMP == 1
    d = W.make_characters([[0, 1, 0], [1, 2, 3]], [0.5, 0.25], 0.02, 0.3, 0.5, 0.2, 9.81, 4.0, 20.0, 3)
    assert d["radius"].tolist() == [0.5, 0.25] and d["skin"].tolist() == [F(0.02)] * 2 and d["layer_mask"].tolist() == [3, 3]
    assert d["fall_speed"].tolist() == [20.0, 20.0] and d["position"][1].tolist() == [1, 2, 3]
    i = W.make_character_inputs([0.1, 0.2], 0.0, [True, False])
    assert i["buttons"].tolist() == [1, 0] and i["walk_x"].tolist() == [F(0.1), F(0.2)]
    for name in ("characters_create", "characters_set_input", "characters_warp", "characters_update", "characters_state", "characters_state_device"):
        assert callable(getattr(W.World, name))


def test_character_calls_reject_a_null_world():
    from banggameengine_amd import _capi
    lib = _capi.lib()
    assert lib.bge_world_characters_create(None, 0, None) == -1
    assert lib.bge_world_characters_set_input(None, 0, 0, None) == -1
    assert lib.bge_world_characters_set_input_device(None, 0, 0, None) == -1
    assert lib.bge_world_characters_warp(None, 0, None, None) == -1
    assert lib.bge_world_characters_update(None, 0.01, 1) == -1
    assert lib.bge_world_characters_download(None, 0, 0, None) == -1
    assert lib.bge_world_characters_state_device(None, None, None) == -1
    assert lib.bge_last_error()


def test_abi_c99_character_records(tmp_path):
    build_and_run_c99(tmp_path, "abi_check_character.c", "character abi ok")


def test_adapter_characters_compile_on_reference_shapes(tmp_path):
    compile_reference_shapes(tmp_path, "character_reference_shapes.cpp")
