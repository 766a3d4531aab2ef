"""Sphere moves (include/bge_world.h "Sphere moves", bge_world_sphere_move*) without a GPU: move_ref of refmodel/moves.py, the rule of
the header in numpy float32 scalars over a caster handed in, on the hand-worked cases of refmodel/move_cases.py, through an analytic
caster of half-spaces and through the float64 shape reference of refmodel/spheres.py; the coverage the GPU comparison relies on; the
exported symbols, the C99 view of the records and the adapter's MoveSphere / MoveSpheres on the reference's types.

move_ref(cast_fn, moves) is the reference of the GPU tests: there cast_fn is World.sphere_cast on the same world, and the device's
result must equal it byte for byte."""
from __future__ import annotations

import math

import numpy as np
import pytest

from banggameengine_amd.world import (MOVE_GROUNDED, MOVE_INVALID, MOVE_OUT_OF_SLIDES, MOVE_PROBE_HIT, MOVE_SLIDES, SPHERE_MOVE_DTYPE,
                                      SPHERE_MOVE_RESULT_DTYPE, make_sphere_moves)

from abi import assert_exported, build_and_run_c99, compile_reference_shapes
from refmodel.rays import ALL
from refmodel.spheres import SphereRef, sweep_all
from refmodel.moves import F, HalfSpaces, caster_of, move_ref, scripted
from refmodel.sphere_cases import scene_world64
from refmodel.move_cases import (BATCHES, HAND_MOVES, MOVER_SEED, PLANE, R, SCENE_N, SCENE_SEED, SKIN, check_coverage, check_hand_move, check_invalid,
                                 coverage, ghost_positions, hand_mover, hand_objects, invalid_movers, mover_batch)

# ------------------------------------------------------------------------------------------------ hand-worked cases


@pytest.mark.parametrize("case", HAND_MOVES, ids=[c[0] for c in HAND_MOVES])
def test_hand_worked_moves(case):
    name, walls, bodies, ghosts, plane, _, want = case
    objs = hand_objects(bodies, ghosts)
    shapes = caster_of(lambda o, d, md, r, mask: sweep_all(objs, o, d, md, r, mask, plane))
    for cast_fn in (HalfSpaces(walls), shapes):
        trace = {}
        got = move_ref(cast_fn, hand_mover(case), trace)[0]
        check_hand_move(name, got, want)
        if "crease" in want:
            assert bool(trace["crease"][0]) == want["crease"], name


def test_out_of_slides_on_a_turning_wall():
    """Four rounds, each met at f = 0.5 by a wall turned 20 degrees further: with u(t) = (cos t, 0, sin t) the round k moves along
    u(20 k) into the normal n_k = (-sin 20(k + 1), 0, cos 20(k + 1)): the approach cosine is sin 20 = 0.342 (above the clamp), the
    slide is |l| cos 20 along u(20 (k + 1)), never into the previous wall (s . n_(k-1) = |s| sin 20 > 0) nor against d0 = (4, 0, 0)
    (80 degrees at the end).  So r_k = 4 (cos 20 / 2)^k u(20 k), every round moves g_k r_k with g_k = 0.5 - 0.01 / (sin 20 |r_k|),
    and after the four rounds remaining = 4 (cos 20 / 2)^4 u(80) with OUT_OF_SLIDES."""
    th = math.radians(20.0)
    rounds = [(0.5, (-math.sin(th * (k + 1)), 0.0, math.cos(th * (k + 1)))) for k in range(4)]
    trace = {}
    got = move_ref(scripted(rounds), make_sphere_moves([(0, 1, 0)], [(4, 0, 0)], R, SKIN, 0.0, 0.7, ALL), trace)[0]
    pos = np.array([0.0, 1.0, 0.0])
    for k in range(4):
        length = 4.0 * (math.cos(th) / 2) ** k
        pos += (0.5 - 0.01 / (math.sin(th) * length)) * length * np.array([math.cos(th * k), 0.0, math.sin(th * k)])
    rem = 4.0 * (math.cos(th) / 2) ** 4 * np.array([math.cos(4 * th), 0.0, math.sin(4 * th)])
    assert got["flags"] == MOVE_OUT_OF_SLIDES and got["n_hits"] == 4 and not trace["crease"][0]
    assert np.allclose(got["position"], pos, atol=1e-5, rtol=0) and np.allclose(got["remaining"], rem, atol=1e-5, rtol=0)
    assert np.allclose(got["hit_normal"], rounds[3][1], atol=1e-6) and got["hit_entity"] == 3
    # one round fewer ends the same chain on a free fourth round: nothing remains
    got = move_ref(scripted(rounds[:3]), make_sphere_moves([(0, 1, 0)], [(4, 0, 0)], R, SKIN, 0.0, 0.7, ALL))[0]
    assert got["flags"] == 0 and got["n_hits"] == 3 and not got["remaining"].any()


def test_grazing_approach_is_clamped():
    # grazing: the approach cosine 0.01 is clamped to 1/16, so the back-off is 16 skins of path: g = 0.5 - 0.16 / 4
    c = 0.01
    got = move_ref(scripted([(0.5, (-c, math.sqrt(1 - c * c), 0.0))]), make_sphere_moves([(0, 1, 0)], [(4, 0, 0)], R, SKIN, 0.0, 0.7, ALL))[0]
    assert got["n_hits"] == 1 and abs(got["position"][0] - 4 * 0.46 - 2 * (1 - c * c)) < 1e-4


def test_invalid_movers_echo_the_position():
    moves = invalid_movers()
    check_invalid(moves, move_ref(HalfSpaces([PLANE]), moves))
    # and a zero displacement is valid: it stays, and still probes
    got = move_ref(HalfSpaces([PLANE]), make_sphere_moves([(0, 0.55, 0)], [(0, 0, 0)], R, SKIN, 0.1, 0.7, ALL))[0]
    assert got["flags"] == MOVE_GROUNDED | MOVE_PROBE_HIT and got["n_hits"] == 0 and got["position"].tolist() == [0, F(0.55), 0]


# ------------------------------------------------------------------------------------------------ the batches of the GPU comparison


def test_reference_alone_clears_the_floors_of_the_gpu_comparison():
    """The GPU test compares World.sphere_move with move_ref over World.sphere_cast on a ticked scene and asserts these floors on
    what it saw.  The same scene (before its first tick) and the same movers through the float64 shape reference must clear them
    too, so the comparison cannot pass by missing everything."""
    w64, _ = scene_world64(SCENE_N, np.random.default_rng(SCENE_SEED))
    moves = mover_batch(np.random.default_rng(MOVER_SEED), max(BATCHES), ghost_positions(w64))
    ref = SphereRef(w64)
    trace = {}
    got = move_ref(caster_of(ref.sweep_all), moves, trace)
    check_coverage(coverage(moves, got, trace["crease"]))
    assert ((got["flags"] & MOVE_INVALID) != 0).sum() == len(range(36, len(moves), 37))


# ------------------------------------------------------------------------------------------------ the ABI


def test_sphere_move_symbols_exported():
    assert_exported(("bge_world_sphere_move", "bge_world_sphere_move_device"))
    from banggameengine_amd.world import World
    assert SPHERE_MOVE_DTYPE.itemsize == 48 and SPHERE_MOVE_RESULT_DTYPE.itemsize == 80 and MOVE_SLIDES == 4
    assert SPHERE_MOVE_DTYPE.fields["layer_mask"][1] == 40 and SPHERE_MOVE_RESULT_DTYPE.fields["ground_normal"][1] == 64
    m = make_sphere_moves([[0, 1, 0], [1, 2, 3]], [[0, -1, 0], [1, 0, 0]], [0.5, 0.25], 0.02, 0.3, 0.5, 3)
    assert m["radius"].tolist() == [0.5, 0.25] and m["skin"].tolist() == [F(0.02)] * 2 and m["layer_mask"].tolist() == [3, 3]
    assert m["probe_distance"].tolist() == [F(0.3)] * 2 and m["min_ground_ny"].tolist() == [0.5, 0.5] and not m["reserved"].any()
    for name in ("sphere_move", "sphere_move_device"):
        assert callable(getattr(World, name))


def test_sphere_moves_reject_null_world_and_zero_count():
    from banggameengine_amd import _capi
    lib = _capi.lib()
    for fn in (lib.bge_world_sphere_move, lib.bge_world_sphere_move_device):
        assert fn(None, 1, None, None) == -1
        assert fn(None, 0, None, None) == -1
    assert lib.bge_last_error()


def test_abi_c99_move_records(tmp_path):
    build_and_run_c99(tmp_path, "abi_check_move.c", "move abi ok")


def test_adapter_sphere_moves_compile_on_reference_shapes(tmp_path):
    compile_reference_shapes(tmp_path, "move_reference_shapes.cpp")
