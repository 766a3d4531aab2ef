"""Crowd separation (include/bge_world.h "Crowd separation", bge_world_crowd_query .., bge_world_characters_crowd ..) without a GPU:
crowd_ref of refmodel/crowd.py — the rule in numpy float32 over all pairs — on the hand cases against worked numbers, its symmetry
and the coverage floors of the seeded batches; separate_ref on a character state; the exported symbols, the C99 view of the two
records and the adapter's crowd members on the reference's types.

crowd_ref is the reference of the GPU tests: there the device's 32-byte records must equal it byte for byte."""
from __future__ import annotations

import numpy as np
import pytest

from banggameengine_amd import world as W

from abi import assert_exported, build_and_run_c99, compile_reference_shapes
from refmodel.characters import fresh_state
from refmodel.character_cases import hand_character
from refmodel.crowd import CLAMPED, HIT_DTYPE, INVALID, PUSHED, SPHERE_DTYPE, crowd_ref, make_spheres, separate_ref
from refmodel.crowd_cases import (BATCH_MAX_PUSH, BATCHES, COVERED, HAND, SWEEP_POINTS, check_crowd_coverage, check_shape, far_batch, seeded_batch,
                                  sweep_batch)
from refmodel.rays import NO_ENTITY

F = np.float32


def ref(name):
    spheres, max_push = HAND[name]
    hits = crowd_ref(spheres, max_push)
    check_shape(spheres, hits, max_push)
    return spheres, hits


def ulps(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


def test_the_records_are_the_bindings():
    assert SPHERE_DTYPE == W.CROWD_SPHERE_DTYPE and HIT_DTYPE == W.CROWD_HIT_DTYPE
    assert (INVALID, PUSHED, CLAMPED) == (W.CROWD_INVALID, W.CROWD_PUSHED, W.CROWD_CLAMPED) and W.CHAR_CROWD_ON == 1
    s = W.make_crowd_spheres([(1, 2, 3)], 0.5)
    assert s.tobytes() == make_spheres([(1, 2, 3)], 0.5).tobytes() and s["group"][0] == 1 and s["mask"][0] == 0xFFFFFFFF


def test_a_level_pair_parts_by_half_the_depth_each_and_touches():
    # d = 0.6, R = 1: depth 0.4, t = 0.2; 0 is pushed along -x, 1 along +x
    spheres, h = ref("level pair")
    assert h["flags"].tolist() == [PUSHED, PUSHED] and h["other"].tolist() == [1, 0] and h["n_overlaps"].tolist() == [1, 1]
    assert h["depth"][0] == h["depth"][1] and abs(h["depth"][0] - 0.4) <= 1e-7
    assert abs(h["push"][0][0] + 0.2) <= 1e-7 and abs(h["push"][1][0] - 0.2) <= 1e-7 and h["push"][0][0] == -h["push"][1][0]
    assert not h["push"][:, 1:].any()
    x = spheres["center"][:, 0] + h["push"][:, 0]
    assert ulps(x[1] - x[0], 1.0) <= 4
    again = crowd_ref(make_spheres(np.stack([x, [0, 0], [0, 0]], axis=1), 0.5))
    assert (again["depth"] <= 4 * np.spacing(F(1))).all()  # touching: what is left is rounding


def test_a_vertical_stack_and_a_coincident_pair_part_along_x_by_index():
    for name, depth in (("vertical stack", 0.5), ("coincident pair", 0.5)):
        _, h = ref(name)
        assert h["flags"].tolist() == [PUSHED, PUSHED] and h["other"].tolist() == [1, 0] and h["depth"].tolist() == [depth, depth]
        assert h["push"].tolist() == [[depth / 2, 0, 0], [-depth / 2, 0, 0]], name  # the lower index goes to +x


def test_equal_depths_go_to_the_lowest_index():
    _, h = ref("tie")
    assert h["other"].tolist() == [1, 0, 0] and h["n_overlaps"].tolist() == [2, 1, 1] and h["depth"].tolist() == [0.25] * 3
    assert h["push"][:, 0].tolist() == [-0.125, 0.125, -0.125]  # 0 moves away from 1 only


def test_a_one_way_filter_is_no_pair():
    _, h = ref("one-way filter")
    assert not h["flags"].any() and (h["other"] == NO_ENTITY).all()


def test_invalid_spheres_are_flagged_and_invisible():
    _, h = ref("invalid")
    assert h["flags"].tolist() == [PUSHED, INVALID, INVALID, INVALID, PUSHED]
    assert h["other"].tolist() == [4, NO_ENTITY, NO_ENTITY, NO_ENTITY, 0] and h["n_overlaps"].tolist() == [1, 0, 0, 0, 1]
    assert abs(h["depth"][0] - 0.1) <= 1e-6 and h["push"][0][2] < 0 < h["push"][4][2]
    for k in (1, 2, 3):
        assert h[k].tobytes() == np.array([(INVALID, NO_ENTITY, 0, 0, (0, 0, 0), 0)], HIT_DTYPE).tobytes()


def test_a_point_inside_a_sphere():
    _, h = ref("radius 0")
    assert h["depth"].tolist() == [0.75, 0.75] and h["push"][:, 2].tolist() == [-0.375, 0.375] and h["other"].tolist() == [1, 0]


def test_max_push_clamps():
    _, h = ref("clamped")
    assert h["flags"].tolist() == [PUSHED | CLAMPED] * 2 and h["push"][:, 0].tolist() == [-0.125, 0.125] and abs(h["depth"][0] - 0.4) <= 1e-7
    spheres, _ = HAND["clamped"]
    assert not (crowd_ref(spheres, 0.25)["flags"] & CLAMPED).any()  # t = 0.2 is within 0.25


@pytest.mark.parametrize("n", BATCHES)
def test_seeded_batches_symmetry_and_floors(n):
    spheres = seeded_batch(n)
    h = crowd_ref(spheres, BATCH_MAX_PUSH)
    check_shape(spheres, h, BATCH_MAX_PUSH)
    mutual = 0
    for i in np.flatnonzero(h["flags"] & PUSHED):
        o = h["other"][i]
        assert h["flags"][o] & PUSHED  # whoever overlaps i is overlapped by i
        if h["other"][o] == i:
            mutual += 1
            assert h["depth"][i].tobytes() == h["depth"][o].tobytes()
    if n in COVERED:
        assert mutual >= n // 4
        check_crowd_coverage(spheres, h)


def test_the_far_spheres_and_the_sweep_say_what_their_cases_claim():
    h = crowd_ref(far_batch())
    assert ((h["flags"] & PUSHED) != 0).tolist() == [True, True, True, True, False, False, True, True, False, False, True, True, True, True]
    assert h["depth"][2] == 144 and np.isfinite(h["push"]).all()
    spheres, n_pairs = sweep_batch(0, 1e3, np.random.default_rng(97))
    assert n_pairs == 2 * SWEEP_POINTS and len(spheres) == 2 * n_pairs
    gap = spheres["center"][1::2, 0].astype(np.float64) - spheres["center"][0::2, 0].astype(np.float64)
    assert (gap[:SWEEP_POINTS] < 1).all() and (gap[SWEEP_POINTS:] >= 1).all() and (gap < 1.001).all()


def test_separate_moves_only_x_and_z_of_the_pushed():
    descs = np.concatenate([hand_character((0.0, 0.51, 0.0)), hand_character((0.6, 0.51, 0.0)), hand_character((-0.0, 0.51, 9.0))])
    state = fresh_state(descs)
    state["vertical_velocity"], state["steps"] = (1, 2, 3), 7
    out, hits = separate_ref(descs, state)
    assert hits["flags"].tolist() == [PUSHED, PUSHED, 0]
    assert abs(out["position"][0][0] + 0.2) <= 1e-7 and abs(out["position"][1][0] - 0.8) <= 1e-6
    assert out[2].tobytes() == state[2].tobytes() and np.signbit(out["position"][2][0])  # untouched, the -0 included
    changed = out.copy()
    changed["position"][:, 0] = state["position"][:, 0]
    assert changed.tobytes() == state.tobytes()  # nothing but x (z where the push has one) changed
    # a filter that hides 0 and 1 from each other: nobody moves
    out, hits = separate_ref(descs, state, group=np.uint32([1, 2, 1]), mask=np.uint32([1, 2, 1]))
    assert not hits["flags"].any() and out.tobytes() == state.tobytes()


def test_symbols_are_exported():
    assert_exported(["bge_world_crowd_query", "bge_world_crowd_query_device", "bge_world_characters_crowd", "bge_world_characters_crowd_hits",
                     "bge_world_characters_crowd_hits_device", "bge_world_characters_update"])


def test_c99_view_of_the_records(tmp_path):
    build_and_run_c99(tmp_path, "abi_check_crowd.c", "crowd abi ok")


def test_adapter_crowd_members_on_reference_shapes(tmp_path):
    compile_reference_shapes(tmp_path, "crowd_reference_shapes.cpp")
