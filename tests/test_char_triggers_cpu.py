"""Character trigger events without a GPU (include/bge_world.h "Character trigger events"): the rule on the reference
char_trigger_ref alone — the hand cases and the seeded walk's coverage floors — and the C ABI of the new entry points."""
from __future__ import annotations

import numpy as np

from banggameengine_amd import world as W

from abi import assert_exported, build_and_run_c99, compile_reference_shapes
from refmodel.char_triggers import CHAR_GROUP, CHAR_MASK, ENTER, EXIT, STAY, char_boxes, char_trigger_ref, pairs_of
from refmodel.char_trigger_cases import (N_CALLS, N_CHARS, N_TRIGGERS, THROUGH_EVENTS, THROUGH_X, UNIT, Walk, check_coverage, coverage,
                                         run_reference)

ALL = 0xFFFFFFFF
F = np.float32


def one(boxes, pos, prev, listed=None, layer=4, mask=ALL, radius=0.5, group=CHAR_GROUP, cmask=CHAR_MASK, stay=True, entity=None):
    """char_trigger_ref with scalars spread over the triggers and the characters."""
    boxes, pos = np.asarray(boxes, F).reshape(-1, 6), np.asarray(pos, F).reshape(-1, 3)
    T, n = len(boxes), len(pos)
    spread = lambda v, k: np.broadcast_to(np.asarray(v, np.uint32), (k,))
    ev, after = char_trigger_ref(boxes, np.ones(T, bool) if listed is None else listed, spread(layer, T), spread(mask, T), pos,
                                 np.broadcast_to(F(radius), (n,)), spread(group, n), spread(cmask, n), prev, stay, entity)
    return ev.tolist(), after


def test_one_character_through_one_box():
    prev = np.zeros((1, 1), bool)
    for x, want in zip(THROUGH_X, THROUGH_EVENTS):
        ev, prev = one(UNIT, [[x, 0, 0]], prev)
        assert [e[0] for e in ev] == want, (x, ev)
        assert all(e[1:] == [0, 0] for e in ev)
    assert not prev.any()


def test_the_boundary_is_closed():
    """The smallest binary32 x whose upper corner (x + 0.5) + 0.02f reaches tmin = -1 exactly overlaps; the next float below it
    does not."""
    x = F(-1.52)
    upper = lambda v: F(F(F(v) + F(0.5)) + F(0.02))
    while upper(x) < F(-1):
        x = np.nextafter(x, F(0))
    while upper(np.nextafter(x, F(-2))) >= F(-1):
        x = np.nextafter(x, F(-2))
    assert upper(x) == F(-1) and upper(np.nextafter(x, F(-2))) < F(-1)
    assert char_boxes([[x, 0, 0]], [0.5])[1][0, 0] == F(-1)
    none = np.zeros((1, 1), bool)
    assert one(UNIT, [[x, 0, 0]], none)[0] == [[ENTER, 0, 0]]
    assert one(UNIT, [[np.nextafter(x, F(-2)), 0, 0]], none)[0] == []
    # and the other side: cmin == tmax
    lower = lambda v: F(F(F(v) - F(0.5)) - F(0.02))
    y = F(1.52)
    while lower(y) > F(1):
        y = np.nextafter(y, F(0))
    while lower(np.nextafter(y, F(2))) <= F(1):
        y = np.nextafter(y, F(2))
    assert lower(y) == F(1)
    assert one(UNIT, [[0, y, 0]], none)[0] == [[ENTER, 0, 0]] and one(UNIT, [[0, np.nextafter(y, F(2)), 0]], none)[0] == []


def test_each_half_of_the_filter_alone_and_group_zero():
    none, inside = np.zeros((1, 1), bool), [[0, 0, 0]]
    assert one(UNIT, inside, none)[0] == [[ENTER, 0, 0]]                       # layer 4 & mask all, group 2 & mask all
    assert one(UNIT, inside, none, cmask=ALL & ~4)[0] == []                    # the character's mask leaves the trigger's layer out
    assert one(UNIT, inside, none, mask=ALL & ~2)[0] == []                     # the trigger's mask leaves the character's group out
    assert one(UNIT, inside, none, mask=8, group=8)[0] == [[ENTER, 0, 0]]
    assert one(UNIT, inside, none, layer=0x10, cmask=0x10)[0] == [[ENTER, 0, 0]]
    assert one(UNIT, inside, none, group=0)[0] == []                           # group 0 overlaps nothing
    # a pair that stops passing the filter Exits
    assert one(UNIT, inside, np.ones((1, 1), bool), group=0)[0] == [[EXIT, 0, 0]]


def test_stay_off_leaves_only_the_stay_records_out():
    boxes = np.concatenate([UNIT, UNIT + F(10)])
    pos = [[0, 0, 0], [0.5, 0, 0], [10, 10, 10], [50, 0, 0]]
    prev = np.array([[1, 0, 0, 1], [0, 0, 1, 1]], bool)
    with_stay, after = one(boxes, pos, prev)
    without, after2 = one(boxes, pos, prev, stay=False)
    assert with_stay == [[STAY, 0, 0], [ENTER, 0, 1], [EXIT, 0, 3], [STAY, 1, 2], [EXIT, 1, 3]]
    assert without == [e for e in with_stay if e[0] != STAY] and np.array_equal(after, after2)


def test_an_unlisted_trigger_is_skipped_and_keeps_its_remembered_set():
    boxes = np.concatenate([UNIT, UNIT])
    prev = np.array([[1, 0], [1, 0]], bool)
    ev, after = one(boxes, [[50, 0, 0], [0, 0, 0]], prev, listed=np.array([True, False]))
    assert ev == [[ENTER, 0, 1], [EXIT, 0, 0]]  # Enter and Stay first, then Exit
    assert after.tolist() == [[False, True], [True, False]]
    ev, after = one(boxes, [[50, 0, 0], [0, 0, 0]], after, listed=np.array([True, True]))
    assert ev == [[STAY, 0, 1], [ENTER, 1, 1], [EXIT, 1, 0]]
    assert pairs_of(after, [7, 9]).tolist() == [[7, 1], [9, 1]]


def test_the_order_with_two_triggers_and_three_characters():
    """Triggers in array order; inside one, Enter and Stay by ascending character, then Exit by ascending character.  The trigger
    is named by its entity."""
    boxes = np.concatenate([UNIT + F(10), UNIT])  # trigger 0 (entity 5) around (10, 10, 10), trigger 1 (entity 3) around the origin
    pos = [[0, 0, 0], [10, 10, 10], [0.2, 0, 0]]
    prev = np.array([[1, 0, 1], [0, 1, 1]], bool)
    ev, after = one(boxes, pos, prev, entity=[5, 3])
    assert ev == [[ENTER, 5, 1], [EXIT, 5, 0], [EXIT, 5, 2], [ENTER, 3, 0], [STAY, 3, 2], [EXIT, 3, 1]]
    assert after.tolist() == [[False, True, False], [True, False, True]]


def test_the_walk_meets_its_floors_on_the_reference():
    walk = Walk()
    assert len(walk.entity) == N_TRIGGERS and len(walk.descs) == N_CHARS
    boxes, positions = walk.model_boxes(), walk.model_positions()
    assert len(positions) == N_CALLS
    runs = run_reference(walk, boxes, np.ones(N_TRIGGERS, bool), positions)
    check_coverage(coverage(walk, boxes, positions, [ev for ev, _ in runs]))
    # Stay off: the same lists less their Stay rows, the same remembered sets
    quiet = run_reference(walk, boxes, np.ones(N_TRIGGERS, bool), positions, stay=False)
    for (ev, after), (ev2, after2) in zip(runs, quiet):
        assert np.array_equal(ev[ev[:, 0] != STAY], ev2) and np.array_equal(after, after2)


def test_python_surface_and_exports():
    assert (W.CHAR_TRIGGER_ENTER, W.CHAR_TRIGGER_STAY, W.CHAR_TRIGGER_EXIT, W.CHAR_TRIGGER_STAY_EVENTS) == (0, 1, 2, 1)
    for name in ("characters_watch_triggers", "characters_trigger_events", "characters_trigger_events_device", "characters_trigger_overlaps",
                 "characters_set_trigger_overlaps", "trigger_boxes"):
        assert callable(getattr(W.World, name))
    assert_exported(["bge_world_characters_watch_triggers", "bge_world_characters_trigger_events", "bge_world_characters_trigger_events_device",
                     "bge_world_characters_trigger_overlaps", "bge_world_characters_set_trigger_overlaps", "bge_world_trigger_boxes"])


def test_character_trigger_calls_reject_a_null_world():
    from banggameengine_amd import _capi
    lib = _capi.lib()
    assert lib.bge_world_characters_watch_triggers(None, 0, None, None, 0, 0) == -1
    assert lib.bge_world_characters_trigger_events(None, None, 0, None) == -1
    assert lib.bge_world_characters_trigger_events_device(None, None, None, None) == -1
    assert lib.bge_world_characters_trigger_overlaps(None, 0, None, None) == -1
    assert lib.bge_world_characters_set_trigger_overlaps(None, 0, None) == -1
    assert lib.bge_world_trigger_boxes(None, 0, None, None, None) == -1
    assert lib.bge_last_error()


def test_abi_c99_character_trigger_records(tmp_path):
    build_and_run_c99(tmp_path, "abi_check_chartrig.c", "chartrig abi ok")


def test_adapter_character_triggers_compile_on_reference_shapes(tmp_path):
    compile_reference_shapes(tmp_path, "chartrig_reference_shapes.cpp")
