"""Character trigger events on the device (include/bge_world.h "Character trigger events", bge_world_characters_watch_triggers ..).

The reference is char_trigger_ref of refmodel/char_triggers.py — the header's rule in numpy, the character box in binary32 — over
the device's own trigger boxes (World.trigger_boxes) and the positions it downloads after every call: the device runs the same
binary32 arithmetic, so the lists must be equal row for row and in order, and the remembered pairs equal.  The walk, its filters and
the coverage floors are those test_char_triggers_cpu.py checks on the reference alone."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import banggameengine_amd as B
from banggameengine_amd.world import make_character_inputs, make_characters

from refmodel.device import FLAGS
from refmodel.char_triggers import ENTER, EXIT, STAY, char_trigger_ref, filter_pass, pairs_of
from refmodel.char_trigger_cases import (BATCHES, DT, N_CHARS, N_TRIGGERS, NOBODY, STEPS_PER_CALL, TRIGGER_COUNTS, Walk, check_coverage, coverage)
from refmodel.char_trigger_device import one_call, run_walk, trigger_world, upload_walk_triggers
from refmodel.character_device import read_device_into

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = 0xFFFFFFFF


def reference_call(walk, order, boxes, listed, pos, n, prev, stay=True, group=None, cmask=None, mask=None):
    """char_trigger_ref for the triggers order[k] of the walk (the uploaded array's order), named by their entities."""
    order = np.asarray(order, np.int64)
    return char_trigger_ref(boxes, listed, walk.layer[order], (walk.mask if mask is None else mask)[order], pos, walk.descs["radius"][:n],
                            walk.group[:n] if group is None else group, walk.cmask[:n] if cmask is None else cmask, prev, stay, walk.entity[order])


def check_run(w, walk, order, n, got, stay=True):
    """Every call of a run equals the reference over the device's boxes and positions, from nothing remembered."""
    boxes, listed = w.trigger_boxes(walk.entity[order])
    assert listed.all() and np.isfinite(boxes).all()
    prev = np.zeros((len(order), n), bool)
    for call, (ev, pos, pairs) in enumerate(got):
        want, prev = reference_call(walk, order, boxes, listed, pos, n, prev, stay)
        assert ev.shape == want.shape and np.array_equal(ev, want), (call, len(ev), len(want), ev[:5], want[:5])
        assert np.array_equal(pairs, pairs_of(prev, walk.entity[order])), call
        assert pairs[:, 1].max(initial=0) < n
    return prev


class Shared:
    """The walk, its world ticked once, and the device's answers for all the characters after every call: made once, never
    changed (the tests that edit the trigger set make their own world)."""

    def __init__(self):
        self.walk = Walk()
        self.order = np.arange(N_TRIGGERS)
        self.w = trigger_world(self.walk)
        self.boxes, self.listed = self.w.trigger_boxes(self.walk.entity)
        self.got = run_walk(self.w, self.walk, N_CHARS)
        self.state_bytes = self.w.characters_state().tobytes()


@pytest.fixture(scope="module")
def shared():
    s = Shared()
    yield s
    s.w.close()


@pytest.mark.parametrize("n", BATCHES)
def test_the_walk_equals_the_rule_row_for_row(shared, n):
    w, walk = shared.w, shared.walk
    got = shared.got if n == N_CHARS else run_walk(w, walk, n)
    prev = check_run(w, walk, shared.order, n, got)
    if n == N_CHARS:
        check_coverage(coverage(walk, shared.boxes, [pos for _, pos, _ in got], [ev for ev, _, _ in got]))
        return
    # the tail bits of the last word: character n - 1 inside a volume whose filter it passes, and no pair names an index >= n
    passes = filter_pass(walk.layer, walk.mask, walk.group[:n], walk.cmask[:n])[:, n - 1]
    t = int(np.nonzero(passes)[0][0])
    w.characters_warp([n - 1], [walk.pos[t]])
    w.characters_set_input(make_character_inputs(np.zeros(n), 0.0))
    w.characters_update(DT, 1)
    ev, pos, pairs = w.characters_trigger_events(), w.characters_state()["position"], w.characters_trigger_overlaps()
    want, after = reference_call(walk, shared.order, shared.boxes, shared.listed, pos, n, prev)
    assert np.array_equal(ev, want) and np.array_equal(pairs, pairs_of(after, walk.entity))
    assert [t, n - 1] in pairs.tolist() and pairs[:, 1].max() == n - 1


@pytest.mark.parametrize("n_triggers", [t for t in TRIGGER_COUNTS if t != N_TRIGGERS])
def test_one_and_two_triggers(n_triggers):
    """(All 70, which also cross the 64 ghosts a workgroup stages in LDS, are the walk above.)"""
    walk = Walk()
    w = trigger_world(walk, n_triggers)
    try:
        boxes, listed = w.trigger_boxes(walk.entity)
        assert listed.tolist() == [True] * n_triggers + [False] * (N_TRIGGERS - n_triggers)
        assert np.array_equal(boxes[n_triggers:], np.tile(np.float32([np.inf] * 3 + [-np.inf] * 3), (N_TRIGGERS - n_triggers, 1)))
        got = run_walk(w, walk, N_CHARS)
        check_run(w, walk, np.arange(n_triggers), N_CHARS, got)
        assert sum(len(ev) for ev, _, _ in got) > 0
    finally:
        w.close()


class Thin:
    """One thin volume, half extents (0.1, 1, 1) at (0, 1, 0): fed as x in [-0.12, 0.12]."""
    entity = np.uint32([0])
    size, pos, euler = np.float32([[0.1, 1, 1]]), np.float32([[0, 1, 0]]), np.float32([[0, 0, 0]])
    layer, mask = np.uint32([4]), np.uint32([ALL])


def thin_character(x):
    return make_characters([[x, 1.0, 0.0]], radius=0.3, gravity=0.0, layer_mask=NOBODY)


def test_one_call_of_three_steps_reports_the_state_after_the_third():
    """The character (box +-0.32 about its centre) walks 1.5 a step from x = -3: -1.5, 0, 1.5.  It is inside the volume after step 2
    alone."""
    w = trigger_world(Thin)
    try:
        w.characters_create(thin_character(-3.0))
        w.characters_watch_triggers()
        w.characters_set_input(make_character_inputs([1.5], 0.0))
        w.characters_update(DT, 3)
        assert w.characters_state()["position"][0].tolist() == pytest.approx([1.5, 1.0, 0.0], abs=1e-5)
        assert len(w.characters_trigger_events()) == 0 and len(w.characters_trigger_overlaps()) == 0
        w.characters_create(thin_character(-3.0))
        w.characters_watch_triggers()
        w.characters_set_input(make_character_inputs([1.5], 0.0))
        lists = []
        for _ in range(3):
            w.characters_update(DT, 1)
            lists.append(w.characters_trigger_events().tolist())
        assert lists == [[], [[ENTER, 0, 0]], [[EXIT, 0, 0]]]
    finally:
        w.close()


def device_list(w):
    """(count, the records the device list holds, capacity) read through the device pointers after an explicit stream sync."""
    import torch
    w.sync()
    ev_ptr, count_ptr, cap = w.characters_trigger_events_device()
    assert ev_ptr and count_ptr and ev_ptr % 4 == 0
    count = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    read_device_into(count, count_ptr)
    count = int(count.cpu().numpy().view(np.uint32)[0])
    held = torch.zeros(3 * min(count, cap), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    if held.numel():
        read_device_into(held, ev_ptr)
    return count, held.cpu().numpy().view(np.uint32).reshape(-1, 3), cap


def test_overflow_loses_nothing_and_the_next_call_is_right(shared):
    w, walk = shared.w, shared.walk
    assert len(shared.got[0][0]) > 4 and len(shared.got[1][0]) > len(shared.got[0][0])
    w.characters_create(walk.descs)
    w.characters_watch_triggers(walk.group, walk.cmask, True, 4)
    assert w.characters_trigger_events_device()[2] == 4
    for call in range(2):
        w.characters_set_input(walk.inputs(call))
        w.characters_update(DT, STEPS_PER_CALL)
        want = shared.got[call][0]
        count, held, cap = device_list(w)
        assert count == len(want) and cap < count  # (call 1 finds more than call 0 grew the list to)
        assert np.array_equal(held, want[:cap])
        assert np.array_equal(w.characters_trigger_events(), want)  # the whole list, in order
        assert w.characters_trigger_events_device()[2] == len(want)  # the new capacity stays
        assert np.array_equal(w.characters_trigger_events(), want)  # fetching does not clear it
        assert np.array_equal(device_list(w)[1], want)
        assert np.array_equal(w.characters_trigger_overlaps(), shared.got[call][2])
    w.characters_watch_triggers(walk.group, walk.cmask, True, 4)  # (watching again never shrinks the list)
    assert w.characters_trigger_events_device()[2] == len(shared.got[1][0])
    got = one_call(w, walk, 2, N_CHARS)
    assert np.array_equal(got[0], shared.got[2][0]) and np.array_equal(got[2], shared.got[2][2])


def test_stay_off_is_the_stay_on_list_less_its_stay_rows(shared):
    got = run_walk(shared.w, shared.walk, N_CHARS, stay=False, calls=6)
    for (ev, pos, pairs), (full, full_pos, full_pairs) in zip(got, shared.got):
        assert np.array_equal(pos, full_pos) and np.array_equal(pairs, full_pairs)
        assert np.array_equal(ev, full[full[:, 0] != STAY]) and (full[:, 0] == STAY).any() == (len(full) != len(ev))
    assert sum(int((full[:, 0] == STAY).sum()) for full, _, _ in shared.got[:6]) >= 100


def test_new_filters_keep_the_remembered_sets_and_a_pair_that_no_longer_passes_exits(shared):
    w, walk, n = shared.w, shared.walk, N_CHARS
    got = run_walk(w, walk, n, calls=4)
    prev = check_run(w, walk, shared.order, n, got)
    group = walk.group.copy()
    group[::2] = 0  # every other character now overlaps nothing
    w.characters_watch_triggers(group, walk.cmask)
    assert np.array_equal(w.characters_trigger_overlaps(), got[-1][2]) and np.array_equal(w.characters_trigger_events(), got[-1][0])
    w.characters_set_input(make_character_inputs(np.zeros(n), 0.0))
    w.characters_update(DT, 1)
    ev, pos = w.characters_trigger_events(), w.characters_state()["position"]
    assert np.array_equal(pos, got[-1][1])  # nobody moved
    want, after = reference_call(walk, shared.order, shared.boxes, shared.listed, pos, n, prev, group=group)
    assert np.array_equal(ev, want) and np.array_equal(w.characters_trigger_overlaps(), pairs_of(after, walk.entity))
    exits = ev[ev[:, 0] == EXIT]
    assert len(exits) >= 10 and (exits[:, 2] % 2 == 0).all() and not (ev[ev[:, 0] != EXIT][:, 2] % 2 == 0).any()
    assert (ev[:, 0] == STAY).sum() >= 10 and not (ev[:, 0] == ENTER).any()


def test_upload_triggers_between_calls():
    """The uploaded array is reversed, one trigger is removed, one gets another mask and one is new: kept triggers give Stay, the
    order follows the new array, the removed one gives no Exit, the one with the changed mask starts empty; before the next tick
    nothing is reported and nothing forgotten."""
    walk = Walk(n_triggers=N_TRIGGERS + 1)
    T, n = N_TRIGGERS, N_CHARS
    w = trigger_world(walk, T)  # (entity T is not a trigger yet)
    try:
        first = np.arange(T)
        got = run_walk(w, walk, n, calls=4)
        prev = check_run(w, walk, first, n, got)
        held = np.nonzero(prev.any(axis=1))[0]
        assert len(held) >= 10
        removed, changed = int(held[0]), int(held[1])
        mask = walk.mask.copy()
        mask[changed] = ALL if walk.mask[changed] != ALL else 0x7FFFFFFF  # (still sees the groups 2 and 8: the pairs come back)
        order = np.array([T] + [t for t in first[::-1] if t != removed])
        upload_walk_triggers(w, walk, order, mask=mask)
        carried = np.zeros((len(order), n), bool)
        for k, t in enumerate(order):
            if t != T and t != changed:
                carried[k] = prev[t]
        assert np.array_equal(w.characters_trigger_overlaps(), pairs_of(carried, walk.entity[order]))
        # between the upload and the next tick no ghost is posed: nothing is reported and nothing forgotten
        assert not w.trigger_boxes(walk.entity)[1].any()
        w.characters_set_input(make_character_inputs(np.zeros(n), 0.0))
        w.characters_update(DT, 1)
        assert len(w.characters_trigger_events()) == 0
        assert np.array_equal(w.characters_trigger_overlaps(), pairs_of(carried, walk.entity[order]))
        w.tick(flags=FLAGS)
        boxes, listed = w.trigger_boxes(walk.entity[order])
        assert listed.all()
        w.characters_update(DT, 1)
        ev, pos = w.characters_trigger_events(), w.characters_state()["position"]
        want, after = reference_call(walk, order, boxes, listed, pos, n, carried, mask=mask)
        assert np.array_equal(ev, want) and np.array_equal(w.characters_trigger_overlaps(), pairs_of(after, walk.entity[order]))
        assert not (ev[:, 1] == removed).any()
        of_changed = ev[ev[:, 1] == changed]
        assert len(of_changed) >= int(prev[changed].sum()) >= 1 and (of_changed[:, 0] == ENTER).all()
        kept = ev[(ev[:, 1] != changed) & (ev[:, 1] != T)]
        assert (kept[:, 0] == STAY).sum() >= 10 and not (kept[:, 0] == ENTER).any()  # (nobody moved since the last call)
        position_in_array = {int(e): k for k, e in enumerate(walk.entity[order])}
        assert np.all(np.diff([position_in_array[int(e)] for e in ev[:, 1]]) >= 0)
    finally:
        w.close()


def test_an_inactive_trigger_is_skipped_and_its_characters_stay_when_it_comes_back():
    walk = Walk()
    T, n = N_TRIGGERS, N_CHARS
    w = trigger_world(walk)
    try:
        order = np.arange(T)
        got = run_walk(w, walk, n, calls=4)
        prev = check_run(w, walk, order, n, got)
        off = int(np.nonzero(prev.any(axis=1))[0][0])
        active = np.ones(T, np.uint8)
        active[off] = 0
        w.characters_set_input(make_character_inputs(np.zeros(n), 0.0))
        for state in (active, np.ones(T, np.uint8)):
            upload_walk_triggers(w, walk, order, active=state)
            w.tick(flags=FLAGS)
            boxes, listed = w.trigger_boxes(walk.entity)
            assert listed.tolist() == state.astype(bool).tolist()
            w.characters_update(DT, 1)
            ev, pos = w.characters_trigger_events(), w.characters_state()["position"]
            want, after = reference_call(walk, order, boxes, listed, pos, n, prev)
            assert np.array_equal(ev, want) and np.array_equal(w.characters_trigger_overlaps(), pairs_of(after, walk.entity))
            assert np.array_equal(after, prev)  # nobody moved: the skipped trigger's set stays, and so does every other
            of_off = ev[ev[:, 1] == off]
            if state[off]:
                assert len(of_off) == prev[off].sum() and (of_off[:, 0] == STAY).all()
            else:
                assert len(of_off) == 0
    finally:
        w.close()


def test_warp_into_a_volume_and_out_of_it():
    w = trigger_world(Thin)
    try:
        w.characters_create(thin_character(-3.0))
        w.characters_watch_triggers()
        lists = []
        for x in (-3.0, 0.0, 0.0, 5.0, 5.0):
            w.characters_warp([0], [[x, 1.0, 0.0]])
            w.characters_update(DT, 1)
            lists.append(w.characters_trigger_events().tolist())
        assert lists == [[], [[ENTER, 0, 0]], [[STAY, 0, 0]], [[EXIT, 0, 0]], []]
    finally:
        w.close()


def test_characters_create_turns_the_watch_off(shared):
    w, walk = shared.w, shared.walk
    run_walk(w, walk, 65, calls=2)
    assert len(w.characters_trigger_events()) and len(w.characters_trigger_overlaps()) and w.characters_trigger_events_device()[0]
    w.characters_create(walk.descs[:65])
    assert len(w.characters_trigger_events()) == 0 and len(w.characters_trigger_overlaps()) == 0
    assert w.characters_trigger_events_device() == (0, 0, 0)
    w.characters_set_input(walk.inputs(0, 65))
    w.characters_update(DT, STEPS_PER_CALL)
    assert len(w.characters_trigger_events()) == 0 and len(w.characters_trigger_overlaps()) == 0


def test_overlaps_round_trip_and_the_errors_of_every_call(shared):
    w, walk, n = shared.w, shared.walk, 65
    got = run_walk(w, walk, n, calls=3)
    pairs = got[-1][2]
    assert len(pairs) >= 5
    w.characters_set_trigger_overlaps(pairs[::-1])  # (any order in, the rule's order out)
    assert np.array_equal(w.characters_trigger_overlaps(), pairs)
    some = np.uint32([[walk.entity[3], 64], [walk.entity[3], 0], [walk.entity[69], 63]])
    w.characters_set_trigger_overlaps(some)
    assert w.characters_trigger_overlaps().tolist() == [[3, 0], [3, 64], [69, 63]]
    # the next call takes them as remembered
    w.characters_set_input(make_character_inputs(np.zeros(n), 0.0))
    w.characters_update(DT, 1)
    prev = np.zeros((N_TRIGGERS, n), bool)
    prev[3, 0] = prev[3, 64] = prev[69, 63] = True
    want, after = reference_call(walk, shared.order, shared.boxes, shared.listed, w.characters_state()["position"], n, prev)
    assert np.array_equal(w.characters_trigger_events(), want) and np.array_equal(w.characters_trigger_overlaps(), pairs_of(after, walk.entity))
    before = w.characters_trigger_overlaps()
    for bad in ([[3, 65]], [[N_TRIGGERS, 0]], [[3, 0], [0xFFFFFFFF, 0]]):
        with pytest.raises(B.BgeError) as e:
            w.characters_set_trigger_overlaps(np.uint32(bad))
        assert e.value.code == -1
    assert np.array_equal(w.characters_trigger_overlaps(), before)  # a refused set leaves the old one
    w.characters_set_trigger_overlaps(np.zeros((0, 2), np.uint32))
    assert len(w.characters_trigger_overlaps()) == 0
    lib, ok = B.lib(), np.zeros(n, np.uint32)
    total = C.c_uint64(0)
    assert lib.bge_world_characters_watch_triggers(w._h, n - 1, None, None, 1, 0) == -1  # a wrong n
    assert lib.bge_world_characters_watch_triggers(w._h, n + 1, ok.ctypes.data, ok.ctypes.data, 1, 0) == -1
    assert lib.bge_world_characters_watch_triggers(w._h, n, None, None, 2, 0) == -1      # an unknown flag bit
    assert lib.bge_world_characters_trigger_events(w._h, None, 0, None) == -1
    assert lib.bge_world_characters_trigger_events_device(w._h, None, None, None) == -1
    assert lib.bge_world_characters_trigger_overlaps(w._h, 0, None, None) == -1
    assert lib.bge_world_characters_set_trigger_overlaps(w._h, 1, None) == -1
    assert lib.bge_world_trigger_boxes(w._h, 1, None, None, None) == -1
    assert lib.bge_world_characters_trigger_events(w._h, None, 0, C.byref(total)) == 0 and total.value == len(want)  # the watch is still on
    boxes, listed = w.trigger_boxes([3, N_TRIGGERS + 5, 0xFFFFFFF0])
    assert listed.tolist() == [True, False, False] and np.array_equal(boxes[0], shared.boxes[3]) and boxes[1].tolist() == [np.inf] * 3 + [-np.inf] * 3
    assert lib.bge_world_characters_watch_triggers(w._h, 0, None, None, 0, 0) == 0  # n = 0 turns the watch off
    assert w.characters_trigger_events_device() == (0, 0, 0) and len(w.characters_trigger_events()) == 0
    with pytest.raises(B.BgeError):
        w.characters_set_trigger_overlaps(np.uint32([[3, 0]]))  # every index is outside the set while the watch is off


def test_the_watch_changes_nothing_it_does_not_own(shared):
    got = run_walk(shared.w, shared.walk, N_CHARS, watch=False)
    assert shared.w.characters_state().tobytes() == shared.state_bytes
    assert all(len(ev) == 0 and len(pairs) == 0 for ev, _, pairs in got)
    assert all(np.array_equal(pos, want) for (_, pos, _), (_, want, _) in zip(got, shared.got))


def test_the_device_forms_equal_the_host_fetch(shared):
    """characters_update with the watch on synchronises nothing of its own (bge_world.cpp chartrig_enqueue: a copy, four launches
    and no read): the count and the list are read through the device pointers only after an explicit stream sync."""
    w, walk, n = shared.w, shared.walk, N_CHARS
    w.characters_create(walk.descs)
    w.characters_watch_triggers(walk.group, walk.cmask)
    for call in range(2):
        w.characters_set_input(walk.inputs(call))
        w.characters_update(DT, STEPS_PER_CALL)
        count, held, cap = device_list(w)
        assert cap == n + 1024 and count == len(shared.got[call][0])
        assert np.array_equal(held, shared.got[call][0]) and np.array_equal(w.characters_trigger_events(), held)


def test_adapter_character_triggers_on_demo_scene(tmp_path):
    cpp = os.path.join(ROOT, "tests", "cpp")
    lib = os.path.join(ROOT, "banggameengine_amd")
    exe = str(tmp_path / "chartrig_demo_scene")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unused-parameter", "-o", exe,
                           os.path.join(cpp, "chartrig_demo_scene.cpp"), f"-L{lib}", "-lbge_world", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "demo_scene.json")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "all checks passed" in r.stdout
