"""Characters in a crowd on the device (include/bge_world.h "Crowd separation", bge_world_characters_crowd ..).

The reference of a step is char_ref of refmodel/characters.py over the device's own queries, applied to separate_ref
(refmodel/crowd.py) of the state the device had before the step: the device runs the same passes and the same binary32
arithmetic, so the 80-byte states and the 32-byte crowd records must be equal byte for byte after every step, through the hashed
grid (BGE_CROWD_GRID_MIN=1) and through all pairs alike."""
from __future__ import annotations

import numpy as np
import pytest

import banggameengine_amd as B
from banggameengine_amd import world as W

from refmodel.characters import char_ref, fresh_state
from refmodel.character_cases import DT, REST_Y, TABLE, hand_character, inputs_of
from refmodel.character_device import device_pen, read_device_into
from refmodel.crowd import PUSHED, crowd_ref, make_spheres, separate_ref
from refmodel.crowd_cases import CROWD_CHAR_SEED, CROWD_CHARS, CROWD_MAX_PUSH, CROWD_STEPS, crowd_walkers, lattice_walkers
from refmodel.device import device_caster
from refmodel.ride_device import device_poses, repose
from refmodel.rides import BODY_STATIC, CARRIED, anchor_ref, carry_ref, fresh_rides
from refmodel.step_cases import FIELD_SEED, NO_ROT, StepField
from refmodel.step_device import field_world, hand_world

pytestmark = pytest.mark.gpu

PATHS = {"grid": "1", "all pairs": str(1 << 31)}


@pytest.fixture(params=list(PATHS))
def path(request, monkeypatch):
    monkeypatch.setenv("BGE_CROWD_GRID_MIN", PATHS[request.param])
    return request.param


def assert_equal_records(got, want, what):
    bad = [i for i in range(len(want)) if got[i].tobytes() != want[i].tobytes()]
    assert not bad, f"{what}: {len(bad)} of {len(want)} differ, first {bad[0]}: {got[bad[0]]} vs {want[bad[0]]}"


class Shared:
    """The step field as a world, the walkers and their script, and the reference's answer for every step from the device's
    state before it: made once by the first path that runs and compared by both."""

    def __init__(self):
        self.w = field_world(StepField(np.random.default_rng(FIELD_SEED)))
        self.descs, self.group, self.mask, self.script = crowd_walkers(np.random.default_rng(CROWD_CHAR_SEED))
        self.want = None

    def run(self):
        """The states and crowd records after every step of the script, one update call per step."""
        w = self.w
        w.characters_create(self.descs)
        w.characters_crowd(True, CROWD_MAX_PUSH, self.group, self.mask)
        out = []
        for inp in self.script:
            w.characters_set_input(inp)
            w.characters_update(DT, 1)
            out.append((w.characters_state(), w.characters_crowd_hits()))
        return out

    def reference(self, got):
        if self.want is None:
            cast_fn, pen_fn = device_caster(self.w), device_pen(self.w)
            self.want, before = [], fresh_state(self.descs)
            for k, inp in enumerate(self.script):
                parted, hits = separate_ref(self.descs, before, self.group, self.mask, CROWD_MAX_PUSH)
                self.want.append((char_ref(cast_fn, pen_fn, self.descs, inp.copy(), parted, DT, True), hits))
                before = got[k][0]
        return self.want


@pytest.fixture(scope="module")
def shared():
    s = Shared()
    yield s
    s.w.close()


def test_every_step_equals_the_rule_over_separate_of_the_state_before(shared, path):
    got = shared.run()
    want = shared.reference(got)
    pushed = 0
    for k in range(CROWD_STEPS):
        assert_equal_records(got[k][1], want[k][1], f"crowd records of step {k}")
        assert_equal_records(got[k][0], want[k][0], f"states after step {k}")
        pushed += int(((got[k][1]["flags"] & PUSHED) != 0).sum())
    print(f"{path}: {pushed} pushes over {CROWD_STEPS} steps of {CROWD_CHARS} characters")
    assert pushed >= CROWD_CHARS * CROWD_STEPS // 4 and (got[-1][1]["n_overlaps"] >= 2).any()
    assert not (got[-1][0]["flags"] & W.CHAR_INVALID).any()


def test_one_call_of_eight_steps_equals_eight_calls_of_one(shared, path):
    w, inp = shared.w, shared.script[0].copy()
    inp["buttons"] = 0  # (the JUMP edge is the first step's alone: its own test is in test_gpu_characters.py)
    ends = []
    for calls, steps in ((1, 8), (8, 1)):
        w.characters_create(shared.descs)
        w.characters_crowd(True, CROWD_MAX_PUSH, shared.group, shared.mask)
        w.characters_set_input(inp)
        for _ in range(calls):
            w.characters_update(DT, steps)
        ends.append((w.characters_state(), w.characters_crowd_hits()))
    assert ends[0][0].tobytes() == ends[1][0].tobytes() and ends[0][1].tobytes() == ends[1][1].tobytes()
    assert (ends[0][1]["flags"] & PUSHED).any() and (ends[0][0]["steps"] == 8).all()


def test_a_set_in_which_nobody_overlaps_is_untouched(shared, path):
    descs, script = lattice_walkers(np.random.default_rng(CROWD_CHAR_SEED + 1))
    w = shared.w
    runs = []
    for on in (False, True):
        w.characters_create(descs)
        if on:
            w.characters_crowd(True)
        states = []
        for inp in script:
            w.characters_set_input(inp)
            w.characters_update(DT, 1)
            states.append(w.characters_state())
            if on:
                h = w.characters_crowd_hits()
                assert not h["flags"].any() and (h["other"] == W.RAY_NO_ENTITY).all()
        runs.append(states)
    # the reference first: over the positions every Separate saw, nobody overlaps
    before = fresh_state(descs)
    for k, after in enumerate(runs[0]):
        assert not crowd_ref(make_spheres(before["position"], descs["radius"]))["n_overlaps"].any(), k
        before = after
    for k in range(len(script)):
        assert runs[0][k].tobytes() == runs[1][k].tobytes(), k
    assert np.signbit(descs["position"][:, 0]).any()  # (-0 coordinates among them)


def test_separate_sees_the_carried_positions(path):
    """Two characters ride a table that moves 0.5 towards two that stand on a second table beside it: 1.3 apart before the
    carry, 0.8 after it, so Separate parts them only if it runs on the carried positions."""
    beside = (TABLE[0], TABLE[1], (4.5, 0.5, 0.0), NO_ROT)  # x from 2.5 to 6.5, the same top
    w = hand_world([TABLE, beside], (), True)
    try:
        y = 1.0 + REST_Y
        descs = np.concatenate([hand_character((1.5, y + 0.01, -1.0)), hand_character((1.5, y + 0.01, 1.0)),
                                hand_character((2.8, y + 0.01, -1.0)), hand_character((2.8, y + 0.01, 1.0))])
        types = np.uint8([BODY_STATIC, BODY_STATIC])
        cast_fn, pen_fn = device_caster(w), device_pen(w)
        w.characters_create(descs)
        w.characters_ride()
        w.characters_crowd(True)
        still = np.concatenate([inputs_of()] * 4)
        w.characters_set_input(still)
        w.characters_update(DT, 2)  # they land, and the riders are anchored
        state, rides = w.characters_state(), w.characters_rides()
        assert rides["entity"].tolist() == [0, 0, 1, 1] and not w.characters_crowd_hits()["flags"].any()
        repose(w, np.uint32([0]), np.float32([(0.5, 0.5, 0.0)]), np.float32([NO_ROT]))
        w.characters_update(DT, 1)
        poses = device_poses(w, types)
        carried, want_rides = carry_ref(state, rides, poses)
        assert (carried["position"][:2, 0] == 2.0).all() and (carried["position"][2:, 0] == state["position"][2:, 0]).all()
        parted, want_hits = separate_ref(descs, carried)
        want = char_ref(cast_fn, pen_fn, descs, still.copy(), parted, DT, True)
        got, hits = w.characters_state(), w.characters_crowd_hits()
        assert_equal_records(hits, want_hits, "crowd records")
        assert_equal_records(got, want, "states")
        assert_equal_records(w.characters_rides(), anchor_ref(want, want_rides, poses), "ride records")
        assert hits["other"].tolist() == [2, 3, 0, 1] and (abs(hits["depth"] - 0.2) <= 1e-6).all()
        assert (w.characters_rides()["flags"][:2] == CARRIED).all()
    finally:
        w.close()


def test_a_trigger_watch_reports_from_the_pushed_positions(path):
    """A trigger box from x = 2.5 and up to z = 0.5.  Character 0 (radius 0.5) at x = 1.85, z = 0.9 reaches x = 2.37 with its box:
    outside.  Character 1 at x = 1.25 overlaps it by 0.4 and pushes it 0.2 along +x: its box reaches 2.57, inside, while the
    sphere stays 0.6 from the volume's edge (the queries see ghosts: one it touched would stop it).  It Enters only with the
    crowd on."""
    ghost = (False, (0.5, 0.5, 0.5), (3.0, 0.5, 0.0), NO_ROT)
    w = hand_world([ghost], (0,), True)
    try:
        descs = np.concatenate([hand_character((1.85, REST_Y, 0.9)), hand_character((1.25, REST_Y, 0.9))])
        seen = []
        for on in (False, True):
            w.characters_create(descs)
            w.characters_watch_triggers()
            if on:
                w.characters_crowd(True)
            w.characters_update(DT, 1)
            seen.append(w.characters_trigger_events().tolist())
            x = w.characters_state()["position"][:, 0]
            assert abs(x[0] - (2.05 if on else 1.85)) <= 1e-6 and abs(x[1] - (1.05 if on else 1.25)) <= 1e-6
        assert seen == [[], [[W.CHAR_TRIGGER_ENTER, 0, 0]]]
    finally:
        w.close()


def test_two_characters_walking_head_on_never_overlap_deeper_than_one_steps_walk(path):
    """Separate parts them to touching (what is left is rounding: 4 ulp of their distance 1, as the hand case of the level pair)
    and the step then walks them 0.05 each towards each other: 0.1 is the deepest they can be found."""
    w = hand_world([], (), True)
    try:
        w.characters_create(np.concatenate([hand_character((-1.0, REST_Y, 0.0)), hand_character((1.0, REST_Y, 0.0))]))
        w.characters_crowd(True)
        w.characters_set_input(np.concatenate([inputs_of(0.05), inputs_of(-0.05)]))
        deepest, met = 0.0, 0
        for _ in range(30):
            w.characters_update(DT, 1)
            p = w.characters_state()["position"].astype(np.float64)
            depth = 1.0 - float(np.linalg.norm(p[0] - p[1]))
            deepest = max(deepest, depth)
            met += int((w.characters_crowd_hits()["flags"] & PUSHED).all())
        print(f"{path}: deepest overlap {deepest:.9f}, parted in {met} of 30 steps")
        assert met >= 15 and deepest > 0.05
        assert deepest <= 0.1 + 4 * float(np.spacing(np.float32(1.0)))
    finally:
        w.close()


def test_lifecycle_device_form_and_errors():
    import torch
    w = hand_world([], (), True)
    lib = B.lib()
    try:
        # no character set: ON is refused, off is fine, and there are no records
        assert lib.bge_world_characters_crowd(w._h, 1, 0.0, 0, None, None) == -1 and lib.bge_world_characters_crowd(w._h, 0, 0.0, 0, None, None) == 0
        assert w.characters_crowd_hits_device() == (0, 0) and len(w.characters_crowd_hits()) == 0
        descs = np.concatenate([hand_character((0.0, REST_Y, 0.0)), hand_character((0.6, REST_Y, 0.0)), hand_character((9.0, REST_Y, 0.0))])
        w.characters_create(descs)
        with pytest.raises(B.BgeError) as e:
            w.characters_crowd_hits(0, 1)
        assert e.value.code == -1 and len(w.characters_crowd_hits(0, 0)) == 0
        for flags, max_push, n in ((2, 0.0, 3), (0x80000001, 0.0, 3), (1, 0.0, 2), (1, 0.0, 4), (1, float("nan"), 3), (1, -0.5, 3), (1, float("inf"), 3)):
            assert lib.bge_world_characters_crowd(w._h, flags, max_push, n, None, None) == -1, (flags, max_push, n)
        assert w.characters_crowd_hits_device() == (0, 0)
        w.characters_crowd(True)
        assert not w.characters_crowd_hits().view(np.uint32).any()  # all words 0 before the first update
        w.characters_update(DT, 1)
        h = w.characters_crowd_hits()
        assert h["flags"].tolist() == [PUSHED, PUSHED, 0] and h["other"].tolist() == [1, 0, W.RAY_NO_ENTITY]
        # the device form equals the download; a part of the set; ranges outside it
        ptr, n = w.characters_crowd_hits_device()
        assert n == 3 and ptr % 4 == 0
        t = torch.zeros(3 * 32, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        w.sync()
        read_device_into(t, ptr)
        assert t.cpu().numpy().tobytes() == h.tobytes() and w.characters_crowd_hits(1, 2).tobytes() == h[1:].tobytes()
        for first, count in ((0, 4), (3, 1), (2, 300)):
            with pytest.raises(B.BgeError):
                w.characters_crowd_hits(first, count)
        # calling it again replaces the filters and max_push and keeps the records
        w.characters_crowd(True, 0.01, group=[1, 2, 1], mask=[1, 2, 1])
        assert w.characters_crowd_hits().tobytes() == h.tobytes() and w.characters_crowd_hits_device() == (ptr, 3)
        w.characters_warp([1], [(0.6, REST_Y, 0.0)])
        w.characters_warp([0], [(0.0, REST_Y, 0.0)])
        w.characters_update(DT, 1)
        assert not w.characters_crowd_hits()["flags"].any()  # 0 and 1 no longer see each other
        w.characters_crowd(True, 0.01)
        w.characters_update(DT, 1)
        h = w.characters_crowd_hits()
        assert (h["flags"][:2] == W.CROWD_PUSHED | W.CROWD_CLAMPED).all() and h["push"][:2, 0].tolist() == [np.float32(-0.01), np.float32(0.01)]
        # switching off drops the records; characters_create switches off
        w.characters_crowd(False)
        assert w.characters_crowd_hits_device() == (0, 0)
        w.characters_crowd(True)
        w.characters_create(descs)
        assert w.characters_crowd_hits_device() == (0, 0)
        with pytest.raises(B.BgeError):
            w.characters_crowd_hits()
        before = w.characters_state()
        w.characters_update(DT, 1)  # with the crowd off nobody is parted
        after = w.characters_state()
        assert after["position"][:, 0].tobytes() == before["position"][:, 0].tobytes()
    finally:
        w.close()
