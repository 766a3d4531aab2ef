"""Characters push Dynamic bodies on the device (include/bge_world.h "Character push", bge_world_characters_push ..).

Composition: world A runs characters_update(dt, steps) with push on; its twin B runs push off, one step at a time, downloads the
states, builds the records with push_ref (refmodel/impulses.py) and hands them to the public apply_impulses.  Body velocities,
activation, character states and the push records must be equal byte for byte.  apply_impulses itself is compared with the rule
in test_gpu_impulses.py.  No JUMP in these cases: the edge belongs to the first step of a call."""
from __future__ import annotations

import numpy as np
import pytest

import banggameengine_amd as B
from banggameengine_amd import world as W

from refmodel.character_cases import CHAR_SEED, DT, INPUT_SEED, REST_Y, character_batch, hand_character, input_script, inputs_of
from refmodel.character_device import read_device_into
from refmodel.device import FLAGS
from refmodel.impulses import ACTIVE_TAG, CENTRAL, IMPULSE_DTYPE, ISLAND_SLEEPING, Bodies, push_ref
from refmodel.rays import ALL, NO_ENTITY
from refmodel.step_cases import FIELD_SEED, StepField
from refmodel.step_device import field_world

pytestmark = pytest.mark.gpu

F = np.float32
FORCE, MAX_NY = 30.0, 0.5
SHUFFLE_OWN, SHUFFLE_PAD = 64, 200  # (the pair the riding tests embed their platforms with)
STATIC, DYNAMIC = W.BODY_STATIC, W.BODY_DYNAMIC
CRATE = (DYNAMIC, (0.5, 0.5, 0.5), (2.0, 0.5, 0.0), 1.0, 1)  # (type, size, position, mass, layer): its -x face is at x = 1.5


def crate_world(items, shuffled=False, sleep_first=False):
    """Bodies given one by one (entity i = item i) on the plane, ticked once so that the queries see them (or until every Dynamic
    one sleeps).  shuffled: embedded among body-less entities under a hierarchy, so that no slot is its entity's index."""
    own = len(items)
    w = B.World(device=0)
    try:
        if shuffled:
            from refmodel.layout_cases import embedded_topology
            assert own <= SHUFFLE_OWN
            w.set_topology(*embedded_topology(SHUFFLE_OWN, SHUFFLE_PAD))
        else:
            w.set_topology(np.full(own, W.NO_PARENT, np.uint32))
        n = w.n
        types = np.full(n, W.BODY_NONE, np.uint8)
        size, pos, mass, layer = np.full((n, 3), 0.5, F), np.zeros((n, 3), F), np.ones(n, F), np.ones(n, np.uint32)
        for i, (t, s, p, m, l) in enumerate(items):
            types[i], size[i], pos[i], mass[i], layer[i] = t, s, p, m, l
        w.upload_trs(pos, np.zeros((n, 3), F), np.ones((n, 3), F))
        w.upload_bodies(types, mass, np.zeros(n, np.uint8), size, layer, np.full(n, ALL, np.uint32))
        w.set_ground_plane(True)
        if sleep_first:
            w.set_sleeping(0.8, 1.0, 0.05)
            w.tick(flags=FLAGS, ticks=12)
            w.set_sleeping(0.8, 1.0, 2.0)
        else:
            w.tick(flags=FLAGS)
        w.types, w.layers = types, layer
    except Exception:
        w.close()
        raise
    return w


def body_image(w):
    pos, _ = w.download_pose()
    return Bodies(w.types, pos, group=w.layers)


def body_state(w):
    b = w.download_bodies()
    st, tm = w.download_activation()
    pos, euler = w.download_pose()
    return dict(linvel=b["linvel"], angvel=b["angvel"], quat=b["quat"], state=st, time=tm, pos=pos, euler=euler)


def assert_same(got, want, what):
    for k in want:
        assert np.ascontiguousarray(got[k]).tobytes() == np.ascontiguousarray(want[k]).tobytes(), f"{what}: {k} differs: {got[k]} vs {want[k]}"


def run_pair(items, descs, walk, steps, settle=True, force=FORCE, max_ny=MAX_NY, body_mask=0xFFFFFFFF, calls=1, world_kw=None, setup=None):
    """(A's push records, the records B built per step, the bodies' state after, the characters' states, the bodies' state before
    the walk): A with push on in `calls` calls of `steps` steps, B by composition; compared here.  setup(w) runs on both worlds once
    the set exists."""
    world_kw = world_kw or {}
    a, b = crate_world(items, **world_kw), crate_world(items, **world_kw)
    try:
        for w in (a, b):
            w.characters_create(descs)
            if setup:
                setup(w)
        a.characters_push(True, force, max_ny, body_mask)
        if settle:  # (two steps with no walk: the characters land, and nobody is pushed by a landing)
            still = np.concatenate([inputs_of()] * len(descs))
            for w in (a, b):
                w.characters_set_input(still)
                w.characters_update(DT, 2)
            assert (a.characters_push_records()["entity"] == NO_ENTITY).all()
            assert_same(body_state(a), body_state(b), "after settling")
        for w in (a, b):
            w.characters_set_input(walk)
        before = body_state(a)
        built = []
        for _ in range(calls):
            a.characters_update(DT, steps)
            for _ in range(steps):
                b.characters_update(DT, 1)
                rec = push_ref(b.characters_state(), body_image(b), DT, force, max_ny, body_mask)
                b.apply_impulses(rec)
                built.append(rec)
        got = a.characters_push_records()
        assert got.tobytes() == built[-1].tobytes(), f"push records: {got} vs {built[-1]}"
        states = a.characters_state()
        assert states.tobytes() == b.characters_state().tobytes()
        after = body_state(a)
        assert_same(after, body_state(b), "bodies")
        return got, built, after, states, before
    finally:
        a.close()
        b.close()


def walker(x=0.8, z=0.0):
    return hand_character((x, REST_Y + 0.02, z))


def walks(*xs):
    return np.concatenate([inputs_of(x) for x in xs])


def near(a, b, tol=1e-3):
    return bool((np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) <= tol).all())


def gained(after, before, e):
    return after["linvel"][e].astype(np.float64) - before["linvel"][e].astype(np.float64)


def pushed(rec):
    return rec["entity"] != NO_ENTITY


def test_a_walker_pushes_a_crate_once_per_step_of_a_call():
    got, built, after, states, before = run_pair([CRATE], walker(), walks(0.3), steps=3)
    m = F(FORCE) * F(DT)
    assert all(pushed(r).all() for r in built) and got["flags"][0] == CENTRAL and got["entity"][0] == 0
    # (the crate has settled on the plane in its first tick: its face looks along -x to within 1e-3, not exactly, and it creeps)
    assert near(got["impulse"][0], [m, 0, 0]) and near(states["hit_normal"][0], [-1, 0, 0]) and got["impulse"][0][1] == 0
    assert near(gained(after, before, 0)[0], 3 * m) and gained(after, before, 0)[1] == 0
    assert after["angvel"].tobytes() == before["angvel"].tobytes()  # a central push turns nothing
    assert after["state"][0] == ACTIVE_TAG and after["time"][0] == 0
    assert states["steps"][0] == 5


def test_two_against_one_face_add_in_character_order_and_one_from_each_side_cancels():
    wide = (DYNAMIC, (0.5, 0.5, 2.0), (2.0, 0.5, 0.0), 4.0, 1)
    descs = np.concatenate([walker(z=-0.9), walker(z=0.9)])
    got, built, after, _, before = run_pair([wide], descs, walks(0.3, 0.3), steps=1)
    m = F(FORCE) * F(DT)
    assert pushed(got).all() and near(gained(after, before, 0)[0], 2 * m * 0.25)
    descs = np.concatenate([walker(0.8), walker(3.2)])
    got, built, after, _, before = run_pair([CRATE], descs, walks(0.3, -0.3), steps=1)
    assert pushed(got).all() and near(got["impulse"][:, 0], [m, -m]) and near(gained(after, before, 0), [0, 0, 0])
    assert after["state"][0] == ACTIVE_TAG and after["time"][0] == 0  # pushed from both sides it still wakes


def test_seventy_characters_against_one_body():
    wall = (DYNAMIC, (0.5, 0.5, 45.0), (2.0, 0.5, 0.0), 7.0, 1)
    descs = np.concatenate([walker(z=-41.4 + 1.2 * i) for i in range(70)])
    got, built, after, _, before = run_pair([wall], descs, walks(*[0.3] * 70), steps=2)
    assert pushed(got).all() and (got["entity"] == 0).all() and after["linvel"][0][0] > 0


def test_who_is_not_pushed():
    """Standing on a crate (a vertical normal), a Static box, the plane, a crate outside body_mask, an INVALID character: no record,
    and the bodies keep their bytes."""
    low = (DYNAMIC, (1.0, 0.25, 1.0), (6.0, 0.25, 0.0), 1.0, 1)    # a character comes down on it
    fixed = (STATIC, (0.5, 0.5, 0.5), (2.0, 0.5, 0.0), 1.0, 1)    # a character walks into it
    other = (DYNAMIC, (0.5, 0.5, 0.5), (2.0, 0.5, 5.0), 1.0, 4)   # a crate of layer 4 against body_mask 3
    # (character 0 never grounds: it comes down on the low crate and its slides hit the top, step after step)
    descs = np.concatenate([hand_character((6.0, 1.012, 0.0), probe_distance=0.0), walker(0.8, 0.0), walker(0.8, 5.0), walker(0.8, 10.0), walker(0.8, 15.0),
                            hand_character((0.8, REST_Y + 0.002, 20.0), probe_distance=0.0)])  # (comes down on the plane, never grounds)
    walk = walks(0.0, 0.3, 0.3, 0.3, np.nan, 0.0)
    before = crate_world([low, fixed, other])
    try:
        start = body_state(before)
    finally:
        before.close()
    got, built, after, states, before = run_pair([low, fixed, other], descs, walk, steps=4, settle=False, body_mask=3)
    assert not any(pushed(r).any() for r in built)
    assert states["hit_kind"][[0, 1, 2]].tolist() == [W.RAY_BODY] * 3 and states["hit_entity"][[0, 1, 2]].tolist() == [0, 1, 2]
    assert abs(states["hit_normal"][0][1]) > 0.99 and states["flags"][4] & W.CHAR_INVALID
    assert states["hit_kind"][5] == W.RAY_GROUND and states["hit_entity"][5] == NO_ENTITY  # a hit on the plane: no record
    assert_same(after, start, "nobody was pushed")
    # the same walkers with every body in the mask: the layer-4 crate is pushed, nothing else
    got, built, after, states, before = run_pair([low, fixed, other], descs, walk, steps=4, settle=False)
    assert pushed(got).tolist() == [False, False, True, False, False, False] and got["entity"][2] == 2


def test_a_sleeping_crate_wakes():
    asleep = crate_world([CRATE], sleep_first=True)
    try:
        assert asleep.download_activation()[0][0] == ISLAND_SLEEPING
    finally:
        asleep.close()
    got, built, after, _, before = run_pair([CRATE], walker(), walks(0.3), steps=1, world_kw=dict(sleep_first=True))
    assert pushed(got).all() and after["state"][0] == ACTIVE_TAG and after["time"][0] == 0 and near(gained(after, before, 0)[0], F(FORCE) * F(DT))


def test_a_world_whose_slots_are_shuffled():
    far = (DYNAMIC, (0.5, 0.5, 0.5), (2.0, 0.5, 8.0), 2.0, 1)
    descs = np.concatenate([walker(), walker(z=8.0)])
    got, built, after, _, before = run_pair([CRATE, far], descs, walks(0.3, 0.3), steps=2, world_kw=dict(shuffled=True))
    assert pushed(got).all() and got["entity"].tolist() == [0, 1] and near(gained(after, before, 1)[0], F(FORCE) * F(DT))


def test_the_query_index_changes_no_byte():
    descs = np.concatenate([walker(z=-0.3), walker(z=0.3)])
    runs = []
    for on in (False, True):
        setup = (lambda w: w.set_query_index(True, min_work=0)) if on else None
        runs.append(run_pair([CRATE], descs, walks(0.3, 0.3), steps=2, setup=setup)[:4])
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][3].tobytes() == runs[1][3].tobytes() and pushed(runs[0][0]).all()
    assert_same(runs[1][2], runs[0][2], "query index on")


def test_riding_and_the_crowd_switched_on_together_with_push():
    """Two walkers that overlap each other (the crowd parts them at the head of every step) walk into the crate, riding on: one
    step per call in both worlds, so that Carry, Separate, the step, Push and the anchors come in the same order."""
    def setup(w):
        w.characters_ride(True, dynamic=True)
        w.characters_crowd(True)

    descs = np.concatenate([walker(0.8, -0.2), walker(0.8, 0.2)])
    a, b = crate_world([CRATE]), crate_world([CRATE])
    try:
        for w in (a, b):
            w.characters_create(descs)
            setup(w)
            w.characters_set_input(walks(0.2, 0.2))
        a.characters_push(True, FORCE, MAX_NY)
        n_pushed, parted = 0, 0
        for k in range(4):
            a.characters_update(DT, 1)
            b.characters_update(DT, 1)
            rec = push_ref(b.characters_state(), body_image(b), DT, FORCE, MAX_NY)
            b.apply_impulses(rec)
            n_pushed += int(pushed(rec).sum())
            parted += int(((b.characters_crowd_hits()["flags"] & W.CROWD_PUSHED) != 0).sum())
            assert a.characters_push_records().tobytes() == rec.tobytes(), k
            assert a.characters_state().tobytes() == b.characters_state().tobytes(), k
            assert a.characters_crowd_hits().tobytes() == b.characters_crowd_hits().tobytes(), k
            assert a.characters_rides().tobytes() == b.characters_rides().tobytes(), k
            assert_same(body_state(a), body_state(b), f"bodies after call {k}")
        assert n_pushed >= 2 and parted >= 2
    finally:
        a.close()
        b.close()


def test_lifecycle_device_form_and_errors():
    import torch
    lib = B.lib()
    w = crate_world([CRATE])
    try:
        d = np.zeros(1, W.CHARACTER_PUSH_DESC_DTYPE)

        def call(flags, force, max_ny, mask=0xFFFFFFFF):
            d[0] = (flags, force, max_ny, mask)
            return lib.bge_world_characters_push(w._h, d.ctypes.data)

        # no character set: ON is refused, off is fine, and there are no records
        assert call(1, 1.0, 0.5) == -1 and call(0, 1.0, 0.5) == 0 and lib.bge_world_characters_push(w._h, None) == -1
        assert w.characters_push_records_device() == (0, 0) and len(w.characters_push_records()) == 0
        w.characters_create(np.concatenate([walker(), walker(z=9.0)]))
        with pytest.raises(B.BgeError) as e:
            w.characters_push_records(0, 1)
        assert e.value.code == -1 and len(w.characters_push_records(0, 0)) == 0
        for flags, force, max_ny in ((2, 1.0, 0.5), (0x80000001, 1.0, 0.5), (1, -1.0, 0.5), (1, float("nan"), 0.5), (1, float("inf"), 0.5),
                                    (1, 1.0, 1.0), (1, 1.0, 1.5), (1, 1.0, -0.1), (1, 1.0, float("nan"))):
            assert call(flags, force, max_ny) == -1, (flags, force, max_ny)
        assert w.characters_push_records_device() == (0, 0)
        w.characters_push(True, FORCE)
        empty = np.zeros(2, IMPULSE_DTYPE)
        empty["entity"] = NO_ENTITY
        assert w.characters_push_records().tobytes() == empty.tobytes()  # empty before the first update
        w.characters_set_input(walks(0.0, 0.0))
        w.characters_update(DT, 2)
        w.characters_set_input(walks(0.3, 0.3))
        w.characters_update(DT, 1)
        rec = w.characters_push_records()
        assert pushed(rec).tolist() == [True, False]
        # the device form equals the download; a part of the set; ranges outside it
        ptr, n = w.characters_push_records_device()
        assert n == 2 and ptr % 4 == 0
        t = torch.zeros(2 * 32, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        w.sync()
        read_device_into(t, ptr)
        assert t.cpu().numpy().tobytes() == rec.tobytes() and w.characters_push_records(1, 1).tobytes() == rec[1:].tobytes()
        for first, count in ((0, 3), (2, 1), (1, 300)):
            with pytest.raises(B.BgeError):
                w.characters_push_records(first, count)
        # calling it again replaces the desc and keeps the records; force 0 pushes with a zero impulse (which still wakes)
        w.characters_push(True, 0.0)
        assert w.characters_push_records().tobytes() == rec.tobytes() and w.characters_push_records_device() == (ptr, 2)
        v = w.download_bodies()["linvel"].copy()
        w.characters_update(DT, 1)
        now = w.characters_push_records()
        assert pushed(now).tolist() == [True, False] and not now["impulse"].any() and w.download_bodies()["linvel"].tobytes() == v.tobytes()
        # switching off drops the records; characters_create switches off; with push off nobody is pushed
        w.characters_push(False)
        assert w.characters_push_records_device() == (0, 0)
        w.characters_push(True, FORCE)
        w.characters_create(walker())
        assert w.characters_push_records_device() == (0, 0)
        with pytest.raises(B.BgeError):
            w.characters_push_records()
        w.characters_set_input(walks(0.3))
        w.characters_update(DT, 3)
        assert w.download_bodies()["linvel"].tobytes() == v.tobytes()
    finally:
        w.close()


def test_push_switched_on_and_off_again_leaves_an_update_as_it_was():
    """The existing character walk (the step field, 257 characters, jumps included) on twin worlds: one never hears of push, the
    other has it switched on and off again before the first update.  Every state is the same bytes."""
    field = StepField(np.random.default_rng(FIELD_SEED))
    descs, heading = character_batch(np.random.default_rng(CHAR_SEED), 257, field)
    script = input_script(np.random.default_rng(INPUT_SEED), heading, 4)
    histories = []
    for touch in (False, True):
        w = field_world(field)
        try:
            w.characters_create(descs)
            if touch:
                w.characters_push(True, FORCE)
                w.characters_push(False)
            h = []
            for inp in script:
                w.characters_set_input(inp)
                w.characters_update(DT, 2)
                h.append(w.characters_state())
            histories.append(h)
        finally:
            w.close()
    for k in range(len(script)):
        assert histories[0][k].tobytes() == histories[1][k].tobytes(), k


def test_end_to_end_a_walker_shoves_a_crate_along():
    """120 frames of characters_update + tick: a walker against a 1 kg crate on the plane.  With push the crate travels along the
    walk and is awake in every frame it was pushed in; without push it does what it does with no character at all."""
    def run(push, characters=True):
        w = crate_world([CRATE])
        try:
            if characters:
                w.characters_create(walker())
                if push:
                    w.characters_push(True, FORCE)
                w.characters_set_input(walks(0.05))
            xs, awake_when_pushed, n_pushed = [], True, 0
            for _ in range(120):
                if characters:
                    w.characters_update(DT, 1)
                    if push and pushed(w.characters_push_records())[0]:
                        n_pushed += 1
                        st, tm = w.download_activation()
                        awake_when_pushed = awake_when_pushed and st[0] == ACTIVE_TAG and tm[0] == 0
                w.tick(dt=DT, flags=FLAGS)
                xs.append(w.download_pose()[0][0].copy())
            return np.array(xs), awake_when_pushed, n_pushed, (w.characters_state() if characters else None)
        finally:
            w.close()

    start = F(CRATE[2])
    xs, awake, n_pushed, state = run(True)
    print(f"pushed in {n_pushed} of 120 frames; the crate went from x = {start[0]} to {xs[-1][0]}, the walker to {state['position'][0][0]}")
    assert n_pushed >= 10 and awake
    assert xs[-1][0] > start[0]
    off, _, _, _ = run(False)
    alone, _, _, _ = run(False, characters=False)
    assert off.tobytes() == alone.tobytes() and off[-1][0] == alone[-1][0]
    print(f"without push the crate ends at {off[-1]}")
