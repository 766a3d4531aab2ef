"""Character platform riding on the device (include/bge_world.h "Character platform riding", bge_world_characters_ride ..).

The reference is ride_run_ref of refmodel/rides.py — Carry, the steps of char_ref and Anchor in numpy float32 scalars — with
World.sphere_cast and World.sphere_penetration on the same world as its caster and penetration function and the device's own poses
(World.download_pose, World.download_bodies) as the bodies: the device runs the same passes and the same binary32 arithmetic, so
the 80-byte states and the 64-byte ride records must be equal byte for byte after every call.  The platform field, its characters,
its scripts and its coverage floors are those test_character_rides_cpu.py checks on the float64 shape reference alone."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import banggameengine_amd as B
from banggameengine_amd import world as W

from refmodel.rays import box_half_extents
from refmodel.rides import BODY_NONE, BODY_STATIC, CARRIED, LOST, fresh_rides
from refmodel.step_cases import FIELD_SEED as STEP_FIELD_SEED, NO_ROT, StepField
from refmodel.character_cases import CHAR_SEED, DT, INPUT_SEED, N_STEPS, REST_Y, TABLE, character_batch, hand_character, input_script
from refmodel.ride_cases import (BATCHES, N_CALLS, N_CHARS, N_PLATFORMS, SHUFFLE_CALLS, SHUFFLE_CHAR_SEED, SHUFFLE_PAD, SHUFFLE_SCRIPT_SEED,
                                 STEPS_PER_CALL, check_ride_coverage, field_case, input_script as ride_input_script, platform_script, ride_coverage,
                                 rider_batch, shuffled_topology)
from refmodel.device import FLAGS
from refmodel.step_device import field_world, hand_world, static_world
from refmodel.character_device import read_device_into
from refmodel.ride_device import DeviceRide, device_poses, repose

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAND_Y = 1.0 + REST_Y  # on the TABLE, whose top is y = 1


def differing(got, want):
    return [i for i in range(len(want)) if got[i].tobytes() != want[i].tobytes()]


def assert_equal_records(got, want, what):
    bad = differing(got, want)
    assert not bad, f"{what}: {len(bad)} of {len(want)} differ, first {bad[0]}: {got[bad[0]]} vs {want[bad[0]]}"


class Shared:
    """The platform field as a world, the poses of every call, and the reference's answers for the whole set after every call:
    made once (the tests that edit a world in other ways make their own)."""

    def __init__(self):
        field, moves, self.descs, self.inputs = field_case()
        self.entities = np.arange(N_PLATFORMS, dtype=np.uint32)
        self.types = np.full(N_PLATFORMS, BODY_STATIC, np.uint8)
        self.w = static_world(np.zeros(N_PLATFORMS, bool), field.size, field.pos, field.euler, ())
        self.start = (field.pos.copy(), field.euler.copy())
        self.poses = []
        for dpos, deuler in moves:
            field.move(dpos, deuler)
            self.poses.append((field.pos.copy(), field.euler.copy()))
        self.got, self.want = self.run(N_CHARS, reference=True)

    def run(self, n, reference=False):
        """Per call (states, records) of the first n characters on the device; with reference=True the reference's too."""
        w = self.w
        repose(w, self.entities, *self.start)
        got, want = [], []
        if reference:
            ride = DeviceRide(w, self.descs[:n], self.types, DT)
        else:
            w.characters_create(self.descs[:n])
            w.characters_ride()
        for k in range(N_CALLS):
            repose(w, self.entities, *self.poses[k])
            if reference:
                gs, gr, ws, wr = ride.call(self.inputs[k][:n], STEPS_PER_CALL)
                want.append((ws, wr))
            else:
                w.characters_set_input(self.inputs[k][:n])
                w.characters_update(DT, STEPS_PER_CALL)
                gs, gr = w.characters_state(), w.characters_rides()
            got.append((gs, gr))
        return got, want


@pytest.fixture(scope="module")
def shared():
    s = Shared()
    yield s
    s.w.close()


@pytest.mark.parametrize("n", BATCHES)
def test_equals_the_rule_over_the_device_queries_and_poses_bit_for_bit_after_every_call(shared, n):
    got = shared.got if n == N_CHARS else shared.run(n)[0]
    for k in range(N_CALLS):  # (a character's answer does not depend on its batch)
        assert_equal_records(got[k][0], shared.want[k][0][:n], f"states after call {k}")
        assert_equal_records(got[k][1], shared.want[k][1][:n], f"ride records after call {k}")
    assert (got[-1][0]["steps"] == N_CALLS * STEPS_PER_CALL).all()
    if n == N_CHARS:
        before = [fresh_rides(n)] + [r for _, r in got[:-1]]
        check_ride_coverage(ride_coverage([(before[k], got[k][1], got[k][0]) for k in range(N_CALLS)]))
        assert not (got[-1][0]["flags"] & W.CHAR_INVALID).any()


def table_run(riding, dpos, calls):
    """The hand character settled on the TABLE, which then moves by dpos before each of `calls` calls of 2 steps: the states after
    every call and the records (None with riding off)."""
    w = hand_world([TABLE], (), True)
    try:
        w.characters_create(hand_character((0.0, STAND_Y + 0.01, 0.0)))
        if riding:
            w.characters_ride()
        w.characters_update(DT, 2)
        s = w.characters_state()[0]
        assert s["flags"] == W.CHAR_GROUNDED and s["ground_entity"] == 0 and abs(s["position"][1] - STAND_Y) <= 1e-6
        pos = np.float32([TABLE[2]])
        out = []
        for _ in range(calls):
            pos = (pos + np.float32(dpos)).astype(np.float32)
            repose(w, np.uint32([0]), pos, np.float32([NO_ROT]))
            w.characters_update(DT, 2)
            out.append((w.characters_state()[0], w.characters_rides()[0] if riding else None))
        return out
    finally:
        w.close()


def test_a_platform_that_moves_along_carries_the_character():
    off = table_run(False, (0.25, 0, 0), 10)
    assert all(s["position"][0] == 0 for s, _ in off) and [bool(s["flags"] & W.CHAR_GROUNDED) for s, _ in off] == [True] * 9 + [False]
    on = table_run(True, (0.25, 0, 0), 12)
    for k, (s, r) in enumerate(on, 1):
        assert s["flags"] == W.CHAR_GROUNDED and abs(s["position"][0] - 0.25 * k) <= 1e-6 and abs(s["position"][1] - STAND_Y) <= 1e-6, (k, s)
        assert r["flags"] == CARRIED and r["entity"] == 0 and np.allclose(r["carried"], (0.25, 0, 0), atol=1e-6, rtol=0) and r["turn"].tolist() == [0, 0, 0, 1]


def test_a_platform_that_descends_takes_the_character_down():
    off = table_run(False, (0, -0.25, 0), 3)
    assert not any(s["flags"] & W.CHAR_GROUNDED for s, _ in off[1:]) and off[-1][0]["vertical_velocity"] < -0.8
    on = table_run(True, (0, -0.25, 0), 4)
    for k, (s, r) in enumerate(on, 1):
        assert s["flags"] == W.CHAR_GROUNDED and abs(s["position"][1] - (1.0 - 0.25 * k + 0.51)) <= 1e-6 and s["vertical_velocity"] == 0, (k, s)
        assert r["flags"] == CARRIED and np.allclose(r["carried"], (0, -0.25, 0), atol=1e-6, rtol=0)


def test_riding_over_a_world_that_does_not_move_changes_nothing():
    """The step field and the walk of test_gpu_characters.py, with riding on and off: the states are byte-identical."""
    field = StepField(np.random.default_rng(STEP_FIELD_SEED))
    descs, heading = character_batch(np.random.default_rng(CHAR_SEED), 257, field)
    script = input_script(np.random.default_rng(INPUT_SEED), heading, N_STEPS)
    w = field_world(field)
    try:
        runs = []
        for riding in (False, True):
            w.characters_create(descs)
            if riding:
                w.characters_ride()
            states = []
            for inp in script:
                w.characters_set_input(inp)
                w.characters_update(DT, 1)
                states.append(w.characters_state())
                if riding:
                    r = w.characters_rides()
                    assert not r["flags"].any() and not r["carried"].any() and (r["turn"] == (0, 0, 0, 1)).all()
            runs.append(states)
        for k in range(N_STEPS):
            assert runs[0][k].tobytes() == runs[1][k].tobytes(), k
        assert (r["entity"] != W.RAY_NO_ENTITY).sum() >= 20  # (characters do stand on bodies of the field)
    finally:
        w.close()


def test_device_forms_forgetting_and_errors():
    import torch
    far = (TABLE[0], TABLE[1], (20.0, 0.5, 0.0), NO_ROT)
    spare = (TABLE[0], TABLE[1], (40.0, 0.5, 0.0), NO_ROT)
    w = hand_world([TABLE, far, spare], (), True)
    lib = B.lib()
    try:
        # no character set: ON is refused, off is fine, and there are no records
        assert lib.bge_world_characters_ride(w._h, 1) == -1 and lib.bge_world_characters_ride(w._h, 0) == 0
        assert w.characters_rides_device() == (0, 0) and len(w.characters_rides()) == 0
        descs = np.concatenate([hand_character((0.0, STAND_Y + 0.01, 0.0)), hand_character((20.0, STAND_Y + 0.01, 0.0)),
                                hand_character((-10.0, REST_Y + 0.01, 0.0))])
        w.characters_create(descs)
        assert w.characters_rides_device() == (0, 0)
        with pytest.raises(B.BgeError) as e:
            w.characters_rides(0, 1)
        assert e.value.code == -1 and len(w.characters_rides(0, 0)) == 0
        for flags in (2, 4, 5, 0x80000001):  # DYNAMIC without ON, unknown bits
            assert lib.bge_world_characters_ride(w._h, flags) == -1
        w.characters_ride()
        assert w.characters_rides().tobytes() == fresh_rides(3).tobytes()
        w.characters_update(DT, 2)
        r = w.characters_rides()
        assert r["entity"].tolist() == [0, 1, W.RAY_NO_ENTITY] and r["anchor_position"][1].tolist() == [20.0, 0.5, 0.0]
        assert r["anchor_rotation"][:2].tolist() == [[0, 0, 0, 1]] * 2 and not r["anchor_rotation"][2].any()
        # the device form equals the download; a part of the set
        ptr, n = w.characters_rides_device()
        assert n == 3 and ptr % 4 == 0
        t = torch.zeros(3 * 64, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        w.sync()
        read_device_into(t, ptr)
        assert t.cpu().numpy().tobytes() == r.tobytes() and w.characters_rides(1, 2).tobytes() == r[1:].tobytes()
        for first, count in ((0, 4), (3, 1), (2, 300)):
            with pytest.raises(B.BgeError):
                w.characters_rides(first, count)
        # switching on again changes the flags and keeps the anchors
        w.characters_ride(True, dynamic=True)
        assert w.characters_rides().tobytes() == r.tobytes() and w.characters_rides_device() == (ptr, 3)
        # upload_bodies over [1, 2) forgets exactly the anchor on entity 1
        w.upload_bodies(np.uint8([W.BODY_STATIC]), None, np.uint8([0]), np.float32([TABLE[1]]), np.uint32([1]), np.uint32([0xFFFFFFFF]), first=1)
        f = w.characters_rides()
        assert f[0].tobytes() == r[0].tobytes() and f[2].tobytes() == r[2].tobytes()
        assert f["entity"][1] == W.RAY_NO_ENTITY and not f["anchor_position"][1].any() and not f["anchor_rotation"][1].any()
        # .. and the indexed form that of its list: entity 2 and 0, not 1
        w.tick(flags=FLAGS)
        w.characters_update(DT, 1)
        assert w.characters_rides()["entity"].tolist() == [0, 1, W.RAY_NO_ENTITY]
        idx, kinds = np.uint32([2, 0]), np.uint8([W.BODY_STATIC, W.BODY_STATIC])
        sizes, ones, alls = np.float32([TABLE[1], TABLE[1]]), np.uint32([1, 1]), np.uint32([0xFFFFFFFF] * 2)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        assert lib.bge_world_upload_bodies_indexed(w._h, 2, vp(idx), vp(kinds), None, None, vp(sizes), vp(ones), vp(alls)) == 0
        assert w.characters_rides()["entity"].tolist() == [W.RAY_NO_ENTITY, 1, W.RAY_NO_ENTITY]
        # a body uploaded since the last tick is not present: the character on it is not anchored by the next call, the other is
        # carried when its platform moves
        repose(w, np.uint32([1]), np.float32([(20.25, 0.5, 0.0)]), np.float32([NO_ROT]))
        w.characters_update(DT, 1)
        s, g = w.characters_state(), w.characters_rides()
        assert g["flags"].tolist() == [0, CARRIED, 0] and abs(s["position"][1][0] - 20.25) <= 1e-6 and g["entity"].tolist() == [0, 1, W.RAY_NO_ENTITY]
        # a body that leaves the world takes its anchor with it
        w.upload_bodies(np.uint8([W.BODY_NONE]), first=1)
        assert w.characters_rides()["entity"][1] == W.RAY_NO_ENTITY  # (forgotten with the upload: nothing to lose any more)
        # set_topology forgets every anchor
        w.set_topology(np.full(3, W.NO_PARENT, np.uint32))
        g = w.characters_rides()
        assert (g["entity"] == W.RAY_NO_ENTITY).all() and not g["anchor_position"].any() and not g["anchor_rotation"].any()
        # characters_create switches riding off
        w.characters_create(descs)
        assert w.characters_rides_device() == (0, 0)
        with pytest.raises(B.BgeError):
            w.characters_rides()
        w.characters_ride()
        w.characters_ride(False)
        assert w.characters_rides_device() == (0, 0)
    finally:
        w.close()


def test_a_dynamic_body_is_ridden_only_with_the_flag_and_lost_without_it():
    """A Dynamic box at rest on the plane: no anchor without BGE_CHAR_RIDE_DYNAMIC, an anchor with it, and LOST, with the position
    untouched, once the flag is dropped under the rider (the body is no longer rideable)."""
    w = B.World(device=0)
    try:
        w.set_topology(np.full(1, W.NO_PARENT, np.uint32))
        w.upload_trs(np.float32([TABLE[2]]), np.float32([NO_ROT]), np.ones((1, 3)))
        w.upload_bodies(np.uint8([W.BODY_DYNAMIC]), np.float32([1.0]), np.uint8([0]), np.float32([TABLE[1]]), np.uint32([1]), np.uint32([0xFFFFFFFF]))
        w.set_ground_plane(True)
        w.tick(flags=FLAGS)
        pos, _ = w.download_pose()
        w.characters_create(hand_character((0.0, float(pos[0][1]) + 0.5 + REST_Y + 0.01, 0.0)))
        w.characters_ride(True, dynamic=False)
        w.characters_update(DT, 2)
        s, r = w.characters_state()[0], w.characters_rides()[0]
        assert s["flags"] & W.CHAR_GROUNDED and s["ground_kind"] == W.RAY_BODY and s["ground_entity"] == 0, s
        assert r["entity"] == W.RAY_NO_ENTITY  # a Dynamic body is no anchor without the flag
        w.characters_ride(True, dynamic=True)
        w.characters_update(DT, 1)
        assert w.characters_rides()[0]["entity"] == 0
        w.characters_ride(True, dynamic=False)
        before = w.characters_state()[0]
        w.characters_update(DT, 1)
        s, r = w.characters_state()[0], w.characters_rides()[0]
        assert r["flags"] == LOST and r["entity"] == W.RAY_NO_ENTITY and not r["carried"].any() and r["turn"].tolist() == [0, 0, 0, 1]
        assert s["position"].tobytes() == before["position"].tobytes() and s["flags"] == W.CHAR_GROUNDED
    finally:
        w.close()


def test_a_world_whose_slots_are_shuffled():
    """Entity i is not slot i: 64 characters, one per platform, byte for byte against the reference.  A carry that reads poses by
    entity index, or an anchor that does, goes wrong here."""
    field, _, _, _ = field_case()
    parent, has_transform = shuffled_topology()
    slot, _, _, info = W.flatten_topology(parent, has_transform)
    assert (slot[:N_PLATFORMS] != np.arange(N_PLATFORMS)).all() and len(parent) == N_PLATFORMS + SHUFFLE_PAD
    w = static_world(np.zeros(N_PLATFORMS, bool), field.size, field.pos, field.euler, (), topology=(parent, has_transform))
    try:
        types = np.full(len(parent), BODY_NONE, np.uint8)
        types[:N_PLATFORMS] = BODY_STATIC
        at = device_poses(w, types)
        half_y = np.array([box_half_extents(s)[1] for s in field.size])
        descs, heading = rider_batch(np.random.default_rng(SHUFFLE_CHAR_SEED), N_PLATFORMS, at.position, at.rotation.astype(np.float64), half_y, per_platform=1)
        rng = np.random.default_rng(SHUFFLE_SCRIPT_SEED)
        moves, inputs = platform_script(rng, SHUFFLE_CALLS), ride_input_script(rng, heading, SHUFFLE_CALLS)
        ride = DeviceRide(w, descs, types, DT)
        entities = np.arange(N_PLATFORMS, dtype=np.uint32)
        carried = anchored = 0
        for k in range(SHUFFLE_CALLS):
            if k:  # (the first call lands them)
                field.move(*moves[k])
                repose(w, entities, field.pos, field.euler)
            inputs[k]["buttons"] = 0
            gs, gr, ws, wr = ride.call(inputs[k], STEPS_PER_CALL)
            assert_equal_records(gs, ws, f"states after call {k}")
            assert_equal_records(gr, wr, f"ride records after call {k}")
            carried += int(((gr["flags"] & CARRIED) != 0).sum())
            anchored += int((gr["entity"] != W.RAY_NO_ENTITY).sum())
            assert (gr["entity"][gr["entity"] != W.RAY_NO_ENTITY] < N_PLATFORMS).all()
        print(f"shuffled: {carried} carries, {anchored} anchors over {SHUFFLE_CALLS} calls of {N_PLATFORMS} characters")
        # Every platform moves before each of the 3 later calls, so every anchored, grounded character is carried then: 192 at the
        # most.  A third of that must happen for the comparison to have seen the carry at shuffled slots.
        assert carried >= 64
    finally:
        w.close()


def test_adapter_platform_riding_on_demo_scene(tmp_path):
    cpp = os.path.join(ROOT, "tests", "cpp")
    lib = os.path.join(ROOT, "banggameengine_amd")
    exe = str(tmp_path / "character_platform_scene")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unused-parameter", "-o", exe,
                           os.path.join(cpp, "character_platform_scene.cpp"), f"-L{lib}", "-lbge_world", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "demo_scene.json")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "all checks passed" in r.stdout
