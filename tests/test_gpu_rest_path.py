"""The tick kernel's rest path (WorldView::rs_word word 1): a wave whose bodies are all asleep reads flags, the
deactivation record and the contact word and stores nothing.  Checked against the CPU oracle bit for bit after every tick —
world, position, rotationEuler, both velocities, activation state — through host edits between ticks (free world), on the
ground plane with the plane switched off and on and an island wake-up under Dynamic contacts, against the path switched off
(BGE_REST_PATH=0, fresh child processes), and white-box: a sentinel in a world row survives exactly while the path runs.

Shapes: 600 flat bodies = 3 tiles, 9 full waves and one of 24 lanes (40 empty slots); one wave holds a Static body and an entity
without a body among sleepers, one wave holds the only body that never sleeps.  Bullet's 2 s at 120 Hz puts the others to sleep
around tick 242 (the C ABI's bge_world_set_sleeping could shorten that; the oracle has no such switch)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import banggameengine_amd as B
from banggameengine_amd import synth
from banggameengine_amd.world import ARRAY_SLOT_OF_ENTITY, ARRAY_WORLD
from oracle import pyoracle as po

from helpers import DT, assert_bits_equal, build_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 600
STATIC, NOBODY, AWAKE = 70, 75, 130  # entities 64..127 share a wave, 128..191 the next one (flat layout: slot = index)
G0 = (0.0, 0.0, 0.0)
SLEEP_TICKS = 255  # every slow body is ISLAND_SLEEPING from tick ~242 on; then ten more


class _NoRef:
    """Stands in for the oracle in the child processes of the on / off comparison: every call is a no-op."""

    def __getattr__(self, name):
        return lambda *a, **k: None


def _free_scene():
    wl = synth.config("flat1m", n=N)
    wl.body_type[:] = 1
    wl.body_type[STATIC] = 0
    wl.body_type[NOBODY] = 255
    rng = np.random.default_rng(3)
    d = rng.normal(size=(N, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
    vel = (d * np.float32(0.2)).astype(np.float32)  # below the 0.8 m/s threshold
    vel[AWAKE] = (1.5, 0.0, 0.0)                     # above it: never sleeps
    vel[[STATIC, NOBODY]] = 0
    return wl, vel


def _compare(w, ref, what):
    if isinstance(ref, _NoRef):
        return None
    pos, eul = w.download_pose()
    rpos, reul = ref.bulk_pose()
    assert_bits_equal(pos, rpos, f"position ({what})")
    assert_bits_equal(eul, reul, f"rotationEuler ({what})")
    assert_bits_equal(w.download_world(), ref.bulk_world()[0], f"world ({what})")
    gb, rb = w.download_bodies(), ref.bulk_bodies()
    ex = rb["exists"]
    assert_bits_equal(gb["linvel"][ex], rb["linvel"][ex], f"linear velocity ({what})")
    assert_bits_equal(gb["angvel"][ex], rb["angvel"][ex], f"angular velocity ({what})")
    st, _ = w.download_activation()
    rst, _ = ref.bulk_activation()
    assert np.array_equal(st[ex], rst[ex].astype(np.uint8)), f"activation state ({what}): {np.flatnonzero(st != rst)[:5].tolist()}"
    return st


def _free_sequence(w, ref, wl, vel, after_tick):
    """Test 1's script.  `after_tick(what)` runs after every tick (compare with the oracle, or take a snapshot)."""
    rng = np.random.default_rng(17)

    def ticks(k, what, flags=B.TICK_ALL):
        for i in range(k):
            w.tick(dt=DT, gravity=G0, flags=flags)
            ref.PhysicsSystemUpdate(DT)
            ref.TransformSystemUpdate()
            after_tick(f"{what}, tick {i}")

    ticks(1, "first tick")
    w.set_velocities(vel)
    ref.bulk_set_velocity(vel)
    ticks(SLEEP_TICKS, "falling asleep")
    # a velocity on one sleeper (the next step wipes it: the body stays asleep)
    one = np.array([[3.0, 0.0, 0.5]], np.float32)
    w.set_velocities(one, np.zeros((1, 3), np.float32), first=10)
    ref.SetVelocity(10 + 1, one[0])
    ticks(3, "velocity on a sleeper")
    # a teleport and a bare mark_dirty: both stay asleep and are re-posed
    p = np.array([[1.0, 2.0, 3.0]], np.float32)
    w.upload_trs(pos=p, first=200)
    ref.bulk_set_trs(200, pos=p)
    ticks(3, "teleported sleeper")
    w.mark_dirty(330, 1)
    ref.MarkDirty(330 + 1)
    ticks(3, "mark_dirty of a sleeper")
    # new euler and new scale (ranges that straddle wave boundaries)
    eul = rng.uniform(-3.0, 3.0, (37, 3)).astype(np.float32)
    w.upload_trs(euler=eul, first=100)
    ref.bulk_set_trs(100, euler=eul)
    ticks(3, "euler upload")
    scl = rng.uniform(0.5, 2.0, (20, 3)).astype(np.float32)
    w.upload_trs(scale=scl, first=500)
    ref.bulk_set_trs(500, scale=scl)
    ticks(3, "scale upload")
    # a sleeping Dynamic body becomes Static
    w.upload_bodies(np.array([0], np.uint8), first=400)
    ref.AddRigidBody(400 + 1, po.BODY_STATIC, 1.0)
    ticks(3, "Dynamic -> Static")
    # re-topology: a few chains of four, then flat again
    chain = wl.parent.copy()
    for i in range(256, 256 + 32, 4):
        for c in (1, 2, 3):
            chain[i + c] = i + c - 1
            ref.SetParent(i + c + 1, i + c)
    w.set_topology(chain)
    ticks(3, "chains of four")
    for i in range(256, 256 + 32, 4):
        for c in (1, 2, 3):
            ref.SetParent(i + c + 1, 0)
    w.set_topology(wl.parent)
    ticks(3, "flat again")
    # a PhysicsSystem::Update whose stepSimulation runs no sub-step (k_pose_only), with one body marked dirty
    w.mark_dirty(20, 1)
    ref.MarkDirty(20 + 1)
    ref.SetAccumulator(True, DT, 4)
    ref.PhysicsSystemUpdate(DT * 0.25)
    ref.TransformSystemUpdate()
    assert w.step_simulation(DT * 0.25, 4, DT, gravity=G0, flags=B.TICK_ALL) == 0
    ref.SetAccumulator(False, DT, 4)
    after_tick("update without a sub-step")
    ticks(3, "after the update without a sub-step")
    # a tick of a variant without the path, then plain ticks again
    ticks(1, "AABB tick", B.TICK_ALL | B.TICK_AABBS)
    ticks(3, "after the AABB tick")


def test_free_world_edits_between_ticks_match_oracle(monkeypatch):
    monkeypatch.delenv("BGE_REST_PATH", raising=False)
    wl, vel = _free_scene()
    ref = build_oracle(wl)
    ref.SetPhysicsOptions(0.0, po.ORIENT_IDEAL, False)
    seen = {}
    with B.World() as w:
        w.load(wl)
        soe = _slots(w)
        assert np.array_equal(soe >> 6, np.arange(N) >> 6)  # the waves the scene was laid out for

        def after(what):
            st = _compare(w, ref, what)
            if what == f"falling asleep, tick {SLEEP_TICKS - 11}":
                seen["asleep"] = st.copy()

        _free_sequence(w, ref, wl, vel, after)
        st, _ = w.download_activation()
    dyn = wl.body_type == 1
    # all asleep ten ticks before the first edit, except the fast one
    assert (seen["asleep"][dyn & (np.arange(N) != AWAKE)] == 2).all() and seen["asleep"][AWAKE] == 1
    assert st[10] == 2 and st[200] == 2 and st[330] == 2 and st[AWAKE] == 1


def _ground_scene():
    n = 540  # 3 tiles: 8 full waves and one of 28 lanes
    wl = synth.Workload("rest-ground", synth.FLAT, n, 4242)
    rng = np.random.default_rng(8)
    k = np.arange(n)
    wl.pos[:, 0] = ((k % 24) * 3.0).astype(np.float32)
    wl.pos[:, 2] = ((k // 24) * 3.0).astype(np.float32)
    wl.pos[:, 1] = rng.uniform(0.55, 0.8, n).astype(np.float32)
    wl.euler[:] = 0.0
    wl.euler[:, 1] = rng.uniform(-0.6, 0.6, n).astype(np.float32)  # (boxes turned by ~45 degrees jitter on the plane and never sleep)
    wl.scale[:] = 1.0
    wl.body_type[:] = 1
    wl.body_type[STATIC] = 0
    wl.body_type[NOBODY] = 255
    return wl


@pytest.mark.parametrize("islands", [False, True], ids=["plane", "plane+dynamic-contacts"])
def test_ground_plane_sleepers_match_oracle(islands, monkeypatch):
    """Boxes land on the plane, rest and fall asleep; the plane is switched off and on.  With Dynamic contacts on, a re-created
    (awake) box is then dropped onto a sleeper: the island wake-up reaches the sleeper in the tick the oracle wakes it, while a
    sentinel in the world matrix of a sleeper of another wave shows that that wave stayed on the rest path."""
    monkeypatch.delenv("BGE_REST_PATH", raising=False)
    wl = _ground_scene()
    n = wl.n
    ref = build_oracle(wl)
    ref.SetGroundPlane(True)
    ref.SetDynamicContacts(islands)
    target, dropper, far = 300, 301, 500
    with B.World() as w:
        w.load(wl)
        w.set_ground_plane(True)
        w.set_dynamic_contacts(islands)

        def ticks(k, what):
            st = None
            for i in range(k):
                w.tick(dt=DT)
                ref.PhysicsSystemUpdate(DT)
                ref.TransformSystemUpdate()
                st = _compare(w, ref, f"{what}, tick {i}")
            return st

        dyn = wl.body_type == 1
        rested = 0
        for i in range(450):  # (landing ~30 ticks, Bullet's 2 s = 240 ticks, then ten ticks of everybody asleep)
            st = ticks(1, f"landing and falling asleep {i}")
            rested = rested + 1 if (st[dyn] == 2).all() else 0
            if rested == 10:
                break
        assert rested == 10, f"{int((st[dyn] != 2).sum())} bodies still awake"
        w.set_ground_plane(False)
        ref.SetGroundPlane(False)
        ticks(3, "plane off")
        w.set_ground_plane(True)
        ref.SetGroundPlane(True)
        st = ticks(3, "plane on again")
        assert (st[dyn] == 2).all()
        if not islands:
            return
        pos, _ = w.download_pose()
        above = (pos[target:target + 1] + np.array([[0.1, 1.25, 0.0]], np.float32)).astype(np.float32)
        w.upload_trs(pos=above, first=dropper)
        ref.bulk_set_trs(dropper, pos=above)
        w.upload_bodies(np.array([1], np.uint8), first=dropper)
        ref.MarkBodyDirty(dropper + 1)
        st = ticks(2, "dropper in the air")  # (the edits moved the epoch: these ticks bring the rest words back)
        assert st[dropper] == 1 and st[target] == 2
        soe = _slots(w)
        assert soe[far] >> 6 != soe[target] >> 6 and soe[far] >> 6 != soe[dropper] >> 6
        sentinel = _poke_world_row0(w, int(soe[far]))
        woke_at = None
        for i in range(60):
            w.tick(dt=DT)
            ref.PhysicsSystemUpdate(DT)
            ref.TransformSystemUpdate()
            # (the sentinel body's world matrix is compared below, everything else here)
            got = w.download_world()
            assert_bits_equal(got[far, :4], sentinel, f"drop tick {i}: sentinel of a sleeping wave the wake-up did not reach")
            w_ref = ref.bulk_world()[0]
            others = np.arange(n) != far
            assert_bits_equal(got[others], w_ref[others], f"drop tick {i}: world")
            assert_bits_equal(got[far, 4:], w_ref[far, 4:], f"drop tick {i}: rows 1..3 of the sentinel body")
            st, _ = w.download_activation()
            rst, _ = ref.bulk_activation()
            ex = ref.bulk_bodies()["exists"]
            assert np.array_equal(st[ex], rst[ex].astype(np.uint8)), f"drop tick {i}: activation state"
            gb, rb = w.download_bodies(), ref.bulk_bodies()
            assert_bits_equal(gb["linvel"][ex], rb["linvel"][ex], f"drop tick {i}: linear velocity")
            assert_bits_equal(gb["angvel"][ex], rb["angvel"][ex], f"drop tick {i}: angular velocity")
            assert_bits_equal(w.download_pose()[0], ref.bulk_pose()[0], f"drop tick {i}: position")
            assert_bits_equal(w.download_pose()[1], ref.bulk_pose()[1], f"drop tick {i}: rotationEuler")
            if woke_at is None and st[target] != 2:
                woke_at = i
        assert woke_at is not None, "the dropped box never woke the sleeper"


_CHILD = r"""
import os, sys
sys.path.insert(0, os.path.join(sys.argv[2], "tests"))
import numpy as np
import banggameengine_amd as B
import test_gpu_rest_path as T
out = []
wl, vel = T._free_scene()
with B.World() as w:
    w.load(wl)
    def snap(what):
        pos, eul = w.download_pose()
        gb = w.download_bodies()
        st, tm = w.download_activation()
        out.append(np.concatenate([a.view(np.uint32).ravel() for a in (w.download_world(), pos, eul, gb["linvel"], gb["angvel"], tm)] + [st.astype(np.uint32)]))
    T._free_sequence(w, T._NoRef(), wl, vel, snap)
np.save(sys.argv[1], np.stack(out))
"""


def _run_child(tmp_path, rest):
    path = tmp_path / f"rest{rest}.npy"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("BGE_REST_PATH", None)
    if rest is not None:
        env["BGE_REST_PATH"] = str(rest)
    r = subprocess.run([sys.executable, "-c", _CHILD, str(path), ROOT], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"child (BGE_REST_PATH={rest}) exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    return np.load(path)


def test_rest_path_on_and_off_give_identical_bytes(tmp_path):
    off = _run_child(tmp_path, 0)
    on = _run_child(tmp_path, None)
    assert off.shape == on.shape
    for k in range(off.shape[0]):
        assert np.array_equal(off[k], on[k]), f"snapshot {k}: bytes differ between BGE_REST_PATH=0 and unset"


def _hip():
    for name in ("libamdhip64.so", "libamdhip64.so.7", "libamdhip64.so.6", "/opt/rocm/lib/libamdhip64.so"):
        try:
            lib = C.CDLL(name)
            lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            return lib
        except OSError:
            continue
    pytest.fail("HIP runtime library not found")


def _slots(w):
    w.sync()
    ptr, count = w.device_array(ARRAY_SLOT_OF_ENTITY)
    soe = np.zeros(int(count), np.uint32)
    assert _hip().hipMemcpy(soe.ctypes.data, ptr, 4 * int(count), 2) == 0  # device -> host
    return soe


def _poke_world_row0(w, slot):
    w.sync()
    ptr, _ = w.device_array(ARRAY_WORLD)
    sentinel = np.array([7.0, -7.0, 7.5, 0.0], np.float32)
    assert _hip().hipMemcpy(ptr + 64 * slot, sentinel.ctypes.data, 16, 1) == 0  # host -> device
    return sentinel


def test_sleeping_waves_store_nothing_until_an_edit(monkeypatch):
    """White box.  Sentinels written into world row 0 of one body in each of two all-asleep waves survive rest-path ticks (the
    full path would overwrite them with the oracle's row: with BGE_REST_PATH=0 this test fails at the first assertion); after
    mark_dirty of the first body its matrix is the oracle's again.  (A host edit moves the epoch, so the tick after it takes every
    wave through the full path once: that a wave nobody touched stays on the rest path while another leaves it inside one launch
    is shown with a device-side wake-up in test_ground_plane_sleepers_match_oracle.  The velocity array is not reachable through
    bge_world_device_array, so no pattern is poked into it; the velocities are compared with the oracle instead.)"""
    monkeypatch.delenv("BGE_REST_PATH", raising=False)
    wl, vel = _free_scene()
    ref = build_oracle(wl)
    ref.SetPhysicsOptions(0.0, po.ORIENT_IDEAL, False)
    a, b = 321, 40
    with B.World() as w:
        w.load(wl)

        def tick():
            w.tick(dt=DT, gravity=G0)
            ref.PhysicsSystemUpdate(DT)
            ref.TransformSystemUpdate()

        tick()
        w.set_velocities(vel)
        ref.bulk_set_velocity(vel)
        for _ in range(SLEEP_TICKS):
            tick()
        st = _compare(w, ref, "asleep")
        soe = _slots(w)
        waves = {int(soe[a]) >> 6, int(soe[b]) >> 6, int(soe[AWAKE]) >> 6}
        assert len(waves) == 3
        for e in (a, b):
            members = np.flatnonzero((soe >> 6) == (soe[e] >> 6))
            assert (st[members] == 2).all()  # an all-asleep wave
        sentinel = _poke_world_row0(w, int(soe[a]))
        _poke_world_row0(w, int(soe[b]))
        for _ in range(3):
            tick()
        got = w.download_world()
        want = ref.bulk_world()[0]
        assert_bits_equal(got[a, :4], sentinel, "sentinel row of wave A (the rest path did not run)")
        assert_bits_equal(got[b, :4], sentinel, "sentinel row of wave B (the rest path did not run)")
        others = ~np.isin(np.arange(N), (a, b))
        assert_bits_equal(got[others], want[others], "world of the other bodies")
        assert_bits_equal(got[[a, b], 4:], want[[a, b], 4:], "rows 1..3 of the sentinel bodies")
        # the awake body's wave was never on the path: its matrices moved with it
        w.mark_dirty(a, 1)
        ref.MarkDirty(a + 1)
        tick()
        _compare(w, ref, "after mark_dirty of the sentinel body")
