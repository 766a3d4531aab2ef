"""The tick kernel's translation-row fast path (WorldView::rs_word): waves whose rotation rows are current store
only row 3 of the world matrices.  Checked against the CPU oracle bit for bit after every tick through edits between ticks,
against the path switched off (BGE_WORLD_ROWS=0, fresh child processes) on scenes that also re-parent, switch the ground plane
on and step without a sub-step, and white-box: a sentinel in a rotation row survives exactly while the path runs."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import banggameengine_amd as B
from banggameengine_amd import synth
from banggameengine_amd.world import ARRAY_SLOT_OF_ENTITY, ARRAY_WORLD

from helpers import DT, assert_bits_equal, build_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1000  # not a multiple of 64: the last wave is partly empty


def _check(w, ref, what):
    got_world = w.download_world()
    got_pos, got_euler = w.download_pose()
    want_world, _ = ref.bulk_world()
    want_pos, want_euler = ref.bulk_pose()
    assert_bits_equal(got_pos, want_pos, f"position ({what})")
    assert_bits_equal(got_euler, want_euler, f"rotationEuler ({what})")
    assert_bits_equal(got_world, want_world, f"world ({what})")


def _tick(w, ref, what, flags=B.TICK_ALL):
    w.tick(dt=DT, flags=flags)
    ref.PhysicsSystemUpdate(DT)
    ref.TransformSystemUpdate()
    _check(w, ref, what)


def test_flat_edits_between_ticks_match_oracle():
    wl = synth.config("flat1m", n=N)
    ref = build_oracle(wl)
    rng = np.random.default_rng(5)
    with B.World() as w:
        w.load(wl)
        for k in range(40):
            _tick(w, ref, f"warm-up tick {k}")
            if k == 0:
                w.set_velocities(wl.vel)
                ref.bulk_set_velocity(wl.vel)
        # euler of some bodies (a range that straddles a wave boundary)
        eul = rng.uniform(-3.0, 3.0, (37, 3)).astype(np.float32)
        w.upload_trs(euler=eul, first=100)
        ref.bulk_set_trs(100, euler=eul)
        for k in range(3):
            _tick(w, ref, f"after euler upload, tick {k}")
        # scale of some bodies
        scl = rng.uniform(0.5, 2.0, (20, 3)).astype(np.float32)
        w.upload_trs(scale=scl, first=500)
        ref.bulk_set_trs(500, scale=scl)
        for k in range(3):
            _tick(w, ref, f"after scale upload, tick {k}")
        # angular velocity on a few bodies, then back to zero
        lin = w.download_bodies()["linvel"].copy()
        ang = np.zeros((N, 3), np.float32)
        ang[[3, 64, 65, 999]] = rng.uniform(-2.0, 2.0, (4, 3)).astype(np.float32)
        w.set_velocities(lin, ang)
        ref.bulk_set_velocity(lin, ang)
        for k in range(3):
            _tick(w, ref, f"spinning, tick {k}")
        lin = w.download_bodies()["linvel"].copy()
        w.set_velocities(lin, np.zeros((N, 3), np.float32))
        ref.bulk_set_velocity(lin, np.zeros((N, 3), np.float32))
        for k in range(3):
            _tick(w, ref, f"spin stopped, tick {k}")
        # ticks of the variants without the fast path, then the fast path again
        _tick(w, ref, "normal-matrix tick", B.TICK_ALL | B.TICK_NORMAL_MATRICES)
        _tick(w, ref, "after the normal-matrix tick")
        _tick(w, ref, "AABB tick", B.TICK_ALL | B.TICK_AABBS)
        for k in range(3):
            _tick(w, ref, f"after the AABB tick, tick {k}")


_CHILD = r"""
import sys
import numpy as np
import banggameengine_amd as B
from banggameengine_amd import synth
from banggameengine_amd.world import ARRAY_SLOT_OF_ENTITY, ARRAY_WORLD
DT = 1.0 / 60.0
N = int(sys.argv[2])
out = []
def snap():
    wd = w.download_world()
    pos, eul = w.download_pose()
    out.append(np.concatenate([wd.view(np.uint32).ravel(), pos.view(np.uint32).ravel(), eul.view(np.uint32).ravel()]))
def ticks(k, flags=B.TICK_ALL):
    for _ in range(k):
        w.tick(dt=DT, flags=flags)
        snap()
wl = synth.config("flat1m", n=N)
rng = np.random.default_rng(11)
with B.World() as w:
    w.load(wl)
    w.tick(dt=DT)
    w.set_velocities(wl.vel)
    ticks(40)
    w.upload_trs(euler=rng.uniform(-3, 3, (50, 3)).astype(np.float32), first=30)
    ticks(3)
    w.upload_trs(scale=rng.uniform(0.5, 2, (50, 3)).astype(np.float32), first=600)
    ticks(3)
    lin = w.download_bodies()["linvel"].copy()
    ang = np.zeros((N, 3), np.float32)
    ang[::97] = 1.5
    w.set_velocities(lin, ang)
    ticks(3)
    w.set_velocities(w.download_bodies()["linvel"].copy(), np.zeros((N, 3), np.float32))
    ticks(3)
    # re-parent into chains of four, then back to flat
    chain = wl.parent.copy()
    for i in range(0, N - 3, 4):
        chain[i + 1], chain[i + 2], chain[i + 3] = i, i + 1, i + 2
    w.set_topology(chain)
    ticks(3)
    w.set_topology(wl.parent)
    ticks(3)
    # ground plane on for a few ticks, then off
    w.set_ground_plane(True)
    ticks(3)
    w.set_ground_plane(False)
    ticks(3)
    ticks(1, B.TICK_ALL | B.TICK_NORMAL_MATRICES)
    ticks(2)
    ticks(1, B.TICK_ALL | B.TICK_AABBS)
    ticks(2)
    ticks(1, B.TICK_TRANSFORMS)
    # a PhysicsSystem::Update whose stepSimulation runs no sub-step (k_pose_only), then the fast path again
    w.mark_dirty(0, 10)
    assert w.step_simulation(DT * 0.25, 4, DT, flags=B.TICK_ALL) == 0
    snap()
    ticks(3)
np.save(sys.argv[1], np.stack(out))
"""


def _run_child(tmp_path, rows):
    path = tmp_path / f"rows{rows}.npy"
    env = dict(os.environ, BGE_WORLD_ROWS=str(rows), PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", _CHILD, str(path), str(N)], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, f"child (BGE_WORLD_ROWS={rows}) exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    return np.load(path)


def test_fast_path_on_and_off_give_identical_bytes(tmp_path):
    off = _run_child(tmp_path, 0)
    on = _run_child(tmp_path, 1)
    assert off.shape == on.shape
    for k in range(off.shape[0]):
        assert np.array_equal(off[k], on[k]), f"snapshot {k}: world / pose bytes differ between BGE_WORLD_ROWS=0 and 1"


def _hip():
    for name in ("libamdhip64.so", "libamdhip64.so.7", "libamdhip64.so.6", "/opt/rocm/lib/libamdhip64.so"):
        try:
            return C.CDLL(name)
        except OSError:
            continue
    pytest.fail("HIP runtime library not found")


def test_rotation_rows_are_not_rewritten_while_current(monkeypatch):
    """White box: a sentinel written into row 0 of one body's world matrix survives fast-path ticks; an euler upload of that
    body makes the next tick rewrite the row (and match the oracle again)."""
    monkeypatch.delenv("BGE_WORLD_ROWS", raising=False)
    hip = _hip()
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    wl = synth.config("flat1m", n=N)
    ref = build_oracle(wl)
    e = 321
    with B.World() as w:
        w.load(wl)
        for k in range(5):
            _tick(w, ref, f"warm-up tick {k}")
            if k == 0:
                w.set_velocities(wl.vel)
                ref.bulk_set_velocity(wl.vel)
        w.sync()
        soe_ptr, _ = w.device_array(ARRAY_SLOT_OF_ENTITY)
        slot = np.zeros(1, np.uint32)
        assert hip.hipMemcpy(slot.ctypes.data, soe_ptr + 4 * e, 4, 2) == 0  # device -> host
        world_ptr, _ = w.device_array(ARRAY_WORLD)
        sentinel = np.array([7.0, -7.0, 7.5, 0.0], np.float32)
        assert hip.hipMemcpy(world_ptr + 64 * int(slot[0]), sentinel.ctypes.data, 16, 1) == 0  # host -> device
        for _ in range(2):
            w.tick(dt=DT)
            ref.PhysicsSystemUpdate(DT)
            ref.TransformSystemUpdate()
        got = w.download_world()
        want, _ = ref.bulk_world()
        assert_bits_equal(got[e, :4], sentinel, "sentinel row (the fast path did not run)")
        assert_bits_equal(got[e, 4:], want[e, 4:], "rows 1..3 of the sentinel body")
        others = np.arange(N) != e
        assert_bits_equal(got[others], want[others], "world of the other bodies")
        eul = w.download_pose()[1][e:e + 1].copy()
        w.upload_trs(euler=eul, first=e)
        ref.bulk_set_trs(e, euler=eul)
        _tick(w, ref, "after the euler upload")
