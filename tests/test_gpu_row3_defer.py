"""The deferred translation row of the flat tick (TickParams::defer_row3, DESIGN.md §4.1 "Deferred translation row"): a wave on the
translation-row path stores position and velocity and leaves world row 3 — a copy of the position — unstored; per-frame readers
compose it, everything else has it stored first (k_row3_sync).  No way of observing the world matrices may tell the difference:
after EVERY tick the downloads (range and shuffled index), the visible list and its matrices (a frustum around everything, and a
plane that cuts the scene), the draw batches and pack_roots are compared with the CPU oracle bit for bit (tests/row3_views.py).

Nothing in this file shows that a store is skipped: reading the world array through its raw pointer pins the world, after which
no tick defers.  That evidence is the write counter of the headline run (WRITE_SIZE per entity).

All scenes are flat unless said otherwise (slot = entity index: 64 consecutive entities share a wave, 256 a tile)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import banggameengine_amd as B
from banggameengine_amd import synth
from banggameengine_amd.world import flatten_topology
from oracle import pyoracle as po

from helpers import DT, build_oracle
import row3_views as V

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
ENVS = ("BGE_DEFER_ROW3", "BGE_WORLD_ROWS", "BGE_FLAG_WORD", "BGE_REST_PATH")


@pytest.fixture(autouse=True)
def _default_paths(monkeypatch):
    for e in ENVS:
        monkeypatch.delenv(e, raising=False)


class Pair:
    """A device world and the oracle's scene, ticked together and compared through every reader after every tick."""

    def __init__(self, w, ref, wl, render=True):
        self.w, self.ref, self.n, self.render = w, ref, wl.n, render
        self.parent = wl.parent.copy()
        self.idx = V.shuffled(wl.n)
        if render:
            V.render_setup(w, wl.n)

    def compare(self, what, render=True):
        """render=False: some Transform is dirty (after a tick without the transform part), so the renderer's list is not everything."""
        render = render and self.render
        rw = self.ref.bulk_world()[0]
        n_roots = int((self.parent == V.NO_PARENT).sum())
        V.assert_same(V.observe(self.w, self.n, self.idx, n_roots, render), V.expect(rw, self.idx, self.parent, render), what)
        pos, eul = self.w.download_pose()
        rpos, reul = self.ref.bulk_pose()
        V.assert_same({"pos": pos, "euler": eul}, {"pos": rpos, "euler": reul}, what)

    def ticks(self, k, what, flags=B.TICK_ALL):
        for i in range(k):
            self.w.tick(dt=DT, flags=flags)
            if flags & B.TICK_PHYSICS:
                self.ref.PhysicsSystemUpdate(DT)
            if flags & B.TICK_TRANSFORMS:
                self.ref.TransformSystemUpdate()
            self.compare(f"{what}, tick {i}", render=bool(flags & B.TICK_TRANSFORMS))

    def seed(self, vel):
        """The tick that creates the bodies, then the velocities: the tick after that edit takes the full path and leaves the rows
        word, every later one of a wave nobody touches is a deferring one."""
        self.ticks(1, "first tick")
        self.w.set_velocities(vel)
        self.ref.bulk_set_velocity(vel)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 337])
def test_sizes_match_oracle_through_every_reader(n):
    """A partial last wave beside full ones; one tile and two."""
    wl, vel = V.scene(n, n)
    with B.World() as w:
        w.load(wl)
        p = Pair(w, build_oracle(wl), wl)
        p.seed(vel)
        p.ticks(6, f"n = {n}")


def test_world_is_stale_after_an_upload_until_the_next_tick():
    """Transform::world keeps the old translation after a position upload until TransformSystem::Update: the row the tick deferred is
    stored before the upload overwrites the position it would be composed from."""
    n = 337
    wl, vel = V.scene(n)
    ref = build_oracle(wl)
    with B.World() as w:
        w.load(wl)
        p = Pair(w, ref, wl)
        p.seed(vel)
        p.ticks(4, "deferring")
        new = np.array([[1.5, 222.0, -3.25]], F)
        w.upload_trs(pos=new, first=70)
        ref.bulk_set_trs(70, pos=new)
        rw = ref.bulk_world()[0]  # (not updated yet)
        assert not np.array_equal(rw[70, 12:15], new[0])
        V.assert_same({"world": w.download_world(), "indexed": V.download_world_indexed(w, p.idx)}, {"world": rw, "indexed": rw[p.idx]},
                      "after upload_trs, before the tick")
        p.ticks(3, "after the position upload")


def test_leaving_and_reentering_the_path_inside_a_scene():
    """One body (or one call) at a time takes its wave — or every wave — off the deferring path and back; the other waves go on."""
    n = 337
    wl, vel = V.scene(n)
    vel[70] = (0.0, 0.9, 0.0)  # rises, slows through |v.y| < 0.8 under gravity (0.08175 m/s per tick) and falls away again
    ref = build_oracle(wl)
    one = lambda a: np.array([a], F)
    with B.World() as w:
        w.load(wl)
        p = Pair(w, ref, wl)
        p.seed(vel)
        # body 70 is inside the sleeping band from tick ~2 to ~21: its wave declines the vouched block, runs its deactivation timer and
        # comes back
        p.ticks(24, "crossing the sleeping threshold and back")
        lin = w.download_bodies(200, 1)["linvel"].copy()
        w.set_velocities(lin, one((0.5, -1.0, 2.0)), first=200)
        ref.SetVelocity(200 + 1, lin[0], (0.5, -1.0, 2.0))
        p.ticks(3, "spin on one body")
        lin = w.download_bodies(200, 1)["linvel"].copy()
        w.set_velocities(lin, one((0.0, 0.0, 0.0)), first=200)
        ref.SetVelocity(200 + 1, lin[0], (0.0, 0.0, 0.0))
        p.ticks(3, "spin stopped")
        w.mark_dirty(5, 1)
        ref.MarkDirty(5 + 1)
        p.ticks(3, "mark_dirty of one body")
        w.set_ground_plane(True)  # (nobody is near it: the contact stage runs and finds nothing)
        ref.SetGroundPlane(True)
        p.ticks(2, "ground plane on")
        w.set_ground_plane(False)
        ref.SetGroundPlane(False)
        p.ticks(3, "ground plane off")
        p.ticks(1, "AABB tick", B.TICK_ALL | B.TICK_AABBS)
        p.ticks(3, "after the AABB tick")
        p.ticks(1, "PHYSICS only", B.TICK_PHYSICS)  # (positions move, Transform::world does not)
        p.ticks(3, "after PHYSICS only")
        ref.SetAccumulator(True, DT, 4)
        ref.PhysicsSystemUpdate(DT * 0.25)
        ref.TransformSystemUpdate()
        assert w.step_simulation(DT * 0.25, 4, DT, flags=B.TICK_ALL) == 0
        ref.SetAccumulator(False, DT, 4)
        p.compare("update without a sub-step")
        p.ticks(3, "after the update without a sub-step")
        chain = wl.parent.copy()
        for i in range(256, 256 + 32, 4):
            for c in (1, 2, 3):
                chain[i + c] = i + c - 1
                ref.SetParent(i + c + 1, i + c)
        w.set_topology(chain)
        p.parent = chain
        p.ticks(3, "chains of four in the second tile")
        for i in range(256, 256 + 32, 4):
            for c in (1, 2, 3):
                ref.SetParent(i + c + 1, 0)
        w.set_topology(wl.parent)
        p.parent = wl.parent.copy()
        p.ticks(3, "flat again")


def test_raw_pointer_pins_the_world():
    """bge_world_device_array(BGE_ARRAY_WORLD) stores what was deferred and keeps every later tick storing: the bytes behind the pointer
    are the oracle's matrices then and after each later tick."""
    n = 337
    wl, vel = V.scene(n)
    ref = build_oracle(wl)
    with B.World() as w:
        w.load(wl)
        p = Pair(w, ref, wl)
        p.seed(vel)
        p.ticks(4, "deferring")
        n_slots = 512
        V.assert_same({"raw": V.raw_world(w, n_slots)[:n]}, {"raw": ref.bulk_world()[0]}, "raw bytes when the pointer is handed out")
        for k in range(3):
            p.ticks(1, f"pinned, tick {k}")
            V.assert_same({"raw": V.raw_world(w, n_slots)[:n]}, {"raw": ref.bulk_world()[0]}, f"raw bytes, pinned, tick {k}")


def _hierarchy(parent, seed):
    n = len(parent)
    wl = synth.config("chains4", n=n)
    wl.parent = np.asarray(parent, np.uint32)
    wl.pos[:, 1] += F(100.0)
    wl.body_type = np.where(wl.parent == V.NO_PARENT, 1, 255).astype(np.uint8)  # Dynamic bodies on the roots
    vel = wl.vel.copy()
    vel[:, 1] = np.random.default_rng(seed).uniform(-3.0, -1.0, n).astype(F)
    return wl, vel


@pytest.mark.parametrize("shape", ["chains4", "star", "flat_and_star"])
def test_scenes_where_no_row_may_be_deferred(shape):
    """chains4 (260 entities): tiles with levels, never on the translation-row path.  star: one root with 259 children, two passes —
    the four children of the second pass sit at level 0 of a wave-local tile and read their parent's matrix from memory.
    flat_and_star: 300 flat bodies in front of that star, so that flat tiles and a later pass share a scene: the tick stores every
    row as it always did."""
    n = 260
    if shape == "chains4":
        parent = synth.config("chains4", n=n).parent
    elif shape == "star":
        parent = np.array([V.NO_PARENT] + [0] * (n - 1), np.uint32)
    else:
        n = 300 + 260
        parent = np.array([V.NO_PARENT] * 301 + [300] * 259, np.uint32)
    slot, level, pas, info = flatten_topology(parent)
    assert info["n_passes"] == (1 if shape == "chains4" else 2)
    wl, vel = _hierarchy(parent, 11)
    ref = build_oracle(wl)
    with B.World() as w:
        w.load(wl)
        p = Pair(w, ref, wl)
        p.seed(vel)
        p.ticks(6, shape)


_CHILD = r"""
import os, sys
sys.path.insert(0, os.path.join(sys.argv[2], "tests"))
import numpy as np
import banggameengine_amd as B
import row3_views as V
from helpers import DT
n = 337
wl, vel = V.scene(n)
idx = V.shuffled(n)
out = []
with B.World() as w:
    w.load(wl)
    V.render_setup(w, n)
    def ticks(k, flags=B.TICK_ALL):
        for _ in range(k):
            w.tick(dt=DT, flags=flags)
            o = V.observe(w, n, idx, n)
            pos, eul = w.download_pose()
            out.append(np.concatenate([np.ascontiguousarray(a).view(np.uint32).ravel() for a in list(o.values()) + [pos, eul]]))
    ticks(1)
    w.set_velocities(vel)
    ticks(5)
    w.upload_trs(pos=np.array([[1.5, 222.0, -3.25]], np.float32), first=70)
    out.append(w.download_world().view(np.uint32).ravel().copy())
    ticks(3)
    w.mark_dirty(5, 1)
    ticks(3)
    ticks(1, B.TICK_PHYSICS)
    ticks(3)
    ticks(1, B.TICK_ALL | B.TICK_AABBS)
    ticks(3)
np.save(sys.argv[1], np.array(out, dtype=object), allow_pickle=True)
"""


def _run_child(tmp_path, name, value):
    path = tmp_path / f"{name}_{value}.npy"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for e in ENVS:
        env.pop(e, None)
    if value is not None:
        env[name] = str(value)
    r = subprocess.run([sys.executable, "-c", _CHILD, str(path), ROOT], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"child ({name}={value}) exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    return np.load(path, allow_pickle=True)


def test_deferral_on_and_off_give_identical_bytes(tmp_path):
    """Fresh processes: BGE_DEFER_ROW3=0 and BGE_WORLD_ROWS=0 against the default, every reader after every tick."""
    on = _run_child(tmp_path, "BGE_DEFER_ROW3", None)
    assert len(on) >= 20  # (a snapshot per tick of the script)
    for name in ("BGE_DEFER_ROW3", "BGE_WORLD_ROWS"):
        off = _run_child(tmp_path, name, 0)
        assert len(off) == len(on)
        for k in range(len(on)):
            assert np.array_equal(off[k], on[k]), f"snapshot {k}: bytes differ between {name}=0 and unset"
