"""Fused ticks (TickParams::serial / n_left, WorldView::adv, DESIGN.md §4.1 "Fused ticks"): inside one bge_world_tick_many call a vouched
wave of the flat tick runs the ticks that remain of its group in registers and touches memory once; the group's later launches
return at once for it.  Nothing may tell: after every CALL the world matrices (range and shuffled index download, pack_roots),
position, rotationEuler, both velocities and the activation state are compared with the CPU oracle bit for bit, for calls of many
lengths under group sizes BGE_FUSE_TICKS = 2, 3, 4 and 8, through bodies that cross the sleeping threshold in every iteration of a
group, beside waves that can never be vouched, through host edits and other tick variants between calls, in scenes that must not
fuse, on a pinned world, through the per-frame readers, and against the switch off (BGE_FUSE_TICKS=1, fresh child processes).

Nothing in this file shows that the block runs: with it dead every test below still passes.  That it runs is shown by the
counters of the headline run (bytes per entity of a group's first and of its later dispatches).

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

from helpers import DT, assert_bits_equal, build_oracle
import row3_views as V

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
ENVS = ("BGE_FUSE_TICKS", "BGE_DEFER_ROW3", "BGE_WORLD_ROWS", "BGE_FLAG_WORD", "BGE_REST_PATH")
GROUPS = (2, 3, 4, 8)
CALLS = (2, 3, 1, 4, 5, 8, 9, 17)  # ticks per call; the first ones follow the seeding edit, where no wave is vouched yet
SLEEP_LIN = 0.8                    # the world's linear sleeping threshold (bge_world_set_sleeping's default, Bullet's)
GDT = 9.81 * DT                    # what gravity takes from v.y per tick


@pytest.fixture(autouse=True)
def _default_paths(monkeypatch):
    for e in ENVS:
        monkeypatch.delenv(e, raising=False)


class Pair:
    """A device world and the oracle's scene, advanced call by call and compared after every call."""

    def __init__(self, w, ref, wl, render=False):
        self.w, self.ref, self.n, self.render = w, ref, wl.n, render
        self.parent = wl.parent.copy()
        self.idx = V.shuffled(wl.n)
        self.static = set()  # entities whose body is Static now and was Dynamic: the device keeps velocities nothing reads
        if render:
            V.render_setup(w, wl.n)

    def compare(self, what, render=True):
        w, ref = self.w, self.ref
        n_roots = int((self.parent == V.NO_PARENT).sum())
        render = render and self.render
        V.assert_same(V.observe(w, self.n, self.idx, n_roots, render), V.expect(ref.bulk_world()[0], self.idx, self.parent, render), what)
        pos, eul = w.download_pose()
        rpos, reul = ref.bulk_pose()
        assert_bits_equal(pos, rpos, f"position ({what})")
        assert_bits_equal(eul, reul, f"rotationEuler ({what})")
        gb, rb = w.download_bodies(), ref.bulk_bodies()
        ex = rb["exists"].copy()
        ex[list(self.static)] = False
        assert_bits_equal(gb["linvel"][ex], rb["linvel"][ex], f"linear velocity ({what})")
        assert_bits_equal(gb["angvel"][ex], rb["angvel"][ex], f"angular velocity ({what})")
        st, tm = w.download_activation()
        rst, rtm = ref.bulk_activation()
        assert np.array_equal(st[ex], rst[ex].astype(np.uint8)), f"activation state ({what}): {np.flatnonzero(st != rst)[:5].tolist()}"
        assert_bits_equal(tm[ex], rtm[ex], f"deactivation time ({what})")

    def call(self, k, what, flags=B.TICK_ALL):
        """ONE bge_world_tick_many call of k ticks; the oracle runs its k updates; compared once, after the call."""
        self.w.tick(dt=DT, flags=flags, ticks=k)
        for _ in range(k):
            if flags & B.TICK_PHYSICS:
                self.ref.PhysicsSystemUpdate(DT)
            if flags & B.TICK_TRANSFORMS:
                self.ref.TransformSystemUpdate()
        self.compare(f"{what}: call of {k}", render=bool(flags & B.TICK_TRANSFORMS))

    def calls(self, ks, what, flags=B.TICK_ALL):
        for k in ks:
            self.call(k, what, flags)

    def seed(self, vel):
        """The tick that creates the bodies, then the velocities.  The tick after that edit takes the ordinary path and leaves the
        words; the one after it is the first that a full wave of identical bodies can spend in the vouched block."""
        self.call(1, "first tick")
        self.w.set_velocities(vel)
        self.ref.bulk_set_velocity(vel)


@pytest.mark.parametrize("T", GROUPS)
@pytest.mark.parametrize("n", [64, 65, 128, 256, 257, 320, 337])
def test_sizes_and_call_lengths_match_oracle(n, T, monkeypatch):
    """Full waves, a partial last wave (never vouched: it ticks once per launch all the same), one tile and two; calls shorter
    than a group, equal to one, and with a remainder."""
    monkeypatch.setenv("BGE_FUSE_TICKS", str(T))
    wl, vel = V.scene(n, n)
    with B.World() as w:
        w.load(wl)
        p = Pair(w, build_oracle(wl), wl)
        p.seed(vel)
        p.calls(CALLS, f"n = {n}, T = {T}")


def _crossing_velocity(m):
    """An upward v.y that is still >= SLEEP_LIN after m ticks of gravity and below it after m + 1 (half a tick's worth of margin
    on either side, 0.04 m/s, against rounding errors of 1e-7)."""
    return SLEEP_LIN + (m + 0.5) * GDT


@pytest.mark.parametrize("T", GROUPS)
def test_one_lane_turns_slow_in_each_iteration_of_a_group(T, monkeypatch):
    """Wave j (j = 0 .. T - 1) holds one body, lane 7 + j, that rises and first fails |v.y| >= 0.8 in iteration j of a group.  Ticks 0
    and 1 after the seeding are calls of one tick (the ordinary path leaves the words, then the first vouched tick); the call of T
    ticks that follows is one group, ticks 2 .. T + 1, and the body of wave j is chosen to fail first in tick 2 + j.  Wave j fuses
    in no launch of that group whose remaining ticks reach tick 2 + j — launch i < j declines and runs one tick, the launches from j
    on find the lane slow at once and take the ordinary path.  The lane stays inside the band for 19 more ticks (1.6 / 0.08175),
    runs its deactivation timer there and drops it: 32 more ticks in calls of 8, after which every wave is vouched and fuses again.
    A last wave of fast bodies fuses throughout."""
    monkeypatch.setenv("BGE_FUSE_TICKS", str(T))
    n = 64 * (T + 1)
    wl, vel = V.scene(n, T)
    riser = [64 * j + 7 + j for j in range(T)]
    for j, e in enumerate(riser):
        vel[e] = (0.0, _crossing_velocity(2 + j), 0.0)
    # the oracle alone first: each chosen body crosses where intended
    probe = build_oracle(wl)
    probe.PhysicsSystemUpdate(DT)
    probe.TransformSystemUpdate()
    probe.bulk_set_velocity(vel)
    vy = []
    for _ in range(2 + T):
        probe.PhysicsSystemUpdate(DT)
        probe.TransformSystemUpdate()
        vy.append(probe.bulk_bodies()["linvel"][:, 1].copy())
    vy = np.abs(np.array(vy))  # [tick][entity]
    for j, e in enumerate(riser):
        assert (vy[: 2 + j, e] >= F(SLEEP_LIN)).all() and vy[2 + j, e] < F(SLEEP_LIN), f"body {e} does not first fail in tick {2 + j}"
    others = np.setdiff1d(np.arange(n), riser)
    assert (vy[:, others] >= F(SLEEP_LIN)).all()
    with B.World() as w:
        w.load(wl)
        p = Pair(w, build_oracle(wl), wl)
        p.seed(vel)
        p.calls((1, 1), "words come back")
        p.call(T, "the group in which every wave but the last declines somewhere")
        timer_seen = bool((w.download_activation()[1] > 0).any())
        for k in range(4):
            p.call(8, f"inside the band and out again, {k}")
            timer_seen = timer_seen or bool((w.download_activation()[1] > 0).any())
        p.calls((T, 2 * T + 1), "fast again")
        assert timer_seen, "no body ever ran its deactivation timer: the scene does not do what the test is about"
        assert (np.abs(w.download_bodies()["linvel"][:, 1]) >= F(SLEEP_LIN)).all()


@pytest.mark.parametrize("T", (3, 8))
@pytest.mark.parametrize("kind", ["two_mass_classes", "one_static_body", "one_spinning_body"])
def test_waves_that_can_never_be_vouched(kind, T, monkeypatch):
    """320 bodies: tile 0 holds the odd wave (wave 1) between three uniform ones, tile 1 one uniform wave.  Mass classes that
    alternate and a spinning body keep their own wave off the block and leave the other waves of the tile to it; a Static body keeps
    its whole tile off (the header bit kHdrAllDynamic is per tile), so there the fused wave is the one of tile 1."""
    monkeypatch.setenv("BGE_FUSE_TICKS", str(T))
    n = 320
    wl, vel = V.scene(n, 3)
    mass = np.ones(n, F)
    ang = np.zeros((n, 3), F)
    if kind == "two_mass_classes":
        mass[65:128:2] = 2.0
    elif kind == "one_static_body":
        wl.body_type[100] = 0
        vel[100] = 0
    else:
        ang[100] = (0.5, -1.0, 2.0)
    ref = build_oracle(wl, mass=mass)
    with B.World() as w:
        w.set_topology(wl.parent)
        w.upload_trs(wl.pos, wl.euler, wl.scale)
        w.upload_bodies(wl.body_type, mass=mass)
        p = Pair(w, ref, wl)
        p.call(1, "first tick")
        w.set_velocities(vel, ang)
        ref.bulk_set_velocity(vel, ang)
        p.calls(CALLS, f"{kind}, T = {T}")


@pytest.mark.parametrize("T", (3, 8))
def test_host_edits_and_other_ticks_between_fused_calls(T, monkeypatch):
    """Every edit lands on a world whose vouched waves were advanced by fused groups in the call before, and is followed by fused
    calls: between calls every wave's memory is at the same tick, whatever launch of its group brought it there."""
    monkeypatch.setenv("BGE_FUSE_TICKS", str(T))
    n = 337
    wl, vel = V.scene(n)
    ref = build_oracle(wl)
    one = lambda a: np.array([a], F)
    after = (T + 1, 2, T)
    with B.World() as w:
        w.load(wl)
        p = Pair(w, ref, wl)
        p.seed(vel)
        p.calls((2, 2 * T + 1), "fused")
        new = one((1.5, 222.0, -3.25))
        w.upload_trs(pos=new, first=70)
        ref.bulk_set_trs(70, pos=new)
        p.calls(after, "position upload")
        w.mark_dirty(5, 1)
        ref.MarkDirty(5 + 1)
        p.calls(after, "mark_dirty of one body")
        lin = w.download_bodies(200, 1)["linvel"].copy()
        lin[0, 0] += F(0.25)
        w.set_velocities(lin, one((0.0, 0.0, 0.0)), first=200)
        ref.SetVelocity(200 + 1, lin[0], (0.0, 0.0, 0.0))
        p.calls(after, "set_velocities on one body")
        w.upload_bodies(np.array([1], np.uint8), mass=one(2.5), first=130)
        ref.AddRigidBody(130 + 1, po.BODY_DYNAMIC, 2.5)
        p.calls(after, "body upload (mass change)")
        w.set_ground_plane(True)  # (nobody is near it: the contact stage runs and finds nothing)
        ref.SetGroundPlane(True)
        p.calls((T + 1, 2), "ground plane on")
        w.set_ground_plane(False)
        ref.SetGroundPlane(False)
        p.calls(after, "ground plane off")
        chain = wl.parent.copy()
        for i in range(256, 256 + 32, 4):
            for c in (1, 2, 3):
                chain[i + c] = i + c - 1
                ref.SetParent(i + c + 1, i + c)
        w.set_topology(chain)
        p.parent = chain
        p.calls(after, "chains of four in the second tile")
        for i in range(256, 256 + 32, 4):
            for c in (1, 2, 3):
                ref.SetParent(i + c + 1, 0)
        w.set_topology(wl.parent)
        p.parent = wl.parent.copy()
        p.calls(after, "flat again")
        p.call(T + 1, "AABB ticks", B.TICK_ALL | B.TICK_AABBS)
        p.calls(after, "after the AABB ticks")
        p.call(2, "PHYSICS only", B.TICK_PHYSICS)  # (positions move, Transform::world does not)
        p.calls(after, "after PHYSICS only")
        ref.SetAccumulator(True, DT, 4)
        for factor, due in ((0.25, 0), (1.0, 1), (3.0, 3)):  # the clock keeps 0.25 of a step throughout
            step = float(np.float64(factor) * np.float64(DT))
            ref.PhysicsSystemUpdate(step)
            ref.TransformSystemUpdate()
            assert w.step_simulation(step, 4, DT, flags=B.TICK_ALL) == due == ref.LastSubSteps()
            p.compare(f"step_simulation with {due} sub-steps due")
            ref.SetAccumulator(False, DT, 4)
            p.calls((T + 1, T), f"after step_simulation with {due} sub-steps due")
            ref.SetAccumulator(True, DT, 4)
        ref.SetAccumulator(False, DT, 4)


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
def test_scenes_that_must_not_fuse(shape, monkeypatch):
    """chains4 (260 entities): tiles with levels.  star: one root with 259 children, two passes.  flat_and_star: 300 flat bodies in
    front of that star — flat tiles and a later pass in one scene: a child of the later pass reads a root's matrix inside every tick."""
    monkeypatch.setenv("BGE_FUSE_TICKS", "4")
    n = 260
    if shape == "chains4":
        parent = synth.config("chains4", n=n).parent
    elif shape == "star":
        parent = np.array([V.NO_PARENT] + [0] * (n - 1), np.uint32)
    else:
        n = 300 + 260
        parent = np.array([V.NO_PARENT] * 301 + [300] * 259, np.uint32)
    info = flatten_topology(parent)[3]
    assert info["n_passes"] == (1 if shape == "chains4" else 2)
    wl, vel = _hierarchy(parent, 11)
    ref = build_oracle(wl)
    with B.World() as w:
        w.load(wl)
        p = Pair(w, ref, wl)
        p.seed(vel)
        p.calls((2, 5, 4, 9, 3), shape)


def test_a_frozen_root_keeps_the_scene_from_fusing(monkeypatch):
    """337 flat bodies; entity 70 hangs under entity 5, which carries no body and then loses its Transform: 70 becomes a root that
    keeps the matrix it had (parent * local) while its position goes on falling, until something marks it dirty.  A flat tile beside
    it would fuse; the scene as a whole does not.  Compared over the entities that still own a Transform."""
    monkeypatch.setenv("BGE_FUSE_TICKS", "4")
    n = 337
    wl, vel = V.scene(n)
    wl.body_type[5] = 255
    wl.parent[70] = 5
    ref = build_oracle(wl)
    has_transform = np.ones(n, np.uint8)
    rows = np.ones(n, bool)

    def call(w, k, what):
        w.tick(dt=DT, ticks=k)
        for _ in range(k):
            ref.PhysicsSystemUpdate(DT)
            ref.TransformSystemUpdate()
        what = f"{what}: call of {k}"
        assert_bits_equal(w.download_world()[rows], ref.bulk_world()[0][rows], f"world ({what})")
        pos, eul = w.download_pose()
        rpos, reul = ref.bulk_pose()
        assert_bits_equal(pos[rows], rpos[rows], f"position ({what})")
        assert_bits_equal(eul[rows], reul[rows], f"rotationEuler ({what})")
        ex = ref.bulk_bodies()["exists"] & rows
        assert_bits_equal(w.download_bodies()["linvel"][ex], ref.bulk_bodies()["linvel"][ex], f"linear velocity ({what})")
        assert np.array_equal(w.download_activation()[0][ex], ref.bulk_activation()[0][ex].astype(np.uint8)), f"activation state ({what})"

    with B.World() as w:
        w.load(wl)
        call(w, 1, "first tick")
        w.set_velocities(vel)
        ref.bulk_set_velocity(vel)
        for k in (2, 5):
            call(w, k, "child of entity 5")
        ref.RemoveTransform(5 + 1)
        has_transform[5] = 0
        rows[5] = False
        w.set_topology(wl.parent, has_transform)
        for k in (4, 9, 3, 8):
            call(w, k, "frozen root")
        w.mark_dirty(70, 1)
        ref.MarkDirty(70 + 1)
        for k in (4, 5):
            call(w, k, "thawed")


def test_pinned_world_stores_the_final_row(monkeypatch):
    """bge_world_device_array(BGE_ARRAY_WORLD) pins the world: no tick defers, fused groups still run and store row 3 of the
    position they end on.  The bytes behind the pointer are the oracle's matrices after each call."""
    monkeypatch.setenv("BGE_FUSE_TICKS", "4")
    n = 337
    wl, vel = V.scene(n)
    ref = build_oracle(wl)
    with B.World() as w:
        w.load(wl)
        p = Pair(w, ref, wl)
        p.seed(vel)
        p.calls((2, 5), "deferring")
        n_slots = 512
        V.assert_same({"raw": V.raw_world(w, n_slots)[:n]}, {"raw": ref.bulk_world()[0]}, "raw bytes when the pointer is handed out")
        for k in (4, 1, 9, 3, 8):
            p.call(k, "pinned")
            V.assert_same({"raw": V.raw_world(w, n_slots)[:n]}, {"raw": ref.bulk_world()[0]}, f"raw bytes, pinned, after a call of {k}")


@pytest.mark.parametrize("T", (4, 8))
def test_per_frame_readers_after_fused_calls(T, monkeypatch):
    """The visible list (everything, and a plane that cuts the scene), the draw batches and pack_roots compose the deferred row from
    the position a fused group stored."""
    monkeypatch.setenv("BGE_FUSE_TICKS", str(T))
    n = 337
    wl, vel = V.scene(n)
    with B.World() as w:
        w.load(wl)
        p = Pair(w, build_oracle(wl), wl, render=True)
        p.seed(vel)
        p.calls((2, T, 2 * T + 1, 3, 17), f"readers, T = {T}")


_CHILD = r"""
import os, sys
sys.path.insert(0, os.path.join(sys.argv[2], "tests"))
import numpy as np
import banggameengine_amd as B
import row3_views as V
from helpers import DT
n = 337
wl, vel = V.scene(n)
vel[70] = (0.0, 1.3, 0.0)  # rises through the sleeping band and falls out of it again
idx = V.shuffled(n)
out = []
with B.World() as w:
    w.load(wl)
    V.render_setup(w, n)
    def call(k, flags=B.TICK_ALL):
        w.tick(dt=DT, flags=flags, ticks=k)
        o = V.observe(w, n, idx, n, bool(flags & B.TICK_TRANSFORMS))
        pos, eul = w.download_pose()
        gb = w.download_bodies()
        st, tm = w.download_activation()
        out.append(np.concatenate([np.ascontiguousarray(a).view(np.uint32).ravel() for a in list(o.values()) + [pos, eul, gb["linvel"], gb["angvel"], tm]]
                                  + [st.astype(np.uint32)]))
    call(1)
    w.set_velocities(vel)
    for k in (2, 3, 1, 4, 5, 8, 9, 17):
        call(k)
    w.upload_trs(pos=np.array([[1.5, 222.0, -3.25]], np.float32), first=70)
    out.append(w.download_world().view(np.uint32).ravel().copy())
    for k in (9, 4):
        call(k)
    w.mark_dirty(5, 1)
    for k in (8, 3):
        call(k)
    call(2, B.TICK_PHYSICS)
    call(17)
    call(3, B.TICK_ALL | B.TICK_AABBS)
    call(16)
    w.step_simulation(DT * 3.25, 4, DT, flags=B.TICK_ALL)
    call(8)
np.save(sys.argv[1], np.array(out, dtype=object), allow_pickle=True)
"""


def _run_child(tmp_path, value):
    path = tmp_path / f"fuse_{value}.npy"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for e in ENVS:
        env.pop(e, None)
    if value is not None:
        env["BGE_FUSE_TICKS"] = str(value)
    r = subprocess.run([sys.executable, "-c", _CHILD, str(path), ROOT], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"child (BGE_FUSE_TICKS={value}) exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    return np.load(path, allow_pickle=True)


def test_fusion_off_default_and_eight_give_identical_bytes(tmp_path):
    """Fresh processes, the same script of calls and edits: BGE_FUSE_TICKS=1 against unset and against 8, every reader after every call."""
    off = _run_child(tmp_path, 1)
    assert len(off) == 19  # (a snapshot per call of the script, and the download after the position upload)
    for value in (None, 8):
        on = _run_child(tmp_path, value)
        assert len(on) == len(off)
        for k in range(len(off)):
            assert np.array_equal(on[k], off[k]), f"snapshot {k}: bytes differ between BGE_FUSE_TICKS=1 and {value}"
