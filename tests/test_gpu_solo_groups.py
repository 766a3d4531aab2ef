"""Solo groups (TickParams::n_solo, the SOLO instantiation of k_tick, DESIGN.md §4.1 "Solo groups"): in a scene whose every tile is
flat, the ticks of one bge_world_tick_many call go out as ONE launch per group, and every wave runs the group's ticks itself — a
vouched wave in registers, every other wave tick after tick by the ordinary path inside the launch.  Nothing may tell: after every
CALL the world matrices (range and shuffled index download, pack_roots), position, rotationEuler, both velocities, the activation
state and the deactivation time are compared with the CPU oracle bit for bit — for calls of many lengths under group sizes
BGE_FUSE_TICKS = 2, 3, 8, 32 and the default, with partly filled waves that iterate alone, through the sleeping band in every
iteration of a group, asleep and awake again under zero gravity, beside waves that never fuse, in a one-pass scene that must keep
round 9's scheme, on a pinned world, through the per-frame readers, and against both switches off (fresh child processes).

As with fused ticks, nothing in this file shows that the solo kernel runs: with BGE_SOLO_GROUPS=0 every test passes all the same.
That it runs is shown by the dispatch count and the counters of the headline run.

All scenes are flat unless said otherwise (slot = entity index: 64 consecutive entities share a wave, 256 a tile)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import banggameengine_amd as B
from banggameengine_amd.world import flatten_topology
from oracle import pyoracle as po

from helpers import DT, assert_bits_equal, build_oracle
import row3_views as V

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
ENVS = ("BGE_SOLO_GROUPS", "BGE_FUSE_TICKS", "BGE_DEFER_ROW3", "BGE_WORLD_ROWS", "BGE_FLAG_WORD", "BGE_REST_PATH")
GROUPS = (2, 3, 8, 32, None)           # BGE_FUSE_TICKS; None: unset, the default size of a solo group
CALLS = (2, 3, 1, 4, 5, 8, 9, 17, 40)  # ticks per call; the first ones follow the seeding edit, where no wave is vouched yet
SLEEP_LIN = 0.8                        # the world's linear sleeping threshold (bge_world_set_sleeping's default, Bullet's)
GDT = 9.81 * DT                        # what gravity takes from v.y per tick
G0 = (0.0, 0.0, 0.0)


@pytest.fixture(autouse=True)
def _default_paths(monkeypatch):
    for e in ENVS:
        monkeypatch.delenv(e, raising=False)


def _group(monkeypatch, T):
    if T is not None:
        monkeypatch.setenv("BGE_FUSE_TICKS", str(T))


class Pair:
    """A device world and the oracle's scene, advanced call by call and compared after every call."""

    def __init__(self, w, ref, wl, render=False, gravity=None):
        self.w, self.ref, self.n, self.render = w, ref, wl.n, render
        self.parent = wl.parent.copy()
        self.idx = V.shuffled(wl.n)
        self.gravity = gravity
        if render:
            V.render_setup(w, wl.n)

    def compare(self, what):
        w, ref = self.w, self.ref
        n_roots = int((self.parent == V.NO_PARENT).sum())
        V.assert_same(V.observe(w, self.n, self.idx, n_roots, self.render), V.expect(ref.bulk_world()[0], self.idx, self.parent, self.render), what)
        pos, eul = w.download_pose()
        rpos, reul = ref.bulk_pose()
        assert_bits_equal(pos, rpos, f"position ({what})")
        assert_bits_equal(eul, reul, f"rotationEuler ({what})")
        gb, rb = w.download_bodies(), ref.bulk_bodies()
        ex = rb["exists"].copy()
        if self.dynamic is not None:
            ex &= self.dynamic
        assert_bits_equal(gb["linvel"][ex], rb["linvel"][ex], f"linear velocity ({what})")
        assert_bits_equal(gb["angvel"][ex], rb["angvel"][ex], f"angular velocity ({what})")
        st, tm = w.download_activation()
        rst, rtm = ref.bulk_activation()
        assert np.array_equal(st[ex], rst[ex].astype(np.uint8)), f"activation state ({what}): {np.flatnonzero(st != rst)[:5].tolist()}"
        # (bge_world_download_activation: the timer while the body is ACTIVE_TAG and 0 otherwise — Bullet keeps a stale value there)
        active = ex & (rst == 1)
        assert_bits_equal(tm[active], rtm[active], f"deactivation time ({what})")
        assert (tm[ex & ~active] == 0).all(), f"deactivation time of a body that is not ACTIVE_TAG ({what})"

    dynamic = None  # (a mask of the entities whose body is Dynamic, where a scene has others: the device keeps velocities nothing reads)

    def call(self, k, what):
        """ONE bge_world_tick_many call of k ticks; the oracle runs its k updates; compared once, after the call."""
        if self.gravity is None:
            self.w.tick(dt=DT, ticks=k)
        else:
            self.w.tick(dt=DT, gravity=self.gravity, ticks=k)
        for _ in range(k):
            self.ref.PhysicsSystemUpdate(DT)
            self.ref.TransformSystemUpdate()
        self.compare(f"{what}: call of {k}")

    def calls(self, ks, what):
        for k in ks:
            self.call(k, what)

    def seed(self, vel, ang=None):
        """The tick that creates the bodies, then the velocities.  The tick after that edit stores full matrices, the one after it
        establishes the flag word, and the third is the first that a full wave of identical bodies can spend in the fused block: a
        call of three or more ticks right after an edit walks a wave through all three inside one launch."""
        self.call(1, "first tick")
        self.w.set_velocities(vel, ang)
        self.ref.bulk_set_velocity(vel, ang)


@pytest.mark.parametrize("T", GROUPS)
@pytest.mark.parametrize("n", [64, 65, 255, 256, 257, 337])
def test_sizes_and_call_lengths_match_oracle(n, T, monkeypatch):
    """Full waves, partly filled last waves (65 and 257: one body; 255, 337: never vouched either — they iterate every tick of every
    group alone, inside the launch), one tile and two; calls shorter than a group, equal to one, with a remainder, and of one tick."""
    _group(monkeypatch, T)
    wl, vel = V.scene(n, n)
    with B.World() as w:
        w.load(wl)
        p = Pair(w, build_oracle(wl), wl)
        p.seed(vel)
        p.calls(CALLS, f"n = {n}, T = {T}")


def test_calls_longer_than_the_default_group():
    """BGE_FUSE_TICKS unset: calls that fill a default group exactly, overflow it by one tick (a group of one: a plain tick) and
    hold several groups; 257 bodies, so the last wave iterates every tick of every group alone."""
    n = 257
    wl, vel = V.scene(n, n)
    with B.World() as w:
        w.load(wl)
        p = Pair(w, build_oracle(wl), wl)
        p.seed(vel)
        p.calls((3, 64, 65, 130, 33), "default group size")


def _crossing_velocity(m):
    """An upward v.y that is still >= SLEEP_LIN after m ticks of gravity and below it after m + 1 (half a tick's worth of margin
    on either side, 0.04 m/s, against rounding errors of 1e-7)."""
    return SLEEP_LIN + (m + 0.5) * GDT


@pytest.mark.parametrize("T", (8, 32, None))
def test_one_lane_enters_the_band_in_each_iteration_of_a_group(T, monkeypatch):
    """Wave j (j = 0 .. 7) holds one body, lane 7 + j, that rises and first fails |v.y| >= 0.8 in iteration j of a group.  Ticks 0 and
    1 after the seeding are calls of one tick (full matrices, then the flag word); the call of 8 ticks that follows is one group
    (or the head of one), ticks 2 .. 9, and the body of wave j fails first in tick 2 + j: the wave's first attempt declines, it runs
    ticks by the ordinary path, and the attempts in between decline until the lane is inside the band.  The lane stays there for 19
    more ticks (1.6 / 0.08175), runs its deactivation timer and drops it again: 40 more ticks in calls of 8, 17 and 15, after which
    every wave is vouched and fuses at its first attempt.  A last wave of fast bodies does so throughout."""
    _group(monkeypatch, T)
    J = 8
    n = 64 * (J + 1)
    wl, vel = V.scene(n, J)
    riser = [64 * j + 7 + j for j in range(J)]
    for j, e in enumerate(riser):
        vel[e] = (0.0, _crossing_velocity(2 + j), 0.0)
    # the oracle alone first: each chosen body crosses where intended
    probe = build_oracle(wl)
    probe.PhysicsSystemUpdate(DT)
    probe.TransformSystemUpdate()
    probe.bulk_set_velocity(vel)
    vy = []
    for _ in range(2 + J):
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
        p.call(J, "the group in which every wave but the last declines somewhere")
        timer_seen = bool((w.download_activation()[1] > 0).any())
        for k in (8, 17, 15):
            p.call(k, "through the band and out again")
            timer_seen = timer_seen or bool((w.download_activation()[1] > 0).any())
        p.calls((8, 33), "fast again")
        assert timer_seen, "no body ever ran its deactivation timer: the scene does not do what the test is about"
        assert (np.abs(w.download_bodies()["linvel"][:, 1]) >= F(SLEEP_LIN)).all()


def test_a_slow_body_falls_asleep_inside_a_group_and_is_woken(monkeypatch):
    """Zero gravity, 129 bodies (two full waves and one body alone): everybody moves at 1.5 m/s along y but body 70, which drifts at
    0.2 m/s.  Its wave never fuses; the others do.  Bullet's 2 s at 120 Hz make body 70 WANTS_DEACTIVATION after tick 241 or so and
    ISLAND_SLEEPING one tick later — inside a call of 40 (checked on the oracle: the call begins with it awake and ends with it
    asleep).  Then its wave goes on ticking beside a sleeper.  A velocity edit does not wake it — the reference never calls
    activate(), the next step wipes the velocity, and the device agrees; what wakes a body is its re-creation.  With that and
    the velocity edit after it the body moves again, and a few ticks later every wave is fused."""
    n = 129
    wl, vel = V.scene(n, 7)
    vel[:] = (0.0, 1.5, 0.0)
    vel[70] = (0.2, 0.0, 0.0)
    ref = build_oracle(wl)
    ref.SetPhysicsOptions(0.0, po.ORIENT_IDEAL, False)
    with B.World() as w:
        w.load(wl)
        p = Pair(w, ref, wl, gravity=G0)
        p.seed(vel)
        p.calls((40,) * 5 + (33,), "drifting")                     # 234 ticks
        assert ref.bulk_activation()[0][70] == 1, "asleep too early"  # ACTIVE_TAG
        p.call(40, "falls asleep inside this call")
        assert ref.bulk_activation()[0][70] == 2, "not asleep yet"     # ISLAND_SLEEPING
        assert (ref.bulk_bodies()["linvel"][70] == 0).all()
        p.calls((3, 40), "beside a sleeper")
        one = np.array([[0.0, 2.0, 0.0]], F)
        w.set_velocities(one, np.zeros((1, 3), F), first=70)
        ref.SetVelocity(70 + 1, one[0], (0.0, 0.0, 0.0))
        p.calls((5, 9), "a velocity edit on the sleeper")
        assert ref.bulk_activation()[0][70] == 2  # (the reference never calls activate(): the next step wipes the velocity)
        w.upload_bodies(np.array([1], np.uint8), mass=np.array([1.0], F), first=70)
        ref.AddRigidBody(70 + 1, po.BODY_DYNAMIC, 1.0)
        p.call(1, "the body re-created")
        w.set_velocities(one, np.zeros((1, 3), F), first=70)
        ref.SetVelocity(70 + 1, one[0], (0.0, 0.0, 0.0))
        p.calls((5, 40, 9), "awake again, with a velocity")
        assert ref.bulk_activation()[0][70] == 1
        assert (ref.bulk_bodies()["linvel"][70] == one[0]).all()


@pytest.mark.parametrize("T", (3, None))
@pytest.mark.parametrize("kind", ["one_spinning_body", "one_static_body", "two_mass_classes", "one_body_removed"])
def test_waves_that_never_fuse_beside_waves_that_do(kind, T, monkeypatch):
    """320 bodies: tile 0 holds the odd wave (wave 1) between three uniform ones, tile 1 one uniform wave.  A spinning body and
    alternating mass classes keep their own wave off the fused block — it runs every tick of every group by the flag path — and leave
    the other waves of the tile to it; a Static body and a removed one keep their whole tile off it (the header bit kHdrAllDynamic
    is per tile), so there the wave that fuses is the one of tile 1."""
    _group(monkeypatch, T)
    n = 320
    wl, vel = V.scene(n, 3)
    mass = np.ones(n, F)
    ang = np.zeros((n, 3), F)
    dynamic = np.ones(n, bool)
    if kind == "two_mass_classes":
        mass[65:128:2] = 2.0
    elif kind == "one_static_body":
        wl.body_type[100] = 0
        vel[100] = 0
        dynamic[100] = False
    elif kind == "one_spinning_body":
        ang[100] = (0.5, -1.0, 2.0)
    ref = build_oracle(wl, mass=mass)
    with B.World() as w:
        w.set_topology(wl.parent)
        w.upload_trs(wl.pos, wl.euler, wl.scale)
        w.upload_bodies(wl.body_type, mass=mass)
        p = Pair(w, ref, wl)
        p.dynamic = dynamic
        p.seed(vel, ang)
        if kind == "one_body_removed":
            p.calls((2, 9), "before the removal")
            w.upload_bodies(np.array([255], np.uint8), first=100)
            ref.RemoveRigidBody(100 + 1)
            dynamic[100] = False
        p.calls(CALLS, f"{kind}, T = {T}")


def test_flat_tiles_beside_chain_tiles_keep_one_launch_per_tick(monkeypatch):
    """337 entities in ONE pass: tile 0 flat, tile 1 with eight chains of four among flat bodies.  The scene is fusable and not
    all-flat: it keeps round 9's scheme — one launch per tick, serials, the per-wave words — and matches as before."""
    n = 337
    wl, vel = V.scene(n, 5)
    chain = wl.parent.copy()
    for i in range(256, 256 + 32, 4):
        for c in (1, 2, 3):
            chain[i + c] = i + c - 1
    wl.parent = chain
    assert flatten_topology(chain)[3]["n_passes"] == 1
    with B.World() as w:
        w.load(wl)
        p = Pair(w, build_oracle(wl), wl)
        p.seed(vel)
        p.calls((2, 3, 9, 17, 40), "flat beside chains")
        # flat again: the same world goes over to solo groups, and back
        w.set_topology(V.scene(n, 5)[0].parent)
        for i in range(256, 256 + 32, 4):
            for c in (1, 2, 3):
                p.ref.SetParent(i + c + 1, 0)
        p.parent = V.scene(n, 5)[0].parent.copy()
        p.calls((5, 17), "flat again")
        w.set_topology(chain)
        for i in range(256, 256 + 32, 4):
            for c in (1, 2, 3):
                p.ref.SetParent(i + c + 1, i + c)
        p.parent = chain.copy()
        p.calls((5, 17), "chains again")


@pytest.mark.parametrize("T", (8, None))
def test_pinned_world_raw_bytes(T, monkeypatch):
    """bge_world_device_array(BGE_ARRAY_WORLD) pins the world: no tick defers.  After an edit, a call of five ticks is one launch in
    which every wave stores full matrices (rows of other lanes' slots, through LDS), then row 3 alone from the slot's own lane,
    then fuses the rest and stores row 3 of the position it ends on.  The bytes behind the pointer are the oracle's after each call."""
    _group(monkeypatch, T)
    n = 337
    wl, vel = V.scene(n)
    ref = build_oracle(wl)
    n_slots = 512
    raw = lambda what: V.assert_same({"raw": V.raw_world(w, n_slots)[:n]}, {"raw": ref.bulk_world()[0]}, what)
    with B.World() as w:
        w.load(wl)
        p = Pair(w, ref, wl)
        p.seed(vel)
        p.calls((2, 5), "deferring")
        raw("raw bytes when the pointer is handed out")
        for k in (5, 1, 9, 3, 40):
            p.call(k, "pinned")
            raw(f"raw bytes, pinned, after a call of {k}")
        w.mark_dirty(5, 1)
        ref.MarkDirty(5 + 1)
        p.call(5, "pinned, after mark_dirty: full path, translation row, fused — one launch")
        raw("raw bytes after the call behind mark_dirty")
        lin = w.download_bodies(200, 1)["linvel"].copy()
        lin[0, 0] += F(0.25)
        w.set_velocities(lin, np.zeros((1, 3), F), first=200)
        ref.SetVelocity(200 + 1, lin[0], (0.0, 0.0, 0.0))
        for k in (4, 17):
            p.call(k, "pinned, after set_velocities")
            raw(f"raw bytes after set_velocities and a call of {k}")


@pytest.mark.parametrize("T", (8, None))
def test_per_frame_readers_after_solo_calls(T, monkeypatch):
    """The visible list (everything, and a plane that cuts the scene), the draw batches and pack_roots compose the deferred row from
    the position a solo launch stored."""
    _group(monkeypatch, T)
    n = 337
    wl, vel = V.scene(n)
    with B.World() as w:
        w.load(wl)
        p = Pair(w, build_oracle(wl), wl, render=True)
        p.seed(vel)
        p.calls((2, 8, 17, 3, 40), f"readers, T = {T}")


def test_a_call_of_seventeen_ticks_counts_seventeen():
    """The ticks that launch nothing still count: one event pair around the call, 17 ticks read back; physics_updates likewise (a
    body uploaded after the call exists from the next update on — the oracle agrees after the call that follows)."""
    n = 337
    wl, vel = V.scene(n)
    with B.World() as w:
        w.load(wl)
        p = Pair(w, build_oracle(wl), wl)
        p.seed(vel)
        p.call(5, "vouched")
        w.profile_enable(1)
        p.call(17, "profiled")
        ms, ticks = w.profile_read()
        assert ticks == 17 and ms > 0.0
        p.call(40, "profiled, two groups or more")
        assert w.profile_read()[1] == 40
        w.profile_enable(0)
        p.call(3, "after profiling")


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
    for k in (2, 3, 1, 4, 5, 8, 9, 17, 40):
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
    call(40)
    w.step_simulation(DT * 3.25, 4, DT, flags=B.TICK_ALL)
    call(8)
    w.upload_bodies(np.array([255], np.uint8), first=100)
    call(33)
np.save(sys.argv[1], np.array(out, dtype=object), allow_pickle=True)
"""


def _run_child(tmp_path, name, **switches):
    path = tmp_path / f"solo_{name}.npy"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for e in ENVS:
        env.pop(e, None)
    env.update(switches)
    r = subprocess.run([sys.executable, "-c", _CHILD, str(path), ROOT], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"child ({switches}) exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    return np.load(path, allow_pickle=True)


def test_switches_give_identical_bytes(tmp_path):
    """Fresh processes, one after the other, the same script of calls and edits: the default against BGE_SOLO_GROUPS=0 (round 9's
    scheme) and against BGE_FUSE_TICKS=1 (one plain tick per launch), every reader after every call."""
    on = _run_child(tmp_path, "default")
    assert len(on) == 21  # (a snapshot per call of the script, and the download after the position upload)
    for name, switches in (("solo_off", {"BGE_SOLO_GROUPS": "0"}), ("fuse_off", {"BGE_FUSE_TICKS": "1"})):
        off = _run_child(tmp_path, name, **switches)
        assert len(off) == len(on)
        for k in range(len(on)):
            assert np.array_equal(on[k], off[k]), f"snapshot {k}: bytes differ between the default and {switches}"
