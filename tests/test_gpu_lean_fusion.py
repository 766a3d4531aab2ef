"""Lean fusion (csrc/bge_fuse_math.hpp fuse::fuse_ticks, DESIGN.md §4.1 "Lean fusion"): the fused ticks of a vouched wave carry only
what changes per tick — x and z velocity are a fixed point, the sleep ballot is decided from v.y's first and last value — and a wave
for which that does not hold runs the exact loop instead.  Nothing may tell.  The scenes here are built around the places where the
two loops part: lanes that cross the sleeping band in the middle of a group, lanes that jump over it (the end test refuses, the
exact loop accepts), v.x = -0.0 (tick 1 changes the sign bit, tick 2 does not), |v.x| near 1e8, and a sideways gravity that some
waves absorb and others do not.

Against the CPU oracle bit for bit after every CALL where gravity is along y (the oracle takes no other); against the same library
with BGE_SOLO_GROUPS=0 and BGE_FUSE_TICKS=1 — one plain tick per launch, code this change does not touch, both switches read per
call — for gravity = (0.3, -9.81, -0.2).  Worlds of 64, 65, 256 and 257 flat Dynamic bodies (slot = entity index: 64 consecutive
entities share a wave), calls of 2, 3, 9, 17, 40 and 520 ticks (longer than the default group of 512), BGE_FUSE_TICKS unset, 8 and 3
(8 and 3 with BGE_SOLO_GROUPS unset are solo groups of that size).  The arithmetic itself, with every class of wave counted, is
tests/test_fuse_math_cpu.py's."""
import os

import numpy as np
import pytest

import banggameengine_amd as B
from oracle import pyoracle as po

from helpers import DT, assert_bits_equal, build_oracle
import row3_views as V

pytestmark = pytest.mark.gpu

F = np.float32
ENVS = ("BGE_SOLO_GROUPS", "BGE_FUSE_TICKS", "BGE_DEFER_ROW3", "BGE_WORLD_ROWS", "BGE_FLAG_WORD", "BGE_REST_PATH")
SIZES = (64, 65, 256, 257)
GROUPS = (None, 8, 3)          # BGE_FUSE_TICKS; None: unset, the default size of a solo group
CALLS = (2, 3, 9, 17, 40, 520)  # ticks per call, after the seeding edit; 520 is longer than the default group (512)
SLEEP_LIN = 0.8                # the world's linear sleeping threshold
GDT = 9.81 * DT                # what gravity takes from v.y per tick
SIDEWAYS = (0.3, -9.81, -0.2)


@pytest.fixture(autouse=True)
def _default_paths(monkeypatch):
    for e in ENVS:
        monkeypatch.delenv(e, raising=False)


def _group(monkeypatch, T):
    if T is not None:
        monkeypatch.setenv("BGE_FUSE_TICKS", str(T))


def crossing_scene(n, fast_wave=False):
    """V.scene's falling bodies, and among them, in every other wave (waves 0, 2, 4):
      * lanes 5, 23, 41 thrown upwards so that v.y is still >= 0.8 after m ticks and inside the band after m + 1, m = 7 .. 40 by
        entity: they cross from above +s to below -s (some 20 ticks) in the middle of the calls of 9, 17 and 40 ticks, and their wave
        is vouched and fast again for the call of 520;
    and in every wave
      * v.x = -0.0 on every fifth entity;
      * |v.x| = 1e8 and v.z = 3e7 on entities 3, 14, 25, ... (a sideways gravity of 0.3 is absorbed there and nowhere else).
    fast_wave: wave 1 as a whole moves at |v.x|, |v.z| near 1e8 — under a sideways gravity the one wave whose x / z velocity is a
    fixed point."""
    wl, vel = V.scene(n, n)
    e = np.arange(n)
    vel[e % 5 == 0, 0] = F(-0.0)
    big = e % 11 == 3
    vel[big, 0] = np.where(e[big] % 2 == 0, F(1e8), F(-1e8))
    vel[big, 2] = F(3e7)
    if fast_wave:
        w1 = (e >= 64) & (e < 128)
        vel[w1, 0] = np.where(e[w1] % 2 == 0, F(1e8), F(-1.5e8))
        vel[w1, 2] = F(-2e8)
    thrown = np.isin(e % 64, (5, 23, 41)) & ((e // 64) % 2 == 0)
    m = 7 + (e[thrown] * 7) % 34
    vel[thrown, 1] = (SLEEP_LIN + (m + 0.5) * GDT).astype(F)
    return wl, vel, thrown


def jumping_scene(n):
    """Gravity -240: the step is 2.0 at the fixed dt, wider than the band.  Lanes 9 and 50 of every wave (and entity 64 of the worlds
    that have one) hold v.y = u + 2.0 * m, u in 0.85 .. 1.0: after m ticks v.y is u, after m + 1 it is u - 2 — on either side of the
    band and never inside.  m = 3 .. 100 by entity, so the jumps fall into every call."""
    wl, vel = V.scene(n, n + 1)
    e = np.arange(n)
    jump = np.isin(e % 64, (9, 50)) | (e == 64)
    rng = np.random.default_rng(11)
    m = 3 + (e[jump] * 29) % 98
    vel[jump, 1] = (rng.uniform(0.85, 1.0, int(jump.sum())) + 2.0 * m).astype(F)
    vel[e % 5 == 0, 0] = F(-0.0)
    return wl, vel, jump


class Pair:
    """A device world and the oracle's scene, advanced call by call and compared after every call."""

    def __init__(self, w, ref, wl, gravity=None):
        self.w, self.ref, self.n, self.gravity = w, ref, wl.n, gravity
        self.parent = wl.parent.copy()
        self.idx = V.shuffled(wl.n)

    def compare(self, what):
        w, ref = self.w, self.ref
        V.assert_same(V.observe(w, self.n, self.idx, self.n, False), V.expect(ref.bulk_world()[0], self.idx, self.parent, False), what)
        pos, eul = w.download_pose()
        rpos, reul = ref.bulk_pose()
        assert_bits_equal(pos, rpos, f"position ({what})")
        assert_bits_equal(eul, reul, f"rotationEuler ({what})")
        gb, rb = w.download_bodies(), ref.bulk_bodies()
        assert_bits_equal(gb["linvel"], rb["linvel"], f"linear velocity ({what})")
        assert_bits_equal(gb["angvel"], rb["angvel"], f"angular velocity ({what})")
        st, tm = w.download_activation()
        rst, rtm = ref.bulk_activation()
        assert np.array_equal(st, rst.astype(np.uint8)), f"activation state ({what}): {np.flatnonzero(st != rst)[:5].tolist()}"
        active = rst == 1
        assert_bits_equal(tm[active], rtm[active], f"deactivation time ({what})")

    def call(self, k, what):
        if self.gravity is None:
            self.w.tick(dt=DT, ticks=k)
        else:
            self.w.tick(dt=DT, gravity=self.gravity, ticks=k)
        for _ in range(k):
            self.ref.PhysicsSystemUpdate(DT)
            self.ref.TransformSystemUpdate()
        self.compare(f"{what}: call of {k}")

    def seed(self, vel):
        """The tick that creates the bodies, then the velocities (the two ticks after the edit store full matrices and establish
        the flag word; the third is the first that a wave can spend in the fused block)."""
        self.call(1, "first tick")
        self.w.set_velocities(vel, None)
        self.ref.bulk_set_velocity(vel, None)


@pytest.mark.parametrize("T", GROUPS)
@pytest.mark.parametrize("n", SIZES)
def test_lanes_cross_the_band_inside_groups(n, T, monkeypatch):
    _group(monkeypatch, T)
    wl, vel, thrown = crossing_scene(n)
    with B.World() as w:
        w.load(wl)
        p = Pair(w, build_oracle(wl), wl)
        p.seed(vel)
        timer_seen = False
        for k in CALLS:
            p.call(k, f"crossing, n = {n}, T = {T}")
            timer_seen = timer_seen or bool((w.download_activation()[1] > 0).any())
        assert timer_seen, "no body ever ran its deactivation timer: no lane was inside the band after a call"
        vy = p.ref.bulk_bodies()["linvel"][:, 1]
        assert (vy <= F(-SLEEP_LIN)).all(), "a thrown lane has not come out below the band: the last call was not a fast one"


@pytest.mark.parametrize("T", GROUPS)
@pytest.mark.parametrize("n", SIZES)
def test_lanes_jump_the_band_inside_groups(n, T, monkeypatch):
    _group(monkeypatch, T)
    wl, vel, jump = jumping_scene(n)
    # the oracle alone first: the chosen bodies change sides without a tick inside the band
    probe = build_oracle(wl)
    probe.SetPhysicsOptions(-240.0, po.ORIENT_IDEAL, False)
    probe.PhysicsSystemUpdate(DT)
    probe.TransformSystemUpdate()
    probe.bulk_set_velocity(vel, None)
    seen = []
    for _ in range(sum(CALLS)):
        probe.PhysicsSystemUpdate(DT)
        probe.TransformSystemUpdate()
        seen.append(probe.bulk_bodies()["linvel"][:, 1].copy())
    seen = np.array(seen)
    assert (np.abs(seen) >= F(SLEEP_LIN)).all(), "a body is inside the band after some tick"
    assert (seen[0, jump] > 0).all() and (seen[-1, jump] < 0).all(), "a chosen body does not change sides"
    ref = build_oracle(wl)
    ref.SetPhysicsOptions(-240.0, po.ORIENT_IDEAL, False)
    with B.World() as w:
        w.load(wl)
        p = Pair(w, ref, wl, gravity=(0.0, -240.0, 0.0))
        p.seed(vel)
        for k in CALLS:
            p.call(k, f"jumping, n = {n}, T = {T}")


def _snapshot(w):
    pos, eul = w.download_pose()
    gb = w.download_bodies()
    st, tm = w.download_activation()
    return {"pos": pos, "euler": eul, "linvel": gb["linvel"], "angvel": gb["angvel"], "world": w.download_world(),
            "dirty": w.download_dirty().astype(np.uint32), "activation": st.astype(np.uint32), "deactivation time": tm}


def _tick_with(w, k, gravity, **env):
    """One call with the given switches in the environment (both are read per call) and nothing of them left behind."""
    old = {e: os.environ.get(e) for e in env}
    os.environ.update(env)
    try:
        w.tick(dt=DT, gravity=gravity, ticks=k)
    finally:
        for e, v in old.items():
            if v is None:
                del os.environ[e]
            else:
                os.environ[e] = v


@pytest.mark.parametrize("T", GROUPS)
@pytest.mark.parametrize("n", SIZES)
def test_sideways_gravity_matches_one_tick_per_launch(n, T, monkeypatch):
    """Two worlds with the same scene in one process: one under the switches of the test, one with BGE_SOLO_GROUPS=0 and
    BGE_FUSE_TICKS=1.  Under gravity (0.3, -9.81, -0.2) the x / z velocity of most lanes changes in every tick — their waves take the
    exact loop — while wave 1 of the larger worlds, at 1e8, absorbs it and stays on the lean one."""
    _group(monkeypatch, T)
    wl, vel, _ = crossing_scene(n, fast_wave=True)
    with B.World() as a, B.World() as b:
        for w in (a, b):
            w.load(wl)
        a.tick(dt=DT, gravity=SIDEWAYS, ticks=1)
        _tick_with(b, 1, SIDEWAYS, BGE_SOLO_GROUPS="0", BGE_FUSE_TICKS="1")
        for w in (a, b):
            w.set_velocities(vel, None)
        for k in CALLS:
            a.tick(dt=DT, gravity=SIDEWAYS, ticks=k)
            _tick_with(b, k, SIDEWAYS, BGE_SOLO_GROUPS="0", BGE_FUSE_TICKS="1")
            V.assert_same(_snapshot(a), _snapshot(b), f"sideways gravity, n = {n}, T = {T}: call of {k}")
        if n > 64:
            vx = a.download_bodies()["linvel"][64:min(n, 128), 0]
            assert (np.abs(vx) >= F(1e8)).all() and (np.abs(vx) <= F(1.5e8)).all()  # (absorbed: wave 1 was a fixed point throughout)


def test_pinned_world_raw_bytes(monkeypatch):
    """BGE_DEFER_ROW3=0 and the pointer handed out: no tick defers, a fused wave stores row 3 of the position it ends on.  The bytes
    behind the pointer are the oracle's after every call."""
    monkeypatch.setenv("BGE_DEFER_ROW3", "0")
    n, n_slots = 257, 512
    wl, vel, _ = crossing_scene(n)
    ref = build_oracle(wl)
    with B.World() as w:
        w.load(wl)
        p = Pair(w, ref, wl)
        p.seed(vel)
        for k in CALLS:
            p.call(k, "pinned")
            V.assert_same({"raw": V.raw_world(w, n_slots)[:n]}, {"raw": ref.bulk_world()[0]}, f"raw bytes, pinned, after a call of {k}")
