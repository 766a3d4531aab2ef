"""The tick kernel's vouched waves (WorldView::rs_word words 2 and 3, DESIGN.md §4.1 "flag word"): a translation-row wave whose 64
flag words are known to be one clean value (valid, Dynamic, one mass class, nothing else) integrates without reading flags.
Checked bit for bit against the CPU oracle after every tick — world, position, rotationEuler, both velocities, activation
state — over wave and tile boundaries, through bodies that cross the sleeping threshold and back, in waves that can never be
vouched, and through host edits and other tick variants between ticks; and against the block switched off (BGE_FLAG_WORD=0,
fresh child processes), byte for byte.

The flag array is not reachable through bge_world_device_array, so there is no white-box poke here, and nothing in this file
shows that the block runs at all: with it dead every test below still passes.  That it runs is shown by the read counters of
the headline run (2 x FETCH_SIZE falls by the 4 B of the flag word per entity).

All scenes are flat (slot = entity index: 64 consecutive entities share a wave, 256 a tile), ticked with TICK_ALL and the default
gravity unless said otherwise.  The header bit kHdrAllDynamic is per tile: one Static body keeps its whole tile off the block."""
import os
import subprocess
import sys

import numpy as np
import pytest

import banggameengine_amd as B
from banggameengine_amd import synth
from oracle import pyoracle as po

from helpers import DT, assert_bits_equal, build_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
G = (0.0, -9.81, 0.0)


class _NoRef:
    """Stands in for the oracle in the child processes of the on / off comparison: every call is a no-op."""

    def __getattr__(self, name):
        return lambda *a, **k: None


def _scene(n, seed=0):
    """n Dynamic bodies of mass 1, far above y = 0, falling faster than the sleeping threshold (0.8 m/s) from the start."""
    wl = synth.config("flat1m", n=n)
    wl.pos[:, 1] += F(100.0)
    rng = np.random.default_rng(100 + seed)
    vel = wl.vel.copy()
    vel[:, 1] = rng.uniform(-3.0, -1.0, n).astype(F)
    return wl, vel


def _compare(w, ref, what, static=()):
    """`static`: entities whose body is Static now and was Dynamic before.  The reference re-creates the body with zero velocities;
    the device leaves what the velocity arrays held, which nothing reads while the body is Static: not compared."""
    if isinstance(ref, _NoRef):
        return
    pos, eul = w.download_pose()
    rpos, reul = ref.bulk_pose()
    assert_bits_equal(pos, rpos, f"position ({what})")
    assert_bits_equal(eul, reul, f"rotationEuler ({what})")
    assert_bits_equal(w.download_world(), ref.bulk_world()[0], f"world ({what})")
    gb, rb = w.download_bodies(), ref.bulk_bodies()
    ex = rb["exists"].copy()
    ex[list(static)] = False
    assert_bits_equal(gb["linvel"][ex], rb["linvel"][ex], f"linear velocity ({what})")
    assert_bits_equal(gb["angvel"][ex], rb["angvel"][ex], f"angular velocity ({what})")
    st, tm = w.download_activation()
    rst, rtm = ref.bulk_activation()
    assert np.array_equal(st[ex], rst[ex].astype(np.uint8)), f"activation state ({what}): {np.flatnonzero(st != rst)[:5].tolist()}"
    assert_bits_equal(tm[ex], rtm[ex], f"deactivation time ({what})")


def _tick(w, ref, what):
    w.tick(dt=DT)
    ref.PhysicsSystemUpdate(DT)
    ref.TransformSystemUpdate()
    _compare(w, ref, what)


def _seed(w, ref, vel):
    """The tick that creates the bodies, then the velocities (an edit: the tick after it takes the full path and leaves both
    words, the one after that is the first a full wave of identical bodies spends in the block)."""
    _tick(w, ref, "first tick")
    w.set_velocities(vel)
    ref.bulk_set_velocity(vel)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257, 320, 337])
def test_sizes_match_oracle(n, monkeypatch):
    """A partial last wave (never vouched: its empty slots carry another flag word) beside full ones; one tile and two."""
    monkeypatch.delenv("BGE_FLAG_WORD", raising=False)
    wl, vel = _scene(n, n)
    ref = build_oracle(wl)
    with B.World() as w:
        w.load(wl)
        _seed(w, ref, vel)
        for k in range(6):
            _tick(w, ref, f"n = {n}, tick {k}")


def test_crossing_the_sleeping_threshold_and_back(monkeypatch):
    """Every body rises, slows under gravity through |v.y| < 0.8 and falls away again.  While one lane of a wave is inside that
    band the wave declines (the ballot) and the ordinary path runs; the bodies with a small horizontal velocity are then slower
    than the threshold altogether, start their deactivation timer (kDrowsy) and drop it when they are fast again: the wave's flag
    words differ meanwhile, so it loses its vouch and gets it back.

    v.y0 is a sorted uniform sample of [0.5, 3], so a wave holds neighbouring values [a, b]; gravity takes 0.08175 m/s per tick.
    A lane is inside the band in the ticks (v.y0 - 0.8) / 0.08175 < k < (v.y0 + 0.8) / 0.08175, counted from the seeding.  Expected
    per wave (two ticks after the seeding edit bring the words back; the last wave has 17 bodies and is never vouched):
        wave 0  [0.50, 0.98]  inside from the start to tick ~21          vouched from ~23 on
        wave 1  [0.98, 1.45]  inside ~3 .. ~27                           vouched at 2, and from ~29 on
        wave 2  [1.45, 1.93]  inside ~8 .. ~33                           vouched 2 .. ~7 and from ~35 on
        wave 3  [1.93, 2.40]  inside ~14 .. ~39                          vouched 2 .. ~13 and from ~41 on
        wave 4  [2.40, 2.88]  inside ~20 .. ~45                          vouched 2 .. ~19, not again within the 45 ticks
    Nobody falls asleep: Bullet's 2 s are 240 ticks."""
    monkeypatch.delenv("BGE_FLAG_WORD", raising=False)
    n = 337
    wl, vel = _scene(n)
    rng = np.random.default_rng(7)
    vel[:, 1] = np.sort(rng.uniform(0.5, 3.0, n)).astype(F)
    slow = (np.arange(n) & 1) == 0
    vel[slow, 0] = rng.uniform(-0.1, 0.1, int(slow.sum())).astype(F)
    vel[slow, 2] = rng.uniform(-0.1, 0.1, int(slow.sum())).astype(F)
    vel[~slow, 0] = rng.uniform(2.0, 3.0, int((~slow).sum())).astype(F)
    vel[~slow, 2] = -rng.uniform(2.0, 3.0, int((~slow).sum())).astype(F)
    ref = build_oracle(wl)
    drowsy_seen = False
    with B.World() as w:
        w.load(wl)
        _seed(w, ref, vel)
        for k in range(45):
            _tick(w, ref, f"tick {k}")
            drowsy_seen = drowsy_seen or bool((w.download_activation()[1] > 0).any())
        st, tm = w.download_activation()
        rst, rtm = ref.bulk_activation()
    assert drowsy_seen, "no body ever ran its deactivation timer: the scene does not do what the test is about"
    assert np.array_equal(st, rst.astype(np.uint8)) and (st == 1).all()
    assert_bits_equal(tm, rtm, "deactivation time at the end")


def test_mixed_waves_match_oracle(monkeypatch):
    """Wave 0: mass classes alternate (equal flag words nowhere); wave 1: one Static body; wave 2: uniform."""
    monkeypatch.delenv("BGE_FLAG_WORD", raising=False)
    n = 192
    wl, vel = _scene(n)
    mass = np.ones(n, F)
    mass[1:64:2] = 2.0
    wl.body_type[100] = 0
    vel[100] = 0
    ref = build_oracle(wl, mass=mass)
    with B.World() as w:
        w.set_topology(wl.parent)
        w.upload_trs(wl.pos, wl.euler, wl.scale)
        w.upload_bodies(wl.body_type, mass=mass)
        _seed(w, ref, vel)
        for k in range(8):
            _tick(w, ref, f"tick {k}")


N_EDIT = 320  # tile 0: waves 0..3, tile 1: wave 4
DT2 = float(F(1.0 / 90.0))


def _edit_sequence(w, ref, wl, vel, after_tick, model_tick):
    """The script of the edit test and of the on / off comparison.  `after_tick(what, static)` runs after every tick that the oracle
    follows (`static` as in _compare); `model_tick(what, gravity, dt)` after the ticks at the end that it cannot (it knows a y gravity only)."""

    static = set()

    def ticks(k, what, flags=B.TICK_ALL, dt=DT):
        for i in range(k):
            w.tick(dt=dt, flags=flags)
            if flags & B.TICK_PHYSICS:
                ref.PhysicsSystemUpdate(dt)
            if flags & B.TICK_TRANSFORMS:
                ref.TransformSystemUpdate()
            after_tick(f"{what}, tick {i}", static)

    one = lambda a: np.array([a], F)
    ticks(1, "first tick")
    w.set_velocities(vel)
    ref.bulk_set_velocity(vel)
    ticks(3, "vouched")
    # --- edits, three ticks after each
    w.mark_dirty(5, 1)
    ref.MarkDirty(5 + 1)
    ticks(3, "mark_dirty of one body")
    w.upload_bodies(np.array([0], np.uint8), mass=one(1.0), first=70)
    ref.AddRigidBody(70 + 1, po.BODY_STATIC, 1.0)
    static.add(70)
    ticks(3, "Dynamic -> Static")
    static.clear()
    w.upload_bodies(np.array([1], np.uint8), mass=one(1.0), first=70)
    ref.AddRigidBody(70 + 1, po.BODY_DYNAMIC, 1.0)
    ticks(3, "Static -> Dynamic")
    w.upload_bodies(np.array([1], np.uint8), mass=one(2.5), first=130)
    ref.AddRigidBody(130 + 1, po.BODY_DYNAMIC, 2.5)
    ticks(3, "mass change")
    lin = w.download_bodies(200, 1)["linvel"].copy()
    w.set_velocities(lin, one((0.5, -1.0, 2.0)), first=200)
    ref.SetVelocity(200 + 1, lin[0], (0.5, -1.0, 2.0))
    ticks(3, "angular velocity on one body")
    lin = w.download_bodies(200, 1)["linvel"].copy()
    w.set_velocities(lin, one((0.0, 0.0, 0.0)), first=200)
    ref.SetVelocity(200 + 1, lin[0], (0.0, 0.0, 0.0))
    ticks(3, "spin stopped")
    eul = one((0.3, -1.1, 2.0))
    w.upload_trs(euler=eul, first=260)
    ref.bulk_set_trs(260, euler=eul)
    ticks(3, "euler upload")
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
    w.set_sleeping(0.8, 1.0, 2.0)  # (Bullet's own values, which the oracle has built in: the call alone is the edit)
    ticks(3, "set_sleeping")
    w.set_ground_plane(True)  # (nobody is near it: the contact stage runs and finds nothing)
    ref.SetGroundPlane(True)
    ticks(2, "ground plane on")
    w.set_ground_plane(False)
    ref.SetGroundPlane(False)
    ticks(3, "ground plane off")
    # --- other tick variants
    ticks(1, "PHYSICS only", B.TICK_PHYSICS)
    ticks(3, "after PHYSICS only")
    ticks(1, "TRANSFORMS only", B.TICK_TRANSFORMS)
    ticks(3, "after TRANSFORMS only")
    ticks(1, "AABB tick", B.TICK_ALL | B.TICK_AABBS)
    ticks(3, "after the AABB tick")
    ref.SetPhysicsOptions(-9.81, po.ORIENT_BASIS, False)
    ticks(1, "Bullet-basis tick", B.TICK_ALL | B.TICK_BULLET_BASIS)
    ref.SetPhysicsOptions(-9.81, po.ORIENT_IDEAL, False)
    ticks(3, "after the Bullet-basis tick")
    ref.SetAccumulator(True, DT, 4)
    ref.PhysicsSystemUpdate(DT * 0.25)
    ref.TransformSystemUpdate()
    assert w.step_simulation(DT * 0.25, 4, DT, flags=B.TICK_ALL) == 0
    ref.SetAccumulator(False, DT, 4)
    after_tick("update without a sub-step", static)
    ticks(3, "after the update without a sub-step")
    # (the Bullet-basis tick left kSettled on the bodies, a bit no vouched flag word has; a re-pose takes it away, so that the
    #  ticks below run in the block again.  Re-posing zeroes the velocities: they are set again.)
    w.mark_dirty(0, N_EDIT)
    for e in range(N_EDIT):
        ref.MarkDirty(e + 1)
    ticks(1, "everything re-posed")
    w.set_velocities(vel)
    ref.bulk_set_velocity(vel)
    ticks(3, "before the other gravities")
    # --- gravity with x and z components, none at all, another dt
    for what, g, dt in (("gravity with x and z", (1.0, -9.81, 2.0), DT), ("zero gravity", (0.0, 0.0, 0.0), DT), ("another dt", G, DT2)):
        for i in range(3):
            w.tick(dt=dt, gravity=g)
            model_tick(f"{what}, tick {i}", g, dt)


def test_edits_between_ticks_match_oracle(monkeypatch):
    monkeypatch.delenv("BGE_FLAG_WORD", raising=False)
    wl, vel = _scene(N_EDIT)
    ref = build_oracle(wl)
    with B.World() as w:
        w.load(wl)
        state = {}

        def model_tick(what, g, dt):
            # v += ((g / m^-1) * m^-1) * dt; x += v * dt in binary32, one rounding per operation (test_gpu_vel_layout.py); rows 0..2
            # stay what the last oracle-checked tick left (nothing spins, nothing is re-posed)
            if not state:
                state["v"] = w_before["linvel"].copy()
                state["pos"] = w_before["pos"].copy()
                state["world"] = w_before["world"].copy()
            mass = np.ones(N_EDIT, F)
            mass[130] = 2.5
            inv = F(1.0) / mass
            for a in range(3):
                imp = ((F(g[a]) / inv).astype(F) * inv).astype(F) * F(dt)
                state["v"][:, a] = state["v"][:, a] + imp
                state["pos"][:, a] = state["pos"][:, a] + state["v"][:, a] * F(dt)
            state["world"][:, 12:15] = state["pos"]
            assert_bits_equal(w.download_bodies()["linvel"], state["v"], f"linear velocity ({what})")
            assert_bits_equal(w.download_pose()[0], state["pos"], f"position ({what})")
            assert_bits_equal(w.download_world(), state["world"], f"world ({what})")

        w_before = {}

        def after_tick(what, static):
            _compare(w, ref, what, static)
            if what.startswith("before the other gravities"):
                w_before.update(linvel=w.download_bodies()["linvel"], pos=w.download_pose()[0], world=w.download_world())

        _edit_sequence(w, ref, wl, vel, after_tick, model_tick)


_CHILD = r"""
import os, sys
sys.path.insert(0, os.path.join(sys.argv[2], "tests"))
import numpy as np
import banggameengine_amd as B
import test_gpu_flag_word as T
out = []
wl, vel = T._scene(T.N_EDIT)
with B.World() as w:
    w.load(wl)
    def snap(what, *a):
        pos, eul = w.download_pose()
        gb = w.download_bodies()
        st, tm = w.download_activation()
        out.append(np.concatenate([a.view(np.uint32).ravel() for a in (w.download_world(), pos, eul, gb["linvel"], gb["angvel"], tm)] + [st.astype(np.uint32)]))
    T._edit_sequence(w, T._NoRef(), wl, vel, snap, snap)
np.save(sys.argv[1], np.stack(out))
"""


def _run_child(tmp_path, flag_word):
    path = tmp_path / f"flag_word_{flag_word}.npy"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("BGE_FLAG_WORD", None)
    if flag_word is not None:
        env["BGE_FLAG_WORD"] = str(flag_word)
    r = subprocess.run([sys.executable, "-c", _CHILD, str(path), ROOT], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"child (BGE_FLAG_WORD={flag_word}) exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    return np.load(path)


def test_block_on_and_off_give_identical_bytes(tmp_path):
    off = _run_child(tmp_path, 0)
    on = _run_child(tmp_path, None)
    assert off.shape == on.shape and off.shape[0] >= 60  # (a snapshot per tick of the script)
    for k in range(off.shape[0]):
        assert np.array_equal(off[k], on[k]), f"snapshot {k}: bytes differ between BGE_FLAG_WORD=0 and unset"
