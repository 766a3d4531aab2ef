"""Linear velocities in per-wave component blocks (bge_device_math.hpp ld_vel / st_vel): per 64 slots a
float2 xz[64] and a float y[64], and the tick stores only the components whose bits it changed.  Nothing of that may show
through the C ABI: velocities go in and come out as rows of three floats, and every kernel that reads or writes them — the
tick, the pose-only step, the uploads, the re-layout after a topology edit, the contact and solver kernels — computes what it
computed before, bit for bit."""
import numpy as np
import pytest

import banggameengine_amd as B
from banggameengine_amd import synth

from helpers import DT, assert_bits_equal, build_oracle

pytestmark = pytest.mark.gpu

F = np.float32
N_FLAT = 1300  # five full 256-slot tiles and a ragged one


def _distinct(n):
    ids = np.arange(n, dtype=np.float32)
    return np.stack([ids, ids + F(0.25), ids + F(0.5)], axis=1)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1300])
def test_velocity_round_trip(n):
    """set_velocities -> download_bodies, whole range and sub-ranges that start and end inside a 64-slot group.  (The C ABI has
    no indexed form of either call.)"""
    wl = synth.config("flat1m", n=n)
    lin = _distinct(n)
    with B.World() as w:
        w.load(wl)
        w.tick(dt=DT)  # bodies are created by the first physics update
        w.set_velocities(lin)
        assert_bits_equal(w.download_bodies()["linvel"], lin, f"linvel of {n} bodies")
        for first, count in ((0, 1), (n // 2, n - n // 2), (max(n - 70, 0), min(n, 67)), (n - 1, 1)):
            count = min(count, n - first)
            assert_bits_equal(w.download_bodies(first, count)["linvel"], lin[first:first + count], f"linvel [{first}, {first + count})")
        # a partial upload leaves the neighbours alone
        first, count = n // 3, max(n // 5, 1)
        part = -_distinct(count) - F(1.0)
        w.set_velocities(part, first=first)
        want = lin.copy()
        want[first:first + count] = part
        assert_bits_equal(w.download_bodies()["linvel"], want, "linvel after a partial upload")


def test_velocity_round_trip_in_a_hierarchy():
    """Slots are not entity indices here, and only every fourth entity carries a body."""
    n = 1024
    wl = synth.config("chains4", n=n)
    dyn = wl.body_type == 1
    lin = _distinct(n)
    with B.World() as w:
        w.load(wl)
        w.tick(dt=DT)
        w.set_velocities(lin)
        got = w.download_bodies()["linvel"]
        assert_bits_equal(got[dyn], lin[dyn], "linvel of the bodies")
        assert not got[~dyn].any(), "entities without a body report zero velocity"
        assert_bits_equal(w.download_bodies(130, 401)["linvel"][dyn[130:531]], lin[130:531][dyn[130:531]], "linvel [130, 531)")


def _flat_scene():
    wl = synth.config("flat1m", n=N_FLAT)
    vel = wl.vel.copy()
    vel[::7, 0] = F(-0.0)   # -0.0 + 0.0 = +0.0: a component a zero impulse changes
    vel[3::11] = 0.0        # zero velocity
    vel[5::13, 1] = F(-0.0)
    return wl, vel


def _compare(w, ref, dyn, what, rows=None):
    rows = slice(None) if rows is None else rows
    pos, euler = w.download_pose()
    rpos, reuler = ref.bulk_pose()
    assert_bits_equal(pos[rows], rpos[rows], f"{what}: position")
    assert_bits_equal(euler[rows], reuler[rows], f"{what}: rotationEuler")
    assert_bits_equal(w.download_bodies()["linvel"][dyn], ref.bulk_bodies()["linvel"][dyn], f"{what}: linear velocity")
    assert_bits_equal(w.download_world()[rows], ref.bulk_world()[0][rows], f"{what}: world")


def _ticks_against_oracle(w, ref, wl, vel, ticks, what):
    dyn = wl.body_type == 1
    for k in range(ticks):
        w.tick(dt=DT)
        ref.PhysicsSystemUpdate(DT)
        ref.TransformSystemUpdate()
        if k == 0:
            w.set_velocities(vel)
            ref.bulk_set_velocity(vel)
        _compare(w, ref, dyn, f"{what}, tick {k}")


def test_flat_matches_oracle():
    wl, vel = _flat_scene()
    ref = build_oracle(wl)
    with B.World() as w:
        w.load(wl)
        # the seeding tick and three ticks with the velocities in place (the last two on the translation-row path)
        _ticks_against_oracle(w, ref, wl, vel, 4, "flat")


@pytest.mark.parametrize("gravity", [(1.0, -9.81, 2.0), (0.0, 0.0, 0.0)])
def test_flat_matches_numpy_under_other_gravity(gravity):
    """v += ((g / m^-1) * m^-1) * dt; x += v * dt in binary32, one rounding per operation (btRigidBody::setGravity divides,
    applyGravity and the solver write-back multiply).  With x and z components every velocity line is written; with no gravity
    at all none is — the positions still move."""
    wl, vel = _flat_scene()
    mass = np.random.default_rng(3).choice([0.3, 1.0, 2.5], N_FLAT).astype(F)
    inv = F(1.0) / mass
    dt = F(DT)
    imp = [((F(g) / inv).astype(F) * inv).astype(F) * dt for g in gravity]
    with B.World() as w:
        w.set_topology(wl.parent)
        w.upload_trs(wl.pos, wl.euler, wl.scale)
        w.upload_bodies(wl.body_type, mass=mass)
        w.tick(dt=DT, gravity=gravity)
        w.set_velocities(vel)
        pos, _ = w.download_pose()
        v = vel.copy()
        for k in range(3):
            w.tick(dt=DT, gravity=gravity)
            for a in range(3):
                v[:, a] = v[:, a] + imp[a]
                pos[:, a] = pos[:, a] + v[:, a] * dt
            assert_bits_equal(w.download_bodies()["linvel"], v, f"gravity {gravity}, tick {k}: linear velocity")
            assert_bits_equal(w.download_pose()[0], pos, f"gravity {gravity}, tick {k}: position")
            assert_bits_equal(w.download_world()[:, 12:15], pos, f"gravity {gravity}, tick {k}: translation row")


@pytest.mark.parametrize("name,n", [("chains4", 1024), ("subtree64", 640)])
def test_hierarchies_match_oracle(name, n):
    wl = synth.config(name, n=n)
    ref = build_oracle(wl)
    with B.World() as w:
        w.load(wl)
        _ticks_against_oracle(w, ref, wl, wl.vel, 4, name)


def test_topology_edit_between_ticks_matches_oracle():
    """Re-parenting moves subtrees to other slots and a removed Transform frees one: the velocities travel with their bodies."""
    n = 1024
    wl = synth.config("chains4", n=n)
    dyn = wl.body_type == 1
    ref = build_oracle(wl)
    parent = wl.parent.copy()
    has_transform = np.ones(n, np.uint8)
    with B.World() as w:
        w.load(wl)
        _ticks_against_oracle(w, ref, wl, wl.vel, 3, "before the edit")
        for c, p in ((8, 3), (400, 130), (404, 401), (900, 2)):     # roots (with their bodies and chains) under other entities
            parent[c] = p
            ref.SetParent(c + 1, p + 1)
        for c in (65, 513):                                          # children become roots
            parent[c] = 0xFFFFFFFF
            ref.SetParent(c + 1, 0)
        for e in (7, 255, 259, 1023):                                # leaves without a body lose their Transform
            assert wl.body_type[e] == 255 and not (parent == e).any()
            ref.RemoveTransform(e + 1)
            has_transform[e] = 0
        w.set_topology(parent, has_transform)
        rows = has_transform == 1
        for k in range(3):
            w.tick(dt=DT)
            ref.PhysicsSystemUpdate(DT)
            ref.TransformSystemUpdate()
            _compare(w, ref, dyn, f"after the edit, tick {k}", rows)


def test_ground_contacts_match_oracle():
    """512 boxes dropped onto the plane from a few centimetres: k_ground and the solver read and write the velocities."""
    n = 512
    rng = np.random.default_rng(21)
    wl = synth.config("flat1m", n=n)
    wl.pos[:, 0] = rng.uniform(-30, 30, n).astype(F)
    wl.pos[:, 2] = rng.uniform(-30, 30, n).astype(F)
    wl.pos[:, 1] = rng.uniform(0.3, 0.6, n).astype(F)
    wl.euler[rng.random(n) < 0.2] = 0.0
    shape = np.zeros(n, np.uint8)
    size = rng.uniform(0.2, 0.6, (n, 3)).astype(F)
    mass = rng.choice([0.3, 1.0, 2.5], n).astype(F)
    ref = build_oracle(wl, shape=shape, size=size, mass=mass)
    ref.SetGroundPlane(True)
    touched = 0
    with B.World() as w:
        w.set_topology(wl.parent)
        w.upload_trs(wl.pos, wl.euler, wl.scale)
        w.upload_bodies(wl.body_type, mass=mass, shape=shape, size=size)
        w.set_ground_plane(True)
        for tick in range(40):
            ref.PhysicsSystemUpdate(DT)
            ref.TransformSystemUpdate()
            w.tick(dt=DT)
            rb, gb = ref.bulk_bodies(), w.download_bodies()
            assert_bits_equal(gb["linvel"], rb["linvel"], f"tick {tick}: linear velocity")
            assert_bits_equal(gb["angvel"], rb["angvel"], f"tick {tick}: angular velocity")
            assert_bits_equal(gb["quat"], rb["quat"], f"tick {tick}: quaternion")
            assert_bits_equal(w.download_pose()[0], ref.bulk_pose()[0], f"tick {tick}: position")
            touched = max(touched, int((w.download_contacts()[0] > 0).sum()))
        assert_bits_equal(w.download_world(), ref.bulk_world()[0], "world matrices at the end")
    assert touched > n // 2, f"only {touched} of {n} boxes reached the plane"
