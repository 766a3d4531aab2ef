"""Shared test plumbing: run the same scene through the oracle (CPU) and the C-ABI world (GPU)."""
from __future__ import annotations

import numpy as np

from oracle import pyoracle as po

NO_PARENT = 0xFFFFFFFF
DT = float(np.float32(0.0083333333))  # assets/config/physics.json:3 as binary32


def parent_i32(parent_u32):
    p = np.asarray(parent_u32)
    return np.where(p == NO_PARENT, -1, p.astype(np.int64)).astype(np.int32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_bits_equal(got, want, what):
    g, w = bits(got), bits(want)
    if np.array_equal(g, w):
        return
    # NaNs may differ in payload/sign; everything else must match bit for bit
    gn, wn = np.isnan(got), np.isnan(want)
    bad = (g != w) & ~(gn & wn)
    if bad.any():
        idx = np.argwhere(bad)[:5]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} words differ, first at {idx.tolist()}: "
                             f"got {got[tuple(idx[0])]!r} want {want[tuple(idx[0])]!r}")


def matrix_rel_err(got, want):
    """Norm-relative error per 4x4 matrix: max |got-want| / max(|want|)."""
    got = np.asarray(got, np.float64).reshape(-1, 16)
    want = np.asarray(want, np.float64).reshape(-1, 16)
    scale = np.maximum(np.abs(want).max(axis=1), 1e-30)
    return (np.abs(got - want).max(axis=1) / scale).max() if len(got) else 0.0


def build_oracle(wl, orient_mode=po.ORIENT_IDEAL, aabbs=False, has_transform=None, **body_kw):
    ref = po.RefScene()
    ref.SetPhysicsOptions(-9.81, orient_mode, aabbs)
    ref.bulk_build(parent_i32(wl.parent), wl.pos, wl.euler, wl.scale, has_transform=has_transform,
                   body_type=wl.body_type, **body_kw)
    return ref


def build_island_oracle(case, basis=False):
    """The oracle's scene of a case of refmodel/island_cases.py: plane and obstacle contacts as the case says, Dynamic boxes
    against each other on."""
    ref = build_oracle(case.wl, orient_mode=po.ORIENT_BASIS if basis else po.ORIENT_IDEAL, has_transform=case.has_transform, size=case.size, mass=case.mass)
    ref.SetGroundPlane(case.plane)
    ref.SetStaticContacts(case.static)
    ref.SetDynamicContacts(True)
    return ref


def run_oracle(ref, wl, ticks, seed_velocity=True, physics=True, angvel=None):
    for k in range(ticks):
        if physics:
            ref.PhysicsSystemUpdate(DT)
        ref.TransformSystemUpdate()
        if k == 0 and seed_velocity and physics:
            ref.bulk_set_velocity(wl.vel, angvel)
    return ref


def run_world(world, wl, ticks, seed_velocity=True, flags=3, angvel=None):
    for k in range(ticks):
        world.tick(dt=DT, flags=flags)
        if k == 0 and seed_velocity and (flags & 1):
            world.set_velocities(wl.vel, angvel)
    return world


def build_obstacle_oracle(case, basis=False):
    """The oracle's scene of a case of refmodel/obstacle_cases.py: plane as the case says, obstacle contacts on, Dynamic boxes against
    each other off (every body is an island of its own: k_ground_select / k_contact_boxes do all the work)."""
    ref = build_oracle(case.wl, orient_mode=po.ORIENT_BASIS if basis else po.ORIENT_IDEAL, has_transform=case.has_transform, size=case.size, mass=case.mass)
    ref.SetGroundPlane(case.plane)
    ref.SetStaticContacts(case.static)
    if case.sub_steps:
        ref.SetAccumulator(True, DT, 4)
    return ref


def compare_obstacle_world(w, ref, tick, dyn, plane, bodies=None):
    """A world of Dynamic boxes on Static / Kinematic boxes against the oracle after a tick, bit for bit: activation states, the
    timers of awake bodies, position, rotationEuler, quaternion, both velocities, and of EVERY Dynamic body (dyn: a mask; bodies:
    the entity indices to take instead, for a world of many thousands) the plane manifold and every box manifold — partner, point count,
    points, impulses; rows beyond a body's manifolds must be free.  Returns the manifolds per body (n,)."""
    rb, gb = ref.bulk_bodies(), w.download_bodies()
    ex = rb["exists"]
    pos, euler = w.download_pose()
    rpos, reuler = ref.bulk_pose()
    st, tm = w.download_activation()
    rst, rtm = ref.bulk_activation()
    assert np.array_equal(st[ex], rst[ex].astype(np.uint8)), f"tick {tick}: activation states differ at {np.flatnonzero(ex)[st[ex] != rst[ex]][:8]}"
    assert_bits_equal(gb["linvel"][dyn], rb["linvel"][dyn], f"tick {tick}: linear velocity")
    assert_bits_equal(gb["angvel"][dyn], rb["angvel"][dyn], f"tick {tick}: angular velocity")
    assert_bits_equal(pos, rpos, f"tick {tick}: position")
    assert_bits_equal(gb["quat"][ex], rb["quat"][ex], f"tick {tick}: quaternion")
    assert_bits_equal(euler, reuler, f"tick {tick}: rotationEuler")
    assert_bits_equal(tm[ex & (rst == 1)], rtm[ex & (rst == 1)], f"tick {tick}: deactivation timers")
    nb, bh, bp = w.download_box_contacts()
    cn, cpts = w.download_contacts() if plane else (None, None)
    for e in (np.flatnonzero(dyn) if bodies is None else bodies):
        want = ref.BoxContacts(int(e) + 1)
        assert nb[e] == len(want), f"tick {tick}: body {e} has {nb[e]} box manifolds {bh[e].tolist()}, oracle {[(o - 1, len(r)) for o, r in want]}"
        for k, (other, rows) in enumerate(want):
            assert bh[e, k, 0] == other - 1 and bh[e, k, 1] == len(rows), f"tick {tick}: body {e} manifold {k}: {bh[e, k]} vs oracle ({other - 1}, {len(rows)})"
            assert_bits_equal(bp[e, k, :len(rows)], rows, f"tick {tick}: body {e} manifold {k} points")
        assert (bh[e, len(want):, 0] == NO_PARENT).all() and (bh[e, len(want):, 1] == 0).all(), f"tick {tick}: body {e} reports rows beyond its manifolds"
        if plane:
            rn, rpts2 = ref.GroundContacts(int(e) + 1)
            assert cn[e] == rn, f"tick {tick}: body {e} has {cn[e]} plane contacts, oracle {rn}"
            assert_bits_equal(cpts[e, :rn], rpts2, f"tick {tick}: plane contact points of body {e}")
    return nb


def compare_dynamic_world(w, ref, tick, dyn, plane, static):
    """A world with Dynamic-against-Dynamic contacts against the oracle after a tick, bit for bit: activation states, the pair cache
    (which pairs, their points, their impulses), velocities, position, quaternion, rotationEuler, the timers of awake bodies, and of
    every third Dynamic body the plane manifold (plane) and the obstacle manifolds (static).  Returns (states, pair header)."""
    rb, gb = ref.bulk_bodies(), w.download_bodies()
    ex = rb["exists"]
    pos, euler = w.download_pose()
    rpos, reuler = ref.bulk_pose()
    st, tm = w.download_activation()
    rst, rtm = ref.bulk_activation()
    assert np.array_equal(st[ex], rst[ex].astype(np.uint8)), f"tick {tick}: activation states differ at {np.flatnonzero(st[ex] != rst[ex])[:8]}"
    hdr, pts = w.download_dynamic_pairs()
    rhdr, rpts = ref.DynamicPairs()
    rhdr = rhdr.copy()
    rhdr[:, :2] -= 1                                                          # entity id -> index
    assert hdr.shape == rhdr.shape and np.array_equal(hdr, rhdr), f"tick {tick}: pair cache {hdr.tolist()[:6]} vs oracle {rhdr.tolist()[:6]}"
    assert_bits_equal(pts, rpts, f"tick {tick}: points of the pair manifolds")
    assert_bits_equal(gb["linvel"][dyn], rb["linvel"][dyn], f"tick {tick}: linear velocity")
    assert_bits_equal(gb["angvel"][dyn], rb["angvel"][dyn], f"tick {tick}: angular velocity")
    assert_bits_equal(pos, rpos, f"tick {tick}: position")
    assert_bits_equal(gb["quat"][ex], rb["quat"][ex], f"tick {tick}: quaternion")
    assert_bits_equal(euler, reuler, f"tick {tick}: rotationEuler")
    assert_bits_equal(tm[ex & (rst == 1)], rtm[ex & (rst == 1)], f"tick {tick}: deactivation timers")
    if plane:
        cn, cpts = w.download_contacts()
        for e in np.flatnonzero(dyn)[::3]:
            rn, rpts2 = ref.GroundContacts(int(e) + 1)
            assert cn[e] == rn, f"tick {tick}: body {e} has {cn[e]} plane contacts, oracle {rn}"
            assert_bits_equal(cpts[e, :rn], rpts2, f"tick {tick}: plane contact points of body {e}")
    if static:
        nb, bh, bp = w.download_box_contacts()
        for e in np.flatnonzero(dyn)[::3]:
            want = ref.BoxContacts(int(e) + 1)
            assert nb[e] == len(want), f"tick {tick}: body {e} has {nb[e]} box manifolds, oracle {len(want)}"
            for k, (other, rows) in enumerate(want):
                assert bh[e, k, 0] == other - 1 and bh[e, k, 1] == len(rows)
                assert_bits_equal(bp[e, k, :len(rows)], rows, f"tick {tick}: body {e} manifold {k} points")
    return st, hdr
