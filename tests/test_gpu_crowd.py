"""The crowd query on the device (include/bge_world.h "Crowd separation", bge_world_crowd_query*).

The reference is crowd_ref of refmodel/crowd.py — the header's rule in numpy float32 over all pairs.  The answer is a maximum with a
stated tie and an integer count, so every comparison is byte for byte, and every case runs through the hashed grid
(BGE_CROWD_GRID_MIN=1) and through all pairs (a value above n): the variable is read per call."""
from __future__ import annotations

import numpy as np
import pytest

import banggameengine_amd as B
from banggameengine_amd import world as W

from refmodel.crowd import PUSHED, crowd_ref
from refmodel.crowd_cases import (BATCH_MAX_PUSH, BATCHES, COVERED, HAND, SWEEP_MAGNITUDES, SWEEP_POINTS, check_crowd_coverage, check_shape, far_batch,
                                  seeded_batch, sweep_batch)
from refmodel.rays import NO_ENTITY

pytestmark = pytest.mark.gpu

PATHS = {"grid": "1", "all pairs": str(1 << 31)}


@pytest.fixture(scope="module")
def w():
    world = B.World(device=0)  # (no topology: the query needs none)
    yield world
    world.close()


@pytest.fixture(params=list(PATHS))
def path(request, monkeypatch):
    monkeypatch.setenv("BGE_CROWD_GRID_MIN", PATHS[request.param])
    return request.param


def assert_equal_records(got, want, what):
    bad = [i for i in range(len(want)) if got[i].tobytes() != want[i].tobytes()]
    assert not bad, f"{what}: {len(bad)} of {len(want)} differ, first {bad[0]}: {got[bad[0]]} vs {want[bad[0]]}"


_wanted = {}


def wanted(key, spheres, max_push):
    """crowd_ref's answer, computed once per batch and shared by the two paths."""
    if key not in _wanted:
        _wanted[key] = crowd_ref(spheres, max_push)
    return _wanted[key]


@pytest.mark.parametrize("name", list(HAND))
def test_hand_cases(w, path, name):
    spheres, max_push = HAND[name]
    assert_equal_records(w.crowd_query(spheres, max_push), wanted(name, spheres, max_push), name)


@pytest.mark.parametrize("n", BATCHES)
def test_seeded_batches_equal_the_rule_byte_for_byte(w, path, n):
    spheres = seeded_batch(n)
    got = w.crowd_query(spheres, BATCH_MAX_PUSH)
    assert_equal_records(got, wanted(n, spheres, BATCH_MAX_PUSH), f"n = {n}")
    check_shape(spheres, got, BATCH_MAX_PUSH)
    if n in COVERED:
        check_crowd_coverage(spheres, got)


def test_host_and_device_entry_and_two_calls_give_the_same_bytes(w, path):
    import torch
    spheres = seeded_batch(1000)
    first = w.crowd_query(spheres, BATCH_MAX_PUSH)
    d_spheres = torch.from_numpy(spheres.view(np.uint8).copy()).to("cuda:0")
    d_hits = torch.zeros(32 * len(spheres), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    w.crowd_query_device(d_spheres, d_hits, BATCH_MAX_PUSH)
    w.sync()
    assert d_hits.cpu().numpy().tobytes() == first.tobytes()
    assert w.crowd_query(spheres, BATCH_MAX_PUSH).tobytes() == first.tobytes()
    # 4-byte aligned is enough: the records one word into their buffers
    o_spheres = torch.zeros(24 * len(spheres) + 4, dtype=torch.uint8, device="cuda:0")
    o_hits = torch.zeros(32 * len(spheres) + 4, dtype=torch.uint8, device="cuda:0")
    o_spheres[4:] = d_spheres
    torch.cuda.synchronize()
    w.crowd_query_device(o_spheres[4:], o_hits[4:], BATCH_MAX_PUSH)
    w.sync()
    assert o_hits[4:].cpu().numpy().tobytes() == first.tobytes() and not o_hits[:4].any()


def test_257_coincident_spheres_fill_one_bucket(w, path):
    spheres = W.make_crowd_spheres(np.tile(np.float32([(3.25, 1.0, -7.5)]), (257, 1)), 0.5)
    got = w.crowd_query(spheres)
    assert (got["n_overlaps"] == 256).all() and got["other"][0] == 1 and (got["other"][1:] == 0).all()
    assert (got["depth"] == 1.0).all() and got["push"][0].tolist() == [0.5, 0, 0] and (got["push"][1:] == (-0.5, 0, 0)).all()
    assert_equal_records(got, wanted("coincident", spheres, 0.0), "coincident")


@pytest.mark.parametrize("magnitude", SWEEP_MAGNITUDES)
@pytest.mark.parametrize("axis", (0, 1, 2))
def test_boundary_sweep(w, path, axis, magnitude):
    """Pairs one float inside and one float outside touching, stepped across +-6R: wherever the implementation's cell boundaries
    lie, pairs straddle them.  The pairs are 8 apart from each other, so the reference runs pair by pair."""
    spheres, n_pairs = sweep_batch(axis, magnitude, np.random.default_rng(97 + axis))
    key = ("sweep", axis, magnitude)
    if key not in _wanted:
        want = np.concatenate([crowd_ref(spheres[2 * k:2 * k + 2]) for k in range(n_pairs)])
        hit = want["other"] != NO_ENTITY
        want["other"][hit] += (np.arange(len(want))[hit] // 2 * 2).astype(np.uint32)
        _wanted[key] = want
    want = _wanted[key]
    # the pairs just outside never overlap; of those just inside most do (where the rounded distance is below R)
    assert not want["n_overlaps"][2 * SWEEP_POINTS:].any() and (want["n_overlaps"][:2 * SWEEP_POINTS] == 1).sum() >= SWEEP_POINTS
    assert_equal_records(w.crowd_query(spheres), want, f"axis {axis} at {magnitude}")


def test_far_spheres(w, path):
    spheres = far_batch()
    want = wanted("far", spheres, 0.0)
    assert ((want["flags"] & PUSHED) != 0).tolist() == [True, True, True, True, False, False, True, True, False, False, True, True, True, True]
    assert_equal_records(w.crowd_query(spheres), want, "far")


def test_errors(w):
    import torch
    lib = B.lib()
    spheres = seeded_batch(4)
    hits = np.zeros(4, W.CROWD_HIT_DTYPE)
    vp = lambda a: a.ctypes.data  # noqa: E731
    for bad in (float("nan"), -1.0, float("inf"), -0.001):
        assert lib.bge_world_crowd_query(w._h, 4, vp(spheres), bad, vp(hits)) == -1
        assert lib.bge_world_crowd_query_device(w._h, 4, 256, bad, 512) == -1
    assert lib.bge_world_crowd_query(w._h, 4, None, 0.0, vp(hits)) == -1 and lib.bge_world_crowd_query(w._h, 4, vp(spheres), 0.0, None) == -1
    assert lib.bge_world_crowd_query(w._h, 0, None, 0.0, None) == 0 and lib.bge_world_crowd_query_device(w._h, 0, None, 0.0, None) == 0
    assert lib.bge_world_crowd_query(w._h, 1 << 30, vp(spheres), 0.0, vp(hits)) == -1
    d_spheres = torch.zeros(24 * 4 + 8, dtype=torch.uint8, device="cuda:0")
    d_hits = torch.zeros(32 * 4 + 8, dtype=torch.uint8, device="cuda:0")
    for off_s, off_h in ((1, 0), (0, 2), (3, 3)):
        assert lib.bge_world_crowd_query_device(w._h, 4, d_spheres.data_ptr() + off_s, 0.0, d_hits.data_ptr() + off_h) == -1
    assert lib.bge_world_crowd_query_device(w._h, 4, d_spheres.data_ptr() + 4, 0.0, d_hits.data_ptr() + 4) == 0
    w.sync()
