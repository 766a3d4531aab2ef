"""The sharded broadphase on the device, stage by stage, against the numpy model of tests/refmodel/slabs.py: bounds, histogram,
route counts, the packed records, the windowed pair search on records the test writes itself, one world searching every slab of
its own scene, and the error paths.  The model is fed the device's own AABBs (download_bodies), so every comparison is exact
except the histogram's, which is held between two float64 counts (slabs.hist_sandwich).  The model itself is checked against the
oracle in tests/test_slab_stages_cpu.py, on the same scenes, cut sets and batches (tests/refmodel/slab_cases.py)."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu

import banggameengine_amd as B  # noqa: E402
from banggameengine_amd import sharding  # noqa: E402
from banggameengine_amd import world as W  # noqa: E402
from refmodel import slab_cases as SC  # noqa: E402
from refmodel import slab_device as SD  # noqa: E402
from refmodel import slabs  # noqa: E402

SCENES = {f"flat{n}": functools.partial(SC.flat, n) for n in SC.FLAT_SIZES}
SCENES.update(hierarchy=SC.hierarchy, removed=SC.removed)
ALL_SCENES = dict(SCENES, large=SC.large)
INVALID, STATE = -1, -4   # BGE_ERR_INVALID, BGE_ERR_STATE


@pytest.fixture(scope="module")
def dev():
    """name -> DeviceScene, built on first use and shared by the module: no test changes a scene's bodies."""
    made = {}

    def get(name, flags=None):
        key = (name, flags)
        if key not in made:
            made[key] = SD.DeviceScene(ALL_SCENES[name](), **({} if flags is None else {"flags": flags}))
        return made[key]
    yield get
    for d in made.values():
        d.close()


def _same_floats(got, want):
    """Bit for bit, except that a zero may have either sign."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return bool(((got == want) & ((got != 0) <= (got.view(np.uint32) == want.view(np.uint32)))).all())


# ---------------------------------------------------------------------------------------------------------------- bounds
@pytest.mark.parametrize("name", list(ALL_SCENES))
def test_bounds_equal_the_model(dev, name):
    d = dev(name)
    mn, mx, n = d.w.aabb_bounds()
    want_mn, want_mx, want_n = slabs.bounds_ref(d.aabb, d.idx)
    assert n == want_n and n > 0
    assert _same_floats(mn, want_mn) and _same_floats(mx, want_mx), (mn, want_mn, mx, want_mx)
    if name == "removed":
        mn0, mx0, n0 = d.bounds_before
        assert len(d.extremes) >= 1 and n == n0 - len(np.setdiff1d(slabs.bodies(d.aabb, d.scene.wl.body_type), d.idx)) == n0 - 101
        assert (mx < mx0).all(), "a removed body's AABB still counts"
    if name == "hierarchy":
        typed_only = (d.body_type != W.BODY_NONE) & (d.scene.has_transform == 0)
        assert typed_only.sum() >= 6 and n == (d.body_type != W.BODY_NONE).sum() - typed_only.sum(), "no Transform, no body"


def test_bounds_of_a_scene_without_bodies():
    with B.World() as w:
        w.set_topology(np.full(70, W.NO_PARENT, np.uint32), np.array([1] * 69 + [0], np.uint8))
        w.upload_trs(np.ones((70, 3), np.float32), np.zeros((70, 3), np.float32), np.ones((70, 3), np.float32))
        w.upload_bodies(np.array([W.BODY_NONE] * 69 + [W.BODY_DYNAMIC], np.uint8))     # the one typed entity has no Transform
        w.tick(dt=0.01, flags=W.TICK_ALL | W.TICK_AABBS, ticks=2)
        mn, mx, n = w.aabb_bounds()
        assert n == 0 and (mn == np.inf).all() and (mx == -np.inf).all()
        assert w.bp_route(0, np.array([0, 0.5, 1], np.float32)).tolist() == [0, 0]
        assert w.axis_histogram(0, 0.0, 1.0, 16).sum() == 0


# ---------------------------------------------------------------------------------------------------------------- histogram
@pytest.mark.parametrize("name", list(ALL_SCENES))
def test_histogram_inside_the_sandwich(dev, name):
    d = dev(name)
    mn, mx, n = d.w.aabb_bounds()
    for axis in range(3):
        x = d.aabb[d.idx, axis]
        inside = (float(np.float32(np.quantile(x, 0.2))), float(np.float32(np.quantile(x, 0.8))))
        for lo, hi in ((float(mn[axis]), float(mx[axis])), inside):
            for bins in SC.BINS[::-1]:   # descending: every call follows one with more bins, whose counts must not show through
                hist = d.w.axis_histogram(axis, lo, hi, bins)
                share = slabs.hist_sandwich(x, lo, hi, bins, hist)
                if (lo, hi) != inside:
                    assert share <= SC.NEAR_EDGE_CAP
        same = float(x[len(x) // 2])
        hist = d.w.axis_histogram(axis, same, same, 64)
        assert hist[0] == n and hist[1:].sum() == 0, "lo == hi: everything lands in bin 0"
        assert d.w.axis_histogram(axis, float(mn[axis]), float(mx[axis]), 1).tolist() == [n]


# ---------------------------------------------------------------------------------------------------------------- route and pack
def _check_route_pack(d, axis, nranks, pack=True):
    for mode, cuts in d.cut_sets(axis, nranks).items():
        routed = slabs.route_ref(d.aabb, d.idx, cuts, axis)
        want_counts = np.array([len(x) for x in routed], np.int64)
        counts = d.w.bp_route(axis, cuts).astype(np.int64)
        assert np.array_equal(counts, want_counts), f"{mode}: counts {counts.tolist()} want {want_counts.tolist()}"
        if not pack:
            continue
        counts, send = SD.route_pack(d.w, axis, cuts)
        assert np.array_equal(counts, want_counts)
        got = SD.words_of(send, int(counts.sum()))
        off = 0
        for s, ids in enumerate(routed):
            seg = got[off: off + len(ids)]
            off += len(ids)
            assert np.array_equal(slabs.sort_records(seg), slabs.sort_records(d.records_of(ids))), f"{mode}: slab {s} of {nranks}"
        if d.scene.name == "hierarchy":
            assert ((got[:, 3] - 7) % 3 == 0).all() and set(((got[:, 3] - 7) // 3).tolist()) == set(d.idx.tolist())
        kin = np.isin(got[:, 3], d.scene.gid[d.idx[d.body_type[d.idx] == W.BODY_KINEMATIC]])
        assert (got[kin, 10] == 0).all() and (got[:, 10] <= 1).all() and (got[:, 7] == 0).all() and (got[:, 11] == 0).all()
        if len(d.idx) > 60:
            assert kin.any() and (got[:, 10] == 1).any()


@pytest.mark.parametrize("nranks,axis", SC.RANKS_AXES)
@pytest.mark.parametrize("name", list(SCENES))
def test_route_counts_and_packed_records_equal_the_model(dev, name, nranks, axis):
    _check_route_pack(dev(name), axis, nranks)


@pytest.mark.parametrize("nranks,axis", SC.RANKS_AXES)
def test_route_counts_of_a_large_scene(dev, nranks, axis):
    _check_route_pack(dev("large"), axis, nranks, pack=False)


# ---------------------------------------------------------------------------------------------------------------- find
@pytest.fixture(scope="module")
def finder():
    """One world for every crafted batch: its record capacity grows with the largest batch and stays."""
    with B.World(pair_capacity=1 << 18) as w:
        w.set_topology(np.full(4, W.NO_PARENT, np.uint32))
        yield w


def _check_batch(w, recs):
    """Every window on every axis; returns the device's answers by (axis, label)."""
    out = {}
    p = slabs.pair_indices(recs)   # (a zero's sign changes no overlap: the rewritten batches have the same record pairs)
    for axis in range(3):
        for label, r, window in SC.find_cases(recs, axis):
            buf = SD.to_device(r)
            got = SD.find(w, buf, 0, len(r), axis, window)
            want = slabs.pairs_ref(r, axis, window, p)
            assert np.array_equal(got, want), f"{len(recs)} records, axis {axis}, window {label}: {len(got)} pairs, want {len(want)}"
            out[axis, label] = got
    return out


def test_find_on_crafted_batches_in_growing_and_shrinking_order(finder):
    """3000, 2, 257, 0, 3000 records through one world; ids from 0xFFFF0000 up come back as unsigned numbers."""
    seen = {}
    for n in SC.FIND_ORDER:
        got = _check_batch(finder, SC.lattice(n))
        if n in seen:
            assert all(a.tobytes() == got[k].tobytes() for k, a in seen[n].items())
        seen[n] = got
    big = seen[3000][0, "all"]
    assert len(big) > 5000 and (big[:, 0] >= SC.LATTICE_ID_BASE).all() and (big[:, 0] < big[:, 1]).all()
    assert len(seen[0][0, "all"]) == 0 and len(seen[2][0, "all"]) <= 1


@pytest.mark.parametrize("n", [1, 255, 256])
def test_find_on_small_batches(finder, n):
    _check_batch(finder, SC.lattice(n))


def test_find_hand_batch_and_no_records(finder):
    buf = SD.to_device(SC.HAND_RECORDS)
    assert np.array_equal(SD.find(finder, buf, 0, 6, SC.HAND_AXIS, SC.HAND_WINDOW), SC.HAND_PAIRS)
    assert np.array_equal(SD.find(finder, buf, 0, 6, SC.HAND_AXIS, (-np.inf, np.inf)), SC.HAND_PAIRS_NO_WINDOW)
    finder.bp_find(0, 0, 0, -np.inf, np.inf)      # no records, NULL pointer
    finder.sync()
    assert len(finder.pairs()) == 0 and finder.pair_count() == 0
    # a later record of the buffer as the start: the segment form the slabs use
    assert np.array_equal(SD.find(finder, buf, 1, 5, SC.HAND_AXIS, SC.HAND_WINDOW), SC.HAND_PAIRS[:2])


# ---------------------------------------------------------------------------------------------------------------- one world, N slabs
@pytest.fixture(scope="module")
def one_world(dev):
    """flat(1500) ticked with TICK_BROADPHASE: its local pair set is the oracle's (ids are the entity indices)."""
    d = dev("flat1500", W.TICK_ALL | W.TICK_AABBS | W.TICK_BROADPHASE)
    local = d.w.pairs(cap=64 * d.scene.n)
    assert len(local) > 1000 and np.array_equal(local, SC.oracle_state(SC.flat(1500))[2])
    return d


def _local_pairs(d):
    """A BROADPHASE tick of dt = 0 and the pair set it must leave in pairs(): the model's over the AABBs the world holds now."""
    d.w.tick(dt=0.0, flags=W.TICK_PHYSICS | W.TICK_BROADPHASE)
    d.refresh()
    local = d.w.pairs(cap=64 * d.scene.n)
    assert np.array_equal(local, slabs.pairs_ref(d.records_of(d.idx), 0, (-np.inf, np.inf))), "pairs() is not the local set"
    return local


@pytest.mark.parametrize("nranks,axis", SC.RANKS_AXES)
def test_one_world_searches_every_slab_of_its_own_scene(one_world, nranks, axis):
    d, w = one_world, one_world.w
    local = _local_pairs(d)
    assert len(local) > 1000
    for mode, cuts in d.cut_sets(axis, nranks).items():
        counts, send = SD.route_pack(w, axis, cuts)
        per_slab = []
        for s in range(nranks):
            per_slab.append(SD.find(w, send, int(counts[:s].sum()), int(counts[s]), axis, sharding.slab_window(cuts, s), cap=64 * d.scene.n))
        got, dups = slabs.union_of_slabs(per_slab)
        assert dups == 0, f"{mode}: {dups} pairs reported by two slabs"
        assert np.array_equal(got, local), f"{mode}: {len(got)} pairs over {nranks} slabs, the local search has {len(local)}"
    assert np.array_equal(_local_pairs(d), local), "a BROADPHASE tick makes pairs() the local set again"


# ---------------------------------------------------------------------------------------------------------------- errors
def test_bad_arguments_are_refused_and_leave_the_world_usable(dev):
    d = dev("flat257")
    w = d.w
    mn, mx, n = w.aabb_bounds()
    good = sharding.uniform_cuts(float(mn[0]), float(mx[0]), 3)
    nan_cut, decreasing = good.copy(), good.copy()
    nan_cut[1] = np.nan
    decreasing[1], decreasing[2] = good[2], good[1]
    assert decreasing[2] < decreasing[1]
    assert SD.rc_route(w, 0, 3, nan_cut) == INVALID
    assert SD.rc_route(w, 0, 3, decreasing) == INVALID
    assert SD.rc_route(w, 0, 0, good) == INVALID
    assert SD.rc_route(w, 0, 65, np.zeros(66, np.float32)) == INVALID
    assert SD.rc_route(w, 3, 3, good) == INVALID
    assert SD.rc_histogram(w, 0, 0.0, 1.0, 0) == INVALID
    assert SD.rc_histogram(w, 0, 0.0, 1.0, 4097) == INVALID
    assert SD.rc_histogram(w, 3, 0.0, 1.0, 16) == INVALID
    assert SD.rc_histogram(w, 0, 1.0, 0.0, 16) == INVALID
    assert SD.rc_histogram(w, 0, float("nan"), 1.0, 16) == INVALID
    with pytest.raises(B.BgeError) as e:
        w.bp_find(0, 5, 0, 0.0, 1.0)               # records announced, none given
    assert e.value.code == INVALID
    with pytest.raises(B.BgeError) as e:
        w.bp_find(0, 0, 3, 0.0, 1.0)
    assert e.value.code == INVALID
    # call order
    assert SD.rc_pack(w, 0) == STATE               # a refused bp_route counts for nothing
    assert SD.rc_route(w, 0, 3, good) == 0
    assert SD.rc_pack(w, 0) == INVALID             # records to send and no buffer
    counts, send = SD.route_pack(w, 0, good)
    assert SD.rc_pack(w, send.data_ptr()) == STATE  # twice
    # ... and the world still does its work
    _check_route_pack(d, 0, 3)
    got = [SD.find(w, send, int(counts[:s].sum()), int(counts[s]), 0, sharding.slab_window(good, s)) for s in range(3)]
    want = [slabs.pairs_ref(d.records_of(ids), 0, sharding.slab_window(good, s)) for s, ids in enumerate(slabs.route_ref(d.aabb, d.idx, good, 0))]
    assert all(np.array_equal(g, x) for g, x in zip(got, want)) and sum(len(g) for g in got) > 500
