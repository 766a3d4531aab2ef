"""The query index on the device (include/bge_world.h "Query index", bge_world_set_query_index ..).

The reference is the same world with the index off: every answer must keep its bytes.  After every indexed call the stats must say
that the index WAS built, and for the cases of refmodel/qindex_cases.py that it routed what the numpy model of the rule
(refmodel/qindex.py) predicts — bodies in cells, bodies on the wide list, queries far: equal bytes from a path that silently fell
back would prove nothing."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import banggameengine_amd as B
from banggameengine_amd import world as W

from refmodel import qindex as Q
from refmodel.qindex_cases import (ALL, BATCH_SIZES, ENTRIES, GRID_SEED, N_BODIES, N_QUERIES, SWEEP, check_claims, coincident_and_colliding,
                                   grid_queries, grid_scene, nan_queries, predicted, touching_pairs)
from refmodel.qindex_device import assert_same, members, off_and_on
from refmodel.device import FLAGS, ask
from refmodel.layout_device import LayoutScene

pytestmark = pytest.mark.gpu


def static_world(pos, shape, size, layer=None, kind=None, plane=True):
    n = len(pos)
    w = B.World(device=0)
    w.set_topology(np.full(n, W.NO_PARENT, np.uint32))
    w.upload_trs(pos, np.zeros((n, 3)), np.ones((n, 3)))
    w.upload_bodies(np.full(n, W.BODY_STATIC, np.uint8) if kind is None else kind, None, shape, size,
                    np.full(n, 1, np.uint32) if layer is None else layer, np.full(n, ALL, np.uint32))
    w.set_ground_plane(plane)
    w.tick(flags=FLAGS)
    return w


class Grid:
    def __init__(self):
        rng = np.random.default_rng(GRID_SEED)
        self.sc = grid_scene(rng)
        n = len(self.sc["pos"])
        kind = np.where(self.sc["dynamic"], W.BODY_DYNAMIC, W.BODY_STATIC).astype(np.uint8)
        kind[N_BODIES:] = W.BODY_NONE
        self.member = kind != W.BODY_NONE
        self.w = static_world(self.sc["pos"], self.sc["shape"], self.sc["size"], self.sc["layer"], kind)
        g = np.arange(N_BODIES, n, dtype=np.uint32)
        self.w.upload_triggers(g, np.uint8([0, 1]), np.float32([[1.0, 1.0, 1.0], [0.7, 0.8, 0.7]]), np.uint32([8, 8]), np.uint32([ALL] * 2),
                               np.uint8([0, 0]), np.uint8([1, 1]))
        self.w.tick(flags=FLAGS)
        self.pos = self.w.download_pose()[0].astype(np.float32)  # (dynamic bodies fell for two ticks)
        self.queries = grid_queries(rng, self.sc["pos"])

    def args(self, entry, n=None):
        return tuple(a[:n] for a in self.queries[entry])

    def run(self, entry, n=None):
        return getattr(self.w, entry)(*self.args(entry, n))

    def predicted(self, entry, n, cell_edge, max_cells):
        return predicted(entry, self.args(entry, n), self.pos, self.sc["shape"], self.sc["size"], self.member, cell_edge, max_cells)


@pytest.fixture(scope="module")
def grid():
    g = Grid()
    yield g
    g.w.close()


def check_stats(st, want, passes=1):
    assert (st["bodies_indexed"], st["bodies_wide"]) == (want["bodies_indexed"], want["bodies_wide"]), (st, want)
    assert (st["queries_indexed"], st["queries_far"]) == (passes * want["queries_indexed"], passes * want["queries_far"]), (st, want)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("case", SWEEP, ids=[c[0] for c in SWEEP])
def test_sweep_of_cell_edge_and_max_cells(grid, case, entry):
    name, cell_edge, max_cells, wide_claim, far_claim = case
    off, on, st = off_and_on(grid.w, lambda: grid.run(entry), cell_edge=cell_edge, max_cells=max_cells)
    assert_same(off, on, f"{entry}, {name}")
    want = grid.predicted(entry, None, cell_edge, max_cells)
    print(f"{name}, {entry}: {st}")
    check_stats(st, want)
    assert st["cell_edge"] == Q.edge(cell_edge) and st["table_size"] == Q.table_size(grid.w.info()["n_slots"])
    check_claims(name, entry, wide_claim, far_claim, N_BODIES, N_QUERIES, nan_queries(entry, grid.args(entry)), st)


@pytest.mark.parametrize("n", BATCH_SIZES)
@pytest.mark.parametrize("entry", ENTRIES)
def test_batch_sizes(grid, entry, n):
    off, on, st = off_and_on(grid.w, lambda: grid.run(entry, n), cell_edge=4.0, max_cells=512)
    assert_same(off, on, f"{entry}, batch of {n}")
    check_stats(st, grid.predicted(entry, n, 4.0, 512))


def test_min_work_keeps_small_batches_on_the_all_bodies_pass(grid):
    w, slots = grid.w, grid.w.info()["n_slots"]
    try:
        w.set_query_index(True, min_work=64 * slots)
        builds = w.query_index_stats()["builds"]
        a = grid.run("sphere_cast", 63)
        st = w.query_index_stats()
        assert st["built"] == 0 and st["builds"] == builds
        b = grid.run("sphere_cast", 64)
        st = w.query_index_stats()
        assert st["built"] == 1 and st["builds"] == builds + 1
        assert_same(a, {k: v[:63] for k, v in b.items()}, "sphere_cast")
    finally:
        w.set_query_index(False)


@pytest.mark.parametrize("kind", ("rays", "spheres"))
def test_layout_scene_host_entry_device_entry_and_a_second_call(kind):
    """Shuffled slots, slots beyond the entity count, ghosts, the plane: all five answers of refmodel.device.ask (which also holds
    the device forms of the closest-hit queries to the host forms), twice."""
    sc = LayoutScene()
    try:
        sc.tick(6)
        batches = sc.batches("layout")
        off, on, st = off_and_on(sc.w, lambda: ask(sc.w, batches))
        assert_same(off, on, "layout scene")
        assert st["bodies_indexed"] + st["bodies_wide"] == members(sc) and st["bodies_wide"] > 0 and st["queries_indexed"] > 0
        _, again, _ = off_and_on(sc.w, lambda: ask(sc.w, batches))
        assert_same(on, again, "second call")
        pen = lambda: sc.w.sphere_penetration(*batches[2])
        assert_same(*off_and_on(sc.w, pen)[:2], "penetration")
    finally:
        sc.close()


def test_coincident_bodies_and_cells_that_share_a_bucket():
    """257 bodies at one place fill one bucket over five strides of a wave; a second group stands exactly table * h away and a
    third in a nearby cell that the model says hashes to the first group's bucket.  A query that visits both colliding cells meets
    that bucket twice; every list must have the length it has without the index."""
    h, table = 2.0, 1024
    pos, off = coincident_and_colliding(table, h)
    n = len(pos)
    cells = Q.cell(pos, h)
    buckets = Q.bucket(cells[:, 0], cells[:, 1], cells[:, 2], table)
    assert buckets[0] == buckets[-1] and not np.array_equal(cells[0], cells[-1]), "the model predicts no collision"
    print(f"buckets: first group {buckets[0]}, group at table * h {buckets[257]}, group {off.tolist()} cells away {buckets[-1]}")
    w = static_world(pos, np.zeros(n, np.uint8), np.full((n, 3), 0.3, np.float32), plane=False)
    try:
        assert Q.table_size(w.info()["n_slots"]) == table
        gap = float(np.linalg.norm(pos[-1] - pos[0]))
        c = np.float32([pos[0], pos[257], pos[-1], pos[0] + [1.0, 0, 0], (pos[0] + pos[-1]) / 2])
        r = np.float32([0.5, 0.5, 0.5, 1.0, gap / 2 + 0.2])
        off_a, on_a, st = off_and_on(w, lambda: w.overlap_sphere(c, r, ALL), cell_edge=h, max_cells=1 << 20)
        assert_same(off_a, on_a, "overlap")
        counts = np.diff(on_a["offsets"].astype(np.int64)).tolist()
        assert counts == [257, 8, 8, 257, 265] and st["bodies_wide"] == 0 and st["queries_far"] == 0, (counts, st)
        assert Q.classify("overlap", dict(origin=c, radius=r), h, 1 << 20).sum() == 0
        d = ((pos[-1] - pos[0]) / gap).astype(np.float32)
        o = np.float32([pos[0] - 3.0 * d] * 2)
        md = np.float32([4.0, gap + 6.0])
        for fn, want in ((lambda: w.raycast_all(o, [d, d], md, ALL), [257, 265]), (lambda: w.sphere_cast_all(o, [d, d], md, 0.2, ALL), [257, 265])):
            off_a, on_a, st = off_and_on(w, fn, cell_edge=h, max_cells=1 << 20)
            assert_same(off_a, on_a, "list")
            assert np.diff(on_a["offsets"].astype(np.int64)).tolist() == want and st["queries_far"] == 0, st
        assert_same(*off_and_on(w, lambda: w.sphere_cast(o, [d, d], md, 0.2, ALL), cell_edge=h)[:2], "sphere_cast")
    finally:
        w.close()


@pytest.mark.parametrize("kind", ("overlap", "cast", "ray", "penetration"))
def test_one_float_inside_and_outside_touching(kind):
    """Per axis, at magnitudes 1, 1e3 and 1e5: the query touches the body's cull sphere to within a float.  The cell edge is 2: the
    bodies at 1e5 carry a position term above 1 and are wide, by the rule."""
    rng = np.random.default_rng(5)
    n = 384
    q, c, rad, _ = touching_pairs(kind, rng, n, magnitudes=(1.0, 1e3, 1e5))
    rad = np.minimum(rad, np.float32(0.9))
    w = static_world(c, np.ones(n, np.uint8), np.stack([rad, np.zeros(n, np.float32), rad], 1), plane=False)
    try:
        passes = Q.cull(kind, q, c, Q.body_rb(np.maximum(rad, np.float32(0.01)), c))
        assert 0.2 * n < passes.sum() < 0.95 * n, "the pairs are not at the edge of the cull"
        if kind in ("ray", "cast"):
            args = (q["origin"], q["direction"], q["max_distance"]) + ((q["radius"],) if kind == "cast" else ()) + (ALL,)
            fns = [lambda: w.raycast(*args), lambda: w.raycast_all(*args)] if kind == "ray" else [lambda: w.sphere_cast(*args), lambda: w.sphere_cast_all(*args)]
        else:
            args = (q["origin"], q["radius"], ALL)
            fns = [lambda: w.overlap_sphere(*args)] if kind == "overlap" else [lambda: w.sphere_penetration(*args)]
        for fn in fns:
            off, on, st = off_and_on(w, fn, cell_edge=2.0, max_cells=4096)
            assert_same(off, on, kind)
            wide = Q.is_wide(Q.body_rb(np.maximum(rad, np.float32(0.01)), c), 2.0)
            assert st["bodies_wide"] == wide.sum() and 0 < st["bodies_wide"] < n and st["queries_indexed"] > 0, st
    finally:
        w.close()


def test_bodies_at_3e9_at_1e30_and_with_a_nan_position(grid):
    sc = grid.sc
    pos = sc["pos"][:N_BODIES].copy()
    pos[0] = [3e9, 1.0, 0.0]
    pos[1] = [1e30, 1.0, -1e30]
    pos[2] = [np.nan, 1.0, 0.0]
    pos[3, 1] = np.inf
    w = static_world(pos, sc["shape"][:N_BODIES], sc["size"][:N_BODIES], sc["layer"][:N_BODIES], plane=True)
    try:
        extra_o = np.float32([[3e9, 50.0, 0.0], [1e30, 5.0, -1e30], [3e9 - 600.0, 1.0, 0.0], [0.0, 1.0, 0.0]])
        extra_d = np.float32([[0, -1, 0], [0, -1, 0], [1, 0, 0], [1, 0, 0]])
        extra_md = np.float32([100.0, 10.0, 1200.0, 3.4e38])
        o, d, md, rad, mask = grid.args("sphere_cast")
        o, d, md = np.concatenate([o, extra_o]), np.concatenate([d, extra_d]), np.concatenate([md, extra_md])
        rad, mask = np.concatenate([rad, np.float32([0.3, 0.3, 0.3, 0.3])]), np.concatenate([mask, np.full(4, ALL, np.uint32)])
        c = np.concatenate([grid.args("overlap_sphere")[0], np.float32([[3e9, 1.0, 0.0], [1e30, 1.0, -1e30], [0, 0, 0]])])
        r = np.concatenate([grid.args("overlap_sphere")[1], np.float32([500.0, 1e25, 3e38])])
        for fn in (lambda: w.raycast(o, d, md, mask), lambda: w.raycast_all(o, d, md, mask), lambda: w.sphere_cast(o, d, md, rad, mask),
                   lambda: w.sphere_cast_all(o, d, md, rad, mask), lambda: w.overlap_sphere(c, r, ALL), lambda: w.sphere_penetration(c, r, ALL)):
            off, on, st = off_and_on(w, fn, cell_edge=4.0, max_cells=512)
            assert_same(off, on, "far-away bodies")
            assert st["bodies_wide"] == 4 and st["bodies_indexed"] == N_BODIES - 4 and st["queries_far"] >= 3, st
        hit = w.raycast(extra_o[:1], extra_d[:1], extra_md[:1], ALL)
        assert hit["entity"][0] == 0, "the body at 3e9 is not hit at all: the case tests nothing"
    finally:
        w.close()


def test_a_list_that_outgrows_its_capacity_is_run_again(grid):
    sc = grid.sc
    c = np.float32([[24.0, 1.0, 24.0]] * 8)
    answers = []
    for on in (False, True):
        w = static_world(sc["pos"][:N_BODIES], sc["shape"][:N_BODIES], sc["size"][:N_BODIES], sc["layer"][:N_BODIES])
        try:
            w.set_query_index(on, cell_edge=2.0, max_cells=512, min_work=0)
            spheres, total = W.make_spheres(c, 100.0, ALL), C.c_uint64(0)  # 8 x 601 records against a fresh list of 4096
            assert B.lib().bge_world_overlap_sphere(w._h, 8, spheres.ctypes.data_as(C.c_void_p), None, 0, None, C.byref(total)) == 0
            st = w.query_index_stats()
            assert st["built"] == int(on) and total.value == 8 * (N_BODIES + 1)
            if on:
                assert st["queries_far"] == 16 and st["queries_indexed"] == 0, st  # (both runs of the pass are counted)
            answers.append(w.overlap_sphere(c, 100.0, ALL))
            if on:
                answers.append(w.overlap_sphere(c[:4], 2.0, ALL))
                assert w.query_index_stats()["queries_indexed"] == 4
                w.set_query_index(False)
                assert_same(w.overlap_sphere(c[:4], 2.0, ALL), answers.pop(), "after the overflow")
        finally:
            w.close()
    assert len(answers[0]["kind"]) == 8 * (N_BODIES + 1)
    assert_same(answers[0], answers[1], "overflowing list")


def test_errors_and_the_default(grid):
    w, lib = grid.w, B.lib()
    d = np.zeros(1, W.QUERY_INDEX_DESC_DTYPE)
    good = grid.run("raycast", 5)
    assert w.query_index_stats()["built"] == 0
    for field, value in (("mode", 2), ("cell_edge", -1.0), ("cell_edge", np.nan), ("cell_edge", np.inf), ("reserved", 1)):
        d[:] = 0
        d["mode"] = 1
        d[field] = value
        assert lib.bge_world_set_query_index(w._h, d.ctypes.data_as(C.c_void_p)) == -1, (field, value)
        grid.run("raycast", 5)
        assert w.query_index_stats()["built"] == 0, "a refused desc switched the index on"
    assert lib.bge_world_set_query_index(None, d.ctypes.data_as(C.c_void_p)) == -1
    assert lib.bge_world_query_index_stats(w._h, None) == -1 and lib.bge_world_query_index_stats(None, d.ctypes.data_as(C.c_void_p)) == -1
    w.set_query_index(True, cell_edge=1e-30, min_work=0)  # (below the floor: counts as the floor, every body is wide)
    assert_same(good, grid.run("raycast", 5), "raycast")
    st = w.query_index_stats()
    assert st["built"] == 1 and st["cell_edge"] == np.float32(1e-18) and st["bodies_indexed"] == 0
    assert lib.bge_world_set_query_index(w._h, None) == 0  # NULL: off
    grid.run("raycast", 5)
    assert w.query_index_stats()["built"] == 0
