"""The query index (include/bge_world.h "Query index", bge_world_set_query_index ..) without a GPU: the rule restated in numpy
float32 (refmodel/qindex.py) covers every (query, body) pair its restated cull passes, on more than a million seeded pairs per kind;
three wrong models are rejected by the same pairs; every GPU case is in the class it claims on the model alone; the arithmetic the
kernels compile (csrc/bge_qindex_math.hpp) is swept by a stand-alone program under ASan + UBSan; exported symbols, the C99 view of
the two structs, the adapter's members."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

from banggameengine_amd import world as W

from abi import assert_exported, build_and_run_c99, compile_reference_shapes
from refmodel import qindex as Q
from refmodel.qindex_cases import (BATCH_SIZES, ENTRIES, GRID_SEED, KIND_OF, MAGNITUDES, N_BODIES, N_QUERIES, SWEEP, as_records, check_claims,
                                   coincident_and_colliding, grid_queries, grid_scene, nan_queries, pairs, predicted, touching_pairs)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "banggameengine_amd", "csrc")
PAIR_SEED = 20261020
_cache = {}


def pairs_of(kind):
    """The pairs of a kind and which of them the restated cull passes: made once, never changed"""
    if kind not in _cache:
        q, c, rad, h = pairs(kind, PAIR_SEED)
        passes, _ = Q.covered(kind, q, c, rad, h)
        _cache[kind] = (q, c, rad, h, passes)
    return _cache[kind]


# ------------------------------------------------------------------------------------------------ (a) coverage


@pytest.mark.parametrize("kind", Q.KINDS)
def test_every_pair_the_cull_passes_is_covered(kind):
    q, c, rad, h, passes = pairs_of(kind)
    _, cov = Q.covered(kind, q, c, rad, h, passes=passes)
    lo, hi, g = Q.extent(kind, q)
    far = Q.query_range(lo, hi, g, h)[2]
    wide = Q.is_wide(Q.body_rb(rad, c), h)
    through_cells = passes & ~far & ~wide
    print(f"{kind}: {len(c)} pairs, {int(passes.sum())} pass the cull: {int(through_cells.sum())} through a cell, {int((passes & wide).sum())} wide, "
          f"{int((passes & far & ~wide).sum())} far; uncovered {int((passes & ~cov).sum())}")
    assert len(c) >= 1_000_000 and passes.sum() > 400_000 and through_cells.sum() > 100_000
    assert not (passes & ~cov).any()
    mag = np.abs(c).max(axis=1)
    for m in MAGNITUDES:  # every magnitude has pairs that pass, and but for 3e9 (always wide at these edges) pairs through a cell
        at = (mag > 0.1 * m) & (mag <= 1.01 * m)
        assert (passes & at).sum() > 1000, m
        assert m > 1e6 or (through_cells & at).sum() > 100, m


def test_touching_pairs_lie_at_the_edge_of_the_cull():
    """The touching pairs are what they say: about half pass the cull, and moving the query one float flips many of them."""
    for kind in Q.KINDS:
        q, c, rad, _ = touching_pairs(kind, np.random.default_rng(1), 20000)
        p = Q.cull(kind, q, c, Q.body_rb(rad, c))
        assert 0.25 < p.mean() < 0.85, (kind, p.mean())


# ------------------------------------------------------------------------------------------------ (c) wrong models


@pytest.mark.parametrize("kind", Q.KINDS)
@pytest.mark.parametrize("wrong", (Q.Model(margin=False), Q.Model(floor_cell=False), Q.Model(position_term=False)),
                         ids=("reach without margin", "cell by truncation", "rb without the position term"))
def test_wrong_models_are_rejected(kind, wrong):
    q, c, rad, h, passes = pairs_of(kind)
    _, cov = Q.covered(kind, q, c, rad, h, model=wrong, passes=passes)
    missed = int((passes & ~cov).sum())
    print(f"{kind}, {wrong}: {missed} pairs the cull passes are not visited")
    assert missed > 0


# ------------------------------------------------------------------------------------------------ (b) the GPU cases, on the model


class GridModel:
    def __init__(self):
        rng = np.random.default_rng(GRID_SEED)
        self.sc = grid_scene(rng)
        self.member = np.arange(len(self.sc["pos"])) < N_BODIES
        self.queries = grid_queries(rng, self.sc["pos"])


@pytest.fixture(scope="module")
def grid():
    return GridModel()


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("case", SWEEP, ids=[c[0] for c in SWEEP])
def test_sweep_cases_are_in_their_classes(grid, case, entry):
    name, cell_edge, max_cells, wide_claim, far_claim = case
    args = grid.queries[entry]
    got = predicted(entry, args, grid.sc["pos"], grid.sc["shape"], grid.sc["size"], grid.member, cell_edge, max_cells)
    assert got["bodies_indexed"] + got["bodies_wide"] == N_BODIES and got["queries_indexed"] + got["queries_far"] == N_QUERIES
    check_claims(name, entry, wide_claim, far_claim, N_BODIES, N_QUERIES, nan_queries(entry, args), got)


@pytest.mark.parametrize("entry", ENTRIES)
def test_batches_claim_the_indexed_route(grid, entry):
    """The batch-size tests run at edge 4, max_cells 512: no body is wide there, and in every batch size some query walks cells."""
    for n in BATCH_SIZES:
        args = tuple(a[:n] for a in grid.queries[entry])
        got = predicted(entry, args, grid.sc["pos"], grid.sc["shape"], grid.sc["size"], grid.member, 4.0, 512)
        assert got["bodies_wide"] == 0 and got["queries_indexed"] > 0, (n, got)
        if KIND_OF[entry] in ("overlap", "penetration"):
            assert got["queries_far"] == nan_queries(entry, args), (n, got)


def test_the_bucket_case_collides_on_the_model():
    pos, off = coincident_and_colliding(1024, 2.0)
    cells = Q.cell(pos, 2.0)
    b = Q.bucket(cells[:, 0], cells[:, 1], cells[:, 2], 1024)
    assert Q.table_size(len(pos)) == 1024 and len(np.unique(b[:257])) == 1 and b[0] == b[-1] and np.abs(off).max() <= 8
    assert np.array_equal(cells[257] - cells[0], [1024, 0, 0])
    assert not np.array_equal(Q.key(*cells[0]), Q.key(*cells[-1])), "the colliding cells share their key bits too"
    assert Q.key(*cells[0]) == Q.key(*cells[257]), "cells 1024 apart share their key bits: that is what max 1024 cells per axis is for"
    assert not Q.is_wide(Q.body_rb(Q.body_rad(False, np.full((1, 3), 0.3, np.float32)), pos), 2.0).any()


def test_the_classes_of_the_rule():
    f = np.float32
    assert Q.is_member([1, 0, 2, 3, 1, 1], [0, 0, 1, 0, 0, 0], [1, 1, 1, 1, 0, 1], [1, 1, 1, 1, 1, 0]).tolist() == [True, False, False, True, False, False]
    rb = Q.body_rb(f([0.5, 0.5, 0.5, 0.5]), f([[0, 0, 0], [1e5, 0, 0], [1e30, 0, 0], [np.nan, 0, 0]]))
    assert Q.is_wide(rb, 2.0).tolist() == [False, True, True, True]
    ground = Q.body_rb(Q.body_rad(False, f([[50.0, 1.0, 50.0]])), f([[0, -1, 0]]))
    assert Q.is_wide(ground, 2.0).all()  # (demo.json's 50 x 1 x 50 Ground)
    q = dict(origin=f([[0, 1, 0], [0, 1, 0], [0, 1, 0], [np.nan, 0, 0], [3e38, 0, 0]]), direction=f([[1, 0, 0], [1, 1, 1], [1, 0, 0], [1, 0, 0], [1, 0, 0]]),
             max_distance=f([3.0, 60.0, 3000.0, 1.0, 3e38]), radius=f([0, 0, 0, 0, 0]))
    assert Q.classify("ray", q, 2.0).tolist() == [False, True, True, True, True]  # short; long diagonal; > 1024 cells on x; NaN; overflow
    assert Q.edge(0) == 4.0 and Q.edge(1e-30) == f(1e-18) and Q.edge(np.inf) == Q.FLT_MAX


# ------------------------------------------------------------------------------------------------ the kernels' own arithmetic


def test_qindex_cover_program(tmp_path):
    exe = str(tmp_path / "qindex_cover")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "cpp", "qindex_cover.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "qindex_cover ok" in r.stdout


def test_the_model_has_the_headers_constants():
    text = open(os.path.join(CSRC, "bge_qindex_math.hpp")).read()
    for line in ("kCellMax = 1048576.0f", "kEdgeMin = 1e-18f", "kEdgeDefault = 4.0f", f"kMaxCellsDefault = {Q.MAX_CELLS_DEFAULT}u", f"kAxisCells = {Q.AXIS_CELLS}",
                 "kMargin = 1.0625f", "kReachMax = 1e18f"):
        assert line in text, line
    assert (Q.CELL_MAX, Q.EDGE_MIN, Q.EDGE_DEFAULT, Q.MARGIN, Q.REACH_MAX) == (2.0 ** 20, np.float32(1e-18), 4.0, 1.0625, np.float32(1e18))


# ------------------------------------------------------------------------------------------------ (d) the surface


def test_symbols_are_exported():
    assert_exported(["bge_world_set_query_index", "bge_world_query_index_stats"])


def test_the_records_are_the_bindings():
    assert W.QUERY_INDEX_DESC_DTYPE.itemsize == 24 and W.QUERY_INDEX_STATS_DTYPE.itemsize == 64
    assert [W.QUERY_INDEX_DESC_DTYPE.fields[k][1] for k in ("mode", "cell_edge", "max_cells", "reserved", "min_work")] == [0, 4, 8, 12, 16]
    assert [W.QUERY_INDEX_STATS_DTYPE.fields[k][1] for k in ("built", "table_size", "bodies_indexed", "bodies_wide", "queries_indexed", "queries_far",
                                                            "cell_edge", "reserved", "builds", "reserved2")] == [0, 4, 8, 16, 24, 32, 40, 44, 48, 56]
    header = open(os.path.join(ROOT, "include", "bge_world.h")).read()
    assert f"#define BGE_QUERY_INDEX_MIN_WORK_DEFAULT ((uint64_t)1 << {W.QUERY_INDEX_MIN_WORK_DEFAULT.bit_length() - 1})" in header


def test_c99_view_of_the_structs(tmp_path):
    build_and_run_c99(tmp_path, "abi_check_query_index.c", "query index abi ok")


def test_adapter_query_index_members_on_reference_shapes(tmp_path):
    compile_reference_shapes(tmp_path, "query_index_reference_shapes.cpp")
