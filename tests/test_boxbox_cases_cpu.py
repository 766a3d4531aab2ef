"""The box-box narrowphase's cases hold their classes, on the oracle alone (refmodel/boxbox_cases.py).

test_gpu_boxbox_paths.py compares the device with the oracle on these pairs and sequences; that comparison proves something only where
a pair really takes the branch it is there for.  Here: every floor is met, read off the oracle's TRACE of the scenes the device will run
(both paths, both schemes); the oracle's own answers pass the float64 checker of refmodel/boxbox64.py inside the cap of undecided pairs;
the checker rejects five wrong answers; the measured deviation is the one tolerances.py states; the constants the cases rest on are
the sources'; the trace changes no result."""
import ast
import os
import re

import numpy as np
import pytest

from helpers import DT, assert_bits_equal, build_island_oracle, build_obstacle_oracle
from refmodel import boxbox64 as b64
from refmodel import boxbox_cases as bc
from refmodel import island_cases as ic
from refmodel import obstacle_cases as oc
from refmodel.tolerances import BOXBOX_MEASURED, BOXBOX_REL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "banggameengine_amd", "csrc")
MODES = pytest.mark.parametrize("path,basis", bc.MODES, ids=[f"{p}-{'bullet_basis' if b else 'default'}" for p, b in bc.MODES])


def _src(*parts):
    return open(os.path.join(*parts)).read()


def _first_tick(ps, path, basis):
    """The scenes of a PairSet stepped once on the oracle: the trace, one row a pair, in the set's order.  On the way, the manifolds the
    tick leaves (what the device's download is compared with, bit for bit) pass the float64 checker as the GPU test applies it."""
    ints, floats = np.zeros((ps.n, 40), np.int32), np.zeros((ps.n, 50), np.float32)
    for case in bc.worlds_of(ps, path):
        ref = bc.build_oracle(case, basis)
        ref.PhysicsSystemUpdate(DT)
        t = bc.scene_trace(ref, case)
        rows, cnt = bc.manifolds_of(ref, case)
        fails, undecided = b64.check(bc.boxes_of(t), bc.answer_of_manifold(rows, cnt, t), BOXBOX_REL, refreshed=True)
        assert fails == [] and (cnt > 0).all(), fails[:8]
        ints[case.rows], floats[case.rows] = t._ints, t._floats
        ref.close()
    return bc.po.BoxTraces(np.zeros((ps.n, 2), np.uint32), ints, floats)


def test_the_constants_are_the_sources():
    det, con, orc = _src(CSRC, "bge_boxbox_device.hpp"), _src(CSRC, "bge_contact_device.hpp"), _src(ROOT, "oracle", "boxbox_ref.h")
    for text in (det, orc):
        assert float(re.search(r"fudge_factor = ([0-9.e+-]+)f;", text).group(1)) == bc.FUDGE_FACTOR == b64.FUDGE_FACTOR
        assert float(re.search(r"fudge2 = ([0-9.e+-]+)f;", text).group(1)) == bc.FUDGE2 == b64.FUDGE2
        assert float(re.search(r"if \(d <= ([0-9.e+-]+)f\)", text).group(1)) == bc.PARALLEL_D == b64.PARALLEL_D
        assert int(re.search(r"int maxc = (\d+);", text).group(1)) == bc.MAXC
        assert text.count(f"if (nr & {bc.CLIP_EXIT})") == 2                                # the 8-point exit, after a kept point and after a crossing
    assert "if (s2 * fudge_factor > s)" in det and "if (s2 * fudge_factor > s)" in orc
    assert "return disc * bt::kContactBreakingThreshold;" in _src(ROOT, "oracle", "contact_ref.h")
    assert re.search(r"kContactBreakingThreshold = ([0-9.]+)f", _src(ROOT, "oracle", "bullet_math.h")).group(1) == str(bc.BREAKING_PER_RADIUS)
    # both kernels take the smaller of the two bodies' thresholds
    assert "fminf(breaking, o.breaking)" in con and "fminf(ct_breaking_threshold(shape_a), ct_breaking_threshold(shape_b))" in _src(CSRC, "bge_island.hip")
    assert np.float32(b64.EPSILON) == np.finfo(np.float32).eps


def test_the_unreachable_list_against_the_source():
    """Five branches are left out, each with its argument; the three that are a statement of their own stand once in the oracle's
    restatement and once in the device's code — nothing else of the two files is without a class."""
    assert len(bc.UNREACHABLE) == 5 and all(len(arg) > 80 for _, arg, _ in bc.UNREACHABLE)
    orc = _src(ROOT, "oracle", "boxbox_ref.h")
    stated = [s for _, _, s in bc.UNREACHABLE if s is not None]
    assert len(stated) == 3 and all(orc.count(s) == 1 for s in stated)
    det, con = _src(CSRC, "bge_boxbox_device.hpp"), _src(CSRC, "bge_contact_device.hpp")
    bp = con[con.index("__device__ int bp_collide("):con.index("// btPlaneSpace1, first tangent")]
    assert det.count("a = 1.0e18f;") == 1 and bp.count("if (depth > breaking) continue;") == 1 and bp.count("if (insert < 0) insert = 0;") == 1
    assert bc.FACE_EXCLUDED == [] and len(bc.FACE_TAGS) == 36


def test_the_float64_model_is_numpy_alone():
    tree = ast.parse(_src(ROOT, "tests", "refmodel", "boxbox64.py"))
    names = {a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names} | {n.module for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)}
    assert names == {"numpy", "__future__"}


def test_what_the_set_is_made_of():
    ps = bc.detector_set()
    assert 300 <= ps.n <= 2 * bc.PAIRS_PER_WORLD
    for k in range(0, ps.n, 2):                                                # every pair is followed by its swap
        assert ps.why[k + 1] == ps.why[k] + ":swapped"
        assert_bits_equal(ps.half_a[k], ps.half_b[k + 1], "swap: sizes")
        assert_bits_equal(ps.euler_a[k], ps.euler_b[k + 1], "swap: orientation")
    kinds = {k: int((ps.kind == k).sum()) for k in ("small", "big", "far1e3", "far1e4", "normal")}
    assert min(kinds.values()) >= 16, kinds
    assert ps.half_a[ps.kind == "small"].max() < 0.06 and ps.half_a[ps.kind == "big"].max() > 30.0
    far = np.abs(ps.pos_b[np.isin(ps.kind, ("far1e3", "far1e4"))]).max(1)
    assert far.min() >= 1e3 and far.max() <= 1.1e4
    assert (np.ptp(ps.half_a, axis=1) > 0.05 * ps.half_a.max(1)).sum() > ps.n // 3              # non-cubic boxes
    # isolated: the world boxes of different pairs, grown by 0.1 (five times the margin Bullet feeds its broadphase with), never overlap
    t = ps.trace
    ext = [np.abs(R.astype(np.float64)) @ h.astype(np.float64)[:, :, None] for R, h in ((t.R1, t.half1), (t.R2, t.half2))]
    lo = np.minimum(t.p1 - ext[0][:, :, 0], t.p2 - ext[1][:, :, 0]) - 0.1
    hi = np.maximum(t.p1 + ext[0][:, :, 0], t.p2 + ext[1][:, :, 0]) + 0.1
    apart = ((lo[:, None] > hi[None]) | (hi[:, None] < lo[None])).any(2) | np.eye(ps.n, dtype=bool)
    assert apart.all()
    c = ps.pos_b.astype(np.float64)
    dist = np.linalg.norm(c[:, None] - c[None], axis=2) + np.where(np.eye(ps.n, dtype=bool), np.inf, 0.0)
    assert dist.min() >= bc.PAIR_SPACING - 1e-3 and dist[ps.kind == "big"][:, ps.kind == "big"].min() >= bc.BIG_SPACING - 1e-3


@MODES
def test_every_detector_floor_is_met_in_the_scenes(path, basis):
    """One tick of the scenes the device will run: the trace of every pair equals the detector's on the same poses (so classes, model and
    checker of the set speak of what the scene does), every class has its floor, and at most a tenth of a class is undecided."""
    ps = bc.detector_set()
    t = _first_tick(ps, path, basis)
    assert np.array_equal(t._ints[:, :14], ps.trace._ints[:, :14]) and np.array_equal(t._ints[:, 15:27], ps.trace._ints[:, 15:27])
    assert_bits_equal(t._floats, ps.trace._floats, "the scene's detector inputs and answers")
    assert (t.ran == 1).all() and (t.n_before == 0).all() and (t.n_out > 0).all()
    tags = bc.tags_of(t, b64.solve(*bc.boxes_of(t)), ps.why)
    counts = bc.tag_counts(tags, ps.decided())
    short = {tag: counts.get(tag, (0, 0))[0] for tag, floor in bc.FLOORS.items() if counts.get(tag, (0, 0))[0] < floor}
    assert short == {}, short
    over = {tag: c for tag, c in counts.items() if tag in bc.FLOORS and tag not in bc.EXEMPT_FROM_CAP and c[1] > 0.1 * c[0]}
    assert over == {}, over
    # what the argument of UNREACHABLE says never happens does not happen here either
    face = t.code <= 6
    assert not np.isin(t.n_clip[face], (1, 2)).any() and (t.culled < 2).all() and (t.action != bc.po.ACT_SKIPPED).all()
    assert max(bin(int(m)).count("1") for m in t.skip_mask) == 3


def test_the_oracle_passes_the_float64_checker_and_the_tolerance_is_the_measured_one():
    ps, sq = bc.detector_set(), bc.sequence_set()
    worst = {}
    for s in (ps, sq):
        fails, undecided = b64.check(s.boxes, bc.answer_of(s.trace), BOXBOX_REL, s.model)
        assert fails == [], fails[:8]
        dev = b64.deviations(s.boxes, bc.answer_of(s.trace), s.model)
        for k in b64.FIGURES:
            held = ~np.isnan(dev[k]) & (~undecided if k in ("normal", "edge") else True)
            worst[k] = max(worst.get(k, 0.0), float(dev[k][held].max()))
        assert not (~undecided & ~dev["code_ok"]).any()
    print("largest deviation of the oracle from the float64 model, relative:", {k: f"{v:.2e}" for k, v in worst.items()})
    assert 0.5 * BOXBOX_MEASURED <= max(worst.values()) <= BOXBOX_MEASURED and BOXBOX_REL == 4 * BOXBOX_MEASURED
    assert int((~ps.decided()).sum()) <= ps.n // 20


def _wrong(ps, rows, **change):
    a = {k: np.array(v[rows]) for k, v in bc.answer_of(ps.trace).items()}
    a.update(change)
    boxes = tuple(b[rows] for b in ps.boxes)
    model = {k: (v[rows] if isinstance(v, np.ndarray) else v) for k, v in ps.model.items()}
    fails, undecided = b64.check(boxes, a, BOXBOX_REL, model)
    assert not undecided.any()
    return {i for i, _, _ in fails}, {what for _, what, _ in fails}


def test_the_checker_rejects_five_wrong_answers():
    ps = bc.detector_set()
    ok = ps.decided(4 * BOXBOX_REL) & (ps.kind == "normal") & np.array([not (t & bc.EXEMPT_FROM_CAP) for t in ps.tags])
    rows = np.flatnonzero(ok)
    every = set(range(len(rows)))
    t, m = ps.trace, ps.model
    nb, pt, dep = t.normal_on_b[rows].astype(np.float64), t.point[rows].astype(np.float64), t.depth[rows].astype(np.float64)
    live = (np.arange(4)[None, :] < t.n_out[rows][:, None])
    assert len(rows) > 150 and _wrong(ps, rows)[0] == set()
    # a flipped normal
    bad, what = _wrong(ps, rows, normal_on_b=-nb)
    assert bad == every and "normal" in what
    # the runner-up axis: its code, its normal, its depth
    ru = m["runner"][rows] - 1
    k = np.arange(len(rows))
    bad, what = _wrong(ps, rows, code=ru + 1, normal_on_b=-m["axis"][rows][k, ru], depth=np.where(live, m["v"][rows][k, ru][:, None], 0.0))
    twins = m["twin"][rows][k, ru]                                             # (boxes laid flat: the facing face of the other box is the same answer)
    assert bad == set(np.flatnonzero(~twins).tolist()) and "code" in what and twins.sum() < len(rows) // 4
    # the points reported on A instead of on B
    bad, what = _wrong(ps, rows, point=pt + nb[:, None, :] * dep[:, :, None])
    assert bad == every and "on_a" in what
    # a depth without the margin: the boxes' implicit dimensions, 0.04 less on either side
    bad, what = _wrong(ps, rows, depth=np.where(live, dep + 0.08, 0.0))
    assert bad == every and "depth" in what
    # an edge answer with alpha = beta = 0: the end of the edge instead of the closest point
    edge = np.flatnonzero(ok & (t.code > 6) & (m["d"] > 0.05) & (np.abs(m["pb"] - m["edge_ends"][:, 0]).max(1) > 0.02) & (np.abs(m["pb"] - m["edge_ends"][:, 1]).max(1) > 0.02))
    assert len(edge) > 40
    pt2 = ps.trace.point[edge].astype(np.float64)
    pt2[:, 0] = m["edge_ends"][edge, 0]
    bad, what = _wrong(ps, edge, point=pt2)
    assert bad == set(range(len(edge))) and "edge" in what


@MODES
def test_every_cache_floor_is_met_in_the_sequences(path, basis):
    sq = bc.sequence_set()
    assert 10 <= sq.n <= 60
    tags, counts, never = bc.run_sequences(sq, path, basis)
    have = {t: sum(t in ts for ts in tags) for t in bc.CACHE_FLOORS}
    assert {t: c for t, c in have.items() if c < bc.CACHE_FLOORS[t]} == {}, have
    assert never == dict(skipped=0, insert_below_zero=0, area_guard=0)
    assert (counts[0] > 0).all()                                               # every sequence starts in contact
    sizes = np.linalg.norm(sq.half_a, axis=1) / np.linalg.norm(sq.half_b, axis=1)
    assert ((sizes > 1.2) | (sizes < 1 / 1.2)).sum() >= 4                      # boxes of different sizes: the smaller threshold is the pair's


def _states(ref, case, trace):
    ref.SetBoxTrace(trace)
    out = []
    for tick in range(case.ticks):
        if hasattr(case, "edits_at"):
            oc.apply_to_oracle(case, tick, ref)
        ref.PhysicsSystemUpdate(DT)
        ref.TransformSystemUpdate()
        rb = ref.bulk_bodies()
        hdr, pts = ref.DynamicPairs()
        boxes = [ref.BoxContacts(e + 1) for e in range(case.n)]
        out.append((rb["origin"].copy(), rb["quat"].copy(), rb["linvel"].copy(), rb["angvel"].copy(), hdr.copy(), pts.copy(), boxes))
        if trace:
            assert len(ref.BoxTrace()) + len(ref.PairTrace()) >= sum(len(b) for b in boxes) + len(hdr)
    ref.close()
    return out


@pytest.mark.parametrize("name", ["twenty-rows", "five-under-a-plank", "on-a-slab", "boundaries"])
def test_the_trace_changes_no_result(name):
    """Existing scenes with the sink set and unset: poses, velocities, every manifold and every impulse, bit for bit, tick by tick."""
    make = {"twenty-rows": (oc.twenty_rows, build_obstacle_oracle), "five-under-a-plank": (oc.five_under_a_plank, build_obstacle_oracle),
            "on-a-slab": (ic.on_a_slab, build_island_oracle), "boundaries": (ic.boundaries, build_island_oracle)}[name]
    runs = []
    for trace in (False, True):
        case = make[0]()
        case.ticks = min(case.ticks, 40)
        runs.append(_states(make[1](case), case, trace))
    for tick, (a, b) in enumerate(zip(*runs)):
        for x, y, what in zip(a[:6], b[:6], ("origin", "quaternion", "linear velocity", "angular velocity", "pair header", "pair points")):
            assert x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32)), f"tick {tick}: {what}"
        for ma, mb in zip(a[6], b[6]):
            assert [o for o, _ in ma] == [o for o, _ in mb]
            for (_, ra), (_, rb_) in zip(ma, mb):
                assert ra.shape == rb_.shape and np.array_equal(ra.view(np.uint32), rb_.view(np.uint32)), f"tick {tick}: obstacle manifold"
