"""Every branch of the box-box narrowphase on the device (boxbox::box_box in bge_boxbox_device.hpp and the persistent-manifold
cache of bp_collide in bge_contact_device.hpp), through both kernels that call it — k_contact_boxes (a Dynamic box against a Static or
Kinematic one) and k_island_narrow (two Dynamic boxes) — in both orientation schemes.

The pairs and sequences of refmodel/boxbox_cases.py stand isolated in one world a path: a pose pair per axis code and sign, per reference
/ incident face choice, per clip count, cull and tie; a tick sequence per action of the cache (replace, append, sort in, the two removal
rules, the copy down, emptied and refilled, the smaller of two breaking thresholds).  After every tick the world equals the oracle bit
for bit (helpers.compare_obstacle_world / compare_dynamic_world: manifold headers, points, normals, distances, impulses, poses,
velocities).  Device == oracle cannot see an error the two share, so on the first tick the DEVICE's points are also held against the
float64 geometry of refmodel/boxbox64.py.  The class every pair claims is asserted here from the oracle's trace of this very run:
a pair that drifts out of its class fails instead of passing for nothing."""
import numpy as np
import pytest

import banggameengine_amd as B
from helpers import DT, assert_bits_equal, compare_dynamic_world, compare_obstacle_world
from refmodel import boxbox64 as b64
from refmodel import boxbox_cases as bc
from refmodel.tolerances import BOXBOX_REL

pytestmark = pytest.mark.gpu

BASIS = pytest.mark.parametrize("basis", [False, True], ids=["default", "bullet_basis"])
PATH = pytest.mark.parametrize("path", [bc.OBSTACLE, bc.ISLAND])


def _open(case):
    w = B.World()
    w.set_topology(case.wl.parent, None)
    w.upload_trs(case.wl.pos, case.wl.euler, case.wl.scale)
    w.upload_bodies(case.wl.body_type, mass=case.mass, size=case.size)
    w.set_ground_plane(False)
    w.set_static_contacts(case.path == bc.OBSTACLE)
    w.set_dynamic_contacts(case.path == bc.ISLAND)
    return w


def _compare(w, ref, case, tick):
    if case.path == bc.OBSTACLE:
        compare_obstacle_world(w, ref, tick, case.dyn, False)
    else:
        compare_dynamic_world(w, ref, tick, case.dyn, False, False)


def _device_manifolds(w, case):
    """(m, 4, 12) rows and (m,) counts of every pair's manifold on the device, in the case's order."""
    m = len(case.rows)
    rows, cnt = np.zeros((m, 4, 12), np.float32), np.zeros(m, np.int64)
    if case.path == bc.OBSTACLE:
        nb, hdr, pts = w.download_box_contacts()
        a = 2 * np.arange(m)
        assert (nb[a] == 1).all() and (hdr[a, 0, 0] == a + 1).all()
        rows, cnt = pts[a, 0].copy(), hdr[a, 0, 1].astype(np.int64)
    else:
        hdr, pts = w.download_dynamic_pairs()
        assert len(hdr) == m and (hdr[:, 0] == 2 * np.arange(m)).all() and (hdr[:, 1] == 2 * np.arange(m) + 1).all()
        rows, cnt = pts.copy(), hdr[:, 2].astype(np.int64)
    return rows, cnt


@PATH
@BASIS
def test_every_detector_branch(path, basis):
    """One tick of every pose pair.  Bit for bit against the oracle; the classes from the trace with their floors; the device's points
    against the float64 model: code (read off the normal) and normal where the winner's margin exceeds the tolerance, depth, both
    points on their boxes, face points in the reference face, edge points at the closest approach of the edge lines."""
    ps = bc.detector_set()
    flags = B.TICK_ALL | (B.TICK_BULLET_BASIS if basis else 0)
    tags = [set() for _ in range(ps.n)]
    for case in bc.worlds_of(ps, path):
        ref = bc.build_oracle(case, basis)
        with _open(case) as w:
            ref.PhysicsSystemUpdate(DT)
            ref.TransformSystemUpdate()
            w.tick(dt=DT, flags=flags)
            _compare(w, ref, case, 0)
            rows, cnt = _device_manifolds(w, case)
            assert_bits_equal(w.download_world(), ref.bulk_world()[0], "world matrices")
        t = bc.scene_trace(ref, case)
        ref.close()
        assert (t.n_out > 0).all() and (cnt > 0).all()
        boxes = bc.boxes_of(t)
        model = b64.solve(*boxes)
        for k, ts in zip(case.rows, bc.tags_of(t, model, ps.why[case.rows])):
            tags[k] = ts
        answer = bc.answer_of_manifold(rows, cnt, t)
        fails, undecided = b64.check(boxes, answer, BOXBOX_REL, model, refreshed=True)
        assert fails == [], [(int(case.rows[i]), what, x) for i, what, x in fails[:8]]
        assert np.array_equal(answer["code"][~undecided], model["code"][~undecided])
    counts = bc.tag_counts(tags, ps.decided())
    short = {tag: counts.get(tag, (0, 0))[0] for tag, floor in bc.FLOORS.items() if counts.get(tag, (0, 0))[0] < floor}
    assert short == {}, short
    over = {tag: c for tag, c in counts.items() if tag in bc.FLOORS and tag not in bc.EXEMPT_FROM_CAP and c[1] > 0.1 * c[0]}
    assert over == {}, over


@PATH
@BASIS
def test_every_cache_branch(path, basis):
    """The tick sequences: B is moved between ticks (a Kinematic B re-posed; a Dynamic B by a velocity pulse), A may slide or spin.
    After every tick bit for bit against the oracle; the classes from the oracle's trace of this run, each with its floor; the first
    tick's points of the device against the float64 model."""
    sq = bc.sequence_set()
    case = bc.seq_world(sq, path)
    assert case.ticks <= 12
    flags = B.TICK_ALL | (B.TICK_BULLET_BASIS if basis else 0)
    ref = bc.build_oracle(case, basis)
    tags = [set() for _ in range(sq.n)]
    counts = np.zeros((case.ticks, sq.n), np.int64)
    with _open(case) as w:
        for tick in range(case.ticks):
            edits = bc.seq_edits(sq, case, tick, ref)
            bc.apply_edits_to_oracle(ref, edits)
            for ed in edits:
                one = lambda a: np.asarray(a, np.float32).reshape(1, 3)       # noqa: E731
                if ed[0] == "trs":
                    w.upload_trs(pos=one(ed[2]), first=int(ed[1]))
                else:
                    w.set_velocities(one(ed[2]), one(ed[3]), first=int(ed[1]))
            before, before_cnt = bc.manifolds_of(ref, case)
            ref.PhysicsSystemUpdate(DT)
            ref.TransformSystemUpdate()
            w.tick(dt=DT, flags=flags)
            _compare(w, ref, case, tick)
            t = bc.scene_trace(ref, case, strict=False)
            for k, ts in enumerate(bc.cache_tags_of(t, before, before_cnt)):
                tags[k] |= ts
            counts[tick] = bc.manifolds_of(ref, case)[1]
            if tick == 0:
                rows, cnt = _device_manifolds(w, case)
                boxes = bc.boxes_of(t)
                model = b64.solve(*boxes)
                fails, _ = b64.check(boxes, bc.answer_of_manifold(rows, cnt, t), BOXBOX_REL, model, refreshed=True)
                assert fails == [] and (cnt > 0).all(), fails[:8]
        assert_bits_equal(w.download_world(), ref.bulk_world()[0], "world matrices at the end")
    ref.close()
    for k in range(sq.n):
        held = np.flatnonzero(counts[:, k] > 0)
        if len(held) and (counts[held[0]:held[-1] + 1, k] == 0).any():
            tags[k].add("emptied-refilled")
    have = {t: sum(t in ts for ts in tags) for t in bc.CACHE_FLOORS}
    assert {t: c for t, c in have.items() if c < bc.CACHE_FLOORS[t]} == {}, have
