"""Sphere penetration and recovery on the device (include/bge_world.h "Sphere penetration and recovery",
bge_world_sphere_penetration*, bge_world_sphere_recover*).

Three references, each for what it can say:
  - the device's own overlap_sphere, exactly: a sphere is penetrated iff its overlap list is not empty, the winner is in that
    list, and outside a shape the signed distance is the overlap's distance bit for bit, so depth == float32(radius - distance);
  - signed_ref of refmodel/recover.py, the header's rule in float64 fed the device's binary32 poses, within the tolerances of
    test_gpu_sphere_queries.py: depth and point as the overlap's distance there, P_REL x (1 + |centre|_inf); the
    normal N_ABS + N_SCALE x (|centre|_1 + radius) / d, where d is the shape's smallest half extent or radius and, where the
    normal is a difference of points divided by its length (outside a box, anywhere about a capsule), the smaller of that and the
    length.  A sphere is set aside where classify() finds the reference's own answer ambiguous (a condition on the reference,
    never on the device's answer); at most half of the penetrating spheres may be, and test_sphere_recover_cpu.py shows the seed
    stays inside that;
  - recover_ref, the Recover rule in numpy float32 scalars, with World.sphere_penetration on the same world as its penetration
    function: the device runs the same queries and the same binary32 arithmetic between them, so the 64-byte results must be
    equal byte for byte."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import banggameengine_amd as B
from banggameengine_amd import world as W

from refmodel.rays import ALL, NO_ENTITY, RAY_BODY, RAY_GROUND, RAY_MISS, RAY_TRIGGER
from refmodel.recover import record_valid, recover_ref
from refmodel.sphere_cases import scene_world64
from refmodel.move_cases import BATCHES, SCENE_N, SCENE_SEED, ghost_positions
from refmodel.recover_cases import HAND_RECOVERS, SPHERE_SEED, check_hand_recover, check_invalid, hand_record, invalid_records, sphere_batch
from refmodel.device import FLAGS, Scene, check_penetration_against_overlap, check_penetrations, penetration, recover

pytestmark = pytest.mark.gpu


class Shared:
    """The scene of the comparison, ticked once, the spheres, and the answers for the largest batch: made once, never changed."""

    def __init__(self):
        self.sc = Scene(SCENE_N, np.random.default_rng(SCENE_SEED), n_triggers=12)
        self.sc.tick(1)
        self.w = self.sc.w
        # the spheres are those of the CPU file, to the bit: drawn around the poses the entities were uploaded with
        w64, pos = scene_world64(SCENE_N, np.random.default_rng(SCENE_SEED))
        self.recs = sphere_batch(np.random.default_rng(SPHERE_SEED), max(BATCHES), pos, ghost_positions(w64))
        self.valid = np.array([record_valid(m) for m in self.recs])
        self.pen = penetration(self.w, self.recs)
        self.want = recover_ref(lambda s: penetration(self.w, s), self.recs)
        self.got = recover(self.w, self.recs)


@pytest.fixture(scope="module")
def shared():
    s = Shared()
    yield s
    s.sc.close()


def test_penetration_equals_the_devices_own_overlap_exactly(shared):
    check_penetration_against_overlap(shared.w, shared.recs, shared.pen, (200, 50))


def test_penetration_against_the_float64_reference(shared):
    check_penetrations(shared.sc.objects(), shared.recs, shared.valid, shared.pen)


@pytest.mark.parametrize("n", BATCHES)
def test_recover_equals_the_stepped_composition_byte_for_byte(shared, n):
    recs = shared.recs[:n]
    got = shared.got if n == len(shared.recs) else recover(shared.w, recs)
    want = shared.want[:n]  # (a sphere's answer does not depend on its batch: recover_ref asks one query per sphere and round)
    bad = [i for i in range(n) if got[i].tobytes() != want[i].tobytes()]
    assert not bad, f"{len(bad)} of {n} differ, first {bad[0]}: {got[bad[0]]} vs {want[bad[0]]}"
    if n == len(shared.recs):
        ok = (got["flags"] & W.RECOVER_INVALID) == 0
        assert (~ok).sum() == len(range(36, n, 37))
        cov = dict(clear=int((ok & (got["flags"] == 0)).sum()), one=int((got["n_pushes"] == 1).sum()), more=int((got["n_pushes"] >= 2).sum()),
                   stuck=int(((got["flags"] & W.RECOVER_STUCK) != 0).sum()))
        print("recoveries:", cov)
        assert cov["clear"] >= 20 and cov["one"] >= 20 and cov["more"] >= 20 and cov["stuck"] >= 1, cov
        assert all((got["hit_kind"] == k).any() for k in (RAY_BODY, RAY_TRIGGER, RAY_GROUND))
        assert ((got["flags"] & W.RECOVER_MOVED) != 0).tolist() == (got["n_pushes"] > 0).tolist() and got["n_pushes"].max() == W.RECOVER_ROUNDS


def test_invalid_records_on_the_device(shared):
    recs = invalid_records()
    check_invalid(recs, recover(shared.w, recs))
    # and as spheres of the penetration query (where a skin plays no part): the overlap's no-hit inputs
    pen = penetration(shared.w, recs)
    bad = ~np.array([np.isfinite(m["position"]).all() and np.isfinite(m["radius"]) and m["radius"] >= 0 and m["layer_mask"] != 0 for m in recs])
    assert bad.sum() == 6 and not pen["kind"][bad].any() and (pen["entity"][bad] == NO_ENTITY).all() and not pen["depth"][bad].any()


def hand_world(bodies, plane):
    n = max(len(bodies), 1)
    w = B.World(device=0)
    w.set_topology(np.full(n, W.NO_PARENT, np.uint32))
    w.upload_trs(np.float32([b[2] for b in bodies] or [[0, 0, 0]]), np.float32([b[3] for b in bodies] or [[0, 0, 0]]), np.ones((n, 3)))
    ghosts = [i for i, b in enumerate(bodies) if b[5]]
    types = np.full(n, W.BODY_STATIC if bodies else W.BODY_NONE, np.uint8)
    types[ghosts] = W.BODY_NONE
    shapes = np.uint8([b[0] for b in bodies] or [0])
    sizes = np.float32([b[1] for b in bodies] or [[0.5, 0.5, 0.5]])
    groups = np.uint32([b[4] for b in bodies] or [1])
    w.upload_bodies(types, None, shapes, sizes, groups, np.full(n, ALL, np.uint32))
    if ghosts:
        g = np.uint32(ghosts)
        w.upload_triggers(g, shapes[g], sizes[g], groups[g], np.full(len(g), ALL, np.uint32), np.zeros(len(g), np.uint8), np.ones(len(g), np.uint8))
    w.set_ground_plane(plane)
    w.tick(flags=FLAGS)
    return w


@pytest.mark.parametrize("case", HAND_RECOVERS, ids=[c[0] for c in HAND_RECOVERS])
def test_hand_worked_recoveries_on_the_device(case):
    name, _, bodies, plane, _, want = case
    w = hand_world(bodies, plane)
    try:
        recs = hand_record(case)
        got = recover(w, recs)
        check_hand_recover(name, got[0], want)
        assert got[0].tobytes() == recover_ref(lambda s: penetration(w, s), recs)[0].tobytes()
    finally:
        w.close()


def test_recovered_spheres_overlap_nothing_and_clear_ones_stay(shared):
    recs, got = shared.recs, shared.got
    free = np.nonzero(shared.valid & ((got["flags"] & W.RECOVER_STUCK) == 0))[0]
    ov = shared.w.overlap_sphere(got["position"][free], recs["radius"][free], recs["layer_mask"][free])
    inside = np.nonzero(np.diff(ov["offsets"].astype(np.int64)) != 0)[0]
    print(f"{len(free)} valid spheres end without STUCK, {((got['flags'][free] & W.RECOVER_MOVED) != 0).sum()} of them pushed; {len(inside)} still overlap")
    assert len(free) >= 300 and len(inside) == 0, (free[inside], ov["distance"])
    # and the STUCK ones do, by what the result says
    stuck = np.nonzero((got["flags"] & W.RECOVER_STUCK) != 0)[0]
    again = penetration(shared.w, W.make_spheres(got["position"][stuck], recs["radius"][stuck], recs["layer_mask"][stuck]))
    assert (again["kind"] != RAY_MISS).all() and again["depth"].tobytes() == got["remaining_depth"][stuck].tobytes()
    still = got["flags"] == 0
    assert still.sum() >= 20 and got["position"][still].tobytes() == recs["position"][still].tobytes() and not got["pushed"][still].any()
    assert not got["n_pushes"][still].any() and (got["hit_entity"][still] == NO_ENTITY).all()


def test_a_move_after_recovery_hits_what_it_walked_through_before():
    """The reason for the feature, on a crate and on the plane.  A sphere of radius 0.3 whose centre is 0.1 from the crate's face
    x = 0.5, asked to move 2 towards the crate: the cast does not see the crate it starts in, so the move goes through it; from
    the recovered position (0.5 + 0.3 + skin) the same move stops at the crate.  And a sphere 0.2 above the plane, asked down."""
    w = hand_world([(False, (0.5, 0.5, 0.5), (0, 0.5, 0), (0, 0, 0), 1, False)], True)
    try:
        start = np.float32([[0.6, 0.5, 0], [5, 0.2, 0]])
        ask = np.float32([[-2, 0, 0], [0, -1, 0]])
        rec = w.sphere_recover(start, 0.3, 0.01, ALL)
        assert (rec["flags"] == W.RECOVER_MOVED).all() and rec["hit_kind"].tolist() == [RAY_BODY, RAY_GROUND] and rec["hit_entity"][0] == 0
        assert np.allclose(rec["position"], [[0.81, 0.5, 0], [5, 0.31, 0]], atol=1e-5)
        through = w.sphere_move(start, ask, 0.3, 0.01, 0.0, 0.7, ALL)
        assert through["n_hits"].tolist() == [0, 0] and np.allclose(through["position"], start + ask, atol=1e-6)
        stopped = w.sphere_move(rec["position"], ask, 0.3, 0.01, 0.0, 0.7, ALL)
        assert (stopped["n_hits"] >= 1).all() and stopped["hit_kind"].tolist() == [RAY_BODY, RAY_GROUND] and stopped["hit_entity"][0] == 0
        assert stopped["position"][0][0] > 0.8 and stopped["position"][1][1] > 0.3
    finally:
        w.close()


def test_determinism_and_the_device_entry_points(shared):
    import torch
    w, recs, n = shared.w, shared.recs, len(shared.recs)
    assert recover(w, recs).tobytes() == shared.got.tobytes() and penetration(w, recs).tobytes() == shared.pen.tobytes()
    lib = B.lib()
    # recover: records and results at 4-byte-aligned offsets that are no multiple of 8
    mo = torch.zeros(n * 28 + 4, dtype=torch.uint8, device="cuda:0")
    ro = torch.zeros(n * 64 + 12, dtype=torch.uint8, device="cuda:0")
    mo[4:].copy_(torch.from_numpy(recs.view(np.uint8).copy()).to("cuda:0"))
    assert mo[4:].data_ptr() % 8 == 4 and ro[12:].data_ptr() % 8 == 4
    torch.cuda.synchronize()
    w.sphere_recover_device(mo[4:], ro[12:])
    w.sync()
    assert ro[12:].cpu().numpy().tobytes() == shared.got.tobytes() and not ro[:12].cpu().numpy().any()
    assert lib.bge_world_sphere_recover_device(w._h, 4, C.c_void_p(mo.data_ptr() + 2), C.c_void_p(ro.data_ptr())) == -1
    assert lib.bge_world_sphere_recover_device(w._h, 4, C.c_void_p(mo.data_ptr()), C.c_void_p(ro.data_ptr() + 1)) == -1
    assert lib.bge_world_sphere_recover_device(w._h, 4, None, C.c_void_p(ro.data_ptr())) == -1
    assert lib.bge_world_sphere_recover_device(w._h, 0, None, None) == 0 and lib.bge_world_sphere_recover(w._h, 0, None, None) == 0
    assert lib.bge_world_sphere_recover(w._h, 4, None, None) == -1
    # penetration
    spheres = W.make_spheres(recs["position"], recs["radius"], recs["layer_mask"])
    so = torch.zeros(n * 20 + 4, dtype=torch.uint8, device="cuda:0")
    ho = torch.zeros(n * 40 + 4, dtype=torch.uint8, device="cuda:0")
    so[4:].copy_(torch.from_numpy(spheres.view(np.uint8).copy()).to("cuda:0"))
    torch.cuda.synchronize()
    w.sphere_penetration_device(so[4:], ho[4:])
    w.sync()
    assert ho[4:].cpu().numpy().tobytes() == shared.pen.tobytes() and not ho[:4].cpu().numpy().any()
    assert lib.bge_world_sphere_penetration_device(w._h, 4, C.c_void_p(so.data_ptr() + 2), C.c_void_p(ho.data_ptr())) == -1
    assert lib.bge_world_sphere_penetration_device(w._h, 4, C.c_void_p(so.data_ptr()), C.c_void_p(ho.data_ptr() + 1)) == -1
    assert lib.bge_world_sphere_penetration_device(w._h, 4, C.c_void_p(so.data_ptr()), None) == -1
    assert lib.bge_world_sphere_penetration_device(w._h, 0, None, None) == 0 and lib.bge_world_sphere_penetration(w._h, 0, None, None) == 0
    assert lib.bge_world_sphere_penetration(w._h, 4, None, None) == -1


def test_a_recovery_changes_nothing_and_shares_no_scratch_with_the_other_queries(shared):
    w, recs = shared.w, shared.recs
    o = recs["position"]
    d = np.tile(np.float32([[1.0, -0.5, 0.25]]), (len(o), 1))

    def state():
        pos, eul = w.download_pose()
        mv = w.sphere_move(o, d, recs["radius"], 0.01, 0.3, 0.7, recs["layer_mask"])
        c, ov = w.sphere_cast(o, d, 2.0, recs["radius"], recs["layer_mask"]), w.overlap_sphere(o, recs["radius"], recs["layer_mask"])
        return [pos.tobytes(), eul.tobytes(), mv.tobytes()] + [c[k].tobytes() for k in sorted(c)] + [ov[k].tobytes() for k in sorted(ov)]

    before = state()
    again = recover(w, recs)
    assert state() == before and again.tobytes() == shared.got.tobytes()
    # a recovery right after a move and a move right after a recovery: neither reads what the other left in its scratch
    mv = w.sphere_move(o, d, recs["radius"], 0.01, 0.3, 0.7, recs["layer_mask"])
    assert recover(w, recs).tobytes() == shared.got.tobytes()
    assert w.sphere_move(o, d, recs["radius"], 0.01, 0.3, 0.7, recs["layer_mask"]).tobytes() == mv.tobytes()


def test_before_set_topology_they_answer_as_the_overlap():
    w = B.World(device=0)
    try:
        lib = B.lib()
        spheres, hits = W.make_spheres([[0, 1, 0]], 0.5), np.zeros(1, W.PENETRATION_HIT_DTYPE)
        recs, res = W.make_sphere_recovers([[0, 1, 0]]), np.zeros(1, W.SPHERE_RECOVER_RESULT_DTYPE)
        total = C.c_uint64(0)
        rc = lib.bge_world_overlap_sphere(w._h, 1, spheres.ctypes.data, None, 0, None, C.byref(total))
        assert rc != 0
        assert lib.bge_world_sphere_penetration(w._h, 1, spheres.ctypes.data, hits.ctypes.data) == rc
        assert lib.bge_world_sphere_recover(w._h, 1, recs.ctypes.data, res.ctypes.data) == rc
    finally:
        w.close()
