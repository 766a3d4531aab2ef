"""Sphere moves on the device (include/bge_world.h "Sphere moves", bge_world_sphere_move*).

The reference is move_ref of refmodel/moves.py — the header's rule in numpy float32 scalars — with World.sphere_cast on the
same world as its caster: the device runs the same casts and the same binary32 arithmetic between them, so the 80-byte records
must be equal byte for byte.  The batches, the scene and the coverage floors are those test_sphere_move_cpu.py checks on the
float64 shape reference alone.  The hand-worked cases carry the numbers derived there, on real shapes, to 1e-5."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

import banggameengine_amd as B
from banggameengine_amd import world as W

from refmodel.tolerances import NEVER_INSIDE_MARGIN
from refmodel.rays import ALL
from refmodel.moves import move_ref
from refmodel.sphere_cases import scene_world64
from refmodel.move_cases import (BATCHES, HAND_MOVES, MOVER_SEED, SCENE_N, SCENE_SEED, check_coverage, check_hand_move, check_invalid, coverage,
                                 ghost_positions, hand_mover, invalid_movers, mover_batch)
from refmodel.device import FLAGS, Scene, device_caster, move

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Shared:
    """The scene of the comparison, ticked once, the movers, and both answers for the largest batch: made once, never changed."""

    def __init__(self):
        self.sc = Scene(SCENE_N, np.random.default_rng(SCENE_SEED), n_triggers=12)
        self.sc.tick(1)
        self.w = self.sc.w
        # the ghosts stand where their entities' Transforms were uploaded: the movers are those of the CPU file, to the bit
        ghosts = ghost_positions(scene_world64(SCENE_N, np.random.default_rng(SCENE_SEED))[0])
        self.moves = mover_batch(np.random.default_rng(MOVER_SEED), max(BATCHES), ghosts)
        self.trace = {}
        self.want = move_ref(device_caster(self.w), self.moves, self.trace)
        self.got = move(self.w, self.moves)


@pytest.fixture(scope="module")
def shared():
    s = Shared()
    yield s
    s.sc.close()


@pytest.mark.parametrize("n", BATCHES)
def test_equals_the_stepped_composition_bit_for_bit(shared, n):
    moves = shared.moves[:n]
    got = shared.got if n == len(shared.moves) else move(shared.w, moves)
    want = shared.want[:n]  # (a mover's answer does not depend on its batch: move_ref asks one cast per mover and round)
    bad = [i for i in range(n) if got[i].tobytes() != want[i].tobytes()]
    assert not bad, f"{len(bad)} of {n} differ, first {bad[0]}: {got[bad[0]]} vs {want[bad[0]]}"
    assert (moves["displacement"] == 0).all(axis=1).sum() == len(range(40, n, 41))
    if n == len(shared.moves):
        check_coverage(coverage(moves, got, shared.trace["crease"]))
        assert ((got["flags"] & W.MOVE_INVALID) != 0).sum() == len(range(36, n, 37))
        assert (got["hit_kind"] == W.RAY_BODY).any() and (got["hit_kind"] == W.RAY_GROUND).any() and (got["hit_kind"] == W.RAY_TRIGGER).any()


def test_invalid_movers_on_the_device(shared):
    moves = invalid_movers()
    check_invalid(moves, move(shared.w, moves))


@pytest.mark.parametrize("case", HAND_MOVES, ids=[c[0] for c in HAND_MOVES])
def test_hand_worked_moves_on_the_device(case):
    name, _, bodies, ghosts, plane, _, want = case
    n = max(len(bodies), 1)
    w = B.World(device=0)
    try:
        w.set_topology(np.full(n, W.NO_PARENT, np.uint32))
        w.upload_trs(np.float32([b[2] for b in bodies] or [[0, 0, 0]]), np.float32([b[3] for b in bodies] or [[0, 0, 0]]), np.ones((n, 3)))
        types = np.full(n, W.BODY_STATIC if bodies else W.BODY_NONE, np.uint8)
        types[list(ghosts)] = W.BODY_NONE
        shapes = np.uint8([b[0] for b in bodies] or [0])
        sizes = np.float32([b[1] for b in bodies] or [[0.5, 0.5, 0.5]])
        w.upload_bodies(types, None, shapes, sizes, np.full(n, 1, np.uint32), np.full(n, ALL, np.uint32))
        if ghosts:
            g = np.uint32(list(ghosts))
            w.upload_triggers(g, shapes[g], sizes[g], np.full(len(g), 1, np.uint32), np.full(len(g), ALL, np.uint32), np.zeros(len(g), np.uint8),
                              np.ones(len(g), np.uint8))
        w.set_ground_plane(plane)
        w.tick(flags=FLAGS)
        moves = hand_mover(case)
        got = move(w, moves)
        check_hand_move(name, got[0], want)
        assert got[0].tobytes() == move_ref(device_caster(w), moves)[0].tobytes()
    finally:
        w.close()


def test_never_inside_and_never_backwards(shared):
    """A mover that starts clear of everything by radius + skin ends clear of everything by radius - 1e-3: the cast is exact, so
    the path it took is free; 1e-3 is over a hundred binary32 spacings at the scene's extent of 64.  And no move ends behind its
    start along the asked direction."""
    moves, got = shared.moves, shared.got
    ok = np.nonzero((got["flags"] & W.MOVE_INVALID) == 0)[0]
    m = moves[ok]
    start = shared.w.overlap_sphere(m["position"], m["radius"] + m["skin"], m["layer_mask"])
    clear = np.diff(start["offsets"].astype(np.int64)) == 0
    end = shared.w.overlap_sphere(got["position"][ok][clear], m["radius"][clear] - NEVER_INSIDE_MARGIN, m["layer_mask"][clear])
    inside = np.nonzero(np.diff(end["offsets"].astype(np.int64)) != 0)[0]
    print(f"{clear.sum()} of {len(ok)} valid movers start clear; {len(inside)} end inside something")
    assert clear.sum() >= 100
    assert len(inside) == 0, (ok[clear][inside], end["distance"])
    d = m["displacement"].astype(np.float64)
    along = ((got["position"][ok].astype(np.float64) - m["position"]) * d).sum(axis=1)
    assert (along >= -1e-5 * (d * d).sum(axis=1)).all()


def test_device_form_alignment_and_a_mask_that_sees_nothing(shared):
    import torch
    w, moves, n = shared.w, shared.moves, len(shared.moves)
    mt = torch.from_numpy(moves.view(np.uint8).copy()).to("cuda:0")
    rt = torch.zeros(n * 80, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    w.sphere_move_device(mt, rt)
    w.sync()
    first = rt.cpu().numpy().tobytes()
    assert first == shared.got.tobytes()
    rt.zero_()
    torch.cuda.synchronize()
    w.sphere_move_device(mt, rt)
    w.sync()
    assert rt.cpu().numpy().tobytes() == first
    # records at 4-byte-aligned offsets that are no multiple of 8 or 16
    mo = torch.zeros(n * 48 + 4, dtype=torch.uint8, device="cuda:0")
    ro = torch.zeros(n * 80 + 12, dtype=torch.uint8, device="cuda:0")
    mo[4:].copy_(mt)
    assert mo[4:].data_ptr() % 8 == 4 and ro[12:].data_ptr() % 8 == 4
    torch.cuda.synchronize()
    w.sphere_move_device(mo[4:], ro[12:])
    w.sync()
    assert ro[12:].cpu().numpy().tobytes() == first and not ro[:12].cpu().numpy().any()
    # a misaligned pointer is refused before anything is enqueued
    lib = B.lib()
    import ctypes as C
    assert lib.bge_world_sphere_move_device(w._h, 4, C.c_void_p(mo.data_ptr() + 2), C.c_void_p(ro.data_ptr())) == -1
    assert lib.bge_world_sphere_move_device(w._h, 4, C.c_void_p(mo.data_ptr()), C.c_void_p(ro.data_ptr() + 1)) == -1
    assert lib.bge_world_sphere_move_device(w._h, 4, None, C.c_void_p(ro.data_ptr())) == -1
    assert lib.bge_world_sphere_move_device(w._h, 0, None, None) == 0 and lib.bge_world_sphere_move(w._h, 0, None, None) == 0
    # layer 16 is nobody's and not the plane's: every valid mover goes its whole way, hits nothing and finds no ground
    blind = moves.copy()
    blind["layer_mask"] = 16
    bt = torch.from_numpy(blind.view(np.uint8).copy()).to("cuda:0")
    rt.zero_()
    torch.cuda.synchronize()
    w.sphere_move_device(bt, rt)
    w.sync()
    got = rt.cpu().numpy().view(W.SPHERE_MOVE_RESULT_DTYPE)
    ok = (got["flags"] & W.MOVE_INVALID) == 0
    assert ok.sum() > 400 and (got["flags"][ok] == 0).all() and (got["n_hits"] == 0).all() and not got["remaining"].any()
    assert np.array_equal(got["position"][ok], (blind["position"] + blind["displacement"])[ok])
    assert move(w, blind).tobytes() == got.tobytes()


def test_a_move_changes_nothing(shared):
    w, moves = shared.w, shared.moves
    o, d = moves["position"], moves["displacement"]

    def state():
        pos, eul = w.download_pose()
        c, r = w.sphere_cast(o, d, 1.0, 0.3, ALL), w.raycast(o, d, 5.0, ALL)
        return [pos.tobytes(), eul.tobytes()] + [c[k].tobytes() for k in sorted(c)] + [r[k].tobytes() for k in sorted(r)]

    before = state()
    again = move(w, moves)
    assert state() == before and again.tobytes() == shared.got.tobytes()
    # a tick after a move equals a tick without it: a second world with the same history but no move
    other = Scene(SCENE_N, np.random.default_rng(SCENE_SEED), n_triggers=12)
    try:
        other.tick(1)
        move(other.w, moves)
        other.tick(1)
        plain = Scene(SCENE_N, np.random.default_rng(SCENE_SEED), n_triggers=12)
        try:
            plain.tick(2)
            for a, b in zip(other.w.download_pose(), plain.w.download_pose()):
                assert a.tobytes() == b.tobytes()
            assert other.w.download_world().tobytes() == plain.w.download_world().tobytes()
        finally:
            plain.close()
    finally:
        other.close()


def test_before_set_topology_it_answers_as_the_sphere_cast():
    w = B.World(device=0)
    try:
        lib = B.lib()
        moves, res = W.make_sphere_moves([[0, 1, 0]], [[1, 0, 0]]), np.zeros(1, W.SPHERE_MOVE_RESULT_DTYPE)
        casts, hits = W.make_sphere_casts([[0, 1, 0]], [[1, 0, 0]]), np.zeros(1, W.RAY_HIT_DTYPE)
        rc = lib.bge_world_sphere_cast(w._h, 1, casts.ctypes.data, hits.ctypes.data)
        assert rc != 0 and lib.bge_world_sphere_move(w._h, 1, moves.ctypes.data, res.ctypes.data) == rc
    finally:
        w.close()


def test_adapter_walk_on_demo_scene(tmp_path):
    cpp = os.path.join(ROOT, "tests", "cpp")
    lib = os.path.join(ROOT, "banggameengine_amd")
    exe = str(tmp_path / "move_demo_scene")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unused-parameter", "-o", exe,
                           os.path.join(cpp, "move_demo_scene.cpp"), f"-L{lib}", "-lbge_world", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "demo_scene.json")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "all checks passed" in r.stdout
