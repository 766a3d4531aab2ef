"""Sphere step moves on the device (include/bge_world.h "Sphere step moves", bge_world_sphere_step_move*).

The reference is step_ref of refmodel/step_moves.py — the header's rule in numpy float32 scalars — with World.sphere_cast on the
same world as its caster: the device runs the same casts and the same binary32 arithmetic between them, so the 80-byte records
must be equal byte for byte.  The step field, the movers and the coverage floors are those test_sphere_step_cpu.py checks on the
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
from refmodel.step_moves import compose_ref, step_ref
from refmodel.step_cases import (BATCHES, FIELD_SEED, HAND_STEPS, STEPPER_SEED, StepField, check_hand_step, check_invalid_steps, check_step_coverage,
                                 hand_stepper, invalid_steppers, step_coverage, stepper_batch)
from refmodel.device import FLAGS, device_caster, move
from refmodel.step_device import device_mover, field_world, hand_world, step_move

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Shared:
    """The step field, ticked once, the movers, and both answers for the largest batch: made once, never changed."""

    def __init__(self):
        self.field = StepField(np.random.default_rng(FIELD_SEED))
        self.w = field_world(self.field)
        self.moves = stepper_batch(np.random.default_rng(STEPPER_SEED), max(BATCHES), self.field)
        self.trace = {}
        self.want = step_ref(device_caster(self.w), self.moves, self.trace)
        self.got = step_move(self.w, self.moves)


@pytest.fixture(scope="module")
def shared():
    s = Shared()
    yield s
    s.w.close()


@pytest.mark.parametrize("n", BATCHES)
def test_equals_the_rule_over_the_device_cast_bit_for_bit(shared, n):
    moves = shared.moves[:n]
    got = shared.got if n == len(shared.moves) else step_move(shared.w, moves)
    want = shared.want[:n]  # (a mover's answer does not depend on its batch: step_ref asks one cast per mover and pass)
    bad = [i for i in range(n) if got[i].tobytes() != want[i].tobytes()]
    assert not bad, f"{len(bad)} of {n} differ, first {bad[0]}: {got[bad[0]]} vs {want[bad[0]]} ({shared.trace['outcome'][bad[0]]})"
    if n == len(shared.moves):
        check_step_coverage(step_coverage(got, shared.trace))
        assert ((got["flags"] & W.MOVE_INVALID) != 0).sum() == len(range(36, n, 37))
        assert (moves["displacement"] == 0).all(axis=1).sum() == len(range(40, n, 41))


@pytest.mark.parametrize("case", HAND_STEPS, ids=[c[0] for c in HAND_STEPS])
def test_hand_worked_steps_on_the_device(case):
    name, _, bodies, ghosts, plane, _, want = case
    w = hand_world(bodies, ghosts, plane)
    try:
        moves = hand_stepper(case)
        got = step_move(w, moves)
        check_hand_step(name, got[0], want)
        assert got[0].tobytes() == step_ref(device_caster(w), moves)[0].tobytes()
    finally:
        w.close()


def test_equals_the_composition_of_public_calls_on_the_device(shared):
    """Not stepped: World.sphere_move's bytes, with STEP_TRIED in addition.  Stepped: World.sphere_cast up, World.sphere_move with
    probe 0 from the raised position, World.sphere_cast down, World.sphere_cast for the probe."""
    want = compose_ref(device_caster(shared.w), shared.moves, shared.got, device_mover(shared.w))
    bad = [i for i in range(len(want)) if want[i].tobytes() != shared.got[i].tobytes()]
    assert not bad, (bad[0], shared.got[bad[0]], want[bad[0]])
    assert ((shared.got["flags"] & W.MOVE_STEPPED) != 0).sum() >= 30 and ((shared.got["flags"] & W.MOVE_STEPPED) == 0).sum() >= 300


def test_without_a_step_height_it_is_the_plain_move(shared):
    flat = shared.moves.copy()
    flat["step_height"] = 0
    got = step_move(shared.w, flat)
    assert got.tobytes() == move(shared.w, flat).tobytes()
    assert not (got["flags"] & (W.MOVE_STEP_TRIED | W.MOVE_STEPPED)).any() and (got["n_hits"] >= 1).sum() > 100


def test_invalid_steppers_on_the_device(shared):
    moves = invalid_steppers()
    check_invalid_steps(moves, step_move(shared.w, moves))


def test_never_inside(shared):
    """A mover that starts clear of everything by radius + skin ends clear of everything by radius - NEVER_INSIDE_MARGIN, stepped or
    not: the casts are exact, so every leg of the path it took is free, and Down backs off by the skin."""
    moves, got = shared.moves, shared.got
    ok = np.nonzero((got["flags"] & W.MOVE_INVALID) == 0)[0]
    m = moves[ok]
    # (the start is asked to be clear of the bodies and ghosts, all on layer 1: of the plane it is clear by radius + skin by
    # construction, to the bit, which an overlap of that very radius cannot tell from touching)
    start = shared.w.overlap_sphere(m["position"], m["radius"] + m["skin"], np.uint32(1))
    clear = np.diff(start["offsets"].astype(np.int64)) == 0
    end = shared.w.overlap_sphere(got["position"][ok][clear], m["radius"][clear] - NEVER_INSIDE_MARGIN, m["layer_mask"][clear])
    inside = np.nonzero(np.diff(end["offsets"].astype(np.int64)) != 0)[0]
    stepped = ((got["flags"][ok][clear] & W.MOVE_STEPPED) != 0).sum()
    print(f"{clear.sum()} of {len(ok)} valid movers start clear, {stepped} of them step; {len(inside)} end inside something")
    assert clear.sum() >= 100 and stepped >= 30
    assert len(inside) == 0, (ok[clear][inside], end["distance"])


def test_device_form_alignment_and_a_mask_that_sees_nothing(shared):
    import ctypes as C
    import torch
    w, moves, n = shared.w, shared.moves, len(shared.moves)
    mt = torch.from_numpy(moves.view(np.uint8).copy()).to("cuda:0")
    rt = torch.zeros(n * 80, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    w.sphere_step_move_device(mt, rt)
    w.sync()
    first = rt.cpu().numpy().tobytes()
    assert first == shared.got.tobytes()
    rt.zero_()
    torch.cuda.synchronize()
    w.sphere_step_move_device(mt, rt)
    w.sync()
    assert rt.cpu().numpy().tobytes() == first
    # records at 4-byte-aligned offsets that are no multiple of 8 or 16
    mo = torch.zeros(n * 48 + 4, dtype=torch.uint8, device="cuda:0")
    ro = torch.zeros(n * 80 + 12, dtype=torch.uint8, device="cuda:0")
    mo[4:].copy_(mt)
    assert mo[4:].data_ptr() % 8 == 4 and ro[12:].data_ptr() % 8 == 4
    torch.cuda.synchronize()
    w.sphere_step_move_device(mo[4:], ro[12:])
    w.sync()
    assert ro[12:].cpu().numpy().tobytes() == first and not ro[:12].cpu().numpy().any()
    # a misaligned or NULL pointer is refused before anything is enqueued
    lib = B.lib()
    ro.zero_()
    torch.cuda.synchronize()
    assert lib.bge_world_sphere_step_move_device(w._h, 4, C.c_void_p(mo.data_ptr() + 2), C.c_void_p(ro.data_ptr())) == -1
    assert lib.bge_world_sphere_step_move_device(w._h, 4, C.c_void_p(mo.data_ptr()), C.c_void_p(ro.data_ptr() + 1)) == -1
    assert lib.bge_world_sphere_step_move_device(w._h, 4, None, C.c_void_p(ro.data_ptr())) == -1
    assert lib.bge_world_sphere_step_move_device(w._h, 4, C.c_void_p(mo.data_ptr()), None) == -1
    w.sync()
    assert not ro.cpu().numpy().any()
    assert lib.bge_world_sphere_step_move_device(w._h, 0, None, None) == 0 and lib.bge_world_sphere_step_move(w._h, 0, None, None) == 0
    # layer 16 is nobody's and not the plane's: every valid mover goes its whole way, hits nothing, tries nothing and finds no ground
    blind = moves.copy()
    blind["layer_mask"] = 16
    bt = torch.from_numpy(blind.view(np.uint8).copy()).to("cuda:0")
    rt.zero_()
    torch.cuda.synchronize()
    w.sphere_step_move_device(bt, rt)
    w.sync()
    got = rt.cpu().numpy().view(W.SPHERE_STEP_RESULT_DTYPE)
    ok = (got["flags"] & W.MOVE_INVALID) == 0
    assert ok.sum() > 400 and (got["flags"][ok] == 0).all() and (got["n_hits"] == 0).all() and not got["remaining"].any() and not got["step_rise"].any()
    assert np.array_equal(got["position"][ok], (blind["position"] + blind["displacement"])[ok])
    assert step_move(w, blind).tobytes() == got.tobytes()


def test_a_step_move_changes_nothing(shared):
    w, moves = shared.w, shared.moves
    o, d = moves["position"], moves["displacement"]

    def state():
        pos, eul = w.download_pose()
        c, r = w.sphere_cast(o, d, 1.0, 0.3, ALL), w.raycast(o, d, 5.0, ALL)
        return [pos.tobytes(), eul.tobytes()] + [c[k].tobytes() for k in sorted(c)] + [r[k].tobytes() for k in sorted(r)]

    before = state()
    again = step_move(w, moves)
    assert state() == before and again.tobytes() == shared.got.tobytes()
    # a tick after a step move equals a tick without it: a second world with the same history but no step move
    other = field_world(shared.field)
    try:
        step_move(other, moves)
        other.tick(flags=FLAGS)
        plain = field_world(shared.field)
        try:
            plain.tick(flags=FLAGS)
            for a, b in zip(other.download_pose(), plain.download_pose()):
                assert a.tobytes() == b.tobytes()
            assert other.download_world().tobytes() == plain.download_world().tobytes()
        finally:
            plain.close()
    finally:
        other.close()


def test_before_set_topology_it_answers_as_the_sphere_cast():
    w = B.World(device=0)
    try:
        lib = B.lib()
        moves, res = W.make_sphere_step_moves([[0, 1, 0]], [[1, 0, 0]], step_height=0.3), np.zeros(1, W.SPHERE_STEP_RESULT_DTYPE)
        casts, hits = W.make_sphere_casts([[0, 1, 0]], [[1, 0, 0]]), np.zeros(1, W.RAY_HIT_DTYPE)
        rc = lib.bge_world_sphere_cast(w._h, 1, casts.ctypes.data, hits.ctypes.data)
        assert rc != 0 and lib.bge_world_sphere_step_move(w._h, 1, moves.ctypes.data, res.ctypes.data) == rc
    finally:
        w.close()


def test_adapter_step_on_demo_scene(tmp_path):
    cpp = os.path.join(ROOT, "tests", "cpp")
    lib = os.path.join(ROOT, "banggameengine_amd")
    exe = str(tmp_path / "step_demo_scene")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unused-parameter", "-o", exe,
                           os.path.join(cpp, "step_demo_scene.cpp"), f"-L{lib}", "-lbge_world", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "demo_scene.json")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "all checks passed" in r.stdout
