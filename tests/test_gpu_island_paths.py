"""Every routing class and capacity regime of the island solver (bge_island.hip) against the oracle, bit for bit.

k_island_solve sends an awake island to one of four solvers — the LDS column solver (<= 4 bodies, <= 16 points), the mid launch (up to
16 bodies, delta velocities in LDS), the one-thread solver in global memory (more bodies on <= big_points points), k_island_solve_big (a
workgroup, level by level) — and the workgroup solver has regimes of its own by island size.  Each scene of refmodel/island_cases.py
exists for one of them; WHICH path a scene takes is not read back from the device: test_island_cases_cpu.py classifies the oracle's
state of every compared tick by the kernel's own rules and asserts that the scene holds its class, with a margin.  Here, after every
compared tick: the pair cache (which pairs, their points, their impulses), pose, quaternion, rotationEuler, velocities, plane
manifolds, activation state and timers (helpers.compare_dynamic_world) equal the oracle's."""
import time

import numpy as np
import pytest

import banggameengine_amd as B
from helpers import DT, assert_bits_equal, build_island_oracle, compare_dynamic_world
from refmodel import island_cases as ic

pytestmark = pytest.mark.gpu

BASIS = pytest.mark.parametrize("basis", [False, True], ids=["default", "bullet_basis"])


def _run(case, monkeypatch, basis=False):
    """Steps the case in the oracle and on the device and compares after every compared tick; the slowest device tick in seconds."""
    monkeypatch.setenv("BGE_ISLAND_BIG_POINTS", str(case.big_points))
    ref = build_island_oracle(case, basis)
    flags = B.TICK_ALL | (B.TICK_BULLET_BASIS if basis else 0)
    wl, dyn = case.wl, case.dyn
    slowest = 0.0
    with B.World() as w:
        w.set_topology(wl.parent, case.has_transform)
        w.upload_trs(wl.pos, wl.euler, wl.scale)
        w.upload_bodies(wl.body_type, mass=case.mass, size=case.size)
        w.set_ground_plane(case.plane)
        w.set_static_contacts(case.static)
        w.set_dynamic_contacts(True)
        for tick in range(case.ticks):
            ref.PhysicsSystemUpdate(DT)
            ref.TransformSystemUpdate()
            t0 = time.perf_counter()
            w.tick(dt=DT, flags=flags)
            w.sync()
            if tick:                                   # (the first tick allocates)
                slowest = max(slowest, time.perf_counter() - t0)
            if tick < case.compare_from:
                continue
            _, hdr = compare_dynamic_world(w, ref, tick, dyn, case.plane, case.static)
            assert len(hdr) > 0
        assert_bits_equal(w.download_world(), ref.bulk_world()[0], "world matrices at the end")
    print(f"{case.name}: {case.n} entities, slowest device tick after the first {slowest * 1e3:.1f} ms")
    return slowest


@BASIS
def test_small_mid_and_global_islands_on_both_sides_of_their_limits(basis, monkeypatch):
    """Stacks of 3 and 4 (LDS column solver), 5 and 16 (mid launch, 16 at its body limit), 17 and 20 (the one-thread solver in global
    memory), rows of 3 and of 4 on the plane (at most 4 bodies, more than 16 points: mid), 16 ticks, all compared."""
    _run(ic.boundaries(), monkeypatch, basis)


@BASIS
def test_the_same_islands_where_slot_order_differs_from_entity_order(basis, monkeypatch):
    """The scene above embedded among pad entities that shuffle its slots: island keys are root SLOT << 32 | entity, so the islands
    come in another order and an island's root is not its lowest entity."""
    _run(ic.boundaries_embedded(), monkeypatch, basis)


@BASIS
def test_obstacle_manifolds_in_an_island(basis, monkeypatch):
    """Three boxes on a Static slab, plane off: the island's own points are obstacle points, and they make it a mid island."""
    _run(ic.on_a_slab(), monkeypatch, basis)


@BASIS
def test_a_mid_list_longer_than_a_launch_of_one_thread_per_five_bodies(basis, monkeypatch):
    """300 rows of four boxes: 1 200 island bodies and 300 entries on the mid list.  A mid launch sized for islands of five bodies or
    more had 256 threads for them: the last 44 rows were never solved (their bodies neither integrated nor their impulses written)."""
    _run(ic.rows_of_four(), monkeypatch, basis)


@BASIS
@pytest.mark.parametrize("big_points", [128, 0], ids=["mid-list-of-several-blocks", "more-big-islands-than-workgroups"])
def test_three_hundred_stacks_of_five(big_points, basis, monkeypatch):
    """Under the product's 128 points the 300 stacks fill five blocks of the mid launch (every LDS lane column is used); under 0 they are
    300 big islands for 256 workgroups: the ticket loop hands some workgroups a second island."""
    _run(ic.stacks_of_five(big_points), monkeypatch, basis)


@BASIS
def test_a_big_island_without_a_contact_point(basis, monkeypatch):
    """Eight boxes in each other's fed AABBs that never touch, plane off, BGE_ISLAND_BIG_POINTS = 0: the workgroup solver's P == 0
    branch — gravity and nothing else."""
    case = ic.free_fall()
    _run(case, monkeypatch, basis)


@BASIS
def test_more_levels_than_the_scan_has_threads(basis, monkeypatch):
    """A row of 40 boxes in index order: 280 points in 280 levels under the product's 128 points — isl_wg_scan sums two elements a
    thread, and every sweep is a chain of 280 barriers."""
    _run(ic.deep_row(), monkeypatch, basis)


@BASIS
@pytest.mark.parametrize("name", ["carpet45", "carpet56", "sparse-line"])
def test_the_workgroup_solver_beyond_its_lds(name, basis, monkeypatch):
    """carpet45: 2 025 bodies on ~28 k points — the level walk reads the rows from global memory, the bodies' delta velocities are in
    LDS.  carpet56: 3 136 bodies — those are in global memory too.  sparse-line: 3 400 falling boxes on 6 800 points — the walk in
    LDS, the bodies not.  Entity indices are shuffled against position."""
    _run(ic.BEYOND_LDS[name](), monkeypatch, basis)


def test_an_island_whose_bodies_last_levels_do_not_fit_the_lds(monkeypatch):
    """193 x 193 boxes: 37 249 bodies on ~500 k points in one island, on one workgroup, 2 ticks (last_in_lds false: the level walk
    keeps every body's last level in global memory).  Measured on an MI355X and its host: 0.38 s a device tick, 2.1 .. 2.5 s the
    whole test.  Default scheme only: a second scheme would cost more than a second."""
    _run(ic.BEYOND_LDS["carpet193"](), monkeypatch)
