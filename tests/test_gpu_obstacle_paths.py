"""Every route, grid regime and capacity edge of the obstacle path (k_obstacles, k_obstacle_grid, k_ground_select,
k_contact_boxes, contact_body, for_each_obstacle_near) against the oracle, bit for bit.

Each scene of refmodel/obstacle_cases.py exists for one of them: a grid size and the side without a grid, the wide list empty, full
and overflowing, bodies too large or too fast for the grid, obstacles 3.6e38 apart, the box list by reach without a partner, the cap of
four manifolds under churn, all twenty solver rows, a box list longer than k_contact_boxes has threads, the obstacle list rebuilt,
shuffled slots, sub-steps, and the switch going off and on.  WHICH route a body takes is not read back from the device:
test_obstacle_cases_cpu.py classifies the oracle's state of every tick by the kernels' own rules and asserts that the scene holds its
class, with a margin.  Here, after every compared tick: activation state and timers, position, rotationEuler, quaternion, both
velocities, the plane manifold and every box manifold (partner, points, impulses) of every Dynamic body
(helpers.compare_obstacle_world); the world matrices at the end."""
import time

import numpy as np
import pytest

import banggameengine_amd as B
from helpers import DT, assert_bits_equal, build_obstacle_oracle, compare_obstacle_world
from refmodel import obstacle_cases as oc

pytestmark = pytest.mark.gpu

BASIS = pytest.mark.parametrize("basis", [False, True], ids=["default", "bullet_basis"])
GRID = pytest.mark.parametrize("grid", [True, False], ids=["grid", "all-obstacles"])


def _apply_to_world(case, tick, w):
    """The edits of that tick on the device's world (the oracle's side is obstacle_cases.apply_to_oracle)."""
    for ed in case.edits_at(tick):
        kind, one = ed[1], (lambda a: np.asarray(a, np.float32).reshape(1, 3))
        if kind == "trs":
            w.upload_trs(pos=one(ed[3]), first=int(ed[2]))
        elif kind == "vel":
            w.set_velocities(one(ed[3]), one(ed[4]), first=int(ed[2]))
        elif kind in ("recreate", "type"):
            e = int(ed[2])
            t = case.types_at(tick)[e:e + 1]
            w.upload_bodies(t, mass=case.mass[e:e + 1], size=case.size[e:e + 1], first=e)
        elif kind == "static":
            w.set_static_contacts(bool(ed[2]))
        else:
            raise ValueError(kind)


def _run(case, monkeypatch, basis=False, grid=True, after_edits=None):
    """Steps the case in the oracle and on the device, the edits applied to both, and compares after every compared tick; the slowest
    device tick in seconds.  after_edits(tick, w, ref): a look at both right after a tick's edits, before the tick."""
    monkeypatch.setenv("BGE_OBSTACLE_GRID", "1" if grid else "0")
    ref = build_obstacle_oracle(case, basis)
    flags = B.TICK_ALL | (B.TICK_BULLET_BASIS if basis else 0)
    wl = case.wl
    slowest = 0.0
    with B.World() as w:
        w.set_topology(wl.parent, case.has_transform)
        w.upload_trs(wl.pos, wl.euler, wl.scale)
        w.upload_bodies(wl.body_type, mass=case.mass, size=case.size)
        w.set_ground_plane(case.plane)
        w.set_static_contacts(case.static)
        for tick in range(case.ticks):
            _apply_to_world(case, tick, w)
            oc.apply_to_oracle(case, tick, ref)
            if after_edits is not None and case.edits_at(tick):
                after_edits(tick, w, ref)
            oc.step_oracle(case, tick, ref, DT, edits=False)
            t0 = time.perf_counter()
            if case.sub_steps:
                assert w.step_simulation(DT * case.sub_steps, 4, DT, flags=flags) == ref.LastSubSteps() == case.sub_steps
            else:
                w.tick(dt=DT, flags=flags)
            w.sync()
            if tick:                                   # (the first tick allocates)
                slowest = max(slowest, time.perf_counter() - t0)
            if tick < case.compare_from:
                continue
            dyn = case.types_at(tick) == oc.DYNAMIC
            bodies = None
            if case.compare_every > 1:                 # (a world of many thousands: every 16th body, and the first and last 128)
                d = np.flatnonzero(dyn)
                bodies = np.unique(np.concatenate([d[:128], d[::case.compare_every], d[-128:]]))
            compare_obstacle_world(w, ref, tick, dyn, case.plane, bodies)
        assert_bits_equal(w.download_world(), ref.bulk_world()[0], "world matrices at the end")
    print(f"{case.name}: {case.n} entities, slowest device tick after the first {slowest * 1e3:.1f} ms")
    return slowest


@BASIS
def test_sixty_four_obstacles_are_the_side_without_a_grid(basis, monkeypatch):
    """64 blocks: the host asks for no grid (more than kObstacleGridMin = 64 are needed); every body walks all obstacles."""
    _run(oc.grid_sizes(64), monkeypatch, basis)


@GRID
@BASIS
@pytest.mark.parametrize("K", [65, 256, 257, 1024, 1025])
def test_every_grid_size_on_both_sides_of_its_limits(K, basis, grid, monkeypatch):
    """65 and 256 obstacles: the 16 x 16 grid; 257 and 1 024: 32 x 32; 1 025: 64 x 64, and the three strided loops of k_obstacle_grid take a
    second trip.  Bodies rain on the two far corners, some of them outside the obstacles' bounds (clamped cells 0 and n - 1).  With the
    grid and with BGE_OBSTACLE_GRID=0 (every body tests every obstacle): both equal the oracle, hence each other."""
    _run(oc.grid_sizes(K), monkeypatch, basis, grid)


@GRID
def test_the_largest_grid_under_four_thousand_obstacles(grid, monkeypatch):
    """4 097 obstacles on the 64 x 64 grid (n stops at kObstacleGridAxis), five trips of the strided loops.  Default scheme only."""
    _run(oc.grid_sizes(4097), monkeypatch, False, grid)


@GRID
@BASIS
@pytest.mark.parametrize("W", [1, 32, 33])
def test_the_wide_list_with_one_entry_full_and_overflowing(W, basis, grid, monkeypatch):
    """70 small blocks and W obstacles that cover more than 64 cells: one, kObstacleGridWide = 32 (the list full), and 33 — the list
    overflows, the grid is marked invalid and every body walks all obstacles."""
    _run(oc.wide_list(W), monkeypatch, basis, grid)


@GRID
@BASIS
def test_a_body_too_large_and_a_body_too_fast_for_the_grid(basis, grid, monkeypatch):
    """300 blocks; a 10 x 10 m plank and a small box at 1 500 m/s cover more than 64 cells and fall back to all obstacles, in
    k_ground_select and in contact_body; the ordinary boxes beside them walk the grid."""
    _run(oc.big_and_fast(), monkeypatch, basis, grid)


@GRID
@BASIS
def test_obstacles_too_far_apart_for_a_grid_still_collide(basis, grid, monkeypatch):
    """70 blocks, two of them at x = -1.8e38 and +1.8e38: the common bounds have no finite span, no obstacle can be put on the grid.
    Such a grid used to be left VALID and empty — every body was told that nothing is near it, and one far-away Static box switched
    off all static collisions (with 64 obstacles or fewer, or BGE_OBSTACLE_GRID=0, the same scene collided).  Now it is marked
    invalid.  The boxes must rest on the near blocks as the oracle's do."""
    case = oc.far_apart()
    _run(case, monkeypatch, basis, grid)


@BASIS
def test_bodies_on_the_box_list_by_reach_without_a_partner(basis, monkeypatch):
    """Boxes at rest on the plane next to a wall: k_ground_select's conservative reach sends them to k_contact_boxes, the exact test finds
    no pair.  contact_body must leave their plane manifold exactly as k_ground would."""
    _run(oc.near_miss(), monkeypatch, basis)


@BASIS
def test_the_cap_of_four_manifolds_under_churn(basis, monkeypatch):
    """A plank across six blocks holds the four lowest.  A Kinematic block of a LOWER entity id arrives (the highest is evicted, its
    row reused), leaves again (the evicted one returns as a new pair), and a held block is re-created (generation)."""
    _run(oc.five_under_a_plank(), monkeypatch, basis)


@BASIS
def test_all_twenty_solver_rows_at_once(basis, monkeypatch):
    """A plank on the plane across four plates: 4 plane points and 4 manifolds of 4 points, kMaxContactRows = 20."""
    _run(oc.twenty_rows(), monkeypatch, basis)


def test_a_box_list_longer_than_k_contact_boxes_has_threads(monkeypatch):
    """16 500 boxes on one slab: the box list is longer than the 256 x 64 threads of k_contact_boxes, whose grid-stride loop takes a
    second trip.  Every 16th body and the first and last 128 are compared in full, every tick.  Default scheme only."""
    _run(oc.long_box_list(), monkeypatch)


@BASIS
def test_the_obstacle_list_rebuilt_when_bodies_change_type(basis, monkeypatch):
    """A Static table becomes Dynamic under resting boxes (asleep and awake), a resting Dynamic box becomes Static and a box lands on
    it, and at last no obstacle is left while a body still holds a row."""
    _run(oc.type_changes(), monkeypatch, basis)


@BASIS
def test_the_same_churn_where_slot_order_differs_from_entity_order(basis, monkeypatch):
    """five_under_a_plank and near_miss among pad entities that shuffle the slots: obstacle numbers ascend with entity ids, not
    with slots, and an obstacle sits at a slot beyond the entity count."""
    _run(oc.embedded(), monkeypatch, basis)


@GRID
@BASIS
def test_the_grid_rebuilt_in_every_sub_step(basis, grid, monkeypatch):
    """grid_sizes(65) and a Kinematic deck through bge_world_step_simulation, three sub-steps a call: k_obstacles and k_obstacle_grid run in
    each of them, the teleport rule in the first only."""
    _run(oc.sub_steps(), monkeypatch, basis, grid)


@BASIS
def test_switching_obstacle_contacts_off_ends_every_pair_and_a_tick_is_safe(basis, monkeypatch):
    """bge_world_set_static_contacts(0) with boxes resting awake on a Static box and one asleep: at once no body reports a box manifold,
    the sleeper included; the ticks that follow are safe (k_ground_select used to route a body that still carried kCiBoxes to a box
    list that does not exist while the switch is off); the awake boxes fall to the plane, the sleeper stays; switching on again
    starts from empty manifolds.  Bit for bit against the oracle through all of it."""
    case = oc.switch_off_and_on()
    seen = {}

    def after_edits(tick, w, ref):
        if tick in (oc.SWITCH_OFF, oc.SWITCH_ON):
            nb, hdr, _ = w.download_box_contacts()
            seen[tick] = nb.copy()
            assert not nb.any(), f"tick {tick}: manifolds {nb.tolist()} right after the switch"
            assert (hdr[:, :, 0] == 0xFFFFFFFF).all()
            assert all(ref.BoxContacts(e + 1) == [] for e in range(case.n))
        if tick == oc.SWITCH_OFF:
            st, _ = w.download_activation()
            assert st[case.sleeper] == 2 and (st[case.awake] == 1).all(), st

    _run(case, monkeypatch, basis, after_edits=after_edits)
    assert sorted(seen) == [oc.SWITCH_OFF, oc.SWITCH_ON]


@BASIS
def test_switching_off_under_an_island_that_rests_on_a_slab(basis):
    """The same switch with Dynamic contacts on: three boxes in one island whose own points are obstacle points (island_cases.on_a_slab,
    plane off).  Off: the island's bodies give up their rows like everybody else and fall; on again: new pairs.  Pair cache, poses,
    velocities, activation and every manifold against the oracle after every tick."""
    from helpers import build_island_oracle, compare_dynamic_world
    from refmodel import island_cases as ic
    case = ic.on_a_slab()
    ref = build_island_oracle(case, basis)
    flags = B.TICK_ALL | (B.TICK_BULLET_BASIS if basis else 0)
    off, on, ticks = 12, 20, 36
    with B.World() as w:
        w.set_topology(case.wl.parent, case.has_transform)
        w.upload_trs(case.wl.pos, case.wl.euler, case.wl.scale)
        w.upload_bodies(case.wl.body_type, mass=case.mass, size=case.size)
        w.set_ground_plane(False)
        w.set_static_contacts(True)
        w.set_dynamic_contacts(True)
        for tick in range(ticks):
            if tick in (off, on):
                held = w.download_box_contacts()[0]
                assert (held[case.dyn] > 0).all() == (tick == off)            # rows held before it goes off, none before it comes back
                w.set_static_contacts(tick == on)
                ref.SetStaticContacts(tick == on)
                assert not w.download_box_contacts()[0].any() and all(ref.BoxContacts(e + 1) == [] for e in range(case.n))
            ref.PhysicsSystemUpdate(DT)
            ref.TransformSystemUpdate()
            w.tick(dt=DT, flags=flags)
            _, hdr = compare_dynamic_world(w, ref, tick, case.dyn, False, True)
            assert len(hdr) > 0                                               # one island of several bodies all the way
            nb = compare_obstacle_world(w, ref, tick, case.dyn, False)
            assert (nb[case.dyn] > 0).all() == (not off <= tick < on), (tick, nb.tolist())
        assert_bits_equal(w.download_world(), ref.bulk_world()[0], "world matrices at the end")
