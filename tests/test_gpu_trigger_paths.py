"""Every route, regime and capacity edge of the world's trigger pass (k_trigger_aabb, k_trigger_pairs,
k_trigger_ghost_pairs, k_bp_classify_boxes, k_bp_query_boxes, k_trigger_diff_cur / _prev, k_trigger_table_build and the host state
machine around them) against the oracle, event for event.  Events are integer triples: every comparison is exact.

Each scene of refmodel/trigger_cases.py exists for one of them, and test_trigger_cases_cpu.py proves on the oracle alone that it holds
its class.  Here, per tick: trigger_events() equals the oracle's TriggerEvents(); a second world with set_trigger_stay_events(False)
reports exactly the oracle's events without the Stay rows; trigger_active equals TriggerIsActive; and bge_world_trigger_diff_stats
moves by exactly the route the case claims for that tick — device, host, or neither.  Per case: stay_suppressed equals the oracle's
Stay count, the world still answers trigger_boxes and download_bodies, and where the case says how the ghosts split between the grid and
the all-bodies pass, trigger_query_stats says the same.

The overflow cases are ordinary error returns: every store into the hit list and the delta list is guarded (`if (at < cap)` in
k_trigger_pairs, k_trigger_ghost_pairs and k_bp_query_boxes, `if (at < d.delta_cap)` in trig_append; k_trigger_diff_cur reads
min(hits, pair_cap) records), which test_trigger_cases_cpu.py pins to the sources."""
import numpy as np
import pytest

import banggameengine_amd as B
from refmodel import trigger_cases as tc
from refmodel import trigger_device as td

pytestmark = pytest.mark.gpu

ids = lambda builders: [tc.case_name(b) for b in builders]


def _run(builder, monkeypatch, device_diff=True, lean=True, after_tick=None):
    """The case on a world with Stay records and (lean) on one without, tick by tick against the expected events."""
    case, events, active, steps = tc.expected(builder)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    if not device_diff:
        monkeypatch.setenv("BGE_TRIGGER_DEVICE_DIFF", "0")
    routes = case.routes if device_diff else case.routes_on_the_host()
    worlds = [td.open_world(case, stay=True)] + ([td.open_world(case, stay=False)] if lean else [])
    try:
        stays = 0
        for tick, t in enumerate(case.ticks):
            want = events[tick]
            trig = case.trig_at(tick)
            for w in worlds:
                before = w.trigger_diff_stats()
                td.apply_edits(case, tick, w)
                if routes[tick] == "E":
                    with pytest.raises(B.BgeError) as err:
                        td.step(case, tick, w)
                    assert str(tc.PAIR_CAP) in str(err.value) and str(tc.PAIR_CAP + 1) in str(err.value), str(err.value)
                else:
                    assert td.step(case, tick, w) == steps[tick]
                got = w.trigger_events()
                want_w = want if w is worlds[0] else want[want[:, 0] != tc.STAY]
                assert np.array_equal(got, want_w), f"{case.name} tick {tick} ({'with' if w is worlds[0] else 'without'} Stay): {len(got)} events, expected {len(want_w)}"
                after = w.trigger_diff_stats()
                moved = (after[0] - before[0], after[1] - before[1])
                assert moved == tc.counts(routes[tick]), f"{case.name} tick {tick}: (device, host) moved by {moved}, the case claims '{routes[tick]}'"
                assert np.array_equal(w.trigger_active(trig.entity), active[tick]), f"{case.name} tick {tick}: TriggerVolume::active"
            stays += int((want[:, 0] == tc.STAY).sum())
            if after_tick is not None:
                after_tick(tick, worlds[0])
        for w in worlds:
            device, host, suppressed = w.trigger_diff_stats()
            assert (device, host) == tc.counts(routes), (case.name, device, host, routes)
            assert suppressed == (0 if w is worlds[0] else stays), (case.name, suppressed, stays)
            boxes, listed = w.trigger_boxes(case.trig_at(len(case.ticks) - 1).entity)          # the world still answers
            assert listed.shape == (len(boxes),) and np.isfinite(boxes[listed.astype(bool)]).all()
            assert len(w.download_bodies(count=min(case.n, 64))["linvel"]) == min(case.n, 64)
        if "E" in routes:                                                                      # ... and a fresh tick succeeds
            for w in worlds:
                w.tick(dt=td.FIXED_DT, flags=td.FLAGS)
                assert set(w.trigger_events()[:, 0].tolist()) <= {tc.STAY}
    finally:
        for w in worlds:
            w.close()
    return case


# ------------------------------------------------------------------------------------------------------------------ A: the difference regimes

QUICK_A = [b for b in tc.FAMILY_A if b is not tc.delta_cap_edge]


@pytest.mark.parametrize("device_diff", [True, False], ids=["device-diff", "host-diff"])
@pytest.mark.parametrize("builder", QUICK_A, ids=ids(QUICK_A))
def test_the_difference_regimes(builder, device_diff, monkeypatch):
    """Quiet ticks; 1 024 | 1 025 deltas (the second copy); the load-factor fallback and the larger rebuild; a different set uploaded
    between two device ticks; set_topology between two device ticks with a ghost frozen; a call that simulates nothing; an entity met
    both ways.  With BGE_TRIGGER_DEVICE_DIFF=0 the events are the same and no tick is the device's."""
    case = _run(builder, monkeypatch, device_diff)
    assert ("d" in case.routes) and (device_diff or "d" not in case.routes_on_the_host())


@pytest.mark.parametrize("device_diff", [True, False], ids=["device-diff", "host-diff"])
def test_sixty_five_thousand_deltas_stay_on_the_device_and_one_more_goes_to_the_host(device_diff, monkeypatch):
    """70 000 bodies change ghosts: 65 536 deltas in a tick are fetched in two copies and applied from the device's list; 65 537 send
    the tick to the host, which rebuilds the table; the tick after that is the device's again."""
    _run(tc.delta_cap_edge, monkeypatch, device_diff)


# ------------------------------------------------------------------------------------------------------------------ B: the pair buffer


@pytest.mark.parametrize("stay", [True, False], ids=["stay", "no-stay"])
def test_exactly_two_to_the_twenty_overlaps_succeed_on_both_paths(stay, monkeypatch):
    """16 ghosts over 65 536 bodies: the buffer exactly full on a first tick (host path), when everybody is teleported back in (the
    device path looks at the count, then leaves the 2^20 deltas to the host) and in a tick of 2^20 Stay on the device."""
    case, events, active, steps = tc.expected(tc.pair_buffer_full)
    with td.open_world(case, stay=stay) as w:
        for tick in range(len(case.ticks)):
            td.apply_edits(case, tick, w)
            td.step(case, tick, w)
            want = events[tick] if stay else events[tick][events[tick][:, 0] != tc.STAY]
            assert np.array_equal(w.trigger_events(), want), f"tick {tick}"
            assert w.trigger_diff_stats()[:2] == tc.counts(case.routes[:tick + 1]), (tick, w.trigger_diff_stats())
        assert w.trigger_diff_stats()[2] == (0 if stay else sum(int((e[:, 0] == tc.STAY).sum()) for e in events))
        assert len(w.download_bodies(count=8)["linvel"]) == 8


@pytest.mark.parametrize("device_diff", [True, False], ids=["device-diff", "host-diff"])
def test_one_overlap_more_fails_and_ticking_goes_on_from_the_sets_before(device_diff, monkeypatch):
    """2^20 + 1 overlaps: BGE_ERR_OOM with both numbers in the message, on a first tick (host path) and on the device path after
    k_trigger_diff_cur has run; nothing faults, the stores are guarded.  The failed tick reports nothing and leaves the remembered sets
    alone (include/bge_world.h): the next tick's events are the numpy ProcessTriggerEvents' against the sets before the failure.
    process_trigger_pairs_fast used to return with the failed tick's 2^20 keys still in the current-tick table and the table still
    marked valid: the next tick then found every hit "already there" — no Enter, no Exit — and the tick after it diffed against that."""
    _run(tc.pair_buffer_overflow, monkeypatch, device_diff, lean=False)


# ------------------------------------------------------------------------------------------------------------------ C: the all-bodies pass


def test_the_slot_loop_of_k_trigger_pairs_takes_a_second_trip(monkeypatch):
    """524 288 + 300 slots, three ghosts: the hits sit in the first 64 slots and in the last 300, which only the second trip reaches."""
    def split(tick, w):
        assert w.trigger_query_stats() == (0, 0)                 # three ghosts: nobody asks the grid
    _run(tc.second_slot_trip, monkeypatch, lean=False, after_tick=split)


@pytest.mark.parametrize("builder", tc.FAMILY_C[1:], ids=ids(tc.FAMILY_C[1:]))
def test_one_wave_of_the_all_bodies_pass(builder, monkeypatch):
    """0, 1, 63, 64 and 65 hits of one ghost in one wave's ballot (65: the next wave's first lane too); a ghost on a body never lists itself."""
    _run(builder, monkeypatch)


# ------------------------------------------------------------------------------------------------------------------ D: the grid look-up


@pytest.mark.parametrize("builder", tc.FAMILY_D[:10], ids=ids(tc.FAMILY_D[:10]))
def test_every_ghost_shape_through_the_grid(builder, monkeypatch):
    """The lattice with 0, 1, 64 and 65 large-list bodies, compact records (9 filter classes) and full ones (300): ghosts inside a cell,
    of 45 to 120 rows of cells, long and thin, hanging out of the grid on every side, outside the bounds, beyond the lattice where only
    large bodies are, with straddling bodies below their first cell.  And 64 | 65 ghosts at the default minimum.  How the ghosts split
    between the grid and the all-bodies pass is asserted exactly: every one of them is far from 8 192 cells."""
    case = tc.expected(builder)[0]

    def split(tick, w):
        assert w.trigger_query_stats() == case.query[tick], (case.name, tick, w.trigger_query_stats())
    _run(builder, monkeypatch, after_tick=split)


def test_more_boxes_than_the_query_has_waves(monkeypatch):
    """8 200 ghosts through the grid: the box loop of k_bp_query_boxes takes a second trip."""
    case = tc.expected(tc.many_boxes)[0]

    def split(tick, w):
        assert w.trigger_query_stats() == case.query[tick]
    _run(tc.many_boxes, monkeypatch, lean=False, after_tick=split)


def test_a_ghost_grows_across_the_cell_limit(monkeypatch):
    """From a few hundred cells to the whole grid, several times 8 192: in the grid at the first step, against all bodies at the last,
    never back in between (the step of the switch depends on the cell the device chose and is not asserted); every step's events are
    the oracle's."""
    seen = []
    _run(tc.cell_sweep, monkeypatch, lean=False, after_tick=lambda tick, w: seen.append(w.trigger_query_stats()))
    assert seen[0] == (2, 0) and seen[-1] == (1, 1), seen
    assert all(s in ((2, 0), (1, 1)) for s in seen) and all(a[1] <= b[1] for a, b in zip(seen, seen[1:])), seen


# ------------------------------------------------------------------------------------------------------------------ E, F


@pytest.mark.parametrize("builder", tc.FAMILY_E, ids=ids(tc.FAMILY_E))
def test_ghost_against_ghost_at_the_tile_edges(builder, monkeypatch):
    """1, 2, 63 | 64 | 65, 255 | 256 | 257 and 513 ghosts that all overlap each other: the 256 x 64 tiles of k_trigger_ghost_pairs full, one short
    and one over; three filter classes of which about half the pairs pass, both ways round; inactive volumes, a frozen ghost, a
    cluster moved apart."""
    _run(builder, monkeypatch)


@pytest.mark.parametrize("grid_min", [1 << 20, 0], ids=["all-bodies", "grid"])
@pytest.mark.parametrize("builder", tc.FAMILY_F, ids=ids(tc.FAMILY_F))
def test_boxes_a_binary32_step_either_side_of_touching(builder, grid_min, monkeypatch):
    """Rows of 200 (ghost, body) and 200 (ghost, ghost) pairs along each axis, the partner beyond the ghost's high face in two rows and
    below its low face in two more, from 100 binary32 steps inside the touching distance to 99 outside; one pair of every row
    touches exactly.  Touching counts, one step more does not — in k_trigger_pairs (the 1 200 ghosts kept out of the grid by a
    minimum above them), in k_bp_query_boxes (every ghost through the grid) and in k_trigger_ghost_pairs."""
    monkeypatch.setenv("BGE_TRIGGER_GRID_MIN", str(grid_min))
    n_trig = len(tc.expected(builder)[0].trig.entity)

    def split(tick, w):
        assert w.trigger_query_stats() == ((n_trig, 0) if grid_min == 0 else (0, 0))
    _run(builder, monkeypatch, after_tick=split)
