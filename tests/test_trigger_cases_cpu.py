"""The coverage claim of test_gpu_trigger_paths.py, checked without a GPU: every scene of refmodel/trigger_cases.py is run through the
ORACLE and held to the class it exists for — the exact Enter + Exit counts of the ticks that sit on an edge, the overlap totals of the
pair buffer cases, the hit counts of the all-bodies cases, the rows of the closed-interval cases, the route of every tick by the host
state machine's rules restated from numbers alone.  A scene that drifts out of its regime fails here, not silently on the device.
The numpy ProcessTriggerEvents (refmodel/trigger_events.py), which states what follows a FAILED tick, is held to the oracle's events on
every scene without one, and to three wrong answers fed to it.  And the constants the scenes were built with are the sources'."""
import os
import re

import numpy as np
import pytest

from banggameengine_amd import world as W
from refmodel import trigger_cases as tc
from refmodel import trigger_events as te
from refmodel.layout_cases import acyclic

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "banggameengine_amd", "csrc")
EVERY = [b for fam in tc.FAMILIES.values() for b in fam]
ids = lambda builders: [tc.case_name(b) for b in builders]


def _counts(ev):
    """(Enter + Stay, Enter + Exit) of a tick's events."""
    return int((ev[:, 0] != tc.EXIT).sum()), int((ev[:, 0] != tc.STAY).sum())


def _pairs(ev, types=(tc.ENTER, tc.STAY)):
    """{(trigger, other)} of the rows of these types."""
    return {(int(t), int(o)) for k, t, o in ev.tolist() if k in types}


# ------------------------------------------------------------------------------------------------------------------ the constants


def test_the_constants_are_the_sources():
    world = open(os.path.join(CSRC, "bge_world.cpp")).read()
    kern = open(os.path.join(CSRC, "bge_kernels.hip")).read()
    bp = open(os.path.join(CSRC, "bge_broadphase.hip")).read()
    shift = lambda name, text: 1 << int(re.search(rf"constexpr uint32_t {name} = 1u << (\d+);", text).group(1))
    num = lambda name, text: int(re.search(rf"constexpr uint32_t {name} = (\d+);", text).group(1))
    assert shift("kTriggerPairCap", world) == tc.PAIR_CAP and shift("kTrigDeltaCap", world) == tc.DELTA_CAP
    assert num("kFirst", world) == tc.FIRST_COPY and "if (n_delta > kFirst)" in world and "n_delta > kTrigDeltaCap" in world
    fn = world[world.index("int rebuild_trigger_mirror"):world.index("int process_trigger_pairs_fast")]
    assert int(re.search(r"uint32_t log2 = (\d+);", fn).group(1)) == tc.TABLE_MIN_LOG2
    assert "(1ull << log2) < 4 * std::max<uint64_t>(keys.size(), w->trig_pairs_host.size() / 2)" in fn          # table_log2
    assert "(static_cast<uint64_t>(host[1]) << 1) > (1ull << w->trig_tab_log2)" in world                         # 2 x fresh > table
    assert world.count("n_pairs > kTriggerPairCap") == 2                                                          # both error returns
    assert int(re.search(r"uint32_t trigger_grid_min = (\d+);", world).group(1)) == tc.GRID_MIN and "n_trig > w->trigger_grid_min" in world
    assert num("kTrigProbeLimit", kern) == tc.PROBE_LIMIT and num("kGhostTileJ", kern) == tc.GHOST_TILE_J
    assert num("kQueryMaxCells", bp) == tc.QUERY_MAX_CELLS and "cells <= kQueryMaxCells" in bp
    launch = re.search(r"k_trigger_pairs, dim3\(static_cast<uint32_t>\(blocks < (\d+) \? blocks : (\d+)\)\), dim3\((\d+)\)", kern)
    assert [int(g) for g in launch.groups()] == [tc.PAIRS_BLOCKS, tc.PAIRS_BLOCKS, tc.PAIRS_THREADS]
    assert "const uint64_t blocks = (n_slots + 255) / 256;" in kern and tc.SLOT_TRIP == 524288
    assert "dim3((n_triggers + 255u) / 256u, (n_triggers + kGhostTileJ - 1u) / kGhostTileJ), dim3(256)" in kern and tc.GHOST_TILE_I == 256
    assert "std::min<uint32_t>(blocks_for(q.n_boxes, 4), 2048u)" in bp and tc.QUERY_WAVES == 8192 and tc.MANY_BOXES > tc.QUERY_WAVES
    assert kern.count("if (at < cap) out[at]") == 2 and bp.count("if (at < cap) out[at]") == 1                    # the guarded stores of the hit list
    assert "if (at < d.delta_cap) d.deltas[at] = record;" in kern and "const uint32_t n = hits < d.pair_cap ? hits : d.pair_cap;" in kern


def test_the_fed_margin():
    ghost1, body_half, ghost_half = tc.fed_half_widths()
    assert max(abs(ghost1 - 1.0 - tc.FED_MARGIN), abs(body_half - 0.5 - tc.FED_MARGIN), abs(ghost_half - 0.5 - tc.FED_MARGIN)) < 1e-6


def test_the_table_rule():
    assert tc.table_log2(0, 0) == 12 and tc.table_log2(1024, 0) == 12 and tc.table_log2(1025, 0) == 13
    assert tc.table_log2(300, 2100) == 14 and tc.table_log2(10, 0, before=19) == 19
    assert tc.table_log2(70000, 70000) == 19 and tc.table_log2(tc.PAIR_CAP, tc.PAIR_CAP) == 22


# ------------------------------------------------------------------------------------------------------------------ every case holds its class


@pytest.mark.parametrize("builder", EVERY, ids=ids(EVERY))
def test_the_case_holds_its_claims_on_the_oracle(builder):
    """The claimed Enter + Exit count of every tick that states one, exactly; the sub-steps; and the route of every tick, from the
    oracle's numbers by the state machine's rules."""
    case, events, active, steps = tc.expected(builder)
    raw = tc.run_oracle(builder)[1]
    deltas = [_counts(ev)[1] for ev in events]
    for tick, t in enumerate(case.ticks):
        if t.deltas is not None:
            assert deltas[tick] == t.deltas, f"{case.name} tick {tick}: {deltas[tick]} Enter + Exit, the case claims {t.deltas}"
        assert steps[tick] == (0 if t.route == "-" else 1), (case.name, tick, steps)
    overlaps = [_counts(ev)[0] for ev in raw]
    assert tc.predict_routes(case, overlaps, deltas) == case.routes, (case.name, overlaps, deltas)
    assert case.routes[0] in "hE" and len(case.trig.entity) > 0
    if getattr(case, "overlaps", None):
        assert overlaps == case.overlaps                                             # the pair buffer cases: exactly 2^20 and 2^20 + 1


def test_family_a_sits_on_both_sides_of_every_edge_and_shows_every_event_type():
    per = {tc.case_name(b): tc.expected(b) for b in tc.FAMILY_A}
    for name, (case, events, _, _) in per.items():
        seen = set(np.concatenate(events)[:, 0].tolist())
        assert seen == {0, 1, 2}, (name, seen)
        assert case.routes.count("d") >= 2, name                                       # really on the device path
    deltas = lambda name: [_counts(ev)[1] for ev in per[name][1]]
    d = deltas("first_copy_edge")
    assert d[1:4] == [tc.FIRST_COPY, tc.FIRST_COPY + 1, tc.FIRST_COPY] and per["first_copy_edge"][0].routes == "hdddd"
    # tick 2: sorted by key the records are ghost 0's and 1's Exits, then ghost 3's Enters — the first and the last differ in trigger
    ev = per["first_copy_edge"][1][2]
    ev = ev[ev[:, 0] != tc.STAY]
    trig = np.sort(ev[:, 1])
    assert trig[0] != trig[-1] and trig[tc.FIRST_COPY] != trig[0] and len(np.unique(trig)) == 3
    assert deltas("delta_cap_edge")[1:3] == [tc.DELTA_CAP, tc.DELTA_CAP + 1] and per["delta_cap_edge"][0].routes == "hdhd"
    case, events, _, _ = per["load_factor"]
    hits = [_counts(ev)[0] for ev in events]
    assert hits == [tc.LOAD_FEW, tc.LOAD_FEW + 1, tc.LOAD_MANY, tc.LOAD_FEW + 1, tc.LOAD_MANY] and case.routes == "hdhdd"
    small = 1 << tc.table_log2(tc.LOAD_FEW, tc.LOAD_FEW)
    assert tc.LOAD_MANY > 4 * tc.LOAD_FEW and tc.LOAD_MANY > 2048 and 2 * tc.LOAD_MANY > small                   # the jump leaves the small table
    assert 2 * tc.LOAD_MANY <= 1 << tc.table_log2(tc.LOAD_MANY, tc.LOAD_MANY, 12) and max(deltas("load_factor")) <= tc.DELTA_CAP
    case, events, _, _ = per["met_both_ways"]
    both = np.concatenate(events)
    t_rows = both[(both[:, 1] == 1) & (both[:, 2] == 0)]
    assert t_rows[:, 0].tolist().count(tc.ENTER) == 1 and t_rows[:, 0].tolist().count(tc.EXIT) == 1 and len(t_rows) == 5 - 1
    assert case.routes == "hdddd"


def test_the_reupload_shifts_indices_and_the_new_topology_moves_the_ghosts():
    case, events, active, _ = tc.expected(tc.reupload)
    before, after = case.trig, case.trig_at(2)
    index = lambda trig: {int(e): k for k, e in enumerate(trig.entity.tolist())}
    ib, ia = index(before), index(after)
    survivors = sorted(set(ib) & set(ia))
    shifts = {e: ia[e] - ib[e] for e in survivors}
    assert len(survivors) == 4 and min(shifts.values()) < 0 < max(shifts.values()) and 0 in shifts.values(), shifts
    assert len(set(ib) - set(ia)) == 1 and len(set(ia) - set(ib)) == 2
    changed = [e for e in survivors if before.mask[ib[e]] != after.mask[ia[e]]]
    assert len(changed) == 1
    ev = events[2]
    kinds = {e: set(ev[ev[:, 1] == e][:, 0].tolist()) for e in ia}
    for e in ia:                                     # survivors remember (Stay), the new ones and the one whose mask changed start over (Enter)
        fresh = e not in ib or e in changed
        assert (tc.ENTER in kinds[e]) == fresh and (tc.STAY in kinds[e]) == (not fresh), (e, kinds[e])
    assert not (ev[:, 1] == list(set(ib) - set(ia))[0]).any()

    case, events, _, _ = tc.expected(tc.new_topology)
    topo = [ed for ed in case.ticks[2].edits if ed[0] == "topology"][0]
    assert acyclic(case.parent) and acyclic(topo[1])
    slot0 = W.flatten_topology(case.parent, case.has_transform)[0]
    slot1 = W.flatten_topology(topo[1], topo[2])[0]
    ghosts = case.trig.entity.astype(np.int64)
    moved = slot0[ghosts] != slot1[ghosts]
    assert (slot0[ghosts] != ghosts).any() and moved.sum() >= 3, (slot0[ghosts], slot1[ghosts])   # slots differ from entities, and they move
    assert topo[2][case.frozen] == 0 and case.has_transform[case.frozen] == 1
    # the frozen ghost goes on reporting from where it was: an Exit in the tick of the change, an Enter a tick later
    assert (int(tc.EXIT), case.frozen, 20) in {tuple(r) for r in events[2].tolist()}
    assert (int(tc.ENTER), case.frozen, 0) in {tuple(r) for r in events[3].tolist()}


def test_the_call_that_simulates_nothing_reports_stay_and_drops_the_deactivated_volume():
    case, events, active, steps = tc.expected(tc.nothing_simulated)
    assert steps == [1, 1, 0, 1, 1] and case.routes == "hd-hd"
    off = int(case.trig.entity[1])
    assert set(events[2][:, 0].tolist()) == {tc.STAY} and not (events[2][:, 1] == off).any() and (events[1][:, 1] == off).any()
    assert active[2].tolist() == [True, False, True]
    assert (int(tc.STAY), int(case.trig.entity[2]), 20) in {tuple(r) for r in events[2].tolist()}       # body 20 has left; nobody looked


def test_the_slot_trip_case_hits_the_first_64_slots_and_the_last_300():
    case, events, _, _ = tc.expected(tc.second_slot_trip)
    n = case.n
    assert n == tc.SLOT_TRIP + tc.SLOT_TAIL and -(-n // tc.SLOT_TRIP) == 2 and len(case.trig.entity) <= tc.GRID_MIN
    slot = W.flatten_topology(case.parent, case.has_transform)[0]
    assert np.array_equal(slot, np.arange(n))                                        # roots in entity order: slot = entity
    wide = int(case.trig.entity[0])
    met = np.sort(events[0][events[0][:, 1] == wide][:, 2])
    want = np.setdiff1d(case.near, [wide])
    assert np.array_equal(met, want) and (want < tc.SLOT_HEAD).sum() == tc.SLOT_HEAD and (want >= tc.SLOT_TRIP).sum() == tc.SLOT_TAIL - 1
    others = np.unique(events[0][:, 2])
    assert np.isin(others, case.near).all()
    gone = events[1][events[1][:, 0] == tc.EXIT][:, 2]
    assert (gone < tc.SLOT_HEAD).any() and (gone >= tc.SLOT_TRIP).any()               # the teleport takes bodies of both trips out


@pytest.mark.parametrize("hits", tc.WAVE_HITS)
def test_the_wave_cases_hit_what_they_say(hits):
    case, events, _, _ = tc.expected(tc.FAMILY_C[1 + tc.WAVE_HITS.index(hits)])
    assert np.array_equal(np.sort(events[0][:, 2]), np.arange(hits)) and (events[0][:, 0] == tc.ENTER).all()
    assert (np.arange(hits) < 64).sum() == min(hits, 64)


def test_nobody_lists_itself():
    case, events, _, _ = tc.expected(tc.self_exclusion)
    ev = np.concatenate(events)
    assert not (ev[:, 1] == ev[:, 2]).any()
    assert _pairs(events[0]) == {(a, b) for a in range(3) for b in range(4) if a != b}


@pytest.mark.parametrize("builder", tc.FAMILY_D[:8], ids=ids(tc.FAMILY_D[:8]))
def test_the_lattice_cases_reach_what_they_are_for(builder):
    case, events, _, _ = tc.expected(builder)
    nb, L = case.n_bodies, case.n_large
    classes = len({(int(a), int(b)) for a, b in zip(case.layer[:nb], case.mask[:nb])})
    assert classes == 9 or classes > 255, classes                                    # compact records, or the palette overflows: full records
    ev = events[0]
    ghosts = case.trig.entity.astype(np.int64)
    c, h = tc.ghost_shapes(tc.LATTICE)
    met = {int(g): ev[(ev[:, 1] == g) & (ev[:, 2] < nb)][:, 2].astype(np.int64) for g in ghosts}
    lattice = nb - L
    # the ghosts outside the bounds meet nothing; the one beyond the lattice meets large bodies only, and all that pass its filter
    outside = [k for k in range(len(c)) if c[k][0] == -40.0 or c[k][1] > 60.0]
    assert len(outside) == 2 and all(len(met[int(ghosts[k])]) == 0 for k in outside)
    beyond = [k for k in range(len(c)) if c[k][2] == 43.0]
    assert len(beyond) == 1 and (met[int(ghosts[beyond[0]])] >= lattice).all()
    if L:
        g = int(ghosts[beyond[0]])
        k = beyond[0]
        passes = ((case.trig.layer[k] or 4) & case.mask[lattice:nb]) != 0
        passes &= (case.layer[lattice:nb] & case.trig.mask[k]) != 0
        assert np.array_equal(np.sort(met[g]), lattice + np.flatnonzero(passes)) and (passes.sum() > 0 or L == 1)
    large_hits = sum(int((m >= lattice).sum()) for m in met.values())
    assert (large_hits > 0) == (L > 0) or L == 1
    # the grid the device builds, by decide_grid's rule: the body's width without large bodies, one growth step of 1.25 with them (the
    # bounds then reach to z = 46) — and the table is not within 3 % of either decision
    grid = tc.grid_of(case, lattice)
    cell, origin, dims, table = grid
    assert abs(cell / 0.94 - (1.25 if L else 1.0)) < 1e-3 and dims.prod() < 0.97 * table, (cell, dims, table)
    if L:
        assert (np.floor(dims - 4) * 1.25 + 4).prod() > 1.03 * table
    lo_g, hi_g = c - (h + tc.FED_MARGIN), c + (h + tc.FED_MARGIN)
    first, count = tc.cells_of(grid, lo_g, hi_g)
    assert (count.prod(1) < tc.QUERY_MAX_CELLS // 8).all()                             # every ghost far from the 8 192 boundary
    # straddling bodies: a body a ghost meets whose min corner lies in the cell BELOW the one the ghost's min corner is in — found
    # only by the `- 1` of box_cells — on every axis
    body_first = tc.cells_of(grid, case.pos[:nb] - (case.size[:nb] + tc.FED_MARGIN), case.pos[:nb])[0] + 1     # (cells_of steps one down)
    ghost_first = first + 1
    straddle = np.zeros(3, np.int64)
    for k, g in enumerate(ghosts.tolist()):
        m = met[g][met[g] < lattice]
        straddle += (body_first[m] < ghost_first[k]).sum(0)
    assert (straddle >= 20).all(), straddle
    # rows = n[1] * n[2]: the cross-section ghosts lie on both sides of 64, a second trip of the row loop
    rows = count[2:9, 1] * count[2:9, 2]
    assert rows.min() < 64 < rows.max() and (rows > 64).sum() >= 2 and (rows <= 64).sum() >= 2, rows
    # the clamps: ghosts that reach below cell 1 and beyond the last cell that holds bodies, on every axis
    assert ((lo_g < origin).any(0)).all() and ((hi_g > origin + cell * (dims - 3)).any(0)).all()
    assert L in tc.LARGE_COUNTS and case.query[0] == (len(ghosts), 0)


def test_the_grid_edges_are_met():
    assert len(tc.expected(tc.FAMILY_D[8])[0].trig.entity) == tc.GRID_MIN and len(tc.expected(tc.FAMILY_D[9])[0].trig.entity) == tc.GRID_MIN + 1
    case, events, _, _ = tc.expected(tc.many_boxes)
    assert len(case.trig.entity) > tc.QUERY_WAVES and len(np.unique(events[0][:, 1])) > 4000
    case, events, _, _ = tc.expected(tc.cell_sweep)
    big = int(case.trig.entity[0])
    n_met = [int(((ev[:, 1] == big) & (ev[:, 0] != tc.EXIT)).sum()) for ev in events]
    assert n_met[0] < 200 and n_met[-1] > 0.5 * tc.LATTICE ** 3 * 0.6 and all(a <= b for a, b in zip(n_met, n_met[1:])), n_met
    sizes = [case.trig_at(k).size[0, 0] for k in range(len(case.ticks))]
    # in cells of the body's width: a few hundred at first; at the end the whole lattice, several times 8 192 were the grid not clamped
    assert (2 * sizes[0] / 0.94 + 2) ** 3 < tc.QUERY_MAX_CELLS / 8 and (2 * sizes[-1] / 1.47) ** 3 > 2 * tc.QUERY_MAX_CELLS / 3
    assert min(2 * sizes[-1], tc.LATTICE) ** 3 / 1.47 ** 3 < 3 * tc.QUERY_MAX_CELLS          # (why the exact step of the switch is the device's to say)


@pytest.mark.parametrize("builder", tc.FAMILY_E, ids=ids(tc.FAMILY_E))
def test_the_ghost_cases_pair_both_ways_and_about_half_pass(builder):
    case, events, active, _ = tc.expected(builder)
    n = len(case.trig.entity)
    assert n in tc.GHOST_COUNTS
    first = _pairs(events[0])
    assert all((b, a) in first for a, b in first)                                     # the filter is symmetric: both directions
    live = int(case.trig.active.sum())
    if n >= 63:
        assert 0.4 < len(first) / (live * (live - 1)) < 0.7, len(first) / (live * (live - 1))
        off = set(np.flatnonzero(case.trig.active == 0).tolist())
        assert len(off) >= 8 and not any(a in off or b in off for a, b in first)
    if n >= 2:
        assert (0, 1) in first and (1, 0) in first
        assert any(a == 1 for a, b in _pairs(events[2])) == (n > 2)                   # the frozen ghost goes on reporting whom it still meets
        assert set(np.concatenate(events)[:, 0].tolist()) == {0, 1, 2} or n == 2
    assert case.routes == "hdd"


@pytest.mark.parametrize("builder", tc.FAMILY_F, ids=ids(tc.FAMILY_F))
def test_the_touching_rows_hold_both_outcomes_with_the_switch_strictly_inside(builder):
    case, events, _, _ = tc.expected(builder)
    met = _pairs(events[0])
    reported = np.array([(int(p), int(q)) in met for p, q in zip(case.first, case.partner)])
    rows = [slice(r * tc.TOUCH_ROW, (r + 1) * tc.TOUCH_ROW) for r in range(4)]
    for row in rows:
        k = int(reported[row].sum())
        assert reported[row][:k].all() and not reported[row][k:].any(), reported[row]     # one switch
        assert tc.TOUCH_MID - 2 <= k <= tc.TOUCH_MID + 2, k                                # ... strictly inside, next to the exact touch
    # on the oracle's own boxes: the gap between the two faces that decide is <= 0 exactly where the pair is reported, and in every row
    # one pair touches EXACTLY (gap == 0) — beyond the high face in two rows, below the low face in the other two, so `<` for `<=` in
    # either comparison of the axis loses a pair
    ref = tc.build_oracle(case)
    ref.PhysicsSystemUpdate(W.FIXED_DT)
    fed = ref.bulk_bodies()["aabb"]
    box = lambda e: ref.TriggerBox(int(e) + 1) if case.body_type[e] == W.BODY_NONE else fed[e]
    ax = case.axis
    gap = np.array([box(q)[ax] - box(p)[3 + ax] if case.side[j] > 0 else box(p)[ax] - box(q)[3 + ax]
                    for j, (p, q) in enumerate(zip(case.first, case.partner))], np.float32)
    ref.close()
    assert np.array_equal(gap <= 0, reported)
    for row in rows:
        assert (gap[row] == 0).sum() == 1 and (np.diff(gap[row]) > 0).all(), gap[row][95:106]
    assert (case.side[rows[0]] > 0).all() and (case.side[rows[3]] < 0).all() and case.is_body[rows[0]].all() and not case.is_body[rows[3]].any()
    both_ways = {(b, a) for a, b in met if a in set(case.partner[~case.is_body].tolist()) or b in set(case.partner[~case.is_body].tolist())}
    assert both_ways <= met and len(both_ways) > 0                                        # a ghost pair reports both ways
    assert np.array_equal(events[1][:, 1:], events[0][:, 1:]) and (events[1][:, 0] == tc.STAY).all()


# ------------------------------------------------------------------------------------------------------------------ the numpy ProcessTriggerEvents


NEVER_FAIL = [b for b in EVERY if b is not tc.pair_buffer_overflow]      # (the oracle cannot fail a tick: that script is what the model is for)


@pytest.mark.parametrize("builder", NEVER_FAIL, ids=ids(NEVER_FAIL))
def test_the_numpy_model_equals_the_oracle(builder):
    """Fed the current sets the oracle's Enter and Stay rows state, the model reports the oracle's events: it remembers, forgets on a
    re-upload and on (de)activation, and orders like it."""
    case, events, active, _ = tc.run_oracle(builder)
    assert "E" not in case.routes
    got = tc.model_events(case, events)
    for tick, (g, want) in enumerate(zip(got, events)):
        assert np.array_equal(g, want), f"{case.name} tick {tick}: {len(g)} events, the oracle {len(want)}"


def test_the_model_walks_uploaded_order_ascending_entities_enter_stay_then_exit():
    m = te.TriggerModel()
    m.upload([7, 3])                                                                  # uploaded order, not entity order
    assert m.process({7: ([5, 2], []), 3: ([9], [7])}).tolist() == [[0, 7, 2], [0, 7, 5], [0, 3, 7], [0, 3, 9]]
    assert m.process({7: ([5, 1], []), 3: ([], [])}).tolist() == [[0, 7, 1], [1, 7, 5], [2, 7, 2], [2, 3, 7], [2, 3, 9]]
    assert m.skip_tick().shape == (0, 3)
    assert m.process({7: ([5], []), 3: ([4], [])}).tolist() == [[1, 7, 5], [2, 7, 1], [0, 3, 4]]   # diffed against the sets before the failure


def test_the_model_rejects_three_wrong_answers():
    # a ghost listing itself
    m = te.TriggerModel()
    m.upload([1, 2])
    assert m.process({1: ([1, 4], [1, 2]), 2: ([], [2, 1])}).tolist() == [[0, 1, 2], [0, 1, 4], [0, 2, 1]]
    # an entity met both ways counted twice
    m = te.TriggerModel()
    m.upload([1, 2])
    assert m.process({1: ([2], [2]), 2: ([], [])}).tolist() == [[0, 1, 2]]
    assert m.process({1: ([], [2]), 2: ([], [])}).tolist() == [[1, 1, 2]]            # the body key goes: no Exit
    assert m.process({1: ([], []), 2: ([], [])}).tolist() == [[2, 1, 2]]
    # a fired one-shot still listed by a later trigger
    m = te.TriggerModel()
    m.upload([1, 2, 3], one_shot=[0, 1, 0])
    ev = m.process({1: ([], [2]), 2: ([], [1, 3]), 3: ([], [2])})
    assert ev.tolist() == [[0, 1, 2], [0, 2, 1], [0, 2, 3]]                          # 1 listed it before it fired; 3, walked after, does not
    assert m.active([1, 2, 3]).tolist() == [True, False, True]
    assert m.process({1: ([], [2]), 2: ([], [1]), 3: ([], [])}).tolist() == [[2, 1, 2]]   # gone from 1's list a tick later, without events of its own


def test_the_failed_ticks_of_the_overflow_script_report_nothing_and_the_next_tick_starts_from_the_sets_before():
    case, events, _, _ = tc.expected(tc.pair_buffer_overflow)
    raw = tc.run_oracle(tc.pair_buffer_overflow)[1]
    assert case.routes == "EhhdEhd" and len(events[0]) == 0 and len(events[4]) == 0
    assert _counts(raw[0])[0] == tc.PAIR_CAP + 1 == _counts(raw[4])[0] and _counts(raw[1])[0] == tc.PAIR_CAP
    assert (events[1][:, 0] == tc.ENTER).all() and len(events[1]) == tc.PAIR_CAP        # the first successful tick: everybody enters
    g1 = int(case.trig.entity[1])
    rows = events[5][events[5][:, 1] == g1]
    by = lambda k: rows[rows[:, 0] == k][:, 2].tolist()
    assert by(tc.ENTER) == list(range(20, 41)) and by(tc.STAY) == list(range(10, 20)) and by(tc.EXIT) == list(range(10))
    # the oracle, which did not fail, says something else there: the model is not the oracle in disguise
    assert not np.array_equal(events[5], raw[5])
    assert _counts(events[6]) == (16 * 31, 160) and np.array_equal(events[6], raw[6])     # one tick on, both agree again
