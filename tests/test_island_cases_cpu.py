"""The coverage claim of test_gpu_island_paths.py, checked without a GPU: every scene of refmodel/island_cases.py is stepped through
the ORACLE for the GPU test's tick count and classified after every compared tick (from DynamicPairs, GroundContacts and BoxContacts) exactly as
k_island_solve routes its islands.  A class or regime counts as covered by a scene only if the scene's islands are in it at half of
the compared ticks at least, and then at least 2 points and 1 body away from a value that is routed differently — except the
deliberate body-count boundaries 4|5 and 16|17 (static: a stack keeps its bodies), and P == 0, which is a point.  And the
classifier itself on hand-made pair headers, one island per class, both sides of every <=."""
import numpy as np
import pytest

from helpers import DT, build_island_oracle
from refmodel import island_cases as ic
from refmodel.island_cases import BIG, GLOBAL, MID, SMALL


def _history(case, basis=False):
    """[(tick, {group: island dict}, pair header, (plane counts, obstacle manifold counts))] of the compared ticks; every group must be
    ONE island, alone in it."""
    ref = build_island_oracle(case, basis)
    out = []
    for tick in range(case.ticks):
        ref.PhysicsSystemUpdate(DT)
        ref.TransformSystemUpdate()
        if tick < case.compare_from:
            continue
        islands, hdr, plane, manifolds = ic.classify_oracle(ref, case)
        by_low = {int(i["bodies"][0]): i for i in islands}
        got = {}
        for name, members in case.groups.items():
            isl = by_low.get(int(members.min()))
            assert isl is not None and np.array_equal(isl["bodies"], np.sort(members)), f"{case.name} tick {tick}: {name} is not one island of its own"
            got[name] = isl
        assert len(islands) == len(case.groups), f"{case.name} tick {tick}: islands nobody asked for"
        st, _ = ref.bulk_activation()
        assert (st[case.dyn] == 1).all(), f"{case.name} tick {tick}: a body is not ACTIVE_TAG (a sleeping island is not routed at all)"
        out.append((tick, got, hdr, (plane, manifolds)))
    return out


def _covered(history, group, cls, flags=None, point_slack=2, body_slack=1):
    """The number of compared ticks at which the group's island is in the class (and regime), far enough from another one."""
    hits = 0
    for _, got, _, _ in history:
        isl = got[group]
        if isl["cls"] != cls or (flags is not None and any(isl["flags"][k] != v for k, v in flags.items())):
            continue
        if isl["point_slack"] >= point_slack and isl["body_slack"] >= body_slack:
            hits += 1
    return hits


def _assert_covered(history, group, cls, **kw):
    hits = _covered(history, group, cls, **kw)
    seen = [(t, g[group]["cls"], g[group]["nb"], g[group]["P"]) for t, g, _, _ in history]
    assert 2 * hits >= len(history), f"{group}: {cls} {kw} at {hits} of {len(history)} compared ticks: {seen}"


# ------------------------------------------------------------------------------------------------------------------ the classifier


def _hdr(chains):
    """A pair header of chains of bodies: [(first entity, bodies, points per link)]."""
    rows = []
    for first, count, points in chains:
        rows += [(first + k, first + k + 1, points) for k in range(count - 1)]
    return np.array(sorted(rows), np.int64).reshape(-1, 3)


@pytest.mark.parametrize("nb,P,big,want", [
    (4, 16, 128, SMALL), (4, 17, 128, MID), (5, 16, 128, MID), (5, 0, 128, MID),           # both sides of nb <= 4 and of P <= 16
    (16, 128, 128, MID), (17, 128, 128, GLOBAL), (16, 129, 128, BIG), (17, 129, 128, BIG),   # nb <= 16, P <= big_points
    (128, 100, 128, GLOBAL), (129, 100, 128, BIG),                                           # nb <= big_points
    (4, 16, 0, SMALL), (4, 17, 0, BIG), (5, 0, 0, BIG), (3, 17, 16, BIG), (2, 0, 0, SMALL),   # big_points below the LDS solver's limits
    (17, 16, 16, BIG), (16, 16, 16, MID), (16, 17, 16, BIG),
])
def test_route_decides_like_k_island_solve_on_both_sides_of_every_threshold(nb, P, big, want):
    assert ic.route(nb, P, big)[0] == want


def test_the_workgroup_solvers_regimes_on_both_sides_of_every_threshold():
    f = lambda nb, P: ic.route(nb, P, 0)[1]
    assert f(8, 0) == dict(p0=True, walk_in_lds=False, last_in_lds=False, bodies_in_lds=False)
    assert f(8, 1)["p0"] is False
    # 12 P + 4 nb <= 147 456
    assert f(3072, 11264)["walk_in_lds"] and not f(3072, 11265)["walk_in_lds"] and not f(3075, 11264)["walk_in_lds"]
    assert f(3072, 5)["bodies_in_lds"] and not f(3073, 5)["bodies_in_lds"]
    assert f(36864, 5)["last_in_lds"] and not f(36865, 5)["last_in_lds"]
    assert ic.BIG_LAST_LDS == 36864 and ic.BIG_LDS_BODIES == 3072
    # isl_wg_scan: one element a thread up to depth + 2 == 256
    assert ic.scan_chunk(254) == 1 and ic.scan_chunk(255) == 2


def test_classify_unites_by_pairs_and_counts_every_kind_of_point():
    """One island per class in one header (big_points = 128), entities interleaved so that the union-find has to work: a pair without
    points unites like any other, a body in no pair is in no island, the plane's and the obstacles' points count."""
    n = 400
    chains = [(0, 4, 4), (10, 4, 4), (20, 9, 3), (40, 20, 2), (100, 30, 5), (200, 150, 0)]
    hdr = _hdr(chains)
    hdr = hdr[np.random.default_rng(3).permutation(len(hdr))]     # (the order of the header does not matter)
    plane = np.zeros(n, np.int64)
    box = np.zeros(n, np.int64)
    plane[0:4] = 1                 # 12 + 4 = 16 points on 4 bodies: small
    plane[10:14] = 1
    box[13] = 1                    # 12 + 4 + 1 = 17 points on 4 bodies: mid
    plane[399] = 4                 # in no pair
    got = {int(i["bodies"][0]): i for i in ic.classify(n, hdr, plane, box, 128)}
    assert sorted(got) == [0, 10, 20, 40, 100, 200]
    assert [(got[k]["nb"], got[k]["P"], got[k]["cls"]) for k in sorted(got)] == [
        (4, 16, SMALL), (4, 17, MID), (9, 24, MID), (20, 38, GLOBAL), (30, 145, BIG), (150, 0, BIG)]
    assert got[200]["flags"]["p0"] and got[100]["flags"] == dict(p0=False, walk_in_lds=True, last_in_lds=True, bodies_in_lds=True)
    assert got[0]["point_slack"] == 0 and got[0]["body_slack"] == 0 and got[10]["point_slack"] == 0
    assert got[40]["body_slack"] == 3 and got[100]["point_slack"] == 145 - 129
    # two chains joined by one point-less pair are one island
    joined = np.concatenate([_hdr(chains[:2]), [[3, 10, 0]]])
    one = ic.classify(n, joined, plane, box, 128)
    assert len(one) == 1 and one[0]["nb"] == 8 and one[0]["P"] == 33 and one[0]["cls"] == MID


def test_level_depth_follows_the_rule_in_the_solvers_row_order():
    # bodies 5, 7, 9: 5 has two plane points and a 3-point pair with 9; 7 a 1-point pair with 9; 9 one plane point
    hdr = np.array([[5, 9, 3], [7, 9, 1]], np.int64)
    plane = np.zeros(10, np.int64)
    plane[5], plane[9] = 2, 1
    rows = ic.island_rows([5, 7, 9], hdr, plane, None)
    assert rows.tolist() == [[0, -1], [0, -1], [0, 2], [0, 2], [0, 2], [1, 2], [2, -1]]
    assert ic.level_depth(rows) == 7                                  # every row shares a body with the one before it
    assert ic.level_depth([[0, -1], [1, -1], [2, -1]]) == 1           # ... and these share none
    assert ic.level_depth([[0, 1], [2, 3], [1, 2], [0, -1]]) == 2
    assert ic.level_depth(np.zeros((0, 2), np.int64)) == 0


# ------------------------------------------------------------------------------------------------------------------ the scenes


@pytest.mark.parametrize("basis", [False, True], ids=["default", "bullet_basis"])
@pytest.mark.parametrize("embedded", [False, True], ids=["flat", "embedded"])
def test_boundaries_hold_small_mid_and_global_islands_on_both_sides_of_the_body_limits(embedded, basis):
    case = ic.boundaries_embedded() if embedded else ic.boundaries()
    h = _history(case, basis)
    _assert_covered(h, "stack3", SMALL)                                         # the LDS column solver, clear of its limits
    _assert_covered(h, "stack4", SMALL, point_slack=0, body_slack=0)            # 4|5; 4 bodies cannot hold more than 16 points
    assert max(g["stack4"]["P"] for _, g, _, _ in h) >= 15                      # ... and it gets there
    _assert_covered(h, "stack5", MID)                                           # 4|5 (one body fewer on 19 points would still be mid)
    _assert_covered(h, "row4", MID)                                             # at most 4 bodies, more than 16 points
    assert all(g["row4"]["nb"] == 4 for _, g, _, _ in h)
    # (row3 is NOT a covered case: at the spacing of 0.99 it settles on 17 .. 18 points, one or two above the LDS column's 16 — a
    #  second look at the class row4 covers, run on the device all the same)
    assert all(g["row3"]["nb"] == 3 and g["row3"]["cls"] == MID for _, g, _, _ in h[len(h) // 2:])
    _assert_covered(h, "stack16", MID, body_slack=0)                            # 16|17
    _assert_covered(h, "stack17", GLOBAL, body_slack=0)
    _assert_covered(h, "stack20", GLOBAL)
    assert all(g["stack20"]["P"] <= 126 and g["stack17"]["P"] <= 126 for _, g, _, _ in h)
    if embedded:
        from refmodel.layout_cases import layout_numbers
        nums, own = layout_numbers(case.wl.parent, case.has_transform, case.n_own)
        print(nums)
        assert nums["off"] >= 0.9 * case.n_own
        # an island's root is its lowest SLOT: for these islands that is not their lowest entity, and the islands' order differs
        low_slot_is_low_entity = [int(np.argmin(own[m])) == 0 for m in case.groups.values()]
        assert not all(low_slot_is_low_entity)
        roots = [int(own[m].min()) for m in case.groups.values()]
        assert roots != sorted(roots)


@pytest.mark.parametrize("basis", [False, True], ids=["default", "bullet_basis"])
def test_obstacle_points_count_as_the_plane_s_do(basis):
    """Three boxes on a Static slab, plane off: GroundContacts is empty, BoxContacts holds the 12 points that make the island mid."""
    case = ic.on_a_slab()
    assert case.static and not case.plane
    h = _history(case, basis)
    _assert_covered(h, "row3", MID)
    for _, got, hdr, (plane, manifolds) in h[len(h) // 2:]:
        assert not plane.any() and [manifolds[e] for e in (1, 2, 3)] == [(4,)] * 3 and manifolds[0] == ()
        assert got["row3"]["P"] == 12 + int(hdr[:, 2].sum()) and int(hdr[:, 2].sum()) <= 8     # without the slab's points: small
        rows = ic.island_rows(got["row3"]["bodies"], hdr, plane, manifolds)
        assert len(rows) == got["row3"]["P"] and rows[:4].tolist() == [[0, -1]] * 4


def test_rows_of_four_are_more_mid_islands_than_a_launch_sized_by_five_bodies_an_island_has_threads():
    case = ic.rows_of_four()
    h = _history(case)
    assert len(h) == 5
    for name in case.groups:
        _assert_covered(h, name, MID)
    n_bodies = case.n
    assert len(case.groups) == ic.N_MANY > ((n_bodies // (ic.LDS_BODIES + 1) + 64) // 64) * 64     # the launch this scene was written against


@pytest.mark.parametrize("big_points", [128, 0])
def test_stacks_of_five_are_a_mid_list_of_several_blocks_or_more_big_islands_than_workgroups(big_points):
    case = ic.stacks_of_five(big_points)
    h = _history(case)
    for name in case.groups:
        if big_points:
            _assert_covered(h, name, MID)
        else:
            _assert_covered(h, name, BIG, flags=dict(p0=False, walk_in_lds=True, last_in_lds=True, bodies_in_lds=True))
    assert len(case.groups) > 4 * 64 and len(case.groups) > ic.BIG_WORKGROUPS


def test_free_fall_is_one_big_island_without_a_point():
    case = ic.free_fall()
    h = _history(case)
    assert len(h) == case.ticks
    for _, got, hdr, _ in h:
        assert len(hdr) >= len(case.groups["line"]) - 1 and not hdr[:, 2].any()      # the pairs exist and hold no points
        assert got["line"]["cls"] == BIG and got["line"]["flags"]["p0"] and got["line"]["body_slack"] >= 1


def test_the_deep_row_has_more_levels_than_the_scan_has_threads():
    case = ic.deep_row()
    h = _history(case)
    _assert_covered(h, "row", BIG, flags=dict(p0=False, walk_in_lds=True, last_in_lds=True, bodies_in_lds=True))
    assert case.big_points == ic.PRODUCT_BIG_POINTS
    for tick, got, hdr, own in h:
        depth = ic.level_depth(ic.island_rows(got["row"]["bodies"], hdr, *own))
        assert depth >= 255 and ic.scan_chunk(depth) > 1, (tick, depth)


_BEYOND_FLAGS = {
    "carpet45": dict(p0=False, walk_in_lds=False, last_in_lds=True, bodies_in_lds=True),
    "carpet56": dict(p0=False, walk_in_lds=False, last_in_lds=True, bodies_in_lds=False),
    "sparse-line": dict(p0=False, walk_in_lds=True, last_in_lds=True, bodies_in_lds=False),
    "carpet193": dict(p0=False, walk_in_lds=False, last_in_lds=False, bodies_in_lds=False),
}


# (the runs of test_gpu_island_paths.py: carpet193 in the default scheme only — a second scheme would cost it more than a second)
@pytest.mark.parametrize("name,basis", [("carpet45", False), ("carpet45", True), ("carpet56", False), ("carpet56", True), ("sparse-line", False),
                                        ("sparse-line", True), ("carpet193", False)])
def test_the_workgroup_solver_beyond_its_lds(name, basis):
    flags = _BEYOND_FLAGS[name]
    case = ic.BEYOND_LDS[name]()
    h = _history(case, basis)
    group = next(iter(case.groups))
    _assert_covered(h, group, BIG, flags=flags)
    for tick, got, hdr, own in h[-1:]:
        isl = got[group]
        depth = ic.level_depth(ic.island_rows(isl["bodies"], hdr, *own))
        print(f"{name}: {isl['nb']} bodies, {isl['P']} points, {depth} levels")
        assert depth < isl["P"] // 64                                                   # shuffled indices keep the walk shallow
    if name == "sparse-line":
        assert all((hdr[:, 2] == 0).sum() >= len(hdr) // 2 - 1 for _, _, hdr, _ in h)  # every other link is AABB-only
