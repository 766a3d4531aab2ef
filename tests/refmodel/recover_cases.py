"""The hand-worked recoveries and their checker, the invalid records, and the seeded batch and caps of the GPU comparison:
shared by test_sphere_recover_cpu.py and test_gpu_sphere_recover.py."""
from __future__ import annotations

import collections
import math

import numpy as np

from banggameengine_amd.world import RECOVER_INVALID, RECOVER_MOVED, RECOVER_STUCK, SPHERE_RECOVER_RESULT_DTYPE, make_sphere_recovers

from .rays import ALL, NO_ENTITY, RAY_BODY, RAY_GROUND, RAY_MISS, RAY_TRIGGER, Obj, box_half_extents, capsule_dims, quat_from_euler, quat_to_mat
from .tolerances import N_ABS, N_SCALE, P_REL
from .recover import classify
from .move_cases import wall_box

UP, DOWN, WEST, EAST = (0.0, 1.0, 0.0), (0.0, -1.0, 0.0), (-1.0, 0.0, 0.0), (1.0, 0.0, 0.0)
PLANE = (UP, (0.0, 0.0, 0.0), RAY_GROUND, NO_ENTITY)
R, SKIN = 0.5, 0.01
S2 = math.sqrt(2.0)
TILT = (0.3, 0.5, math.pi / 2)  # the pose of the capsule whose axis the sphere is centred on
TILT_X = tuple(quat_to_mat(quat_from_euler(np.asarray(TILT)))[:, 0])  # its local +x in the world


def body(capsule, size, position, euler=(0.0, 0.0, 0.0), group=1, ghost=False):
    return (capsule, size, position, euler, group, ghost)


def cube(position, **kw):
    return body(False, (1.0, 1.0, 1.0), position, **kw)


# (name, half-spaces of the analytic function or None where they cannot say it, bodies of the shape reference and of the device
#  (body(...); body i of the list is entity i), plane, sphere (position, layer mask), expected fields).  Every sphere has radius
#  0.5 and skin 0.01.  Sizes of 1, 2, 3, 4, 8 and 0.5 keep the library's half extents at the sizes themselves.
HAND_RECOVERS = [
    # 0.3 above the plane: sd = 0.3, depth 0.2, t = 0.21: up to y = 0.51 = radius + skin, where the next query finds nothing
    ("over the plane", [PLANE], [], True, ((0, 0.3, 0), ALL),
     dict(position=(0, 0.51, 0), pushed=(0, 0.21, 0), flags=RECOVER_MOVED, n_pushes=1, hit_kind=RAY_GROUND, hit_entity=NO_ENTITY, hit_normal=UP,
          hit_depth=0.2)),
    # the same below it: the plane is two-sided, the centre goes further down
    ("under the plane", None, [], True, ((0, -0.3, 0), ALL),
     dict(position=(0, -0.51, 0), pushed=(0, -0.21, 0), flags=RECOVER_MOVED, n_pushes=1, hit_kind=RAY_GROUND, hit_entity=NO_ENTITY, hit_normal=DOWN,
          hit_depth=0.2)),
    # the centre inside the box (1, 2, 3), 0.2 from its +x face (1.9 and 2.8 from the others): sd = -0.2, depth 0.7, t = 0.71: one
    # push to x = 1.51 = h.x + radius + skin
    ("inside a box near its +x face", [(EAST, (1, 0, 0), RAY_BODY, 0)], [body(False, (1.0, 2.0, 3.0), (0, 5, 0))], False, ((0.8, 5.1, 0.2), ALL),
     dict(position=(1.51, 5.1, 0.2), pushed=(0.71, 0, 0), flags=RECOVER_MOVED, n_pushes=1, hit_kind=RAY_BODY, hit_entity=0, hit_normal=EAST,
          hit_depth=0.7)),
    # 0.5 from the -x, +y and +z faces of a cube alike: the lowest axis wins, x, with the sign of q.x: out to x = -1 - 0.51
    ("face tie inside a cube", None, [cube((0, 5, 0))], False, ((-0.5, 5.5, 0.5), ALL),
     dict(position=(-1.51, 5.5, 0.5), pushed=(-1.01, 0, 0), flags=RECOVER_MOVED, n_pushes=1, hit_kind=RAY_BODY, hit_entity=0, hit_normal=WEST,
          hit_depth=1.0)),
    # the centre of a tilted capsule (radius 0.5) is on its axis: a = 0, sd = -0.5, depth 1, out along the capsule's local +x by 1.01
    ("on a capsule's axis", None, [body(True, (0.5, 1.0, 0.5), (2, 5, -1), TILT)], False, ((2, 5, -1), ALL),
     dict(position=tuple(np.array([2.0, 5.0, -1.0]) + 1.01 * np.array(TILT_X)), pushed=tuple(1.01 * np.array(TILT_X)), flags=RECOVER_MOVED,
          n_pushes=1, hit_kind=RAY_BODY, hit_entity=0, hit_normal=TILT_X, hit_depth=1.0)),
    # the corner of the floor and the wall x = 2: the wall is deeper (sd 0.2, depth 0.3) than the floor (sd 0.3, depth 0.2): first out
    # of the wall to x = 1.8 - 0.31, then out of the floor to y = 0.3 + 0.21; the third query finds nothing
    ("floor and wall corner", [PLANE, (WEST, (2, 0, 0), RAY_BODY, 0)], [wall_box(WEST, (2, 1, 0)) + (1, False)], True, ((1.8, 0.3, 0), ALL),
     dict(position=(1.49, 0.51, 0), pushed=(-0.31, 0.21, 0), flags=RECOVER_MOVED, n_pushes=2, hit_kind=RAY_GROUND, hit_entity=NO_ENTITY, hit_normal=UP,
          hit_depth=0.2)),
    # a slot 0.8 wide between the faces x = -0.4 (cube 0) and x = 0.4 (cube 1): from x = 0.05 cube 1 is deeper (0.15 against 0.05):
    # to -0.11; there cube 0 reaches in by 0.21: to 0.11; then cube 1 by 0.21: to -0.11; then cube 0: to 0.11.  Four pushes, and
    # the check still finds cube 1 in by 0.21: STUCK
    ("slot narrower than the sphere", [(EAST, (-0.4, 0, 0), RAY_BODY, 0), (WEST, (0.4, 0, 0), RAY_BODY, 1)],
     [cube((-1.4, 5, 0)), cube((1.4, 5, 0))], False, ((0.05, 5, 0), ALL),
     dict(position=(0.11, 5, 0), pushed=(0.06, 0, 0), flags=RECOVER_MOVED | RECOVER_STUCK, n_pushes=4, hit_kind=RAY_BODY, hit_entity=0,
          hit_normal=EAST, hit_depth=0.21, remaining_depth=0.21)),
    # two cubes at the same place reach equally deep: the lower object code wins
    ("equal depth: lowest code", [(EAST, (1, 0, 0), RAY_BODY, 0), (EAST, (1, 0, 0), RAY_BODY, 1)], [cube((0, 5, 0)), cube((0, 5, 0))], False,
     ((1.2, 5, 0), ALL),
     dict(position=(1.51, 5, 0), pushed=(0.31, 0, 0), flags=RECOVER_MOVED, n_pushes=1, hit_kind=RAY_BODY, hit_entity=0, hit_normal=EAST, hit_depth=0.3)),
    # a trigger ghost on layer 4: a sphere that sees layer 4 is pushed out of it, one that sees layers 1 and 2 is left where it is
    ("ghost through its layer", [(EAST, (1, 0, 0), RAY_TRIGGER, 0)], [cube((0, 5, 0), group=4, ghost=True)], False, ((1.2, 5, 0), 4),
     dict(position=(1.51, 5, 0), pushed=(0.31, 0, 0), flags=RECOVER_MOVED, n_pushes=1, hit_kind=RAY_TRIGGER, hit_entity=0, hit_normal=EAST,
          hit_depth=0.3)),
    ("ghost on a layer not asked", [], [cube((0, 5, 0), group=4, ghost=True)], False, ((1.2, 5, 0), 3),
     dict(position=(1.2, 5, 0), pushed=(0, 0, 0), flags=0, n_pushes=0, hit_kind=RAY_MISS, hit_entity=NO_ENTITY, hit_normal=(0, 0, 0), hit_depth=0)),
    # a cube turned 45 degrees about y (the library's euler.x: quat_from_euler): its vertical edge at sqrt 2 on the x axis.  From
    # x = 1.8 the edge is 0.3858 away, depth 0.1142, and the way out is along x: to sqrt 2 + radius + skin
    ("rotated box", [(EAST, (S2, 0, 0), RAY_BODY, 0)], [cube((0, 5, 0), euler=(math.pi / 4, 0.0, 0.0))], False, ((1.8, 5.5, 0), ALL),
     dict(position=(S2 + 0.51, 5.5, 0), pushed=(S2 + 0.51 - 1.8, 0, 0), flags=RECOVER_MOVED, n_pushes=1, hit_kind=RAY_BODY, hit_entity=0,
          hit_normal=EAST, hit_depth=0.5 - (1.8 - S2))),
    # clear of everything: back unchanged
    ("clear", [PLANE], [cube((0, 5, 0))], True, ((3, 2, 0), ALL),
     dict(position=(3, 2, 0), pushed=(0, 0, 0), flags=0, n_pushes=0, hit_kind=RAY_MISS, hit_entity=NO_ENTITY, hit_normal=(0, 0, 0), hit_depth=0)),
]


def hand_record(case):
    pos, mask = case[4]
    return make_sphere_recovers([pos], R, SKIN, mask)


def hand_objects(bodies):
    return [Obj(RAY_TRIGGER if ghost else RAY_BODY, i, group, ALL, cap, capsule_dims(size) if cap else box_half_extents(size), pos,
                quat_from_euler(np.asarray(e, np.float64))) for i, (cap, size, pos, e, group, ghost) in enumerate(bodies)]


def check_hand_recover(name, got, want, tol=1e-5):
    for k, v in want.items():
        if k in ("position", "pushed", "hit_normal", "hit_depth", "remaining_depth"):
            assert np.allclose(got[k], v, atol=tol, rtol=0), f"{name}: {k} {got[k]} vs {v}"
        else:
            assert int(got[k]) == int(v), f"{name}: {k} {got[k]} vs {v}"
    if "remaining_depth" not in want:
        assert got["remaining_depth"] == 0, name
    assert got["reserved"] == 0


INVALID_RECORDS = [
    ("nan position", dict(position=(0, float("nan"), 0))), ("inf position", dict(position=(float("inf"), 0, 0))),
    ("negative radius", dict(radius=-0.5)), ("nan radius", dict(radius=float("nan"))), ("inf radius", dict(radius=float("inf"))),
    ("zero skin", dict(skin=0.0)), ("negative skin", dict(skin=-0.01)), ("nan skin", dict(skin=float("nan"))), ("inf skin", dict(skin=float("inf"))),
    ("empty mask", dict(layer_mask=0)),
]


def invalid_records():
    recs = make_sphere_recovers([(0, 0.3, 0)] * len(INVALID_RECORDS), R, SKIN, ALL)
    for i, (_, fields) in enumerate(INVALID_RECORDS):
        for k, v in fields.items():
            recs[k][i] = v
    return recs


def check_invalid(recs, got):
    for i in range(len(recs)):
        want = np.zeros(1, SPHERE_RECOVER_RESULT_DTYPE)
        want["position"], want["flags"], want["hit_entity"] = recs["position"][i], RECOVER_INVALID, NO_ENTITY
        assert got[i].tobytes() == want[0].tobytes(), (i, got[i])


SPHERE_SEED = 71


def sphere_batch(rng, n, body_pos, ghost_pos, spread=28.0):
    """Spheres where there is something to be pushed out of: centres drawn around body positions.  Every 5th is near the plane
    beside the cluster instead (above and below it, seeing every layer), every 7th free in the air above the cluster, every 19th
    around a trigger ghost's position seeing every layer.  Every 37th is invalid (the classes of INVALID_RECORDS in turn)."""
    pos = body_pos[rng.integers(0, len(body_pos), n)] + rng.normal(scale=0.45, size=(n, 3))
    recs = make_sphere_recovers(pos, rng.uniform(0.1, 0.5, n), rng.choice([0.002, 0.01, 0.05], n),
                                rng.choice(np.array([1, 2, 3, 6, ALL, ALL, ALL], np.uint32), n))
    low = np.arange(3, n, 5)
    recs["position"][low] = np.stack([rng.uniform(spread + 4, spread + 12, len(low)) * rng.choice([-1.0, 1.0], len(low)),
                                      rng.uniform(-0.45, 0.45, len(low)), rng.uniform(-spread, spread, len(low))], 1)
    recs["radius"][low] = rng.uniform(0.3, 0.5, len(low))
    recs["layer_mask"][low] = ALL
    air = np.arange(5, n, 7)
    recs["position"][air] = np.stack([rng.uniform(-spread, spread, len(air)), rng.uniform(9.0, 12.0, len(air)), rng.uniform(-spread, spread, len(air))], 1)
    aim = np.arange(7, n, 19)
    recs["position"][aim] = ghost_pos[rng.integers(0, len(ghost_pos), len(aim))] + rng.normal(scale=0.1, size=(len(aim), 3))
    recs["layer_mask"][aim] = ALL
    for k, i in enumerate(range(36, n, 37)):
        for f, v in INVALID_RECORDS[k % len(INVALID_RECORDS)][1].items():
            recs[f][i] = v
    return recs


def check_caps(n_valid, n_pen, n_skipped, kinds, n_axis):
    print(f"{n_pen} of {n_valid} valid spheres start in penetration; {n_skipped} of them set aside as ambiguous; winners by kind {dict(kinds)}; "
          f"{n_axis} compared axis normals inside boxes")
    assert n_axis >= 20, n_axis
    assert 2 * n_pen >= n_valid, (n_pen, n_valid)
    assert 2 * n_skipped <= n_pen, (n_skipped, n_pen)
    assert all(kinds.get(k, 0) >= 1 for k in (RAY_BODY, RAY_TRIGGER, RAY_GROUND)), kinds


def check_penetrations(w64, recs, valid, pen):
    """The penetration hits of the valid records against signed_ref on the World64, within refmodel/tolerances.py; a sphere is set
    aside where classify() finds the reference's own answer ambiguous.  Ends in check_caps."""
    n_valid = n_pen = n_skipped = n_axis = 0
    kinds = collections.Counter()
    share_d = share_p = share_n = 0.0
    for i in np.nonzero(valid)[0]:
        m, got = recs[i], pen[i]
        n_valid += 1
        cands, winner_clear, normal_clear = classify(w64, m)
        if not cands:
            assert got["kind"] == RAY_MISS, f"sphere {i}: hit where the reference finds nothing near"
            continue
        if cands[0].depth < 0:
            continue  # (only grazing candidates: hit or miss is the overlap's to say, exactly)
        n_pen += 1
        n_skipped += not normal_clear
        if not winner_clear:
            continue
        h = cands[0]
        kinds[h.kind] += 1
        assert (got["kind"], got["entity"]) == (h.kind, h.entity), f"sphere {i}: {got['kind']}/{got['entity']} != {h.kind}/{h.entity}"
        c = m["position"].astype(np.float64)
        tol = P_REL * (1.0 + float(np.abs(c).max()))
        ed = abs(float(got["depth"]) - h.depth) / tol
        assert ed <= 1.0, f"sphere {i}: depth {got['depth']} vs {h.depth}"
        share_d = max(share_d, ed)
        if not normal_clear:
            continue
        ep = float(np.max(np.abs(got["point"] - h.point))) / tol
        n_tol = N_ABS + N_SCALE * float(np.abs(c).sum() + m["radius"]) / min(w64.min_dim(h.code), h.cond)
        en = float(np.max(np.abs(got["normal"] - h.normal))) / n_tol
        assert ep <= 1.0 and en <= 1.0, f"sphere {i}: point {got['point']} vs {h.point}, normal {got['normal']} vs {h.normal}; shares {ep:.2f} {en:.2f}"
        share_p, share_n = max(share_p, ep), max(share_n, en)
        n_axis += h.kind != RAY_GROUND and np.isfinite(h.gap)  # the centre inside a box: one of its axes, chosen as the reference does
    print(f"worst share of tolerance: depth {share_d:.3g}, point {share_p:.3g}, normal {share_n:.3g}")
    check_caps(n_valid, n_pen, n_skipped, kinds, n_axis)
