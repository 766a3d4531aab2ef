"""Edge geometry of the query kernels without a GPU: the backward-error ("sandwich") checker of refmodel/sandwich.py, built on the
float64 references of refmodel/rays.py and refmodel/spheres.py, on the input families of refmodel/edge_cases.py that the GPU tests of
test_gpu_query_edges.py ask the device, and the proof that the checker bites.

The forward checkers (check_against_reference, check_casts) compare the fraction with the float64 fraction.  At grazing incidence
the fraction is ill-conditioned whatever a binary32 kernel does, so they cannot be pointed there.  The sandwich asks instead
whether the answer is the exact answer of a world whose shapes moved by at most

    B_j = N_SCALE * (|from|_1 + |delta|_1 + |origin_j|_1 + bounding radius_j [+ cast radius])

(N_SCALE of refmodel/tolerances.py: "the entry point is known to a few binary32 ulp of the ray's magnitudes").  f_out is the
reference fraction against shape j grown by B_j, f_in against it shrunk by B_j; grown contains true contains shrunk, so
f_out <= f_true <= f_in, and with tau_j = B_j / |delta|:

  closest hit (j, f, point, normal)   j's grown shape is hit (or the query starts inside the grown and outside the shrunk shape:
                                      f_out = 0); f_out - tau <= f <= f_in + tau (no upper side when the shrunk shape is
                                      missed); no other object is certainly earlier; the point lies within B_j of j's surface
                                      (a cast: the centre from + delta f within B_j of distance radius from it, too); the normal
                                      is within N_ABS + N_SCALE (...) / min_dim of the float64 outward normal at the reported
                                      point, unless that point lies within B_j of an edge, a corner or a capsule seam
  miss                                no object is certainly hit (shrunk shape hit from outside the grown shape)
  all hits                            every certain object is listed, every listed object is possible with f in its interval,
                                      the list ascends in (f, code), offsets are consistent, its head is the closest hit
  the plane                           takes part with B = N_SCALE * (|from.y| + |delta.y| + radius)

A query is UNDECIDED when the sandwich does not force the answer (closest: the winner; all hits: the set).  Per family and kind
at most 10 % may be, at least 100 must be certain hits and 30 certain misses: asserted here on the reference alone, so a GPU
failure cannot hide behind them.  Overlaps and penetrations are well conditioned (distance is 1-Lipschitz): they go through the
existing check_overlaps and the penetration comparison of test_gpu_sphere_recover.py (check_penetrations of
refmodel/sandwich.py is that comparison, its tolerances imported); only the inputs are new.

Every tolerance here is imported from refmodel/tolerances.py or exact by construction.  The families' clearances (depth inside
a corner, offset from a face) are max(1e-2 x size, 30 x B)."""
from __future__ import annotations

import functools

import numpy as np
import pytest

from refmodel.rays import ALL, CODE_PLANE
from refmodel.spheres import SphereRef
from refmodel.recover import signed_ref
from refmodel.sandwich import MIN_HITS, Sandwich, check_caps, check_penetrations
from refmodel.edge_cases import (FAMILIES, FAR, KINDS, TIE_SPHERE, Spec, check_ties, family_queries, overlap_counts, penetration_answers,
                                 sphere_records, tie_world64)

# ------------------------------------------------------------------------------------------------ the reference alone


@functools.lru_cache(maxsize=None)
def reference(name):
    """(World64 at the uploaded poses, the family's queries)."""
    w64 = Spec(name).world64()
    return w64, family_queries(name, w64)


@functools.lru_cache(maxsize=None)
def sandwich(name, cast):
    w64, qs = reference(name)
    return Sandwich(w64, qs["cast" if cast else "ray"], cast)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(FAMILIES))
def test_reference_passes_its_own_checker_inside_the_caps(name, kind):
    w64, qs = reference(name)
    if kind == "overlap":
        check_caps(f"{name} {kind}", overlap_counts(SphereRef(w64), qs["sphere"]))
    elif kind == "penetration":
        recs = sphere_records(qs["sphere"])
        check_caps(f"{name} {kind}", check_penetrations(w64, recs, penetration_answers(w64, recs))["counts"])
    else:
        sw = sandwich(name, kind.startswith("cast"))
        got, allh = sw.answers()
        res = sw.check_all(allh, got) if kind.endswith("_all") else sw.check_closest(got)
        print({k: v for k, v in res.items() if k != "counts"})
        check_caps(f"{name} {kind}", res["counts"])


def test_radius_zero_casts_of_the_scale_family_are_its_rays():
    rays, casts = sandwich("scale", False), sandwich("scale", True)
    assert not reference("scale")[1]["cast"][3].any()
    n = 0
    for a, b in zip(rays.q, casts.q):
        assert [h[1] for h in a.true] == [h[1] for h in b.true]
        assert set(a.iv) == set(b.iv) and [k for k, v in a.iv.items() if v.certain] == [k for k, v in b.iv.items() if v.certain]
        n += bool(a.true)
    assert n >= MIN_HITS


def test_the_sandwich_decides_the_moves_own_pattern():
    """A sphere at radius + skin from a face or a side, cast along it, cannot have touched that body; with a tilt that closes
    more than skin + 30 B it certainly has.  So check_closest and check_all reject a device that reports the first or drops
    the second."""
    sw = sandwich("grazing", True)
    tags = reference("grazing")[1]["cast_tags"]
    along = [i for i, (tag, _) in enumerate(tags) if tag == "along"]
    closing = [i for i, (tag, _) in enumerate(tags) if tag == "closing"]
    assert len(along) >= 100 and len(closing) >= 100
    assert all(tags[i][1] not in sw.q[i].iv for i in along)
    assert all(sw.q[i].iv[tags[i][1]].certain for i in closing)


# ------------------------------------------------------------------------------------------------ the checker bites


CLOSEST_LOST = "are certainly hit|is certainly earlier"  # what check_closest says of a miss, and of a later object, in place of a certain winner
NOT_LISTED, NOT_ASCENDING = "is certainly hit and not listed", "not ascending"
OFF = r"outside \[|off the surface"  # a fraction that leaves its interval, a point that leaves the surface


def _closest_rejected(sw, i, hits, match):
    """check_closest rejects query i, asked alone, answered with these hits, and says why."""
    one = sw.only(i)
    got, _ = one.answers([hits])
    with pytest.raises(AssertionError, match=match):
        one.check_closest(got)


def _list_rejected(sw, i, hits, match):
    one = sw.only(i)
    with pytest.raises(AssertionError, match=match):
        one.check_all(one.answers([hits])[1])


def _drops_rejected(sw, lists):
    """Lists with hits dropped, one query at a time: wherever a dropped object is certain check_all misses it, wherever the
    dropped object is the certain winner check_closest does; returns how many of each."""
    n_closest = n_listed = 0
    for i, (q, hits) in enumerate(zip(sw.q, lists)):
        if len(hits) == len(q.true):
            continue
        kept = {h[1] for h in hits}
        if any(q.iv[h[1]].certain for h in q.true if h[1] not in kept and h[1] in q.iv):
            _list_rejected(sw, i, hits, NOT_LISTED)
            n_listed += 1
        if sw.status_closest(i) == "hit" and q.true[0][1] not in kept:
            _closest_rejected(sw, i, hits, CLOSEST_LOST)
            n_closest += 1
    return n_closest, n_listed


def _approach(sw, q, code):
    """Closest approach of the query's segment to the object's centre, as a share of its bounding radius grown by the radius."""
    k = sw.index[code]
    wv = sw.w.origin[k] - q.frm
    t = min(max(float(wv @ q.delta) / float(q.delta @ q.delta), 0.0), 1.0)
    return float(np.linalg.norm(wv - t * q.delta)) / (sw.brad[k] + q.r)


@pytest.mark.parametrize("cast", [False, True], ids=["rays", "casts"])
@pytest.mark.parametrize("name", ["shell"])
def test_a_cull_one_percent_tight_is_rejected(name, cast):
    """(a) hits dropped where the closest approach to the body's centre exceeds 0.99 of the bounding radius; every dropped
    certain hit is missed by name.  (In the far worlds 30 B is more than 1 % of the sizes, so no certain hit lies in that
    shell: (b) is the mutation that applies there.)"""
    sw = sandwich(name, cast)
    lists = [[h for h in q.true if h[1] == CODE_PLANE or _approach(sw, q, h[1]) <= 0.99] for q in sw.q]
    dropped = sum(len(q.true) - len(x) for q, x in zip(sw.q, lists))
    n_closest, n_listed = _drops_rejected(sw, lists)
    print(f"{name}: {dropped} hits dropped, rejected as winners {n_closest} times and as list entries {n_listed} times")
    assert dropped >= 20 and n_closest >= 20 and n_listed >= 20


@pytest.mark.parametrize("cast", [False, True], ids=["rays", "casts"])
@pytest.mark.parametrize("name", FAR + ("scale",))
def test_a_forgotten_slack_term_is_rejected(name, cast):
    """(b) hits dropped for bodies with |origin|_1 > 1e3."""
    sw = sandwich(name, cast)
    lists = [[h for h in q.true if h[1] == CODE_PLANE or sw.o1[sw.index[h[1]]] <= 1e3] for q in sw.q]
    n_closest, n_listed = _drops_rejected(sw, lists)
    print(f"{name}: rejected as winners {n_closest} times and as list entries {n_listed} times")
    assert n_closest >= 20 and n_listed >= 20


@pytest.mark.parametrize("cast", [False, True], ids=["rays", "casts"])
@pytest.mark.parametrize("name", list(FAMILIES))
def test_a_point_ten_b_off_the_surface_is_rejected(name, cast):
    """(c) the winner's fraction moved so that its point leaves the surface by 10 B; one query at a time, every one rejected."""
    sw = sandwich(name, cast)
    tried = 0
    for i, q in enumerate(sw.q):
        if sw.status_closest(i) != "hit":
            continue
        h = q.true[0]
        closing = abs(float(h[4] @ q.delta))
        if closing == 0.0:
            continue
        f = h[0] - 10.0 * q.iv[h[1]].b / closing
        if f < 0.0:
            f = h[0] + 10.0 * q.iv[h[1]].b / closing
        if f > 1.0:
            continue
        moved = (f,) + tuple(h[1:5]) + ((q.frm + q.delta * f - q.r * h[4],) if sw.cast else ())
        _closest_rejected(sw, i, [moved] + list(q.true[1:]), OFF)
        tried += 1
    assert tried >= MIN_HITS, tried


@pytest.mark.parametrize("cast", [False, True], ids=["rays", "casts"])
@pytest.mark.parametrize("name", list(FAMILIES))
def test_the_second_closest_object_and_broken_lists_are_rejected(name, cast):
    """(e) the second-closest object reported where the first is certain (a miss where there is no second); (f) an entry of an
    all-hits list omitted, and two entries swapped.  One query at a time, every one rejected for that reason."""
    sw = sandwich(name, cast)
    sw.check_all(sw.answers()[1])
    sure = [i for i in range(len(sw.q)) if sw.status_closest(i) == "hit"]
    assert len(sure) >= MIN_HITS
    for i in sure:
        _closest_rejected(sw, i, sw.q[i].true[1:], CLOSEST_LOST)
    sure_all = [i for i in range(len(sw.q)) if sw.status_all(i) == "hit"]
    assert len(sure_all) >= MIN_HITS
    for i in sure_all:
        _list_rejected(sw, i, sw.q[i].true[:-1], NOT_LISTED)
    two = [i for i, q in enumerate(sw.q) if len(q.true) >= 2 and np.float32(q.true[0][0]) != np.float32(q.true[1][0])]
    if name not in ("scale", "far5"):  # (their rays meet one body each: short ones, and bodies 6,000 units apart)
        assert two
    for i in two:
        q = sw.q[i]
        _list_rejected(sw, i, [q.true[1], q.true[0]] + list(q.true[2:]), NOT_ASCENDING)


# ------------------------------------------------------------------------------------------------ exact ties


def test_exact_ties_on_the_reference_and_the_checker_rejects_the_higher_entity():
    """(d) the tie rule: the lower object code wins; the lists hold both at identical fraction bits in code order."""
    w64 = tie_world64()
    assert np.array_equal(w64.dims, [[1, 1, 1], [1, 1, 1], [0.5, 0.5, 0.5], [1, 1, 1], [0.5, 1, 0.5]])
    cands = signed_ref(w64, TIE_SPHERE[0], TIE_SPHERE[1], ALL)
    assert [c.entity for c in cands[:2]] == [1, 3] and cands[0].depth == cands[1].depth == 0.25

    def hits(q):
        o, d, md, r = q[:4]
        return SphereRef(w64).sweep_all(o, d, md, r, ALL) if r else w64.cast_all(o, d, md, ALL)

    check_ties(lambda q: (hits(q)[0][3], hits(q)[0][0]), lambda q: [(h[3], h[0]) for h in hits(q)])
    with pytest.raises(AssertionError):  # the higher entity on the tie
        check_ties(lambda q: (hits(q)[1][3], hits(q)[1][0]), lambda q: [(h[3], h[0]) for h in hits(q)])
    with pytest.raises(AssertionError):  # the list out of code order
        check_ties(lambda q: (hits(q)[0][3], hits(q)[0][0]), lambda q: [(h[3], h[0]) for h in hits(q)][1::-1])
