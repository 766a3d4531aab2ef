"""Edge geometry of the query kernels on the device (csrc/bge_query.hip, bge_ray_device.hpp, bge_sphere_device.hpp): the input
families of refmodel/edge_cases.py — the outer shell of the bounding spheres, worlds 1e3 .. 1e5 from the origin, sizes 0.01 and
500 in one world, grazing incidence and the seams of the rounded box, exact ties — asked of the device and checked by that file's
sandwich: the answer must be the exact answer of a world whose shapes moved by at most B, a few binary32
ulp of the query's and the body's magnitudes.  Overlaps and penetrations go through the existing forward checks at their existing
tolerances.  Every tolerance is imported; the caps on undecided queries are asserted on the device's poses here and on the
uploaded poses, without a GPU, there.

Each world has 300 bodies (a full workgroup and a partial one), a few of them Dynamic, 4 trigger ghosts, and is asked 600 queries
of each kind (two chunks of 256 and a partial one) generated from the poses the device holds after one tick."""
from __future__ import annotations

import numpy as np
import pytest

import banggameengine_amd as B
from banggameengine_amd import world as W

from refmodel.tolerances import NEVER_INSIDE_MARGIN
from refmodel.rays import ALL, RAY_BODY, RAY_MISS
from refmodel.spheres import SphereRef
from refmodel.moves import move_ref
from refmodel.sandwich import Sandwich, check_caps, check_penetrations, code_of
from refmodel.edge_cases import FAMILIES, KINDS, N_BODIES, TIE_BODIES, TIE_SPHERE, Spec, check_ties, family_queries, overlap_counts, sphere_records
from refmodel.device import FLAGS, Scene, ask, check_overlaps, device_caster, move

pytestmark = pytest.mark.gpu


class EdgeScene(Scene):
    """refmodel.device.Scene holding a family's world instead of its random one."""

    def __init__(self, spec):
        self.n = N_BODIES
        self.w = B.World(device=0)
        self.w.set_topology(np.full(self.n, W.NO_PARENT, np.uint32))
        self.w.upload_trs(spec.pos, spec.euler, np.ones((self.n, 3)))
        self.type, self.trig, self.shape, self.size, self.layer, self.mask = spec.type, spec.trig, spec.shape, spec.size, spec.layer, spec.mask
        self.w.upload_bodies(self.type, None, self.shape, self.size, self.layer, self.mask)
        self.plane = spec.plane
        self.w.set_ground_plane(self.plane)
        self.t_active = np.ones(len(self.trig), np.uint8)
        self.t_oneshot = np.zeros(len(self.trig), np.uint8)
        self.upload_triggers()


class Family:
    """A family's world ticked once, its queries from the device's poses, the device's answers and the sandwiches: made once."""

    def __init__(self, name):
        self.name = name
        self.sc = EdgeScene(Spec(name))
        self.sc.tick(1)
        self.w64 = self.sc.objects()
        self.qs = family_queries(name, self.w64)
        self.ans = ask(self.sc.w, (self.qs["ray"], self.qs["cast"], self.qs["sphere"]))  # (device forms == host forms, byte for byte)
        self._sw = {}

    def sandwich(self, cast):
        if cast not in self._sw:
            self._sw[cast] = Sandwich(self.w64, self.qs["cast" if cast else "ray"], cast)
        return self._sw[cast]


@pytest.fixture(scope="module")
def families():
    made = {}

    def get(name):
        if name not in made:
            made[name] = Family(name)
        return made[name]
    yield get
    for fam in made.values():
        fam.sc.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(FAMILIES))
def test_family_on_the_device(families, name, kind):
    fam = families(name)
    what = f"{name} {kind}"
    if kind == "overlap":
        ref = SphereRef(fam.w64)
        check_overlaps(ref, fam.qs["sphere"], fam.ans["overlap"])
        check_caps(what, overlap_counts(ref, fam.qs["sphere"]))
        return
    if kind == "penetration":
        recs = sphere_records(fam.qs["sphere"])
        h = fam.sc.w.sphere_penetration(recs["position"], recs["radius"], recs["layer_mask"])
        pen = np.zeros(len(recs), W.PENETRATION_HIT_DTYPE)
        for k, v in h.items():
            pen[k] = v
        res = check_penetrations(fam.w64, recs, pen)
        print(f"{what}: worst share of tolerance: depth {res['depth']:.3g}, point {res['point']:.3g}, normal {res['normal']:.3g}")
        check_caps(what, res["counts"])
        return
    cast = kind.startswith("cast")
    sw = fam.sandwich(cast)
    got = fam.ans["cast" if cast else "ray"]
    if kind.endswith("_all"):
        res = sw.check_all(fam.ans[kind], got)
        print(f"{what}: worst f {res['f']:.3g} B outside its interval")
    else:
        res = sw.check_closest(got)
        print(f"{what}: worst f {res['f']:.3g} B outside its interval ({res['forward']:.3g} B from the float64 fraction), point {res['point']:.3g} B "
              f"off the surface, normal {res['normal']:.3g} of its tolerance ({res['normals_skipped']} at an edge or a seam)")
        assert (got["kind"] == RAY_BODY).any() and (got["kind"] == RAY_MISS).any()
    check_caps(what, res["counts"])
    if name == "grazing" and kind == "cast":  # the move's own pattern on the device's poses: along a face never it, closing always it
        tags = fam.qs["cast_tags"]
        codes = [None if got["kind"][i] == RAY_MISS else code_of(int(got["kind"][i]), got["entity"][i]) for i in range(len(tags))]
        along = [i for i, (tag, _) in enumerate(tags) if tag == "along"]
        closing = [i for i, (tag, _) in enumerate(tags) if tag == "closing"]
        assert len(along) >= 100 and len(closing) >= 100
        assert all(tags[i][1] not in sw.q[i].iv for i in along) and all(sw.q[i].iv[tags[i][1]].certain for i in closing)
        assert all(codes[i] != tags[i][1] for i in along), "a cast along a face at radius + skin reports that face"
        late = [i for i in closing if codes[i] != tags[i][1] and sw.status_closest(i) == "hit" and sw.q[i].true[0][1] == tags[i][1]]
        assert not late, f"casts {late} close on their face by more than skin + 30 B and do not report it"
    if name == "scale" and kind == "cast":  # radius 0: the rays' answers in kind and entity wherever the sandwich forces the winner
        rays = fam.sandwich(False)
        sure = [i for i in range(len(rays.q)) if rays.status_closest(i) != "undecided"]
        assert len(sure) >= 0.9 * len(rays.q)
        assert np.array_equal(got["kind"][sure], fam.ans["ray"]["kind"][sure]) and np.array_equal(got["entity"][sure], fam.ans["ray"]["entity"][sure])


# the far-1e3 world: movers beside its bodies.  The skin follows the header's rule for that extent ("well above the binary32
# spacing at the scene's extent (1e-3 .. 1e-2 for a scene of a few hundred units)"): 1e-2 at a few hundred units is some 330
# spacings; beyond 1,024 a spacing is 2^-13, so 0.04.  The never-inside margin is that of refmodel/tolerances.py, unchanged:
# 8 spacings here.
FAR_SKIN = 0.04
FAR_EXTENT = 1024.0
FAR_MARGIN = NEVER_INSIDE_MARGIN
N_MOVERS = 257


def far_movers(w64):
    rng = np.random.default_rng(FAMILIES["far3"]["seed"] + 2000)
    live = np.nonzero(w64.omask != 0)[0]
    j = live[rng.integers(0, len(live), N_MOVERS)]
    brad = np.where(w64.capsule[j], w64.dims[j, 0] + w64.dims[j, 1], np.linalg.norm(w64.dims[j], axis=1))
    out = rng.normal(size=(N_MOVERS, 3))
    out /= np.linalg.norm(out, axis=1, keepdims=True)
    radius = rng.uniform(0.3, 0.6, N_MOVERS)
    pos = w64.origin[j] + out * (brad + radius + rng.uniform(0.1, 3.0, N_MOVERS))[:, None]
    disp = -out * rng.uniform(0.5, 2.0, N_MOVERS)[:, None] * brad[:, None] + rng.normal(scale=0.5, size=(N_MOVERS, 3))
    return W.make_sphere_moves(pos, disp, radius, FAR_SKIN, 0.5, layer_mask=ALL)


def test_sphere_moves_in_the_far_world(families):
    """sphere_move == move_ref over the device's own casts, byte for byte, 1e3 from the origin; a mover that starts clear of
    everything by radius + skin ends clear of everything by radius - margin."""
    fam = families("far3")
    w = fam.sc.w
    moves = far_movers(fam.w64)
    got = move(w, moves)
    want = move_ref(device_caster(w), moves)
    bad = [i for i in range(len(moves)) if got[i].tobytes() != want[i].tobytes()]
    assert not bad, f"{len(bad)} of {len(moves)} differ, first {bad[0]}: {got[bad[0]]} vs {want[bad[0]]}"
    assert (got["flags"] & W.MOVE_INVALID).sum() == 0 and (got["n_hits"] > 0).sum() >= 50
    assert FAR_MARGIN < FAR_SKIN and np.abs(fam.w64.origin).max() >= FAR_EXTENT
    start = w.overlap_sphere(moves["position"], moves["radius"] + moves["skin"], moves["layer_mask"])
    clear = np.diff(start["offsets"].astype(np.int64)) == 0
    end = w.overlap_sphere(got["position"][clear], moves["radius"][clear] - FAR_MARGIN, moves["layer_mask"][clear])
    inside = np.nonzero(np.diff(end["offsets"].astype(np.int64)) != 0)[0]
    print(f"{clear.sum()} of {len(moves)} movers start clear, {(got['n_hits'] > 0).sum()} hit something; {len(inside)} end inside something")
    assert clear.sum() >= 100
    assert len(inside) == 0, (np.nonzero(clear)[0][inside], end["distance"])


def test_exact_ties():
    """Two Static boxes at one pose, and two of different size entered at one representable fraction: the lower entity wins the
    ray, the cast and the penetration; the lists hold both with identical fraction bits in code order.  No tolerance."""
    n = len(TIE_BODIES)
    w = B.World(device=0)
    try:
        w.set_topology(np.full(n, W.NO_PARENT, np.uint32))
        w.upload_trs(np.float32([p for _, p in TIE_BODIES]), np.zeros((n, 3)), np.ones((n, 3)))
        w.upload_bodies(np.full(n, W.BODY_STATIC, np.uint8), None, np.zeros(n, np.uint8), np.float32([s for s, _ in TIE_BODIES]),
                        np.full(n, 1, np.uint32), np.full(n, ALL, np.uint32))
        w.set_ground_plane(False)
        w.tick(flags=FLAGS)

        def closest(q):
            o, d, md, r = q[:4]
            h = w.sphere_cast([o], [d], md, r, ALL) if r else w.raycast([o], [d], md, ALL)
            assert h["kind"][0] == RAY_BODY
            return int(h["entity"][0]), h["fraction"][0]

        def listed(q):
            o, d, md, r = q[:4]
            a = w.sphere_cast_all([o], [d], md, r, ALL) if r else w.raycast_all([o], [d], md, ALL)
            return list(zip(a["entity"].tolist(), a["fraction"]))

        check_ties(closest, listed)
        pen = w.sphere_penetration([TIE_SPHERE[0]], TIE_SPHERE[1], ALL)
        assert pen["kind"][0] == RAY_BODY and pen["entity"][0] == TIE_SPHERE[2] and pen["depth"][0] == np.float32(0.25)
    finally:
        w.close()
