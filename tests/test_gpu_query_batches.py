"""The part the ray, sphere-cast and overlap queries share (csrc/bge_query.hip): the walk over the body
workgroups and the staging of a batch through chunks of 256 queries with a partial last chunk.

For each host entry point and for batches of 1, 255, 256, 257 and 513 queries, the batch's result must equal, byte for byte, the
results of the same queries issued one per call and concatenated (for the lists: the per-query segments concatenated and the
offsets rebuilt).  Byte equality is the right bound: the arithmetic of one (query, body) pair does not depend on the batch, the
closest hit is an order-independent minimum over (fraction, object code) keys, and the lists are totally ordered on the host.

World: 600 bodies (two full workgroups of 256 and a partial third), boxes and capsules standing on the ground plane, and two
trigger ghosts above them; ticked once.  The queries come from one seed; each test asserts that hits, misses, ghost hits and
plane hits all occur among the first 255, and a few invalid records (zero direction, NaN origin, negative radius or distance)
sit in the first chunk and at the chunk boundaries."""
from __future__ import annotations

import numpy as np
import pytest

import banggameengine_amd as B
from banggameengine_amd import world as W

from refmodel.rays import RAY_BODY, RAY_GROUND, RAY_MISS, RAY_TRIGGER

pytestmark = pytest.mark.gpu

N_BODIES, N_QUERIES = 600, 513
BATCHES = (1, 255, 256, 257, 513)
ENTRIES = ("raycast", "raycast_all", "sphere_cast", "sphere_cast_all", "overlap_sphere")
GHOST_POS = np.float32([[6.0, 5.0, 9.0], [31.0, 5.5, 20.0]])
INVALID = (7, 100, 200, 255, 256, 512)  # a few in the first chunk, the rest at the seams of the chunks
FLAGS = W.TICK_ALL | W.TICK_BROADPHASE


def build_world(rng):
    n = N_BODIES + len(GHOST_POS)
    w = B.World(device=0)
    w.set_topology(np.full(n, W.NO_PARENT, np.uint32))
    shape = rng.integers(0, 2, n).astype(np.uint8)
    size = rng.uniform(0.2, 0.8, (n, 3)).astype(np.float32)
    # a 25 x 24 grid, 2 units apart; each body stands on the plane (a capsule's half height is size.y + its radius size.x)
    ix = np.arange(N_BODIES)
    half = np.where(shape[:N_BODIES] == 1, size[:N_BODIES, 1] + size[:N_BODIES, 0], size[:N_BODIES, 1])
    pos = np.concatenate([np.stack([2.0 * (ix % 25), half, 2.0 * (ix // 25)], 1), GHOST_POS]).astype(np.float32)
    w.upload_trs(pos, np.zeros((n, 3)), np.ones((n, 3)))
    kind = rng.choice([W.BODY_STATIC, W.BODY_DYNAMIC], n).astype(np.uint8)
    kind[N_BODIES:] = W.BODY_NONE
    layer = rng.choice(np.uint32([1, 4]), n)
    w.upload_bodies(kind, None, shape, size, layer, np.full(n, 0xFFFFFFFF, np.uint32))
    g = np.arange(N_BODIES, n, dtype=np.uint32)
    w.upload_triggers(g, np.uint8([0, 1]), np.float32([[1.0, 1.0, 1.0], [0.7, 0.8, 0.7]]), np.uint32([8, 8]),
                      np.uint32([0xFFFFFFFF] * 2), np.uint8([0, 0]), np.uint8([1, 1]))
    w.set_ground_plane(True)
    w.tick(flags=FLAGS)
    return w, pos


def make_queries(rng, pos):
    """Five kinds of query in random order: down onto a body, up into the sky, at a ghost, down at the plane alone, and level
    through a row of bodies (many hits for the lists)."""
    n = N_QUERIES
    cat = rng.integers(0, 5, n)
    at = pos[rng.integers(0, N_BODIES, n)]
    ghost = GHOST_POS[rng.integers(0, len(GHOST_POS), n)]
    jit = rng.normal(scale=0.15, size=(n, 3))
    o = np.stack([at[:, 0] + jit[:, 0], np.full(n, 7.0), at[:, 2] + jit[:, 2]], 1)
    d = np.tile([0.0, -1.0, 0.0], (n, 1)) + 0.05 * jit
    md = rng.uniform(8.0, 12.0, n)
    mask = np.full(n, 0xFFFFFFFF, np.uint32)
    d[cat == 1] *= -1.0
    away = rng.normal(size=(n, 3)) * [6.0, 1.0, 6.0] + [0.0, 6.0, 0.0]
    o[cat == 2] = (ghost + away)[cat == 2]
    d[cat == 2] = (ghost + 0.3 * jit - o)[cat == 2]
    md[cat == 2] = 1.5
    mask[cat == 2] = 8
    mask[cat == 3] = rng.choice(np.uint32([2, 10]), n)[cat == 3]
    o[cat == 4] = np.stack([np.full(n, -3.0), rng.uniform(0.2, 0.6, n), at[:, 2] + jit[:, 2]], 1)[cat == 4]
    d[cat == 4] = (np.tile([1.0, 0.0, 0.0], (n, 1)) + 0.02 * jit)[cat == 4]
    md[cat == 4] = 60.0
    radius = np.where(rng.random(n) < 0.2, 0.0, rng.uniform(0.05, 0.6, n))
    # overlap spheres: around a body, in the sky, around a ghost, low over the plane alone, around a body for one layer
    c = at + [0.0, 0.3, 0.0] + 2.0 * jit
    c[cat == 1] += [0.0, 50.0, 0.0]
    c[cat == 2] = (ghost + 3.0 * jit)[cat == 2]
    srad = rng.uniform(0.2, 2.5, n)
    smask = np.select([cat == 2, cat == 3, cat == 4], [np.uint32(8), np.uint32(2), np.uint32(1)], np.uint32(0xFFFFFFFF)).astype(np.uint32)
    o, d, md, radius, c, srad = (a.astype(np.float32) for a in (o, d, md, radius, c, srad))
    ray_md, cast_radius = md.copy(), radius.copy()
    for k, i in enumerate(INVALID):
        if k % 3 == 0:  # zero direction; a negative radius for the overlap
            d[i] = 0.0
            srad[i] = -1.0
        elif k % 3 == 1:  # NaN origin or centre
            o[i, 1] = np.nan
            c[i, 2] = np.nan
        else:  # a negative distance for the ray, a negative radius for the cast (its distance stays valid) and the overlap
            ray_md[i] = -md[i]
            cast_radius[i] = -0.25
            srad[i] = -0.5
    return {"raycast": (o, d, ray_md, mask), "raycast_all": (o, d, ray_md, mask), "sphere_cast": (o, d, md, cast_radius, mask),
            "sphere_cast_all": (o, d, md, cast_radius, mask), "overlap_sphere": (c, srad, smask)}


class Batches:
    def __init__(self):
        rng = np.random.default_rng(20261017)
        self.w, pos = build_world(rng)
        self.queries = make_queries(rng, pos)
        self.single = {}

    def run(self, entry, lo, hi):
        return getattr(self.w, entry)(*(a[lo:hi] for a in self.queries[entry]))

    def one_per_call(self, entry):
        """The N_QUERIES queries of `entry` issued one per call, computed once and never changed."""
        if entry not in self.single:
            self.single[entry] = [self.run(entry, i, i + 1) for i in range(N_QUERIES)]
        return self.single[entry]


@pytest.fixture(scope="module")
def batches():
    b = Batches()
    yield b
    b.w.close()


def concatenated(singles):
    out = {k: np.concatenate([s[k] for s in singles]) for k in singles[0] if k != "offsets"}
    if "offsets" in singles[0]:
        counts = [int(s["offsets"][1]) for s in singles]
        assert all(s["offsets"][0] == 0 and len(s["kind"]) == c for s, c in zip(singles, counts))
        out["offsets"] = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    return out


@pytest.mark.parametrize("n", BATCHES)
@pytest.mark.parametrize("entry", ENTRIES)
def test_batch_equals_one_query_per_call(batches, entry, n):
    want = concatenated(batches.one_per_call(entry)[:n])
    got = batches.run(entry, 0, n)
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (k, got[k].shape, want[k].shape)
        assert got[k].tobytes() == want[k].tobytes(), f"{entry}, batch of {n}: {k} differs from the one-per-call results"


@pytest.mark.parametrize("entry", ENTRIES)
def test_first_chunk_holds_every_kind_of_answer(batches, entry):
    """Hits, misses, ghost hits and plane hits all occur within the first 255 queries, and the invalid records answer nothing."""
    singles = batches.one_per_call(entry)
    first = concatenated(singles[:255])
    kinds = set(first["kind"].tolist())
    assert {RAY_BODY, RAY_TRIGGER, RAY_GROUND} <= kinds, kinds
    if "offsets" in first:
        counts = np.diff(first["offsets"].astype(np.int64))
        assert (counts == 0).sum() >= 10 and (counts >= 2).sum() >= 10, counts  # misses, and lists longer than one record
        empty = [int(s["offsets"][1]) == 0 for s in singles]
    else:
        assert RAY_MISS in kinds
        empty = [int(s["kind"][0]) == RAY_MISS for s in singles]
    assert all(empty[i] for i in INVALID)
    assert sum(empty[:255]) <= 255 - 60  # most queries find something
