"""The GPU side of the comparisons: Scene drives a World and rebuilds the reference's objects from what the device holds; the
check_* functions compare device answers with the float64 reference within refmodel/tolerances.py; device_caster, move, ask,
penetration and recover call the device in the forms the references expect.  With the *_device modules built on it, the only part
of refmodel that opens a World."""
from __future__ import annotations

import math

import numpy as np

import banggameengine_amd as B
from banggameengine_amd import world as W

from .tolerances import F_ABS, F_REL, N_ABS, N_SCALE, P_REL
from .rays import NO_ENTITY, RAY_BODY, RAY_MISS, RAY_TRIGGER, World64, quat_from_euler
from .recover_cases import check_penetrations  # noqa: F401  (kept where a *_cpu test can reach it; the GPU tests take it from here)

FLAGS = W.TICK_ALL | W.TICK_BROADPHASE


class Scene:
    """A world plus what the reference needs to rebuild its objects."""

    def __init__(self, n, rng, n_triggers=0, spread=30.0, plane=True, parent=None, has_transform=None):
        self.n = n
        self.w = B.World(device=0)
        self.w.set_topology(np.full(n, W.NO_PARENT, np.uint32) if parent is None else parent, has_transform)
        pos = np.stack([rng.uniform(-spread, spread, n), rng.uniform(0.3, 6.0, n), rng.uniform(-spread, spread, n)], 1)
        self.w.upload_trs(pos, rng.uniform(-math.pi, math.pi, (n, 3)), np.ones((n, 3)))
        self.type = rng.choice([W.BODY_STATIC, W.BODY_DYNAMIC, W.BODY_KINEMATIC], n, p=[0.3, 0.5, 0.2]).astype(np.uint8)
        self.trig = np.zeros(0, np.int64)
        if n_triggers:
            self.trig = rng.choice(n, n_triggers, replace=False)
            self.type[self.trig] = W.BODY_NONE
        self.shape = rng.integers(0, 2, n).astype(np.uint8)
        self.size = rng.uniform(0.1, 1.5, (n, 3)).astype(np.float32)
        self.layer = (1 << rng.integers(0, 4, n)).astype(np.uint32)
        self.mask = rng.choice(np.array([0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0x3, 0], np.uint32), n)
        self.w.upload_bodies(self.type, None, self.shape, self.size, self.layer, self.mask)
        self.plane = plane
        self.w.set_ground_plane(plane)
        self.t_active = np.ones(len(self.trig), np.uint8)
        self.t_oneshot = np.zeros(len(self.trig), np.uint8)
        if len(self.trig):
            self.upload_triggers()

    def upload_triggers(self):
        self.w.upload_triggers(self.trig, self.shape[self.trig], self.size[self.trig], self.layer[self.trig], self.mask[self.trig],
                               self.t_oneshot, self.t_active)

    def tick(self, k=1):
        for _ in range(k):
            self.ghost_pose = self.w.download_pose()  # ghosts are posed from the Transforms as they are before the step
            self.w.tick(flags=FLAGS)

    def dims(self):
        """Per entity: the box's half extents with margin or the capsule's (radius, half height, radius), as the library holds them."""
        h = np.maximum(self.size, np.float32(0.01))
        m0 = np.float32(0.04)
        safe = (np.float32(0.1) * h.min(axis=1))[:, None]
        inner = h - m0
        box = np.where(safe < m0, ((inner + m0) - safe) + safe, inner + m0).astype(np.float32)
        cap = np.stack([h[:, 0], np.maximum(self.size[:, 1], np.float32(0)), h[:, 0]], 1)
        return np.where(self.shape[:, None] == 1, cap, box)

    def bodies_in_world(self):
        return np.nonzero(self.type != W.BODY_NONE)[0]

    def ghosts_in_world(self):
        return self.trig[self.t_active.astype(bool)]

    def objects(self):
        """The reference's world: every body at the pose the device holds, every active ghost at its posed pose."""
        pos, _ = self.w.download_pose()
        quat = self.w.download_bodies()["quat"].astype(np.float64)
        dims = self.dims()
        live, ghosts = self.bodies_in_world(), self.ghosts_in_world()
        gp, ge = self.ghost_pose
        gq = np.array([quat_from_euler(ge[e].astype(np.float64)) for e in ghosts]).reshape(-1, 4)
        ent = np.concatenate([live, ghosts])
        kind = np.concatenate([np.full(len(live), RAY_BODY), np.full(len(ghosts), RAY_TRIGGER)])
        return World64.from_arrays(kind, ent, self.layer[ent], self.mask[ent], self.shape[ent] == 1, dims[ent],
                                   np.concatenate([pos[live], gp[ghosts]]), np.concatenate([quat[live], gq]), self.plane)

    def close(self):
        self.w.close()


def check_against_reference(ref, o, d, md, mask, got, need_hits=50):
    checked = hits = 0
    err_f = err_p = err_n = 0.0
    for i in range(len(o)):
        if not ref.clear(o[i], d[i], md[i], mask[i]):
            continue
        checked += 1
        want = ref.cast_all(o[i], d[i], md[i], mask[i])
        if not want:
            assert got["kind"][i] == RAY_MISS and got["entity"][i] == NO_ENTITY, f"ray {i}: hit where the reference misses"
            continue
        f, code, kind, ent, n = want[0]
        assert (got["kind"][i], got["entity"][i]) == (kind, ent), f"ray {i}: {got['kind'][i]}/{got['entity'][i]} != {kind}/{ent}"
        hits += 1
        gf = float(got["fraction"][i])
        assert abs(gf - f) <= F_REL * f + F_ABS, f"ray {i}: fraction {gf} vs {f}"
        p = o[i].astype(np.float64) + (d[i] * md[i]).astype(np.float64) * f
        assert np.all(np.abs(got["point"][i] - p) <= P_REL * (1.0 + np.abs(p))), f"ray {i}: point {got['point'][i]} vs {p}"
        # the entry point carries binary32 rounding of the ray's magnitudes; the normal turns by that over the shape's size
        n_tol = N_ABS + N_SCALE * float(np.abs(o[i]).sum() + np.abs(d[i] * md[i]).sum()) / ref.min_dim(code)
        assert np.all(np.abs(got["normal"][i] - n) <= n_tol), f"ray {i}: normal {got['normal'][i]} vs {n}"
        assert got["distance"][i] == np.float32(got["fraction"][i] * md[i])
        err_f = max(err_f, abs(gf - f) / max(f, 1e-6))
        err_p = max(err_p, float(np.max(np.abs(got["point"][i] - p) / (1.0 + np.abs(p)))))
        err_n = max(err_n, float(np.max(np.abs(got["normal"][i] - n))))
    assert checked >= 0.5 * len(o) and hits >= need_hits, (checked, hits)
    print(f"checked {checked} of {len(o)} rays, {hits} hits; max rel err f {err_f:.2e}, point {err_p:.2e}, normal {err_n:.2e}")
    return hits


def check_all_hits(ref, o, d, md, mask, got, allh):
    """All hits: per-ray sets in (f, code) order, offsets, and the first one is the closest hit (got: the closest hits of the
    same rays, or of a batch these rays begin)."""
    off = allh["offsets"].astype(np.int64)
    assert off[0] == 0 and np.all(np.diff(off) >= 0) and off[-1] == len(allh["kind"])
    for i in range(len(o)):
        want = ref.cast_all(o[i], d[i], md[i], mask[i])
        seg = slice(off[i], off[i + 1])
        if ref.clear(o[i], d[i], md[i], mask[i]):
            got_set = sorted(zip(allh["kind"][seg].tolist(), allh["entity"][seg].tolist()))
            assert got_set == sorted((h[2], h[3]) for h in want), f"ray {i}"
        fr = allh["fraction"][seg]
        assert np.all(np.diff(fr) >= 0)
        if off[i + 1] > off[i]:
            for k in ("kind", "entity", "fraction", "distance"):
                assert allh[k][off[i]] == got[k][i], (i, k)
            assert np.array_equal(allh["point"][off[i]], got["point"][i]) and np.array_equal(allh["normal"][off[i]], got["normal"][i])
        else:
            assert got["kind"][i] == RAY_MISS


def check_casts(ref, casts, got, need_hits=50):
    o, d, md, rad, mask = casts
    w64 = ref.w
    index_of = {int(c): i for i, c in enumerate(w64.code)}
    checked = hits = 0
    share_f = share_p = share_n = 0.0
    for i in range(len(o)):
        want, clear = ref.sweep_clear(o[i], d[i], md[i], rad[i], mask[i])
        if not clear:
            continue
        checked += 1
        if not want:
            assert got["kind"][i] == RAY_MISS and got["entity"][i] == NO_ENTITY, f"cast {i}: hit where the reference misses"
            continue
        f, code, kind, ent, n, p = want[0]
        assert (got["kind"][i], got["entity"][i]) == (kind, ent), f"cast {i}: {got['kind'][i]}/{got['entity'][i]} != {kind}/{ent}"
        hits += 1
        gf = float(got["fraction"][i])
        ef = abs(gf - f) / (F_REL * f + F_ABS)
        ep = float(np.max(np.abs(got["point"][i] - p) / (P_REL * (1.0 + np.abs(p)))))
        small = w64.min_dim(code)
        k = index_of.get(code)
        if k is not None and not w64.capsule[k] and np.count_nonzero(np.abs(w64.basis[k].T @ n) > 1e-6) > 1:
            small = min(small, float(rad[i]))  # an edge or a corner of a box
        n_tol = N_ABS + N_SCALE * float(np.abs(o[i]).sum() + np.abs(d[i] * md[i]).sum() + rad[i]) / small
        en = float(np.max(np.abs(got["normal"][i] - n))) / n_tol
        print_line = f"cast {i}: f {gf} vs {f}, point {got['point'][i]} vs {p}, normal {got['normal'][i]} vs {n}; shares {ef:.2f} {ep:.2f} {en:.2f}"
        assert ef <= 1.0 and ep <= 1.0 and en <= 1.0, print_line
        assert got["distance"][i] == np.float32(got["fraction"][i] * md[i])
        share_f, share_p, share_n = max(share_f, ef), max(share_p, ep), max(share_n, en)
    print(f"checked {checked} of {len(o)} casts, {hits} hits; worst share of tolerance: f {share_f:.2f}, point {share_p:.2f}, normal {share_n:.2f}")
    assert checked >= 0.5 * len(o) and hits >= need_hits, (checked, hits)
    return hits


def check_overlaps(ref, spheres, got, need_found=50):
    c, rad, mask = spheres
    off = got["offsets"].astype(np.int64)
    assert off[0] == 0 and np.all(np.diff(off) >= 0) and off[-1] == len(got["kind"])
    compared = found = 0
    share_d = 0.0
    for i in range(len(c)):
        want, clear = ref.overlap(c[i], rad[i], mask[i])
        if not clear:
            continue
        compared += 1
        seg = slice(off[i], off[i + 1])
        have = list(zip(got["kind"][seg].tolist(), got["entity"][seg].tolist()))
        assert have == [(h[1], h[2]) for h in want], f"sphere {i}: {have} vs {[(h[1], h[2]) for h in want]}"
        tol = P_REL * (1.0 + float(np.abs(c[i]).max()))
        for g, h in zip(got["distance"][seg], want):
            share_d = max(share_d, abs(float(g) - h[3]) / tol)
        found += len(want)
    print(f"compared {compared} of {len(c)} spheres, {found} objects; worst share of the distance tolerance {share_d:.2f}")
    assert share_d <= 1.0
    assert compared >= 0.9 * len(c) and found >= need_found, (compared, found)


def check_all_casts(ref, casts, got, allh):
    """All hits: per-cast sets in (f, code) order, offsets, and the first one is the closest hit (got: the closest hits of the
    same casts, or of a batch these casts begin).  At least half of the casts must be compared."""
    o, d, md, rad, mask = casts
    off = allh["offsets"].astype(np.int64)
    assert off[0] == 0 and np.all(np.diff(off) >= 0) and off[-1] == len(allh["kind"])
    compared = 0
    for i in range(len(o)):
        want, clear = ref.sweep_clear(o[i], d[i], md[i], rad[i], mask[i])
        seg = slice(off[i], off[i + 1])
        if clear:
            compared += 1
            got_set = sorted(zip(allh["kind"][seg].tolist(), allh["entity"][seg].tolist()))
            assert got_set == sorted((h[2], h[3]) for h in want), f"cast {i}"
        assert np.all(np.diff(allh["fraction"][seg]) >= 0)
        if off[i + 1] > off[i]:
            for k in ("kind", "entity", "fraction", "distance"):
                assert allh[k][off[i]] == got[k][i], (i, k)
            assert np.array_equal(allh["point"][off[i]], got["point"][i]) and np.array_equal(allh["normal"][off[i]], got["normal"][i])
        else:
            assert got["kind"][i] == RAY_MISS
    assert compared >= 0.5 * len(o)


FIELDS = ("position", "displacement", "radius", "skin", "probe_distance", "min_ground_ny", "layer_mask")


def device_caster(w):
    def cast_fn(casts):
        h = w.sphere_cast(casts["origin"], casts["direction"], casts["max_distance"], casts["radius"], casts["layer_mask"])
        hits = np.zeros(len(casts), W.RAY_HIT_DTYPE)
        for k, v in h.items():
            hits[k] = v
        return hits
    return cast_fn


def move(w, moves):
    return w.sphere_move(*(moves[k] for k in FIELDS))


RECOVER_FIELDS = ("position", "radius", "skin", "layer_mask")


def penetration(w, spheres):
    """World.sphere_penetration as a PENETRATION_HIT_DTYPE array; spheres: any records with center / position, radius, layer_mask."""
    centers = spheres["center"] if "center" in spheres.dtype.names else spheres["position"]
    h = w.sphere_penetration(centers, spheres["radius"], spheres["layer_mask"])
    hits = np.zeros(len(spheres), W.PENETRATION_HIT_DTYPE)
    for k, v in h.items():
        hits[k] = v
    return hits


def recover(w, recs):
    return w.sphere_recover(*(recs[k] for k in RECOVER_FIELDS))


def check_penetration_against_overlap(w, recs, pen, floors):
    """The penetration hits against the device's own overlap_sphere, exactly: a sphere is penetrated iff its overlap list is not
    empty, the winner is in that list, and outside a shape depth == float32(radius - distance) bit for bit.  floors = (penetrated
    spheres, winners with the centre outside the shape) the batch must show."""
    ov = w.overlap_sphere(recs["position"], recs["radius"], recs["layer_mask"])
    off = ov["offsets"].astype(np.int64)
    n_hit = n_outside = 0
    for i in range(len(recs)):
        seg = slice(off[i], off[i + 1])
        listed = list(zip(ov["kind"][seg].tolist(), ov["entity"][seg].tolist()))
        if not listed:
            assert pen[i].tobytes() == np.array([(RAY_MISS, NO_ENTITY, 0, (0, 0, 0), (0, 0, 0), 0)], W.PENETRATION_HIT_DTYPE)[0].tobytes(), i
            continue
        n_hit += 1
        assert (int(pen["kind"][i]), int(pen["entity"][i])) in listed, (i, pen[i], listed)
        assert pen["depth"][i] >= 0 and pen["reserved"][i] == 0
        r = recs["radius"][i]
        for (kind, ent), dist in zip(listed, ov["distance"][seg]):
            if dist > 0:  # outside the shape the signed distance is this distance: no object reaches deeper than the winner
                depth = np.float32(r - dist)
                assert depth <= pen["depth"][i], (i, kind, ent)
                if (kind, ent) == (pen["kind"][i], pen["entity"][i]):
                    n_outside += 1
                    assert depth.tobytes() == pen["depth"][i].tobytes(), (i, depth, pen["depth"][i])
            else:  # inside it, or on its surface: at least the radius deep
                assert pen["depth"][i] >= r or (kind, ent) != (pen["kind"][i], pen["entity"][i]), i
    print(f"{n_hit} of {len(recs)} spheres penetrated, {n_outside} winners with the centre outside the shape")
    assert n_hit >= floors[0] and n_outside >= floors[1], (n_hit, n_outside, floors)


def ask(w, batches):
    """The five answers to a phase's batches; the device forms of the two closest-hit queries must equal the host forms."""
    import torch
    (o, d, md, mask), (co, cd, cmd, crad, cmask), spheres = batches
    ans = dict(ray=w.raycast(o, d, md, mask), ray_all=w.raycast_all(o, d, md, mask), cast=w.sphere_cast(co, cd, cmd, crad, cmask),
               cast_all=w.sphere_cast_all(co, cd, cmd, crad, cmask), overlap=w.overlap_sphere(*spheres))
    for name, records, fn in (("ray", W.make_rays(o, d, md, mask), w.raycast_device),
                              ("cast", W.make_sphere_casts(co, cd, cmd, crad, cmask), w.sphere_cast_device)):
        rt = torch.from_numpy(records.view(np.uint8)).to("cuda:0")
        ht = torch.zeros(len(records) * 40, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        fn(rt, ht)
        w.sync()
        hd = ht.cpu().numpy().view(W.RAY_HIT_DTYPE)
        for k, v in ans[name].items():
            assert np.ascontiguousarray(hd[k]).tobytes() == v.tobytes(), (name, k)
    return ans
