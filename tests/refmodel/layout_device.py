"""The GPU side of the layout comparisons: LayoutScene, the ray tests' scene under the layout topology with the book-keeping of what
is in the world through its edit history, and the checks every answer on it goes through: check_members (every entity reported is
in the world), compare (the float64 references on what is in the world), answer_bytes (what a re-layout may not change)."""
from __future__ import annotations

import ctypes as C

import numpy as np

import banggameengine_amd as B
from banggameengine_amd import world as W

from .rays import RAY_BODY, RAY_MISS
from .spheres import SphereRef
from .layout_cases import (N, N_GROWN, N_TRIGGERS, SCENE_SEED, check_members, layout_topology, penetration_batches, query_batches,
                           scene_reference)
from .device import Scene, ask, check_against_reference, check_all_casts, check_all_hits, check_casts, check_overlaps

N_ALL = 256  # the all-hits lists are compared for the first 256 queries of a batch, as the flat-scene tests do


class LayoutScene(Scene):
    """The ray tests' scene under the layout topology, with the book-keeping of what is in the world."""

    def __init__(self):
        _, _, trig = scene_reference()
        self.parent, self.ht = layout_topology(N, trig)
        super().__init__(N, np.random.default_rng(SCENE_SEED), n_triggers=N_TRIGGERS, parent=self.parent, has_transform=self.ht)
        assert np.array_equal(np.sort(self.trig), trig), "the scene's draws are no longer those scene_world64 repeats"
        self.fresh = np.zeros(N, bool)  # body uploaded since the last physics tick
        self.posed = False              # a tick has posed the ghosts since the last upload_triggers
        info = self.w.info()
        slot, _, _, flat = W.flatten_topology(self.parent, self.ht)
        has = self.ht.astype(bool)
        print(f"layout: {flat['n_transforms']} transforms in {flat['n_slots']} slots, {int((slot[has] != np.arange(N)[has]).sum())} entities "
              f"off their index, largest slot {int(slot[has].max())}, depth {flat['max_depth']}")
        assert info["n_slots"] == flat["n_slots"] > info["n_transforms"] and slot[has].max() >= N

    def upload_triggers(self):
        super().upload_triggers()
        self.posed = False

    def tick(self, k=1):
        super().tick(k)
        self.fresh[:] = False
        self.posed = True

    def set_topology(self, parent, ht):
        self.w.set_topology(parent, ht)
        self.parent, self.ht = parent, ht

    def bodies_in_world(self):
        return np.nonzero(self.ht.astype(bool) & (self.type != W.BODY_NONE) & ~self.fresh)[0]

    def ghosts_in_world(self):
        if not self.posed:
            return self.trig[:0]
        return self.trig[self.t_active.astype(bool) & self.w.trigger_active(self.trig)]

    def members(self):
        return np.sort(np.concatenate([self.bodies_in_world(), self.ghosts_in_world()]))

    def batches(self, phase):
        pos, _ = self.w.download_pose()
        return query_batches(phase, pos[self.members()])

    def spheres(self, phase):
        """The recover records of a phase, drawn around the device's positions of the bodies and the ghosts in the world."""
        pos, _ = self.w.download_pose()
        return penetration_batches(phase, pos[self.bodies_in_world()], pos[np.sort(self.ghosts_in_world())])

    def remove(self, ents):
        """BODY_NONE for the listed entities: they leave the world at once."""
        idx, none = np.ascontiguousarray(ents, np.uint32), np.full(len(ents), W.BODY_NONE, np.uint8)
        rc = B.lib().bge_world_upload_bodies_indexed(self.w._h, len(idx), idx.ctypes.data_as(C.c_void_p), none.ctypes.data_as(C.c_void_p),
                                                     None, None, None, None, None)
        assert rc == 0
        self.type[idx] = W.BODY_NONE

    def grow(self, ed):
        """Entities N .. N_GROWN - 1 with TRS and bodies: in the world after the next tick."""
        self.set_topology(ed.parent_grown, ed.has_transform_grown)
        self.w.upload_trs(ed.pos, ed.euler, np.ones((len(ed.pos), 3)), first=N)
        self.w.upload_bodies(ed.type, None, ed.shape, ed.size, ed.layer, ed.mask, first=N)
        for k in ("type", "shape", "size", "layer", "mask"):
            setattr(self, k, np.concatenate([getattr(self, k), getattr(ed, k)]))
        self.fresh = np.concatenate([self.fresh, np.ones(len(ed.pos), bool)])
        self.n = N_GROWN

    def drop_above(self, n):
        """What the header asks of a caller that drops entities: their triggers leave the uploaded set and their bodies are removed
        before the call."""
        keep = self.trig < n
        self.trig, self.t_active, self.t_oneshot = self.trig[keep], self.t_active[keep], self.t_oneshot[keep]
        self.upload_triggers()
        self.w.upload_bodies(np.full(self.n - n, W.BODY_NONE, np.uint8), first=n)
        self.type[n:] = W.BODY_NONE

    def shrink(self, n, ed):
        self.set_topology(ed.parent_shrunk, ed.has_transform_shrunk)
        for k in ("type", "shape", "size", "layer", "mask", "fresh"):
            setattr(self, k, getattr(self, k)[:n])
        self.n = n


def answer_bytes(answer):
    return {k: np.ascontiguousarray(v).tobytes() for k, v in answer.items()}


def head(allh, k):
    """The all-hits answer of the first k queries of a batch."""
    end = int(allh["offsets"][k])
    out = {key: v[:end] for key, v in allh.items() if key != "offsets"}
    out["offsets"] = allh["offsets"][:k + 1]
    return out


def compare(sc, batches, kind, ans=None):
    """The answers to a phase's batches against the float64 references on what is in the world."""
    ans = ask(sc.w, batches) if ans is None else ans
    check_members(sc, ans)
    ref = sc.objects()
    rays, casts, spheres = batches
    if kind == "rays":
        check_against_reference(ref, *rays, ans["ray"])
        assert (ans["ray"]["kind"] == RAY_BODY).any() and (ans["ray"]["kind"] == RAY_MISS).any()
        check_all_hits(ref, *(a[:N_ALL] for a in rays), ans["ray"], head(ans["ray_all"], N_ALL))
    else:
        sref = SphereRef(ref)
        check_casts(sref, casts, ans["cast"])
        assert (ans["cast"]["kind"] == RAY_BODY).any() and (ans["cast"]["kind"] == RAY_MISS).any()
        check_all_casts(sref, tuple(a[:N_ALL] for a in casts), ans["cast"], head(ans["cast_all"], N_ALL))
        check_overlaps(sref, spheres, ans["overlap"])
    return ans
