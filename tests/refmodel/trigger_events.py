"""ProcessTriggerEvents in plain numpy (oracle/physics_ref.h states the rule; include/bge_world.h "Trigger volumes" the contract):
a remembered set per trigger, the triggers walked in uploaded order, per trigger Enter / Stay over the current set in ascending
entity order and then Exit, an entity met as a body and as a ghost counted once, the trigger's own entity never, a one-shot volume
that fires out of the world at once — so that a trigger walked LATER in the same tick no longer lists it.

The model is fed the overlap sets, it computes none: {trigger entity: (bodies, ghosts)} per tick, as a broadphase would hand them
over BEFORE the loop runs (a ghost may still list itself there, an entity may stand in both lists, a one-shot that is about to fire
is still in the others' lists).  It exists for what the oracle cannot do: a tick that FAILS (skip_tick) reports nothing and leaves
every remembered set as it was; the next tick is diffed against those sets."""
from __future__ import annotations

import numpy as np

ENTER, STAY, EXIT = 0, 1, 2
DEFAULT_LAYER = 4
_EMPTY = np.zeros(0, np.int64)


class TriggerModel:
    def __init__(self):
        self.order = []        # trigger entities, uploaded order
        self.volume = {}       # entity -> dict(layer, mask, one_shot, active)
        self.sets = {}         # entity -> ascending int64 array: the remembered overlaps

    def upload(self, entity, layer=None, mask=None, one_shot=None, active=None):
        """bge_world_upload_triggers: the whole set again.  A volume that was there keeps its remembered set unless layer or mask
        changed or it is (de)activated; everybody else starts empty."""
        entity = [int(e) for e in entity]
        n = len(entity)
        pick = lambda a, k, d: d if a is None else a[k]
        volume, sets = {}, {}
        for k, e in enumerate(entity):
            v = dict(layer=int(pick(layer, k, 0)) or DEFAULT_LAYER, mask=int(pick(mask, k, 0xFFFFFFFF)), one_shot=bool(pick(one_shot, k, False)),
                     active=bool(pick(active, k, True)))
            old = self.volume.get(e)
            keep = old is not None and old["layer"] == v["layer"] and old["mask"] == v["mask"] and old["active"] and v["active"]
            volume[e] = v
            sets[e] = self.sets[e] if keep else _EMPTY
        assert len(volume) == n, "an entity carries two triggers"
        self.order, self.volume, self.sets = entity, volume, sets

    def active(self, entity):
        return np.array([self.volume[int(e)]["active"] if int(e) in self.volume else False for e in entity], bool)

    def skip_tick(self):
        """A tick that failed: no event, every remembered set as it was."""
        return np.zeros((0, 3), np.uint32)

    def process(self, overlaps):
        """One tick.  overlaps: {trigger entity: (bodies, ghosts)} (a missing trigger overlaps nothing).  Returns the events in the
        order the loop reports them, (type, trigger, other) rows."""
        out = []
        for t in self.order:
            v = self.volume[t]
            if not v["active"]:
                continue
            bodies, ghosts = overlaps.get(t, (_EMPTY, _EMPTY))
            bodies = np.asarray(bodies, np.int64).ravel()
            ghosts = np.asarray(ghosts, np.int64).ravel()
            # a ghost that has left the world since the lists were made (a one-shot that fired earlier in this loop) no longer counts
            ghosts = np.array([g for g in ghosts.tolist() if g in self.volume and self.volume[g]["active"]], np.int64)
            cur = np.union1d(bodies, ghosts)                                      # (sorted, unique: met both ways counts once)
            cur = cur[cur != t]                                                   # (never itself)
            prev = self.sets[t]
            was = np.isin(cur, prev, assume_unique=True)
            rows = [np.stack([np.where(was, STAY, ENTER), np.full(len(cur), t), cur], 1)]
            gone = prev[~np.isin(prev, cur, assume_unique=True)]
            rows.append(np.stack([np.full(len(gone), EXIT), np.full(len(gone), t), gone], 1))
            out.extend(rows)
            self.sets[t] = cur
            if v["one_shot"] and len(cur):
                v["active"] = False
                self.sets[t] = _EMPTY
        return np.concatenate(out).astype(np.uint32) if out else np.zeros((0, 3), np.uint32)


def sort_events(ev):
    """The order World.trigger_events and RefScene.TriggerEvents hand events out in: by type, trigger, other."""
    ev = np.asarray(ev, np.uint32).reshape(-1, 3)
    return ev[np.lexsort((ev[:, 2], ev[:, 1], ev[:, 0]))] if len(ev) else ev


def overlaps_of_events(ev):
    """{trigger: (others, ())}: the current sets a tick's Enter and Stay rows state."""
    ev = np.asarray(ev).reshape(-1, 3)
    now = ev[ev[:, 0] != EXIT]
    out = {}
    if len(now):
        order = np.argsort(now[:, 1], kind="stable")
        now = now[order]
        trig, first = np.unique(now[:, 1], return_index=True)
        for t, chunk in zip(trig.tolist(), np.split(now[:, 2], first[1:])):
            out[int(t)] = (chunk.astype(np.int64), _EMPTY)
    return out
