"""The GPU side of the character-trigger comparisons: a world whose entities are trigger rows (BODY_NONE with a Transform, as
refmodel/step_device.py makes its ghosts), ticked once so that the ghosts are posed, and a walk driven call by call with the
device's list, positions and remembered pairs kept after every call."""
from __future__ import annotations

import numpy as np

import banggameengine_amd as B
from banggameengine_amd import world as W

from .device import FLAGS
from .char_trigger_cases import DT, N_CALLS, STEPS_PER_CALL


def upload_walk_triggers(w, walk, order, active=None, mask=None):
    """The triggers order[k] of the walk, in that order of the uploaded array."""
    order = np.asarray(order, np.int64)
    k = len(order)
    w.upload_triggers(walk.entity[order], np.zeros(k, np.uint8), walk.size[order], walk.layer[order], (walk.mask if mask is None else mask)[order],
                      np.zeros(k, np.uint8), np.ones(k, np.uint8) if active is None else np.asarray(active, np.uint8), keep_order=True)


def trigger_world(walk, n_triggers=None, topology=None):
    """A World with one entity per trigger of the walk, no bodies and no plane; the first n_triggers (all by default) are uploaded as
    triggers in entity order, and one BGE_TICK_BROADPHASE tick poses them.  topology = (parent, has_transform) makes it a world of
    len(parent) entities under that hierarchy instead of a flat one: the entities beyond the walk's are BODY_NONE with the identity
    TRS.  The caller closes it."""
    T = len(walk.entity)
    n = T if topology is None else len(topology[0])
    assert n >= T
    pad = n - T
    w = B.World(device=0)
    try:
        if topology is None:
            w.set_topology(np.full(T, W.NO_PARENT, np.uint32))
        else:
            w.set_topology(*topology)
        w.upload_trs(np.concatenate([walk.pos, np.zeros((pad, 3), np.float32)]), np.concatenate([walk.euler, np.zeros((pad, 3), np.float32)]),
                     np.ones((n, 3)))
        w.upload_bodies(np.full(n, W.BODY_NONE, np.uint8), None, np.zeros(n, np.uint8), np.concatenate([walk.size, np.full((pad, 3), 0.5, np.float32)]),
                        np.full(n, 1, np.uint32), np.full(n, 0xFFFFFFFF, np.uint32))
        upload_walk_triggers(w, walk, np.arange(T if n_triggers is None else n_triggers))
        w.set_ground_plane(False)
        w.tick(flags=FLAGS)
    except Exception:
        w.close()
        raise
    return w


def one_call(w, walk, call, n):
    """Update call `call` of the walk: (events, positions, remembered pairs) as the device has them afterwards."""
    w.characters_set_input(walk.inputs(call, n))
    w.characters_update(DT, STEPS_PER_CALL)
    return w.characters_trigger_events(), w.characters_state()["position"].copy(), w.characters_trigger_overlaps()


def run_walk(w, walk, n, stay=True, event_capacity=0, calls=N_CALLS, watch=True):
    """Creates the first n characters, turns the watch on with the walk's filters and runs the calls: [(events, positions, pairs)]."""
    w.characters_create(walk.descs[:n])
    if watch:
        w.characters_watch_triggers(walk.group[:n], walk.cmask[:n], stay, event_capacity)
    return [one_call(w, walk, call, n) for call in range(calls)]
