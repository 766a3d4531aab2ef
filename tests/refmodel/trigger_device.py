"""A case of refmodel/trigger_cases.py on a World: what opens it, applies a tick's edits and steps it.  The comparison with the
oracle is test_gpu_trigger_paths.py's."""
from __future__ import annotations

import numpy as np

import banggameengine_amd as B
from banggameengine_amd.world import FIXED_DT

from . import trigger_cases as tc

FLAGS = B.TICK_ALL | B.TICK_BROADPHASE


def upload_triggers(w, trig):
    w.upload_triggers(trig.entity, None, trig.size, trig.layer, trig.mask, None, trig.active)


def open_world(case, stay=True):
    """A World with the case's scene and volumes in it (set the case's environment BEFORE: bge_world_create reads it)."""
    w = B.World()
    w.set_topology(case.parent, case.has_transform)
    w.upload_trs(case.pos, case.euler, case.scale)
    w.upload_bodies(case.body_type, size=case.size, layer=case.layer, mask=case.mask)
    upload_triggers(w, case.trig)
    if not stay:
        w.set_trigger_stay_events(False)
    return w


def apply_edits(case, tick, w):
    for ed in case.ticks[tick].edits:
        if ed[0] == "move":
            first, pos = int(ed[1]), np.asarray(ed[2], np.float32)
            w.upload_trs_indexed(np.arange(first, first + len(pos), dtype=np.uint32), pos=pos)
        elif ed[0] == "triggers":
            upload_triggers(w, ed[1])
        elif ed[0] == "topology":
            w.set_topology(ed[1], ed[2])
        else:
            raise ValueError(ed[0])


def step(case, tick, w):
    """The tick itself; the sub-steps it ran.  A tick of route 'E' raises BgeError."""
    if case.accumulate:
        return w.step_simulation(tc.dt_of(case, tick), 4, FIXED_DT, flags=FLAGS)
    w.tick(dt=FIXED_DT, flags=FLAGS)
    return 1
