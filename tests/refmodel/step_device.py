"""The GPU side of the step-move comparisons: worlds made of Static bodies and trigger ghosts given one by one (the hand-worked
cases, the step field of refmodel/step_cases.py), ticked once, and the device calls in the forms step_ref and compose_ref expect."""
from __future__ import annotations

import numpy as np

import banggameengine_amd as B
from banggameengine_amd import world as W

from .rays import ALL
from .device import FIELDS, FLAGS

STEP_FIELDS = FIELDS + ("step_height",)


def static_world(capsule, size, pos, euler, ghosts, plane=True):
    """A World of Static bodies (entity i = row i; layer 1, seen by every mask), the rows of `ghosts` trigger ghosts instead,
    ticked once so that the queries see it.  The caller closes it."""
    n = max(len(pos), 1)
    empty = len(pos) == 0
    w = B.World(device=0)
    try:
        w.set_topology(np.full(n, W.NO_PARENT, np.uint32))
        w.upload_trs(np.float32([[0, 0, 0]] if empty else pos), np.float32([[0, 0, 0]] if empty else euler), np.ones((n, 3)))
        types = np.full(n, W.BODY_NONE if empty else W.BODY_STATIC, np.uint8)
        types[list(ghosts)] = W.BODY_NONE
        shapes = np.uint8([0] if empty else capsule)
        sizes = np.float32([[0.5, 0.5, 0.5]] if empty else size)
        w.upload_bodies(types, None, shapes, sizes, np.full(n, 1, np.uint32), np.full(n, ALL, np.uint32))
        if len(ghosts):
            g = np.uint32(list(ghosts))
            w.upload_triggers(g, shapes[g], sizes[g], np.full(len(g), 1, np.uint32), np.full(len(g), ALL, np.uint32), np.zeros(len(g), np.uint8),
                              np.ones(len(g), np.uint8))
        w.set_ground_plane(plane)
        w.tick(flags=FLAGS)
    except Exception:
        w.close()
        raise
    return w


def hand_world(bodies, ghosts, plane):
    return static_world([b[0] for b in bodies], [b[1] for b in bodies], [b[2] for b in bodies], [b[3] for b in bodies], ghosts, plane)


def field_world(field):
    return static_world(field.capsule, field.size, field.pos, field.euler, field.ghosts)


def step_move(w, moves):
    return w.sphere_step_move(*(moves[k] for k in STEP_FIELDS))


def device_mover(w):
    """The plain move of compose_ref: bge_sphere_move records -> World.sphere_move's results."""
    return lambda plain: w.sphere_move(*(plain[k] for k in FIELDS))
