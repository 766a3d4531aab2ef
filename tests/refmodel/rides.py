"""The reference of character platform riding (include/bge_world.h "Character platform riding"): carry_ref and anchor_ref, the
header's rule in numpy float32 scalars (written from the header, not from the kernel), and ride_run_ref, one
bge_world_characters_update call with riding on: Carry, run_ref, Anchor.

The bodies come in as a Poses: per entity index the body's type where it is present (BODY_NONE where it is not), its position and
its quaternion (xyzw), all as that call sees them.  On the CPU they are made from the bodies of a World64; on the GPU from
World.download_pose and World.download_bodies, so the same code runs over both."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .characters import GROUNDED, run_ref
from .moves import F
from .rays import NO_ENTITY, RAY_BODY

BODY_STATIC, BODY_DYNAMIC, BODY_KINEMATIC, BODY_NONE = 0, 1, 2, 255
RIDE_ON, RIDE_DYNAMIC = 1, 2
CARRIED, LOST = 1, 2
RIDE_DTYPE = np.dtype([("flags", "<u4"), ("entity", "<u4"), ("anchor_position", "<f4", (3,)), ("anchor_rotation", "<f4", (4,)),
                       ("carried", "<f4", (3,)), ("turn", "<f4", (4,))])


@dataclass
class Poses:
    type: np.ndarray      # (entities,) uint8: the body's type where it is present, BODY_NONE where it is not
    position: np.ndarray  # (entities, 3) float32
    rotation: np.ndarray  # (entities, 4) float32, xyzw

    def __post_init__(self):
        self.type = np.asarray(self.type, np.uint8)
        self.position = np.ascontiguousarray(self.position, np.float32).reshape(-1, 3)
        self.rotation = np.ascontiguousarray(self.rotation, np.float32).reshape(-1, 4)
        assert len(self.type) == len(self.position) == len(self.rotation)

    def rideable(self, entity, dynamic):
        if entity == NO_ENTITY or entity >= len(self.type) or self.type[entity] == BODY_NONE:
            return False
        return self.type[entity] in (BODY_STATIC, BODY_KINEMATIC) or (dynamic and self.type[entity] == BODY_DYNAMIC)

    def words(self, entity):
        """The 7 words of the pose."""
        return np.concatenate([self.position[entity], self.rotation[entity]]).astype(np.float32)


def fresh_rides(n):
    """What bge_world_characters_ride leaves when it switches riding on: no anchor."""
    rides = np.zeros(n, RIDE_DTYPE)
    rides["entity"] = NO_ENTITY
    rides["turn"][:, 3] = 1
    return rides


def conj(q):
    return (-q[0], -q[1], -q[2], q[3])


def rot(q, v):
    qx, qy, qz, qw = (F(c) for c in q)
    vx, vy, vz = (F(c) for c in v)
    two = F(2)
    tx = (qy * vz - qz * vy) * two
    ty = (qz * vx - qx * vz) * two
    tz = (qx * vy - qy * vx) * two
    return ((vx + qw * tx) + (qy * tz - qz * ty), (vy + qw * ty) + (qz * tx - qx * tz), (vz + qw * tz) + (qx * ty - qy * tx))


def mul(p, q):
    px, py, pz, pw = (F(c) for c in p)
    qx, qy, qz, qw = (F(c) for c in q)
    return (((pw * qx + px * qw) + py * qz) - pz * qy, ((pw * qy + py * qw) + pz * qx) - px * qz, ((pw * qz + pz * qw) + px * qy) - py * qx,
            ((pw * qw - px * qx) - py * qy) - pz * qz)


def carry_ref(state, rides, poses, dynamic=False):
    """Carry for every character: (the states with the carried positions, the records with flags, carried and turn of this call)."""
    state, rides = state.copy(), rides.copy()
    with np.errstate(all="ignore"):
        for i in range(len(state)):
            r = rides[i]
            r["flags"], r["carried"], r["turn"] = 0, 0, (0, 0, 0, 1)
            e = int(r["entity"])
            if not (state["flags"][i] & GROUNDED) or e == NO_ENTITY:
                continue
            if not poses.rideable(e, dynamic):
                r["flags"] = LOST
                continue
            anchor = np.concatenate([r["anchor_position"], r["anchor_rotation"]]).astype(np.float32)
            cur = poses.words(e)
            if anchor.tobytes() == cur.tobytes():
                continue
            p = [F(c) for c in state["position"][i]]
            a_p, a_q, c_p, c_q = anchor[:3], anchor[3:], cur[:3], cur[3:]
            local = rot(conj(a_q), (p[0] - F(a_p[0]), p[1] - F(a_p[1]), p[2] - F(a_p[2])))
            m = rot(c_q, local)
            t = [F(c_p[k]) + m[k] for k in range(3)]
            if not all(np.isfinite(c) for c in t):
                r["flags"] = LOST
                continue
            r["carried"] = [t[k] - p[k] for k in range(3)]
            r["turn"] = mul(c_q, conj(a_q))
            r["flags"] = CARRIED
            state["position"][i] = t
    return state, rides


def anchor_ref(state, rides, poses, dynamic=False):
    """Anchor for every character: the records with the anchor of the next call."""
    rides = rides.copy()
    for i in range(len(state)):
        r = rides[i]
        e = int(state["ground_entity"][i])
        if (state["flags"][i] & GROUNDED) and state["ground_kind"][i] == RAY_BODY and poses.rideable(e, dynamic):
            r["entity"], r["anchor_position"], r["anchor_rotation"] = e, poses.position[e], poses.rotation[e]
        else:
            r["entity"], r["anchor_position"], r["anchor_rotation"] = NO_ENTITY, 0, 0
    return rides


def ride_run_ref(cast_fn, pen_fn, descs, inputs, state, rides, poses, dt, steps, dynamic=False, history=None, **batches):
    """One bge_world_characters_update(dt, steps) with riding on, over the world whose bodies are `poses`: (state, rides)."""
    state, rides = carry_ref(state, rides, poses, dynamic)
    state = run_ref(cast_fn, pen_fn, descs, inputs, state, dt, steps, history, **batches)
    return state, anchor_ref(state, rides, poses, dynamic)
