"""The reference of the characters (include/bge_world.h "Characters"): char_ref, one step of the header's rule in numpy float32
scalars (written from the header, not from the kernel), composed from recover_ref and step_ref over the penetration function and the
caster handed in; run_ref, several steps of it as bge_world_characters_update runs them; and fresh_state, what
bge_world_characters_create leaves.  char_ref takes the two batches as functions too, so that the same arithmetic can be run over
the public World.sphere_recover / World.sphere_step_move."""
from __future__ import annotations

import numpy as np

from .records import MOVE_GROUNDED, MOVE_INVALID, MOVE_OUT_OF_SLIDES, RECOVER_INVALID, RECOVER_MOVED, RECOVER_STUCK
from .rays import NO_ENTITY, RAY_MISS
from .moves import F
from .recover import recover_ref
from .step_moves import STEP_MOVE_DTYPE, STEPPED, step_ref

INVALID, GROUNDED, JUMPED, LANDED, HEAD_BUMP, RECOVERED, STUCK, CHAR_STEPPED, OUT_OF_SLIDES = 1, 2, 4, 8, 16, 32, 64, 128, 256
BUTTON_JUMP = 1
DESC_DTYPE = np.dtype([("position", "<f4", (3,)), ("radius", "<f4"), ("skin", "<f4"), ("step_height", "<f4"), ("min_ground_ny", "<f4"),
                       ("probe_distance", "<f4"), ("gravity", "<f4"), ("jump_speed", "<f4"), ("fall_speed", "<f4"), ("layer_mask", "<u4")])
INPUT_DTYPE = np.dtype([("walk_x", "<f4"), ("walk_z", "<f4"), ("buttons", "<u4"), ("reserved", "<u4")])
STATE_DTYPE = np.dtype([("position", "<f4", (3,)), ("vertical_velocity", "<f4"), ("flags", "<u4"), ("ground_kind", "<u4"),
                        ("ground_entity", "<u4"), ("ground_normal", "<f4", (3,)), ("hit_kind", "<u4"), ("hit_entity", "<u4"),
                        ("hit_normal", "<f4", (3,)), ("step_rise", "<f4"), ("recovered", "<f4", (3,)), ("steps", "<u4")])
RECOVER_DTYPE = np.dtype([("position", "<f4", (3,)), ("radius", "<f4"), ("skin", "<f4"), ("layer_mask", "<u4"), ("reserved", "<u4")])


def fresh_state(descs):
    """What bge_world_characters_create leaves: at the desc's position, not grounded, at rest, steps 0."""
    state = np.zeros(len(descs), STATE_DTYPE)
    state["position"] = descs["position"]
    state["ground_entity"] = state["hit_entity"] = NO_ENTITY
    return state


def char_ref(cast_fn, pen_fn, descs, inputs, state, dt, first_step, recover_fn=None, step_fn=None):
    """One step of the rule for every character: the new states (STATE_DTYPE).  inputs is changed as the step changes it: the
    first step of a call clears the JUMP edge.  recover_fn(records) / step_fn(moves) are the two batches (recover_ref over pen_fn
    and step_ref over cast_fn if None)."""
    if recover_fn is None:
        recover_fn = lambda rec: recover_ref(pen_fn, rec)  # noqa: E731
    if step_fn is None:
        step_fn = lambda mv: step_ref(cast_fn, mv)  # noqa: E731
    n = len(descs)
    dt = F(dt)
    out = state.copy()
    with np.errstate(all="ignore"):
        # Input
        invalid = [not (np.isfinite(inputs["walk_x"][i]) and np.isfinite(inputs["walk_z"][i])) for i in range(n)]
        jump = [False] * n
        if first_step:
            jump = [bool(b & BUTTON_JUMP) for b in inputs["buttons"]]
            inputs["buttons"] &= ~np.uint32(BUTTON_JUMP)
        # Recover (an invalid character hands a record that asks nothing)
        rec = np.zeros(n, RECOVER_DTYPE)
        rec["position"], rec["radius"], rec["skin"] = state["position"], descs["radius"], descs["skin"]
        rec["layer_mask"] = np.where(invalid, 0, descs["layer_mask"])
        R = recover_fn(rec)
        invalid = [bool(invalid[i] or (R["flags"][i] & RECOVER_INVALID)) for i in range(n)]
        # Vertical
        mv = np.zeros(n, STEP_MOVE_DTYPE)
        vv, was, jumped = [None] * n, [None] * n, [None] * n
        for i in range(n):
            d = descs[i]
            was[i] = bool(state["flags"][i] & GROUNDED)
            jumped[i] = jump[i] and was[i]
            v, dy, walking = F(state["vertical_velocity"][i]), F(0), False
            if jumped[i]:
                v = F(d["jump_speed"])
            elif was[i]:
                v, walking = F(0), True
            if not walking:
                v = v - F(d["gravity"]) * dt
                if v > F(d["jump_speed"]):
                    v = F(d["jump_speed"])
                if v < -F(d["fall_speed"]):
                    v = -F(d["fall_speed"])
                dy = v * dt
            vv[i] = v
            mv[i] = (R["position"][i], (inputs["walk_x"][i], dy, inputs["walk_z"][i]), d["radius"], d["skin"], d["probe_distance"], d["min_ground_ny"],
                     0 if invalid[i] else d["layer_mask"], d["step_height"] if walking else 0)
        # Move
        M = step_fn(mv)
        for i in range(n):
            o = out[i]
            o["steps"] = state["steps"][i] + np.uint32(1)
            if invalid[i] or (M["flags"][i] & MOVE_INVALID):
                o["flags"] = INVALID | (state["flags"][i] & GROUNDED)
                o["ground_kind"] = o["hit_kind"] = RAY_MISS
                o["ground_entity"] = o["hit_entity"] = NO_ENTITY
                o["ground_normal"] = o["hit_normal"] = o["recovered"] = 0
                o["step_rise"] = 0
                continue
            m, v = M[i], vv[i]
            q = [F(m["position"][0]), F(m["position"][1]), F(m["position"][2])]
            flags = (JUMPED if jumped[i] else 0) | (RECOVERED if R["flags"][i] & RECOVER_MOVED else 0) | (STUCK if R["flags"][i] & RECOVER_STUCK else 0)
            flags |= (CHAR_STEPPED if m["flags"] & STEPPED else 0) | (OUT_OF_SLIDES if m["flags"] & MOVE_OUT_OF_SLIDES else 0)
            # Ground
            if (m["flags"] & MOVE_GROUNDED) and not v > 0:
                e = F(m["ground_distance"]) - F(descs["skin"][i])
                if not e > 0:
                    e = F(0)
                q[1] = q[1] - e
                v = F(0)
                flags |= GROUNDED | (0 if was[i] else LANDED)
            # Head
            if v > 0 and m["n_hits"] >= 1 and F(m["hit_normal"][1]) < 0:
                v = F(0)
                flags |= HEAD_BUMP
            o["position"], o["vertical_velocity"], o["flags"] = q, v, flags
            o["ground_kind"], o["ground_entity"], o["ground_normal"] = m["ground_kind"], m["ground_entity"], m["ground_normal"]
            o["hit_kind"], o["hit_entity"], o["hit_normal"], o["step_rise"] = m["hit_kind"], m["hit_entity"], m["hit_normal"], m["step_rise"]
            o["recovered"] = R["pushed"][i]
    return out


def run_ref(cast_fn, pen_fn, descs, inputs, state, dt, steps, history=None, **batches):
    """One bge_world_characters_update(dt, steps): the state after it; history, if a list, gets the state after every step."""
    for k in range(steps):
        state = char_ref(cast_fn, pen_fn, descs, inputs, state, dt, k == 0, **batches)
        if history is not None:
            history.append(state)
    return state
