"""The GPU side of the impulse comparisons: the scene of refmodel/impulse_cases.py as a World (flat, or embedded in a hierarchy
that shuffles its slots), brought into the mixed activation state the scene asks for, and the device's state as the Bodies image
apply_ref works on."""
from __future__ import annotations

import numpy as np

import banggameengine_amd as B
from banggameengine_amd import world as W

from .impulse_cases import N_OWN, SHUFFLE_PAD
from .impulses import BODY_DYNAMIC, Bodies

F = np.float32
DT = float(F(1.0 / 60.0))
NO_GRAVITY = (0.0, 0.0, 0.0)
SLEEP_SECONDS = 0.1  # six ticks of DT


def scene_world(scene, shuffled=False):
    """The scene's entities 0 .. N_OWN - 1 (with SHUFFLE_PAD body-less entities after them when shuffled), no plane, no gravity,
    prepared.  The caller closes it."""
    w = B.World(device=0)
    try:
        if shuffled:
            from .layout_cases import embedded_topology
            parent, has_transform = embedded_topology(N_OWN, SHUFFLE_PAD)
            w.set_topology(parent, has_transform)
        else:
            w.set_topology(np.full(scene.n, W.NO_PARENT, np.uint32))
        w.set_sleeping(0.8, 1.0, SLEEP_SECONDS)
        prepare(w, scene)
    except Exception:
        w.close()
        raise
    return w


def prepare(w, scene):
    """(Re)creates every body where the scene has it and brings the world into the state the scene's groups stand for: ten ticks
    with the groups' velocities put group 0 to sleep; group 1 then slows down and runs its timer for two ticks.  The same calls
    give the same bytes every time."""
    n, total = scene.n, w.n
    pad = total - n
    w.upload_trs(np.concatenate([scene.pos, np.zeros((pad, 3), F)]), np.concatenate([scene.euler, np.zeros((pad, 3), F)]), np.ones((total, 3), F))
    types = np.concatenate([scene.types, np.full(pad, W.BODY_NONE, np.uint8)])
    w.upload_bodies(types, np.concatenate([scene.mass, np.ones(pad, F)]), np.concatenate([scene.capsule.astype(np.uint8), np.zeros(pad, np.uint8)]),
                    np.concatenate([scene.size, np.full((pad, 3), 0.5, F)]), np.concatenate([scene.layer, np.ones(pad, np.uint32)]),
                    np.full(total, 0xFFFFFFFF, np.uint32))
    w.tick(dt=DT, gravity=NO_GRAVITY)  # (creates the bodies; their velocities start at zero)
    group = np.arange(n) % 3
    lin, ang = np.zeros((total, 3), F), np.zeros((total, 3), F)
    lin[:n], ang[:n] = np.where((group == 0)[:, None], scene.slow, scene.fast), scene.spin
    w.set_velocities(lin, ang)
    w.tick(dt=DT, gravity=NO_GRAVITY, ticks=10)
    lin[:n] = np.where((group == 2)[:, None], scene.fast, scene.slow)
    w.set_velocities(lin, ang)
    w.tick(dt=DT, gravity=NO_GRAVITY, ticks=2)


def device_bodies(w, scene):
    """The Bodies image of the world as it stands (every entity, the pad included)."""
    total = w.n
    pad = total - scene.n
    pos, _ = w.download_pose()
    b = w.download_bodies()
    state, time = w.download_activation()
    types = np.concatenate([scene.types, np.full(pad, W.BODY_NONE, np.uint8)])
    return Bodies(types, pos, b["quat"], b["linvel"], b["angvel"], state, time, np.concatenate([scene.capsule, np.zeros(pad, bool)]),
                  np.concatenate([scene.size, np.full((pad, 3), 0.5, F)]), np.concatenate([scene.mass, np.ones(pad, F)]),
                  np.concatenate([scene.layer, np.ones(pad, np.uint32)]))


def snapshot(w):
    """Everything an impulse call must leave alone or change by the rule, as bytes-comparable arrays."""
    pos, euler = w.download_pose()
    b = w.download_bodies()
    state, time = w.download_activation()
    return dict(pos=pos, euler=euler, quat=b["quat"], aabb=b["aabb"], linvel=b["linvel"], angvel=b["angvel"], state=state, time=time,
                world=w.download_world())


def assert_matches(snap, want, before, what):
    """The snapshot after a call: velocities, state and timer are the model's, the rest is what it was."""
    def same(a, b, name):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        if a.tobytes() != b.tobytes():
            rows = np.flatnonzero((a.reshape(len(a), -1).view(np.uint8) != b.reshape(len(b), -1).view(np.uint8)).any(axis=1))
            raise AssertionError(f"{what}: {name} differs at {len(rows)} entities, first {rows[0]}: {a[rows[0]]} vs {b[rows[0]]}")

    same(snap["linvel"], want.linvel, "linear velocity")
    same(snap["angvel"], want.angvel, "angular velocity")
    dyn = want.types == BODY_DYNAMIC
    same(snap["state"][dyn], want.state[dyn], "activation state")
    same(snap["time"][dyn], want.time[dyn], "deactivation timer")
    for k in ("pos", "euler", "quat", "aabb", "world"):
        same(snap[k], before[k], k)
    same(snap["state"][~dyn], before["state"][~dyn], "activation state of the others")
