"""The scene and the seeded batches of the impulse comparisons (include/bge_world.h "Impulses"): shared by test_impulses_cpu.py,
which runs the model over them and checks what each batch claims to cover, and test_gpu_impulses.py, which runs the device over
them.  Nothing here needs a GPU."""
from __future__ import annotations

import numpy as np

from .impulses import (AT_POINT, BODY_DYNAMIC, BODY_KINEMATIC, BODY_NONE, BODY_STATIC, CENTRAL, IMPULSE_DTYPE, TORQUE, WORLD_POINT, make_impulses)

F = np.float32
SCENE_SEED, BATCH_SEED = 2501, 2502
N_OWN = 64          # the scene's own entities
SHUFFLE_PAD = 200   # the entities that carry the hierarchy of the slot-shuffled form (layout_cases.embedded_topology)
SIZES = (0, 1, 63, 64, 65, 257)
RUNS = (2, 3, 65, 300)  # records on ONE body: within a wave, across a wave, across a workgroup of 256
# Every 8th entity is not a Dynamic body: 7 Static, 15 Kinematic, 23 no body, 31 Static, ...
NOT_DYNAMIC = {7: BODY_STATIC, 15: BODY_KINEMATIC, 23: BODY_NONE, 31: BODY_STATIC, 39: BODY_KINEMATIC, 47: BODY_NONE, 55: BODY_STATIC, 63: BODY_NONE}


class Scene:
    """N_OWN entities: Dynamic boxes and capsules of seeded size, mass, pose and velocity, and the NOT_DYNAMIC ones among them.
    Dynamic entity e is meant to be ASLEEP when the batch arrives if e % 3 == 0, awake with a running timer if e % 3 == 1 and
    awake and fast (timer 0) if e % 3 == 2."""

    def __init__(self):
        rng = np.random.default_rng(SCENE_SEED)
        n = N_OWN
        self.n = n
        self.types = np.full(n, BODY_DYNAMIC, np.uint8)
        for e, t in NOT_DYNAMIC.items():
            self.types[e] = t
        self.dynamic = np.flatnonzero(self.types == BODY_DYNAMIC)
        self.pos = np.stack([np.arange(n) * 4.0 - 2.0 * n, rng.uniform(5.0, 9.0, n), rng.uniform(-3.0, 3.0, n)], 1).astype(F)
        self.euler = rng.uniform(-3.0, 3.0, (n, 3)).astype(F)
        self.euler[::5] = 0  # (some unrotated)
        self.capsule = (np.arange(n) % 4 == 1)
        self.size = rng.uniform(0.2, 1.2, (n, 3)).astype(F)
        self.size[2] = (0.5, 0.5, 0.5)
        self.size[6] = (0.05, 0.3, 0.02)  # (below Bullet's margin: the safe margin applies)
        self.mass = rng.choice(F([0.25, 1.0, 2.0, 7.5, 0.001]), n).astype(F)
        self.layer = (1 << (np.arange(n) % 3)).astype(np.uint32)
        self.fast = np.stack([rng.uniform(1.0, 2.0, n), rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n)], 1).astype(F)   # |v| >= 1 > 0.8
        self.slow = rng.uniform(-0.05, 0.05, (n, 3)).astype(F)
        self.spin = rng.uniform(-0.2, 0.2, (n, 3)).astype(F)
        self.spin[::2] = 0  # (half of them do not spin before the call)


def scene_bodies(scene):
    """The scene as a Bodies image without a device: orientations from the eulers, and the activation state the groups stand for
    (asleep with zero velocities; awake, slow, timer at two ticks; awake, fast, timer 0)."""
    from .impulses import ACT_NONE, ACTIVE_TAG, DISABLE_DEACTIVATION, ISLAND_SLEEPING, Bodies
    from .rays import quat_from_euler
    n = scene.n
    group = np.arange(n) % 3
    dyn = scene.types == BODY_DYNAMIC
    lin = np.where((group == 2)[:, None], scene.fast, scene.slow) * dyn[:, None]
    ang = scene.spin * dyn[:, None]
    lin[group == 0], ang[group == 0] = 0, 0
    state = np.full(n, ACT_NONE, np.uint8)
    state[scene.types == BODY_STATIC] = ISLAND_SLEEPING
    state[scene.types == BODY_KINEMATIC] = DISABLE_DEACTIVATION
    state[dyn] = np.where(group[dyn] == 0, ISLAND_SLEEPING, ACTIVE_TAG)
    time = np.where(dyn & (group == 1), F(2.0 / 60.0), F(0)).astype(F)
    quat = np.stack([quat_from_euler(e.astype(np.float64)) for e in scene.euler]).astype(F)
    return Bodies(scene.types, scene.pos, quat, lin.astype(F), ang.astype(F), state, time, scene.capsule, scene.size, scene.mass, scene.layer)


def random_records(rng, n, entities, scene, bad=0.0):
    """n records over the given entities: every kind, WORLD_POINT on some AT_POINT records, magnitudes over six decades so that
    the order of the additions shows in the bits; a share `bad` of them is spoiled (a float, or the flags)."""
    rec = np.zeros(n, IMPULSE_DTYPE)
    if n == 0:
        return rec
    rec["entity"] = rng.choice(np.asarray(entities, np.uint32), n)
    kind = rng.choice([AT_POINT, AT_POINT, CENTRAL, TORQUE], n).astype(np.uint32)
    world = (kind == AT_POINT) & (rng.random(n) < 0.5)
    rec["flags"] = kind | np.where(world, WORLD_POINT, 0).astype(np.uint32)
    scale = 10.0 ** rng.uniform(-3.0, 3.0, (n, 1))
    rec["impulse"] = (rng.uniform(-1.0, 1.0, (n, 3)) * scale).astype(F)
    rel = rng.uniform(-1.5, 1.5, (n, 3)).astype(F)
    origin = scene.pos[np.minimum(rec["entity"], scene.n - 1)]
    rec["point"] = np.where(world[:, None], origin + rel, rel).astype(F)
    for i in np.flatnonzero(rng.random(n) < bad):
        what = int(rng.integers(0, 6))
        if what == 0:
            rec["impulse"][i][int(rng.integers(0, 3))] = np.nan
        elif what == 1:
            rec["impulse"][i][int(rng.integers(0, 3))] = np.inf
        elif what == 2:
            rec["point"][i][int(rng.integers(0, 3))] = -np.inf  # (spoils AT_POINT records only: the others do not read it)
        elif what == 3:
            rec["flags"][i] = 3
        elif what == 4:
            rec["flags"][i] = rng.choice(np.uint32([8, 0x10 | CENTRAL, 0x80000000, 0xFFFFFFFF]))
        else:
            rec["flags"][i] = rng.choice(np.uint32([CENTRAL | WORLD_POINT, TORQUE | WORLD_POINT]))
    return rec


def batches(scene):
    """name -> IMPULSE_DTYPE records, in a fixed order."""
    rng = np.random.default_rng(BATCH_SEED)
    everyone = np.arange(scene.n)
    dyn = scene.dynamic
    out = {}
    for n in SIZES:
        out[f"n = {n}"] = random_records(rng, n, everyone, scene, bad=0.1)
    for k, run in enumerate(RUNS):
        body = int(dyn[3 + k])  # entities 3, 4, 5, 6: asleep, timer running, fast, asleep
        out[f"{run} on one body"] = random_records(rng, run, [body], scene)
    out["interleaved"] = random_records(rng, 96, dyn[[8, 9, 10]], scene)
    out["interleaved"]["entity"] = np.tile(dyn[[8, 9, 10]], 32)
    out["interleaved"]["point"] = rng.uniform(-1.0, 1.0, (96, 3)).astype(F)
    out["interleaved"]["flags"] &= ~np.uint32(WORLD_POINT)
    # Static, Kinematic, body-less, one past the own entities (no body in either form of the world), far out of range
    strangers = np.uint32(sorted(NOT_DYNAMIC) + [0x7FFFFFFF, 0xFFFFFFFE, 0xFFFFFFFF])
    out["not dynamic"] = make_impulses(strangers, np.tile(F([1, 2, 3]), (len(strangers), 1)), flags=CENTRAL)
    # every way a record is invalid, on a Dynamic body that is asleep, with valid records around them; point is not read by
    # CENTRAL and TORQUE: a NaN there is fine
    b = int(dyn[0])
    nan, inf = np.nan, np.inf
    rows = [(b, CENTRAL, (1, 0, 0), (0, 0, 0)), (b, CENTRAL, (nan, 0, 0), (0, 0, 0)), (b, AT_POINT, (0, inf, 0), (0, 0, 0)),
            (b, AT_POINT, (0, 1, 0), (0, nan, 0)), (b, CENTRAL, (0, 1, 0), (nan, inf, -inf)), (b, TORQUE, (0, 0, 1), (nan, 0, 0)),
            (b, TORQUE, (0, 0, -inf), (0, 0, 0)), (b, AT_POINT | WORLD_POINT, (1, 1, 1), (0, 0, -inf)), (b, 3, (1, 0, 0), (0, 0, 0)),
            (b, 3 | WORLD_POINT, (1, 0, 0), (0, 0, 0)), (b, CENTRAL | WORLD_POINT, (1, 0, 0), (0, 0, 0)), (b, TORQUE | WORLD_POINT, (1, 0, 0), (0, 0, 0)),
            (b, 8, (1, 0, 0), (0, 0, 0)), (b, 0x80000000 | CENTRAL, (1, 0, 0), (0, 0, 0)), (0xFFFFFFFF, 3, (nan, 0, 0), (0, 0, 0)),
            (b, AT_POINT, (0, 0, 2), (0.5, 0, 0))]
    out["bad floats and flags"] = np.array(rows, IMPULSE_DTYPE)
    # zero impulses: the caller's activate().  One per group of three (asleep, timer running, fast), each kind, and a -0
    z = dyn[[12, 13, 14, 15, 16, 17]]
    out["zero impulses"] = make_impulses(z, np.zeros((6, 3), F), np.ones((6, 3), F), flags=np.uint32([CENTRAL, CENTRAL, CENTRAL, AT_POINT, TORQUE, AT_POINT]))
    out["zero impulses"]["impulse"][3] = (-0.0, 0.0, -0.0)
    return out


def covered(scene, records):
    """What a batch holds: counts of kinds, of WORLD_POINT, and the longest run on one entity."""
    kind = records["flags"] & 3
    ents, counts = np.unique(records["entity"], return_counts=True)
    return dict(at_point=int((kind == AT_POINT).sum()), central=int((kind == CENTRAL).sum()), torque=int((kind == TORQUE).sum()),
                world=int(((records["flags"] & WORLD_POINT) != 0).sum()), longest=int(counts.max()) if len(counts) else 0, bodies=len(ents))
