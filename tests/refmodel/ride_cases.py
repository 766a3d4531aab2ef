"""The cases of character platform riding (include/bge_world.h "Character platform riding"): Platforms, a handful of boxes whose poses
a script changes between update calls, as the float64 shape reference and the reference's Poses see them; RideRun, a character set
over them driven call by call; and the seeded platform field with its characters, script and coverage floors: shared by
test_character_rides_cpu.py and test_gpu_character_rides.py."""
from __future__ import annotations

import math

import numpy as np

from banggameengine_amd.world import CHAR_BUTTON_JUMP, CHAR_GROUNDED, CHARACTER_INPUT_DTYPE, make_characters

from .characters import fresh_state, run_ref
from .moves import caster_of
from .rays import ALL, NO_ENTITY, RAY_BODY, World64, box_half_extents, quat_from_euler, quat_to_mat
from .recover import pen_of
from .rides import BODY_NONE, BODY_STATIC, CARRIED, Poses, fresh_rides, ride_run_ref
from .spheres import SphereRef

DT = 1.0 / 60.0
# ToBtQuaternion(euler) = setEulerZYX(yaw = e.y, pitch = e.x, roll = e.z): euler[0] turns about the world's y (the vertical), euler[1]
# about z, euler[2] about x
YAW, TILT_Z, TILT_X = 0, 1, 2


class Platforms:
    """Boxes, entity i = row i: type (BODY_NONE = not in the world), size, position and euler in binary32 as they would be uploaded."""

    def __init__(self, types, sizes, pos, euler, plane=True):
        self.type = np.asarray(types, np.uint8).copy()
        self.size = np.float32(sizes).reshape(-1, 3)
        self.pos = np.float32(pos).reshape(-1, 3).copy()
        self.euler = np.float32(euler).reshape(-1, 3).copy()
        self.plane = plane

    def __len__(self):
        return len(self.type)

    def quat(self):
        return np.float32([quat_from_euler(e.astype(np.float64)) for e in self.euler]).reshape(-1, 4)

    def poses(self):
        return Poses(self.type, self.pos, self.quat())

    def view(self):
        """(caster, penetration function) of the float64 shape reference over the bodies that are in the world, at these poses."""
        live = np.nonzero(self.type != BODY_NONE)[0]
        dims = np.array([box_half_extents(self.size[i]) for i in live]).reshape(-1, 3)
        w64 = World64.from_arrays(np.full(len(live), RAY_BODY), live, np.ones(len(live), np.int64), np.full(len(live), ALL), np.zeros(len(live), bool),
                                  dims, self.pos[live], self.quat()[live].astype(np.float64), self.plane)
        return caster_of(SphereRef(w64).sweep_all), pen_of(w64)

    def move(self, dpos=None, deuler=None, rows=None):
        rows = slice(None) if rows is None else rows
        if dpos is not None:
            self.pos[rows] = (self.pos[rows] + np.float32(dpos)).astype(np.float32)
        if deuler is not None:
            self.euler[rows] = (self.euler[rows] + np.float32(deuler)).astype(np.float32)


class RideRun:
    """A character set over Platforms on the CPU: update() as one bge_world_characters_update call goes, with riding on or off."""

    def __init__(self, platforms, descs, riding, dynamic=False):
        self.platforms, self.descs, self.riding, self.dynamic = platforms, descs, riding, dynamic
        self.state = fresh_state(descs)
        self.rides = fresh_rides(len(descs))
        self.inputs = np.zeros(len(descs), CHARACTER_INPUT_DTYPE)
        self.history = []  # the states after every step

    def update(self, steps=2, inputs=None):
        if inputs is not None:
            self.inputs = inputs.copy()
        cast_fn, pen_fn = self.platforms.view()
        if self.riding:
            self.state, self.rides = ride_run_ref(cast_fn, pen_fn, self.descs, self.inputs, self.state, self.rides, self.platforms.poses(), DT, steps,
                                                  self.dynamic, self.history)
        else:
            self.state = run_ref(cast_fn, pen_fn, self.descs, self.inputs, self.state, DT, steps, self.history)
        return self.state

    def warp(self, i, position):
        self.state["position"][i] = position
        self.state["vertical_velocity"][i] = 0
        self.state["flags"][i] &= ~np.uint32(CHAR_GROUNDED)


# ------------------------------------------------------------------------------------------------ the seeded platform field

N_PLATFORMS, N_RIDERS, N_CHARS, N_CALLS, STEPS_PER_CALL = 64, 192, 257, 6, 2
BATCHES = (1, 255, 256, 257)
FIELD_SEED, CHAR_SEED, SCRIPT_SEED = 31, 32, 33
# The issue's floors over the 257 x 6 character-calls
FLOORS = {"carried": 500, "carried with a rotation": 200, "anchor dropped off the ground": 20}


def top_position(c, quat, h_y, lx, lz, clearance):
    """The point `clearance` above the top face of a box (centre c, quaternion, half height h_y) over its local (lx, lz)."""
    return np.asarray(c, np.float64) + quat_to_mat(quat) @ np.array([lx, h_y + clearance, lz])


def platform_field(rng):
    """64 level Static boxes on a grid spaced 8 apart: half extents [1, 2] x 0.25 x [1, 2], centres 0.5 .. 3 high, any yaw; every 4th
    tilted by up to 0.05 rad about each of the other two axes."""
    k = np.arange(N_PLATFORMS)
    pos = np.stack([(k % 8 - 3.5) * 8.0, rng.uniform(0.5, 3.0, N_PLATFORMS), (k // 8 - 3.5) * 8.0], 1)
    size = np.stack([rng.uniform(1.0, 2.0, N_PLATFORMS), np.full(N_PLATFORMS, 0.25), rng.uniform(1.0, 2.0, N_PLATFORMS)], 1)
    euler = np.zeros((N_PLATFORMS, 3))
    euler[:, YAW] = rng.uniform(-math.pi, math.pi, N_PLATFORMS)
    tilt = rng.uniform(-0.05, 0.05, (N_PLATFORMS, 2))
    euler[::4, TILT_Z], euler[::4, TILT_X] = tilt[::4, 0], tilt[::4, 1]
    return Platforms(np.full(N_PLATFORMS, BODY_STATIC, np.uint8), size, pos, euler, plane=True)


def platform_script(rng, calls=N_CALLS, n=N_PLATFORMS):
    """Per call (dpos (n, 3), deuler (n, 3)): every platform moves by a uniform +-0.3 per axis, every second also yaws by +-0.2."""
    out = []
    for _ in range(calls):
        dpos = rng.uniform(-0.3, 0.3, (n, 3))
        deuler = np.zeros((n, 3))
        deuler[1::2, YAW] = rng.uniform(-0.2, 0.2, len(deuler[1::2]))
        out.append((np.float32(dpos), np.float32(deuler)))
    return out


def rider_batch(rng, n, pos, quat, half_y, per_platform=3):
    """n characters of radius 0.15 .. 0.4: character i stands on platform i // per_platform (poses given: pos, quat, half heights),
    within +-0.4 of its centre in the platform's frame, 0.005 above where it would rest.  Returns (descs, heading (n, 2))."""
    radius = rng.uniform(0.15, 0.4, n).astype(np.float32)
    skin = rng.choice(np.float32([0.002, 0.01]), n)
    at = np.zeros((n, 3))
    for i in range(n):
        b = i // per_platform
        lx, lz = rng.uniform(-0.4, 0.4, 2)
        at[i] = top_position(pos[b], quat[b], half_y[b], lx, lz, float(radius[i]) + float(skin[i]) + 0.005)
    az = rng.uniform(0, 2 * math.pi, n)
    descs = make_characters(at, radius, skin, 0.3, 0.7071, 0.1, 9.81, rng.uniform(3.0, 5.0, n), 29.43, ALL)
    return descs, np.stack([np.cos(az), np.sin(az)], 1)


def field_characters(rng, field):
    """The 257 characters of the field: 192 stand 3 per platform, the other 65 on the plane at the grid's corners, between the
    platforms."""
    descs, heading = rider_batch(rng, N_RIDERS, field.pos, field.quat(), np.array([box_half_extents(s)[1] for s in field.size]))
    n = N_CHARS - N_RIDERS
    radius = rng.uniform(0.15, 0.4, n).astype(np.float32)
    k = np.arange(n)
    at = np.stack([(k % 9 - 4.0) * 8.0, radius + 0.01 + 0.005, (k // 9 - 4.0) * 8.0], 1)
    az = rng.uniform(0, 2 * math.pi, n)
    walkers = make_characters(at, radius, 0.01, 0.3, 0.7071, 0.1, 9.81, rng.uniform(3.0, 5.0, n), 29.43, ALL)
    return np.concatenate([descs, walkers]), np.concatenate([heading, np.stack([np.cos(az), np.sin(az)], 1)])


def input_script(rng, heading, calls=N_CALLS):
    """Per call a CHARACTER_INPUT_DTYPE array: a walk of up to 0.1 per step along the character's heading, JUMP with probability
    1/16."""
    n = len(heading)
    out = []
    for _ in range(calls):
        inp = np.zeros(n, CHARACTER_INPUT_DTYPE)
        length = rng.uniform(0.0, 0.1, n)
        inp["walk_x"], inp["walk_z"] = heading[:, 0] * length, heading[:, 1] * length
        inp["buttons"] = np.where(rng.random(n) < 1.0 / 16.0, CHAR_BUTTON_JUMP, 0)
        out.append(inp)
    return out


def field_case():
    """(platforms, platform script, descs, input script) of the seeded field."""
    field = platform_field(np.random.default_rng(FIELD_SEED))
    descs, heading = field_characters(np.random.default_rng(CHAR_SEED), field)
    rng = np.random.default_rng(SCRIPT_SEED)
    return field, platform_script(rng), descs, input_script(rng, heading)


def ride_coverage(calls):
    """Counts over the character-calls of a run.  calls: per call (records before, records after, states after)."""
    cov = dict.fromkeys(FLOORS, 0)
    for before, after, state in calls:
        carried = (after["flags"] & CARRIED) != 0
        cov["carried"] += int(carried.sum())
        cov["carried with a rotation"] += int((carried & (after["turn"][:, :3] != 0).any(axis=1)).sum())
        dropped = (before["entity"] != NO_ENTITY) & (after["entity"] == NO_ENTITY) & ((state["flags"] & CHAR_GROUNDED) == 0)
        cov["anchor dropped off the ground"] += int(dropped.sum())
    return cov


def check_ride_coverage(cov):
    print("coverage:", cov)
    for k, floor in FLOORS.items():
        assert cov[k] >= floor, (k, cov)


# ------------------------------------------------------------------------------------------------ the slot-shuffled world

# The field's 64 platforms as entities 0 .. 63 of a world of 64 + SHUFFLE_PAD entities under the layout recipe: no platform sits at
# the slot of its index.
SHUFFLE_PAD = 200
SHUFFLE_CHAR_SEED, SHUFFLE_SCRIPT_SEED, SHUFFLE_CALLS = 34, 35, 4


def shuffled_topology():
    from .layout_cases import embedded_topology
    return embedded_topology(N_PLATFORMS, SHUFFLE_PAD)
