"""The GPU side of the platform-riding comparisons: the device's poses in the form ride_run_ref expects, and DeviceRide, a world of
platforms with a riding character set driven call by call next to the reference over the device's own queries and poses."""
from __future__ import annotations

import numpy as np

from .characters import fresh_state
from .device import FLAGS, device_caster
from .character_device import device_pen
from .rides import Poses, fresh_rides, ride_run_ref


def device_poses(w, types):
    """Poses of the world's entities as a characters_update call sees them now.  types: per entity the body's type where it is in
    the queries' world (uploaded and ticked since), BODY_NONE where it is not."""
    pos, _ = w.download_pose()
    return Poses(types, pos, w.download_bodies()["quat"])


def repose(w, entities, pos, euler):
    """The Transforms of `entities` set to (pos, euler), and a tick so that the queries see them there."""
    w.upload_trs_indexed(entities, pos, euler, np.ones((len(entities), 3)))
    w.tick(flags=FLAGS)


class DeviceRide:
    """A character set with riding on over the world w, and the reference's states and records next to it.  call() is one
    bge_world_characters_update on both; it returns (got states, got records, wanted states, wanted records)."""

    def __init__(self, w, descs, types, dt, dynamic=False):
        self.w, self.descs, self.types, self.dt, self.dynamic = w, descs, np.asarray(types, np.uint8), dt, dynamic
        w.characters_create(descs)
        w.characters_ride(True, dynamic)
        self.state, self.rides = fresh_state(descs), fresh_rides(len(descs))
        self.cast_fn, self.pen_fn = device_caster(w), device_pen(w)

    def call(self, inputs, steps):
        self.w.characters_set_input(inputs)
        self.w.characters_update(self.dt, steps)
        got = self.w.characters_state(), self.w.characters_rides()
        self.state, self.rides = ride_run_ref(self.cast_fn, self.pen_fn, self.descs, inputs.copy(), self.state, self.rides,
                                              device_poses(self.w, self.types), self.dt, steps, self.dynamic)
        return got[0], got[1], self.state, self.rides
