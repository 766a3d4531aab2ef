"""Character trigger events: the hand cases and the seeded walk with its coverage floors, shared by test_char_triggers_cpu.py
(the rule on the reference alone) and test_gpu_char_triggers.py (the device against the reference).

The walk: 70 trigger boxes with half extents 0.5 .. 3 and centres in +-20 x [0.5, 3] x +-20, two thirds of them yawed, layers
drawn from {4, 4, 4, 0x10} and masks from {all, all, 2, 8}.  257 characters of radius 0.3 .. 0.6 with gravity 0 and a layer_mask bit
that no body carries, so they move level and meet nothing; each walks 0.2 .. 0.6 a step on a random heading and halfway through the
calls turns round at half speed.  Groups are drawn from {2, 2, 2, 8}, masks from {all, all, 4, 0x10}.  12 update calls of 3 steps."""
from __future__ import annotations

import math

import numpy as np

from banggameengine_amd.world import make_character_inputs, make_characters

from .rays import ALL, box_half_extents, quat_from_euler, quat_to_mat
from .char_triggers import ENTER, EXIT, STAY, char_trigger_ref, filter_pass, geometric_overlap

DT = 1.0 / 60.0
TRIGGER_SEED, CHAR_SEED = 41, 411
N_TRIGGERS, N_CHARS, N_CALLS, STEPS_PER_CALL = 70, 257, 12, 3
BATCHES = (1, 63, 64, 65, 256, 257)  # the wave, ballot-word and workgroup edges
TRIGGER_COUNTS = (1, 2, 70)          # 70 also crosses the 64 ghosts a workgroup stages in LDS
NOBODY = 0x20                        # a layer no body, ghost or plane of these worlds carries: the characters meet nothing
# Floors at about half of what a float64 model of this recipe gave over five seeds (Enter 419-467, Stay 1,102-1,209, Exit 284-320,
# filtered out 977-1,260, most events in one call 173-190, characters 192..256 ever inside 41-45)
FLOORS = {"enter": 200, "stay": 500, "exit": 150, "filtered out": 400, "most in one call": 150, "tail characters inside": 20, "calls with enter": N_CALLS}


class Walk:
    """The triggers (entity t = row t of the world = trigger t of the uploaded array), the characters and their walk."""

    def __init__(self, trigger_seed=TRIGGER_SEED, char_seed=CHAR_SEED, n_triggers=N_TRIGGERS, n_chars=N_CHARS):
        rng = np.random.default_rng(trigger_seed)
        T = n_triggers
        self.size = rng.uniform(0.5, 3.0, (T, 3)).astype(np.float32)
        self.pos = np.stack([rng.uniform(-20, 20, T), rng.uniform(0.5, 3.0, T), rng.uniform(-20, 20, T)], axis=1).astype(np.float32)
        yaw = np.where(rng.random(T) < 2.0 / 3.0, rng.uniform(-math.pi, math.pi, T), 0.0)
        self.euler = np.stack([np.zeros(T), yaw, np.zeros(T)], axis=1).astype(np.float32)
        self.layer = rng.choice(np.uint32([4, 4, 4, 0x10]), T)
        self.mask = rng.choice(np.uint32([ALL, ALL, 2, 8]), T)
        self.entity = np.arange(T, dtype=np.uint32)
        rng = np.random.default_rng(char_seed)
        n = n_chars
        start = np.stack([rng.uniform(-20, 20, n), rng.uniform(0.5, 3.0, n), rng.uniform(-20, 20, n)], axis=1)
        self.descs = make_characters(start, radius=rng.uniform(0.3, 0.6, n), gravity=0.0, layer_mask=NOBODY)
        az, speed = rng.uniform(0, 2 * math.pi, n), rng.uniform(0.2, 0.6, n)
        self.step = np.stack([np.cos(az) * speed, np.sin(az) * speed], axis=1).astype(np.float32)
        self.group = rng.choice(np.uint32([2, 2, 2, 8]), n)
        self.cmask = rng.choice(np.uint32([ALL, ALL, 4, 0x10]), n)

    def inputs(self, call, n=None):
        """The input of every step of update call `call`: the walk, and from the middle call on its reverse at half speed."""
        s = self.step if call < N_CALLS // 2 else (self.step * np.float32(-0.5)).astype(np.float32)
        s = s[:n]
        return make_character_inputs(s[:, 0], s[:, 1])

    def model_boxes(self):
        """The triggers' boxes for the CPU test, which has no device to pose them: the AABB of the turned box plus the contact
        threshold, in float64 rounded to binary32.  (The GPU test takes the device's own boxes from World.trigger_boxes.)"""
        out = np.zeros((len(self.pos), 6), np.float32)
        for t in range(len(self.pos)):
            B = quat_to_mat(quat_from_euler(self.euler[t].astype(np.float64)))
            bb = np.abs(B) @ box_half_extents(self.size[t]).astype(np.float64) + 0.02
            out[t, :3], out[t, 3:] = self.pos[t] - bb, self.pos[t] + bb
        return out

    def model_positions(self, n=None):
        """The positions after every call where nothing is met: position + walk per step, in binary32."""
        p = self.descs["position"][:n].copy()
        history = []
        for call in range(N_CALLS):
            inp = self.inputs(call, n)
            for _ in range(STEPS_PER_CALL):
                p[:, 0] = p[:, 0] + inp["walk_x"]
                p[:, 2] = p[:, 2] + inp["walk_z"]
            history.append(p.copy())
        return history


def run_reference(walk, boxes, listed, positions, n=None, triggers=None, stay=True):
    """char_trigger_ref over the calls of the walk from nothing remembered: [(events, remembered)] per call."""
    t = slice(None) if triggers is None else slice(0, triggers)
    prev = np.zeros((len(walk.entity[t]), len(positions[0])), bool)
    out = []
    for p in positions:
        ev, prev = char_trigger_ref(boxes[t], listed[t], walk.layer[t], walk.mask[t], p, walk.descs["radius"][:n], walk.group[:n], walk.cmask[:n],
                                    prev, stay, walk.entity[t])
        out.append((ev, prev))
    return out


def coverage(walk, boxes, positions, event_lists):
    """What a run of all the characters saw: event_lists[k] is the list of call k (of the device, or of the reference)."""
    cov = dict.fromkeys(FLOORS, 0)
    inside = np.zeros(len(positions[0]), bool)
    passes = filter_pass(walk.layer, walk.mask, walk.group, walk.cmask)
    for p, ev in zip(positions, event_lists):
        cov["enter"] += int((ev[:, 0] == ENTER).sum())
        cov["stay"] += int((ev[:, 0] == STAY).sum())
        cov["exit"] += int((ev[:, 0] == EXIT).sum())
        cov["most in one call"] = max(cov["most in one call"], len(ev))
        cov["calls with enter"] += int((ev[:, 0] == ENTER).any())
        cov["filtered out"] += int((geometric_overlap(boxes, p, walk.descs["radius"]) & ~passes).sum())
        inside[ev[ev[:, 0] != EXIT, 2]] = True
    cov["tail characters inside"] = int(inside[192:].sum())
    return cov


def check_coverage(cov):
    print("coverage:", cov)
    for k, floor in FLOORS.items():
        assert cov[k] >= floor, (k, cov)


# ------------------------------------------------------------------------------------------------ hand cases
# One trigger box [-1, 1]^3 as fed (threshold included), layer 4, mask all; a character of radius 0.5 has the box
# [x - 0.52, x + 0.52]: it overlaps for x in [-1.52, 1.52] (up to the rounding the boundary case works out).
UNIT = np.float32([[-1, -1, -1, 1, 1, 1]])
# A character walking along x through UNIT, one position per call, and the list of every call
THROUGH_X = (-3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0)
THROUGH_EVENTS = ([], [], [ENTER], [STAY], [STAY], [EXIT], [])
