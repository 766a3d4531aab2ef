"""The fixtures of the impulse tests: tests/golden/impulses_<scene>.json, the output of tests/cpp/impulse_oracle.cpp (the oracle's own
headers, the rule of include/bge_world.h "Impulses" applied to its body runtimes at stated ticks).  test_impulses_cpu.py rebuilds
the program and requires the same bytes; test_gpu_impulses.py runs the scenes on the device against what is decoded here."""
from __future__ import annotations

import json
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SOURCE = os.path.join(ROOT, "tests", "cpp", "impulse_oracle.cpp")
SCENES = ("a", "b", "c", "d", "e", "f")
# the oracle's own build flags (oracle/Makefile): one rounding per operation
CXXFLAGS = ["-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-Wno-unused-parameter"]


def path(scene):
    return os.path.join(GOLDEN, f"impulses_{scene}.json")


def build(directory):
    exe = os.path.join(str(directory), "impulse_oracle")
    subprocess.check_call(["g++", *CXXFLAGS, "-o", exe, SOURCE])
    return exe


def run(exe, scene):
    r = subprocess.run([exe, scene], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def f32(hexes):
    return np.array([int(h, 16) for h in hexes], np.uint32).view(np.float32)


def decode_bodies(row):
    """One tick's strings -> dict of arrays over the bodies: origin, quat, linvel, angvel (float32), state, time."""
    words = np.array([[int(s[8 * k:8 * k + 8], 16) for k in range(15)] for s in row], np.uint32)
    f = words.view(np.float32)
    return dict(origin=f[:, 0:3].copy(), quat=f[:, 3:7].copy(), linvel=f[:, 7:10].copy(), angvel=f[:, 10:13].copy(), state=words[:, 13].astype(np.uint8),
                time=f[:, 14].copy())


class Fixture:
    def __init__(self, scene):
        with open(path(scene)) as fh:
            d = json.load(fh)
        self.scene = scene
        self.dt = float(f32([d["dt"]])[0])
        self.gravity = (0.0, float(f32([d["gravity_y"]])[0]), 0.0)
        self.plane, self.static_contacts, self.dynamic_contacts, self.basis = (bool(d[k]) for k in ("plane", "static_contacts", "dynamic_contacts", "bullet_basis"))
        self.warmup = d["warmup_ticks"]
        self.types = np.array([b["type"] for b in d["bodies"]], np.uint8)  # 0 Static, 1 Dynamic: bge_body_type
        self.size = np.stack([f32(b["size"]) for b in d["bodies"]])
        self.pos = np.stack([f32(b["position"]) for b in d["bodies"]])
        self.mass = np.array([f32([b["mass"]])[0] for b in d["bodies"]], np.float32)
        self.kicks = [(k["before_tick"], k["entity"], k["flags"], f32(k["impulse"]), f32(k["point"])) for k in d["kicks"]]
        self.after_warmup = decode_bodies(d["after_warmup"])
        self.ticks = [decode_bodies(row) for row in d["ticks"]]
        self.asleep_after = d["body0_asleep_after_ticks"]
