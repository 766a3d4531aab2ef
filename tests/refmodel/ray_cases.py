"""Seeded objects and rays that test_raycast_cpu.py and the GPU suites both use."""
from __future__ import annotations

import numpy as np

from .rays import RAY_BODY, RAY_TRIGGER, Obj, box_half_extents, capsule_dims

def random_objects(rng, n, spread=6.0):
    objs = []
    for i in range(n):
        capsule = bool(rng.integers(0, 2))
        size = rng.uniform(0.1, 1.5, 3)
        dims = capsule_dims(size) if capsule else box_half_extents(size)
        q = rng.normal(size=4)
        kind = RAY_BODY if i % 5 else RAY_TRIGGER
        objs.append(Obj(kind, i, int(rng.choice([1, 2, 4, 5])), int(rng.choice([0xFFFFFFFF, 0xFFFFFFFF, 0])), capsule, dims,
                        rng.uniform(-spread, spread, 3), q / np.linalg.norm(q)))
    return objs


def random_rays(rng, n, scene_pos, spread=30.0):
    o = np.stack([rng.uniform(-spread, spread, n), rng.uniform(-2.0, 12.0, n), rng.uniform(-spread, spread, n)], 1)
    d = rng.normal(size=(n, 3))
    aim = rng.random(n) < 0.6  # most rays aimed at a body, the rest anywhere
    tgt = scene_pos[rng.integers(0, len(scene_pos), n)] + rng.normal(scale=0.3, size=(n, 3))
    d[aim] = tgt[aim] - o[aim]
    d *= rng.uniform(0.5, 2.0, (n, 1))
    md = rng.uniform(0.5, 1.5, n) * np.where(aim, 1.0, 20.0)
    mask = rng.choice(np.array([1, 2, 4, 8, 3, 6, 0xFFFFFFFF], np.uint32), n)
    return o.astype(np.float32), d.astype(np.float32), md.astype(np.float32), mask


IDQ = (0.0, 0.0, 0.0, 1.0)
