#!/usr/bin/env python3
"""Cost of one step of a character set (bge_world_characters_update) beside the two batches it is made of.

Run on an MI355X:  python tools/measure_characters.py [n_bodies]
Scene: that of tools/measure_step_move.py — n_bodies (default 1 M) boxes and capsules mixed, resting on the plane over 2,000 x 2,000
units, with n_bodies / 8 Static flat slabs added.  1,024 characters of radius 0.4 and skin 0.01 (step_height 0.5, probe 0.3) are
created a hair above the plane, settled for three steps and then walk 0.03 .. 0.06 a step (a walk speed of 1.8 .. 3.6 at 1/60 s).
Timed with HIP events on the world's stream (warm-up first, then the median of the repeats), in the same process on the same world:
  update_us    one World.characters_update(dt, 1): 5 penetration passes, 7 sphere-cast passes (4 of them over two casts per character)
               and the three glue kernels
  recover_us   one World.sphere_recover_device call for the same 1,024 spheres, where the characters are after the timed steps
  step_us      one World.sphere_step_move_device call for the same 1,024 spheres asking their walk as a level displacement
The expectation is update_us = recover_us + step_us: the glue kernels touch 1,024 records.  Not a test, and not part of bench.py.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import banggameengine_amd as B  # noqa: E402
from banggameengine_amd import world as W  # noqa: E402


def timed_device(stream, call, reps):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for k in range(2 + reps):
        ev0.record(stream)
        call()
        ev1.record(stream)
        ev1.synchronize()
        if k >= 2:
            times.append(ev0.elapsed_time(ev1) * 1e3)
    return round(float(np.median(times)), 2)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
    n_slabs = n // 8
    rng = np.random.default_rng(3)
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    with B.World(device=0, stream=stream.cuda_stream) as w, torch.cuda.stream(stream):
        total = n + n_slabs
        w.set_topology(np.full(total, W.NO_PARENT, np.uint32))
        size = rng.uniform(0.2, 1.0, (n, 3)).astype(np.float32)
        shape = rng.integers(0, 2, n).astype(np.uint8)
        btype = rng.choice([W.BODY_STATIC, W.BODY_DYNAMIC, W.BODY_KINEMATIC], n, p=[0.34, 0.5, 0.16]).astype(np.uint8)
        rest = np.where(shape == 1, size[:, 0] + size[:, 1], np.maximum(size[:, 1], 0.01))
        pos = np.stack([rng.uniform(-1000, 1000, n), rest, rng.uniform(-1000, 1000, n)], 1).astype(np.float32)
        top = rng.uniform(0.1, 0.6, n_slabs)
        s_size = np.stack([rng.uniform(0.5, 2.0, n_slabs), top / 2, rng.uniform(0.5, 2.0, n_slabs)], 1).astype(np.float32)
        s_pos = np.stack([rng.uniform(-1000, 1000, n_slabs), top / 2, rng.uniform(-1000, 1000, n_slabs)], 1).astype(np.float32)
        euler = np.zeros((total, 3), np.float32)
        euler[n:, 1] = rng.uniform(-np.pi, np.pi, n_slabs)
        w.upload_trs(np.concatenate([pos, s_pos]), euler, np.ones((total, 3), np.float32))
        w.upload_bodies(np.concatenate([btype, np.full(n_slabs, W.BODY_STATIC, np.uint8)]), None,
                        np.concatenate([shape, np.zeros(n_slabs, np.uint8)]), np.concatenate([size, s_size]))
        w.set_ground_plane(True)
        w.set_sleeping(0.8, 1.0, 0.05)
        w.tick(flags=W.TICK_ALL, ticks=30)
        nc, dt, reps = 1024, 1.0 / 60.0, 7
        radius, skin, probe, height = 0.4, 0.01, 0.3, 0.5
        p = np.stack([rng.uniform(-1000, 1000, nc), np.full(nc, radius + skin + 0.005), rng.uniform(-1000, 1000, nc)], 1)
        az = rng.uniform(0, 2 * np.pi, nc)
        walk = np.stack([np.cos(az), np.sin(az)], 1) * rng.uniform(0.03, 0.06, nc)[:, None]
        w.characters_create(W.make_characters(p, radius, skin, height, 0.7071068, probe))
        w.characters_update(dt, 3)
        w.characters_set_input(W.make_character_inputs(walk[:, 0], walk[:, 1]))
        row = {"bodies": n, "slabs": n_slabs, "characters": nc}
        row["update_us"] = timed_device(stream, lambda: w.characters_update(dt, 1), reps)
        s = w.characters_state()
        disp = np.stack([walk[:, 0], np.zeros(nc), walk[:, 1]], 1)
        rec = torch.from_numpy(W.make_sphere_recovers(s["position"], radius, skin).view(np.uint8)).to("cuda:0")
        rec_out = torch.zeros(nc * 64, dtype=torch.uint8, device="cuda:0")
        mv = torch.from_numpy(W.make_sphere_step_moves(s["position"], disp, radius, skin, probe, step_height=height).view(np.uint8)).to("cuda:0")
        mv_out = torch.zeros(nc * 80, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        row["recover_us"] = timed_device(stream, lambda: w.sphere_recover_device(rec, rec_out), reps)
        row["step_us"] = timed_device(stream, lambda: w.sphere_step_move_device(mv, mv_out), reps)
        row["update_over_sum"] = round(row["update_us"] / (row["recover_us"] + row["step_us"]), 3)
        row["steps_run"] = int(s["steps"][0])
        for name, bit in (("grounded", W.CHAR_GROUNDED), ("stepped", W.CHAR_STEPPED), ("recovered", W.CHAR_RECOVERED), ("invalid", W.CHAR_INVALID)):
            row[name] = int(((s["flags"] & bit) != 0).sum())
        print(json.dumps(row))


if __name__ == "__main__":
    main()
