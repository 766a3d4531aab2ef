#!/usr/bin/env python3
"""Cost of the sphere queries (bge_world_sphere_cast*, bge_world_overlap_sphere) on a big world, beside the ray query.

Run on the GPU box:  python tools/measure_sphere_queries.py [n_bodies]
Scene: that of tools/measure_raycast.py — n_bodies (default 1 M) boxes and capsules mixed, resting on the plane over
2,000 x 2,000 units.  Batches of 1, 1,024 and 65,536 queries straight down from above the scene over 200 units (layer mask all
ones), timed with HIP events on the world's stream around each *_device call (warm-up first, then the median of the repeats):
  raycast            World.raycast_device on the same origins: the yardstick (the streaming pass is the same)
  cast r=0           bge_world_sphere_cast_device with radius 0: a large gap to the ray means the exact tests are reached too often
  cast r=0.5         the same with radius 0.5
sphere_cast_all (radius 0.5) and overlap_sphere (centres 1 above the plane, radius 2) are synchronous calls (launch pair, count
read-back, list download, sort on the host) and are timed on the wall clock.
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import banggameengine_amd as B  # noqa: E402
from banggameengine_amd import world as W  # noqa: E402


def timed_device(stream, call, reps):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for k in range(3 + reps):
        ev0.record(stream)
        call()
        ev1.record(stream)
        ev1.synchronize()
        if k >= 3:
            times.append(ev0.elapsed_time(ev1) * 1e3)
    return round(float(np.median(times)), 2)


def timed_wall(call, reps):
    for _ in range(2):
        call()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = call()
        times.append((time.perf_counter() - t0) * 1e6)
    return round(float(np.median(times)), 1), r


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
    rng = np.random.default_rng(3)
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    with B.World(device=0, stream=stream.cuda_stream) as w:
        w.set_topology(np.full(n, W.NO_PARENT, np.uint32))
        size = rng.uniform(0.2, 1.0, (n, 3)).astype(np.float32)
        shape = rng.integers(0, 2, n).astype(np.uint8)
        btype = rng.choice([W.BODY_STATIC, W.BODY_DYNAMIC, W.BODY_KINEMATIC], n, p=[0.34, 0.5, 0.16]).astype(np.uint8)
        rest = np.where(shape == 1, size[:, 0] + size[:, 1], np.maximum(size[:, 1], 0.01))
        pos = np.stack([rng.uniform(-1000, 1000, n), rest, rng.uniform(-1000, 1000, n)], 1).astype(np.float32)
        w.upload_trs(pos, np.zeros((n, 3), np.float32), np.ones((n, 3), np.float32))
        w.upload_bodies(btype, None, shape, size)
        w.set_ground_plane(True)
        w.set_sleeping(0.8, 1.0, 0.05)
        w.tick(flags=W.TICK_ALL, ticks=30)
        out = {"bodies": n, "batches": []}
        down = np.float32([0.0, -1.0, 0.0])
        for nq in (1, 1024, 65536):
            o = np.stack([rng.uniform(-1000, 1000, nq), np.full(nq, 150.0), rng.uniform(-1000, 1000, nq)], 1)
            dirs = np.tile(down, (nq, 1))
            reps = 30 if nq == 1 else (10 if nq == 1024 else 3)
            row = {"queries": nq}
            ht = torch.zeros(nq * 40, dtype=torch.uint8, device="cuda:0")
            rt = torch.from_numpy(W.make_rays(o, dirs, 200.0).view(np.uint8)).to("cuda:0")
            torch.cuda.synchronize()
            row["raycast_us"] = timed_device(stream, lambda: w.raycast_device(rt, ht), reps)
            ray_kinds = np.bincount(ht.cpu().numpy().view(W.RAY_HIT_DTYPE)["kind"], minlength=4).tolist()
            for name, radius in (("cast_r0_us", 0.0), ("cast_r05_us", 0.5)):
                ct = torch.from_numpy(W.make_sphere_casts(o, dirs, 200.0, radius).view(np.uint8)).to("cuda:0")
                torch.cuda.synchronize()
                row[name] = timed_device(stream, lambda: w.sphere_cast_device(ct, ht), reps)
                kinds = np.bincount(ht.cpu().numpy().view(W.RAY_HIT_DTYPE)["kind"], minlength=4).tolist()
                if radius == 0.0:
                    row["r0_kinds_equal_ray"] = kinds == ray_kinds
                row[name.replace("_us", "_kinds")] = kinds
            wall_reps = 10 if nq <= 1024 else 2
            row["cast_all_wall_us"], r = timed_wall(lambda: w.sphere_cast_all(o, dirs, 200.0, 0.5), wall_reps)
            row["cast_all_hits"] = int(r["offsets"][-1])
            c = o.copy()
            c[:, 1] = 1.0
            row["overlap_wall_us"], r = timed_wall(lambda: w.overlap_sphere(c, 2.0), wall_reps)
            row["overlap_found"] = int(r["offsets"][-1])
            out["batches"].append(row)
            print(json.dumps(row), flush=True)
        print(json.dumps(out))


if __name__ == "__main__":
    main()
