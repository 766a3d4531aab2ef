#!/usr/bin/env python3
"""Cost of the ray queries (bge_world_raycast_device, bge_world_raycast_all) on a big world.

Run on the GPU box:  python tools/measure_raycast.py [n_bodies]
Scene: n_bodies (default 1 M) boxes and capsules mixed, a third Static, half Dynamic (resting on the plane, asleep), the rest
Kinematic, spread over 2,000 x 2,000 units; the plane is on.  Batches of 1 (the HUD ray), 64 and 4,096 rays, straight down
from above the scene over 200 units (layer mask all ones), are timed with HIP events on the world's stream around each
bge_world_raycast_device call (warm-up first, then the median of the repeats); raycast_all of 64 rays is timed on the wall clock
(a synchronous call: launch pair, count read-back, list download, sort on the host).
The body pass reads 44 bytes per body slot (flags, position, collider, contact word, filter words); the achieved rate of a
batch is that over the event time, against the ~6.3 TB/s the tick kernel reaches on this device.
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

BYTES_PER_BODY = 44
TICK_RATE = 6.3e12


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
        # resting poses on the plane: a box's half height, a capsule's radius + half height
        rest = np.where(shape == 1, size[:, 0] + size[:, 1], np.maximum(size[:, 1], 0.01))
        pos = np.stack([rng.uniform(-1000, 1000, n), rest, rng.uniform(-1000, 1000, n)], 1).astype(np.float32)
        w.upload_trs(pos, np.zeros((n, 3), np.float32), np.ones((n, 3), np.float32))
        w.upload_bodies(btype, None, shape, size)
        w.set_ground_plane(True)
        w.set_sleeping(0.8, 1.0, 0.05)
        w.tick(flags=W.TICK_ALL, ticks=30)
        state, _ = w.download_activation()
        asleep = int((state == 2).sum())
        out = {"bodies": n, "asleep": asleep, "bytes_per_body": BYTES_PER_BODY, "batches": []}
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for n_rays in (1, 64, 4096):
            o = np.stack([rng.uniform(-1000, 1000, n_rays), np.full(n_rays, 150.0), rng.uniform(-1000, 1000, n_rays)], 1)
            rays = W.make_rays(o, np.tile([0.0, -1.0, 0.0], (n_rays, 1)), 200.0, 0xFFFFFFFF)
            rt = torch.from_numpy(rays.view(np.uint8)).to("cuda:0")
            ht = torch.zeros(n_rays * 40, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            reps = 50 if n_rays < 4096 else 10
            times = []
            for k in range(5 + reps):
                ev0.record(stream)
                w.raycast_device(rt, ht)
                ev1.record(stream)
                ev1.synchronize()
                if k >= 5:
                    times.append(ev0.elapsed_time(ev1) * 1e3)
            us = float(np.median(times))
            hits = ht.cpu().numpy().view(W.RAY_HIT_DTYPE)
            rate = BYTES_PER_BODY * n / (us * 1e-6)
            out["batches"].append({"rays": n_rays, "us_per_batch": round(us, 2), "us_min": round(float(np.min(times)), 2),
                                   "rays_per_s": round(n_rays / (us * 1e-6)), "body_pass_GBps": round(rate / 1e9, 1),
                                   "of_tick_rate": round(rate / TICK_RATE, 3), "hit_kinds": np.bincount(hits["kind"], minlength=4).tolist()})
            print(json.dumps(out["batches"][-1]), flush=True)
        o = np.stack([rng.uniform(-1000, 1000, 64), np.full(64, 150.0), rng.uniform(-1000, 1000, 64)], 1)
        for _ in range(3):
            w.raycast_all(o, np.tile([0.0, -1.0, 0.0], (64, 1)), 200.0)
        times = []
        for _ in range(20):
            t0 = time.perf_counter()
            r = w.raycast_all(o, np.tile([0.0, -1.0, 0.0], (64, 1)), 200.0)
            times.append((time.perf_counter() - t0) * 1e6)
        out["raycast_all_64"] = {"us_wall_median": round(float(np.median(times)), 1), "hits": int(r["offsets"][-1])}
        print(json.dumps(out["raycast_all_64"]), flush=True)
        print(json.dumps(out))


if __name__ == "__main__":
    main()
