#!/usr/bin/env python3
"""Cost of a batch of sphere moves (bge_world_sphere_move_device) beside the sphere-cast passes it is made of.

Run on the GPU box:  python tools/measure_move.py [n_bodies]
Scene: that of tools/measure_sphere_queries.py — n_bodies (default 1 M) boxes and capsules mixed, resting on the plane over
2,000 x 2,000 units.  Batches of 1,024 and 65,536 movers of radius 0.4 start 0.5 .. 2 above the plane and ask a displacement of
length 1 .. 4 down and sideways, with a ground probe of 0.5.  Timed with HIP events on the world's stream (warm-up first, then the
median of the repeats), in the same process on the same world:
  move_us    one World.sphere_move_device call: BGE_MOVE_SLIDES + 1 closest-hit passes and the begin / step / finish kernels
  casts_us   BGE_MOVE_SLIDES + 1 plain World.sphere_cast_device calls of the same batch size (the movers' first-round casts)
  ratio      move_us / casts_us.  The kernels between the passes touch about 150 bytes per mover, so the ratio is expected near 1;
             it can fall below 1 because a mover that has finished asks a cast that no body is tested against.
Not a test, and not part of bench.py.
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
        out = {"bodies": n, "slides": W.MOVE_SLIDES, "batches": []}
        for nm in (1024, 65536):
            p = np.stack([rng.uniform(-1000, 1000, nm), rng.uniform(0.5, 2.0, nm), rng.uniform(-1000, 1000, nm)], 1)
            az, down = rng.uniform(0, 2 * np.pi, nm), rng.uniform(0.1, 1.0, nm)
            d = np.stack([np.cos(az) * (1 - down), -down, np.sin(az) * (1 - down)], 1)
            d *= (rng.uniform(1.0, 4.0, nm) / np.linalg.norm(d, axis=1))[:, None]
            reps = 7 if nm == 1024 else 3
            mt = torch.from_numpy(W.make_sphere_moves(p, d, 0.4, 0.01, 0.5).view(np.uint8)).to("cuda:0")
            rt = torch.zeros(nm * 80, dtype=torch.uint8, device="cuda:0")
            ct = torch.from_numpy(W.make_sphere_casts(p, d, 1.0, 0.4).view(np.uint8)).to("cuda:0")
            ht = torch.zeros(nm * 40, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()

            def casts():
                for _ in range(W.MOVE_SLIDES + 1):
                    w.sphere_cast_device(ct, ht)

            row = {"movers": nm}
            row["move_us"] = timed_device(stream, lambda: w.sphere_move_device(mt, rt), reps)
            row["casts_us"] = timed_device(stream, casts, reps)
            row["ratio"] = round(row["move_us"] / row["casts_us"], 3)
            res = rt.cpu().numpy().view(W.SPHERE_MOVE_RESULT_DTYPE)
            row["n_hits_histogram"] = np.bincount(res["n_hits"], minlength=W.MOVE_SLIDES + 1).tolist()
            row["grounded"] = int(((res["flags"] & W.MOVE_GROUNDED) != 0).sum())
            row["out_of_slides"] = int(((res["flags"] & W.MOVE_OUT_OF_SLIDES) != 0).sum())
            out["batches"].append(row)
            print(json.dumps(row), flush=True)
        print(json.dumps(out))


if __name__ == "__main__":
    main()
