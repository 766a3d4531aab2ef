#!/usr/bin/env python3
"""Cost of a batch of sphere step moves (bge_world_sphere_step_move_device) beside what a caller composes from the plain move.

Run on an MI355X:  python tools/measure_step_move.py [n_bodies]
Scene: that of tools/measure_move.py — n_bodies (default 1 M) boxes and capsules mixed, resting on the plane over 2,000 x 2,000
units — with n_bodies / 8 Static flat slabs added (half extents 0.5 .. 2, tops 0.1 .. 0.6 above the plane, turned about y).
Batches of 1,024 and 65,536 movers of radius 0.4 and skin 0.01 stand on the plane and ask a level displacement of length 1 .. 4
with step_height 0.5 and a probe of 0.3.  Timed with HIP events on the world's stream (warm-up first, then the median of the
repeats), in the same process on the same world:
  step_us      one World.sphere_step_move_device call: 7 passes, 4 of them over two casts per mover
  compose_us   the caller's recipe from World.sphere_move_device: the plain move, an up move, a forward move from where that ended,
               a down move by the rise plus the probe, and the choice — four calls, 20 passes, the records glued in torch on the
               same stream (no host round trip, which a caller without torch would add)
  move_us      one World.sphere_move_device call of the same batch
The composition is the recipe INTEGRATION.md used to give, not the rule bit for bit (its Up and Down are moves, not casts), so
only its cost is compared; how many of its movers end stepped is printed beside the device's count.
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
        out = {"bodies": n, "slabs": n_slabs, "batches": []}
        radius, skin, probe, height = 0.4, 0.01, 0.3, 0.5
        for nm in (1024, 65536):
            p = np.stack([rng.uniform(-1000, 1000, nm), np.full(nm, radius + skin), rng.uniform(-1000, 1000, nm)], 1)
            az = rng.uniform(0, 2 * np.pi, nm)
            d = np.stack([np.cos(az), np.zeros(nm), np.sin(az)], 1) * rng.uniform(1.0, 4.0, nm)[:, None]
            reps = 7 if nm == 1024 else 3
            st = torch.from_numpy(W.make_sphere_step_moves(p, d, radius, skin, probe, step_height=height).view(np.uint8)).to("cuda:0")
            rt = torch.zeros(nm * 80, dtype=torch.uint8, device="cuda:0")
            mv = torch.from_numpy(W.make_sphere_moves(p, d, radius, skin, probe).view(np.float32).reshape(nm, 12)).to("cuda:0")
            rec = [torch.zeros_like(mv) for _ in range(3)]
            res = [torch.zeros(nm, 20, dtype=torch.float32, device="cuda:0") for _ in range(4)]
            chosen = torch.zeros(nm, 20, dtype=torch.float32, device="cuda:0")
            took = torch.zeros(nm, dtype=torch.bool, device="cuda:0")
            torch.cuda.synchronize()

            def compose():
                plain, up, fwd, down = res
                w.sphere_move_device(mv, plain)
                r_up, r_fwd, r_down = rec
                r_up.copy_(mv)
                r_up[:, 3:6] = 0
                r_up[:, 4] = height
                r_up[:, 8] = 0
                w.sphere_move_device(r_up, up)
                r_fwd.copy_(mv)
                r_fwd[:, 0:3] = up[:, 0:3]
                r_fwd[:, 4] = 0
                r_fwd[:, 8] = 0
                w.sphere_move_device(r_fwd, fwd)
                r_down.copy_(mv)
                r_down[:, 0:3] = fwd[:, 0:3]
                r_down[:, 3:6] = 0
                r_down[:, 4] = -((up[:, 1] - mv[:, 1]) + probe)
                w.sphere_move_device(r_down, down)
                grounded = (down.view(torch.int32)[:, 6] & W.MOVE_GROUNDED) != 0
                hit = plain.view(torch.int32)[:, 7] >= 1
                gs = (down[:, 0] - mv[:, 0]) * mv[:, 3] + (down[:, 2] - mv[:, 2]) * mv[:, 5]
                gp = (plain[:, 0] - mv[:, 0]) * mv[:, 3] + (plain[:, 2] - mv[:, 2]) * mv[:, 5]
                torch.logical_and(torch.logical_and(grounded, hit), gs > gp, out=took)
                torch.where(took[:, None], down, plain, out=chosen)

            row = {"movers": nm}
            row["step_us"] = timed_device(stream, lambda: w.sphere_step_move_device(st, rt), reps)
            row["compose_us"] = timed_device(stream, compose, reps)
            row["move_us"] = timed_device(stream, lambda: w.sphere_move_device(mv, res[0]), reps)
            row["step_over_compose"] = round(row["step_us"] / row["compose_us"], 3)
            row["step_over_move"] = round(row["step_us"] / row["move_us"], 3)
            got = rt.cpu().numpy().view(W.SPHERE_STEP_RESULT_DTYPE)
            row["tried"] = int(((got["flags"] & W.MOVE_STEP_TRIED) != 0).sum())
            row["stepped"] = int(((got["flags"] & W.MOVE_STEPPED) != 0).sum())
            row["compose_stepped"] = int(took.sum().item())
            out["batches"].append(row)
            print(json.dumps(row), flush=True)
        print(json.dumps(out))


if __name__ == "__main__":
    main()
