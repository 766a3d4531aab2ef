#!/usr/bin/env python3
"""Cost of the draw-batch query (bge_world_draw_batches*) on big flat worlds, against what a caller had to do without it.

Run on the GPU box:  python tools/measure_batches.py [--sizes 1048576,4194304] [--keys 64,4096] [--label text]
Per size: entities uniform in a cube, one transforms tick, then three views whose field of view is bisected (with
bge_world_visible's own count) to roughly 1 %, 10 % and 100 % visible; per view, uniformly random keys over 64 and over 4096
values (one and two sort passes).  Per point:
  device     HIP events on the world's stream around bge_world_draw_batches_device (batches, indices + world matrices out):
             warm-up, then five regions of REPS calls, the median region / REPS.
  cull       the same around bge_world_visible_device alone (indices + world matrices out): the grouping's cost over plain
             compaction is device / cull.
  yardstick  what the parent commit offers for the same answer: bge_world_visible (host form, indices + world matrices), then a
             stable numpy sort of the visible entities' keys, the gather of indices and matrices in that order and a bincount for
             the batches, wall time (median of three).  Its result must equal the host form of the new query byte for byte.
  host form  wall time of World.draw_batches (batches, indices + world matrices), median of three.  The Python method counts
             first and then asks for the records, as World.visible does, so it runs the test and scan passes twice; the C entry
             point called once with room for n_entities records does them once.  yardstick_over_host_form therefore understates
             bge_world_draw_batches itself (the yardstick's World.visible pays the same double count).
One JSON line per point.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import banggameengine_amd as B  # noqa: E402
from banggameengine_amd import world as W  # noqa: E402
from measure_cull import EXTENT, F, REPS, planes_of, tune  # noqa: E402


def timed(stream, call):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        call()
    stream.synchronize()
    regions = []
    for _ in range(5):
        ev0.record(stream)
        for _ in range(REPS):
            call()
        ev1.record(stream)
        ev1.synchronize()
        regions.append(ev0.elapsed_time(ev1) * 1e3 / REPS)
    return float(np.median(regions)), float(np.min(regions))


def yardstick(w, planes, keys, n_keys):
    vis = w.visible(planes, want_world=True)
    k = keys[vis["entities"]]
    order = np.argsort(k, kind="stable")  # (every key is below n_keys here; the list is in entity order)
    count = np.bincount(k, minlength=n_keys).astype(np.uint32)
    first = (np.cumsum(count, dtype=np.uint64) - count).astype(np.uint32)
    return np.stack([first, count], axis=1), vis["entities"][order], vis["world"][order]


def measure(n, key_counts, label):
    rng = np.random.default_rng(9)
    stream = torch.cuda.Stream()
    with B.World(device=0, stream=stream.cuda_stream) as w:
        w.set_topology(np.full(n, W.NO_PARENT, np.uint32))
        w.upload_trs(rng.uniform(-EXTENT, EXTENT, (n, 3)).astype(F), rng.uniform(-3, 3, (n, 3)).astype(F), rng.uniform(0.25, 4, (n, 3)).astype(F))
        w.upload_bounds(rng.uniform(-1, 1, (n, 3)).astype(F), rng.uniform(0.05, 2, (n, 3)).astype(F))
        w.tick(flags=W.TICK_TRANSFORMS)
        d_total = torch.zeros(1, dtype=torch.int64, device="cuda:0")
        d_ent = torch.empty(n, dtype=torch.int32, device="cuda:0")
        d_world = torch.empty((n, 16), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        for target in (0.01, 0.10, 1.00):
            planes = planes_of(tune(w, n, target)) if target < 1.0 else None
            nv = w.visible_count(planes)
            cull_us, _ = timed(stream, lambda: w.visible_device(planes, d_ent.data_ptr(), d_world.data_ptr(), 0, n, d_total.data_ptr()))
            for n_keys in key_counts:
                keys = rng.integers(0, n_keys, n).astype(np.uint32)
                w.upload_draw_keys(keys)
                d_batches = torch.empty((n_keys, 2), dtype=torch.int32, device="cuda:0")
                torch.cuda.synchronize()
                us, us_min = timed(stream, lambda: w.draw_batches_device(planes, n_keys, d_batches.data_ptr(), d_ent.data_ptr(),
                                                                         d_world.data_ptr(), 0, n, d_total.data_ptr()))
                assert int(d_total.item()) == nv
                host, yard = [], []
                for k in range(4):
                    t0 = time.perf_counter()
                    got = w.draw_batches(planes, n_keys, want_world=True)
                    t1 = time.perf_counter()
                    ref = yardstick(w, planes, keys, n_keys)
                    t2 = time.perf_counter()
                    if k:
                        host.append((t1 - t0) * 1e6)
                        yard.append((t2 - t1) * 1e6)
                assert got["batches"].tobytes() == ref[0].tobytes() and got["entities"].tobytes() == ref[1].tobytes()
                assert got["world"].tobytes() == ref[2].tobytes(), "the device's records differ from the host's sort of bge_world_visible"
                assert d_ent[:nv].cpu().numpy().view(np.uint32).tobytes() == ref[1].tobytes()
                row = {"label": label, "entities": n, "visible": nv, "share": round(nv / n, 4), "n_keys": n_keys,
                       "device_us": round(us, 1), "device_us_min": round(us_min, 1), "cull_device_us": round(cull_us, 1),
                       "device_over_cull": round(us / cull_us, 2), "host_form_us": round(float(np.median(host)), 1),
                       "yardstick_us": round(float(np.median(yard)), 1), "yardstick_over_device": round(float(np.median(yard)) / us, 1),
                       "yardstick_over_host_form": round(float(np.median(yard)) / float(np.median(host)), 2)}
                print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1048576,4194304")
    ap.add_argument("--keys", default="64,4096")
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    for n in (int(s) for s in args.sizes.split(",")):
        measure(n, [int(k) for k in args.keys.split(",")], args.label)


if __name__ == "__main__":
    main()
