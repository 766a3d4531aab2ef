#!/usr/bin/env python3
"""Cost of the frustum culling query (bge_world_visible*) on big flat worlds, against the only other way to the same answer.

Run on the GPU box:  python tools/measure_cull.py [--sizes 1048576,4194304] [--label text]
Per size: entities uniform in a cube, one transforms tick, then three views whose field of view is bisected (with the query's own
count) to roughly 1 %, 10 % and 100 % visible.  Per view:
  device   HIP events on the world's stream around bge_world_visible_device (its three kernels back to back; indices + world
           matrices out): warm-up, then five regions of REPS calls, the median region / REPS.
  host     wall time of bge_world_visible (count, read-back of the total, emit, copy of the records), median of five.
  yardstick  what a caller had to do before: bge_world_download_world of all N matrices, then the rule in numpy binary32 on the
           host, wall time (median of three at 1 M, of two beyond).
Bytes are the algorithmic ones: 4 (slot) + 24 (bounds) + 1 (dirty) + 64 (matrix) read per entity, 4 + 64 written
per visible entity; the rate is set against the 8 TB/s HBM peak.  One JSON line per row.

--frames K: a frame instead — N flat Dynamic bodies falling, per frame one bge_world_tick and one bge_world_visible_device (10 % and
100 % visible), HIP events around five regions of K frames, the median region / K; and, the same way, K ticks alone and K queries
alone (the queries right after a tick, so with whatever the tick leaves to its readers).  BGE_WORLD_LIB gives the A/B.
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import banggameengine_amd as B  # noqa: E402
from banggameengine_amd import world as W  # noqa: E402

F = np.float32
HBM_PEAK = 8.0e12
REPS = 10
EXTENT = 500.0


def planes_of(fov_deg):
    """Eye at (0, 0, -3 * EXTENT) looking down +z, square aspect, far plane behind the cube."""
    h = 1.0 / math.tan(math.radians(fov_deg) * 0.5)
    near, far = 1.0, 8.0 * EXTENT
    view = np.eye(4)
    view[3, :3] = (0.0, 0.0, 3.0 * EXTENT)
    proj = np.zeros((4, 4))
    proj[0, 0], proj[1, 1], proj[2, 3] = h, h, 1.0
    proj[2, 2], proj[3, 2] = far / (far - near), -near * far / (far - near)
    return W.frustum_planes((view @ proj).astype(F).reshape(16), False)


def rule_numpy(m, c, h, planes):
    """include/bge_world.h's rule in binary32 (every entity here is renderable and clean)."""
    vis = np.ones(len(m), bool)
    cw = [((c[:, 0] * m[:, j] + c[:, 1] * m[:, 4 + j]) + c[:, 2] * m[:, 8 + j]) + m[:, 12 + j] for j in range(3)]
    for a, b, c4, d in planes:
        e = [(a * m[:, 4 * i] + b * m[:, 4 * i + 1]) + c4 * m[:, 4 * i + 2] for i in range(3)]
        r = (np.abs(e[0]) * h[:, 0] + np.abs(e[1]) * h[:, 1]) + np.abs(e[2]) * h[:, 2]
        sd = ((a * cw[0] + b * cw[1]) + c4 * cw[2]) + d
        vis &= sd >= -r
    return np.nonzero(vis)[0].astype(np.uint32)


def tune(w, n, share):
    lo, hi = 0.01, 120.0
    if w.visible_count(planes_of(hi)) <= share * n:
        return hi
    for _ in range(30):
        mid = 0.5 * (lo + hi)
        if w.visible_count(planes_of(mid)) > share * n:
            hi = mid
        else:
            lo = mid
    return hi


def measure(n, label):
    rng = np.random.default_rng(9)
    stream = torch.cuda.Stream()
    center = rng.uniform(-1, 1, (n, 3)).astype(F)
    half = rng.uniform(0.05, 2, (n, 3)).astype(F)
    with B.World(device=0, stream=stream.cuda_stream) as w:
        w.set_topology(np.full(n, W.NO_PARENT, np.uint32))
        w.upload_trs(rng.uniform(-EXTENT, EXTENT, (n, 3)).astype(F), rng.uniform(-3, 3, (n, 3)).astype(F), rng.uniform(0.25, 4, (n, 3)).astype(F))
        w.upload_bounds(center, half)
        w.tick(flags=W.TICK_TRANSFORMS)
        d_total = torch.zeros(1, dtype=torch.int64, device="cuda:0")
        d_ent = torch.empty(n, dtype=torch.int32, device="cuda:0")
        d_world = torch.empty((n, 16), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for target in (0.01, 0.10, 1.00):
            planes = planes_of(tune(w, n, target)) if target < 1.0 else None
            nv = w.visible_count(planes)
            for _ in range(3):
                w.visible_device(planes, d_ent.data_ptr(), d_world.data_ptr(), 0, n, d_total.data_ptr())
            w.sync()
            regions = []
            for _ in range(5):
                ev0.record(stream)
                for _ in range(REPS):
                    w.visible_device(planes, d_ent.data_ptr(), d_world.data_ptr(), 0, n, d_total.data_ptr())
                ev1.record(stream)
                ev1.synchronize()
                regions.append(ev0.elapsed_time(ev1) * 1e3 / REPS)
            assert int(d_total.item()) == nv
            us = float(np.median(regions))
            host = []
            for k in range(6):
                t0 = time.perf_counter()
                got = w.visible(planes, want_world=True)
                if k:
                    host.append((time.perf_counter() - t0) * 1e6)
            yard = []
            for k in range(3 if n <= (1 << 20) else 2):
                t0 = time.perf_counter()
                ref = rule_numpy(w.download_world(), center, half, np.zeros((0, 4), F) if planes is None else planes)
                yard.append((time.perf_counter() - t0) * 1e6)
            assert np.array_equal(ref, got["entities"]), "the device list differs from the rule on the downloaded matrices"
            nbytes = n * (4 + 24 + 1 + 64) + nv * (4 + 64)
            row = {"label": label, "entities": n, "visible": nv, "share": round(nv / n, 4), "device_us": round(us, 1),
                   "device_us_min": round(float(np.min(regions)), 1), "algorithmic_MB": round(nbytes / 1e6, 1),
                   "GBps": round(nbytes / (us * 1e-6) / 1e9, 1), "of_hbm_peak": round(nbytes / (us * 1e-6) / HBM_PEAK, 3),
                   "host_form_us": round(float(np.median(host)), 1), "yardstick_us": round(float(np.median(yard)), 1),
                   "yardstick_over_host_form": round(float(np.median(yard)) / float(np.median(host)), 1)}
            print(json.dumps(row), flush=True)


def measure_frames(n, label, frames):
    rng = np.random.default_rng(9)
    stream = torch.cuda.Stream()
    pos = rng.uniform(-EXTENT, EXTENT, (n, 3)).astype(F)
    vel = np.zeros((n, 3), F)
    vel[:, 1] = rng.uniform(-3, -1, n).astype(F)  # (faster than the sleeping threshold from the start)
    with B.World(device=0, stream=stream.cuda_stream) as w:
        w.set_topology(np.full(n, W.NO_PARENT, np.uint32))
        w.upload_trs(pos, rng.uniform(-3, 3, (n, 3)).astype(F), rng.uniform(0.25, 4, (n, 3)).astype(F))
        w.upload_bodies(np.ones(n, np.uint8))
        w.upload_bounds(rng.uniform(-1, 1, (n, 3)).astype(F), rng.uniform(0.05, 2, (n, 3)).astype(F))
        w.tick()
        w.set_velocities(vel)
        w.tick(ticks=20)
        d_total = torch.zeros(1, dtype=torch.int64, device="cuda:0")
        d_ent = torch.empty(n, dtype=torch.int32, device="cuda:0")
        d_world = torch.empty((n, 16), dtype=torch.float32, device="cuda:0")
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def regions(body):
            for _ in range(10):
                body()
            w.sync()
            out = []
            for _ in range(5):
                ev0.record(stream)
                for _ in range(frames):
                    body()
                ev1.record(stream)
                ev1.synchronize()
                out.append(ev0.elapsed_time(ev1) * 1e3 / frames)
            return [round(x, 2) for x in out]

        for target in (0.10, 1.00):
            planes = planes_of(tune(w, n, target)) if target < 1.0 else None
            cull = lambda: w.visible_device(planes, d_ent.data_ptr(), d_world.data_ptr(), 0, n, d_total.data_ptr())
            frame = regions(lambda: (w.tick(), cull()))
            tick = regions(lambda: w.tick())
            query = regions(cull)
            print(json.dumps({"label": label, "entities": n, "share": round(w.visible_count(planes) / n, 4), "frames_per_region": frames,
                              "frame_us": float(np.median(frame)), "frame_us_all": frame, "tick_us": float(np.median(tick)),
                              "tick_us_all": tick, "query_us": float(np.median(query)), "query_us_all": query,
                              "lib": os.environ.get("BGE_WORLD_LIB", "in-tree")}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1048576,4194304")
    ap.add_argument("--label", default="")
    ap.add_argument("--frames", type=int, default=0, help="measure frames of one tick and one query instead (see above)")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    for n in (int(s) for s in args.sizes.split(",")):
        if args.frames:
            measure_frames(n, args.label, args.frames)
        else:
            measure(n, args.label)


if __name__ == "__main__":
    main()
