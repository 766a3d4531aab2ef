#!/usr/bin/env python3
"""Cost of the debug overlay query (bge_world_debug_lines_device) on big worlds.

Run on the GPU box:  python tools/measure_debug_lines.py
Cases: 1 M boxes (336 MB of lines: fits the Infinity Cache only partly), 4 M boxes (1.3 GB: beyond it), 100 k capsules, 1 M boxes
with a region holding ~1,000 of them, and the contact pass alone (BGE_DEBUG_CONTACTS) on 100 k crates resting on the plane.
Each case is timed with HIP events on the world's stream around the call (warm-up first, then the median of the repeats).  The
rate reported is bytes of lines written / time; reads are a few % of that (DESIGN.md 4.12 sets it against the whole-line store
rate of tools/ubench_world_rows.hip).
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


def case(name, n, capsules, flags=W.DEBUG_SHAPES, region=None, plane=False, rest=False, reps=20):
    rng = np.random.default_rng(5)
    stream = torch.cuda.Stream()
    with B.World(device=0, stream=stream.cuda_stream) as w:
        w.set_topology(np.full(n, W.NO_PARENT, np.uint32))
        size = np.full((n, 3), 0.5, np.float32)
        y = np.full(n, 0.5 if rest else 5.0)
        pos = np.stack([rng.uniform(-1000, 1000, n), y, rng.uniform(-1000, 1000, n)], 1).astype(np.float32)
        w.upload_trs(pos, rng.uniform(-3, 3, (n, 3)).astype(np.float32) * (0.0 if rest else 1.0), np.ones((n, 3), np.float32))
        w.upload_bodies(np.full(n, W.BODY_DYNAMIC if rest else W.BODY_STATIC, np.uint8), None, np.full(n, 1 if capsules else 0, np.uint8), size)
        w.set_ground_plane(plane)
        w.tick(flags=W.TICK_ALL, ticks=20 if rest else 1)
        total = torch.zeros(1, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        w.debug_lines_device(0, 0, total.data_ptr(), flags, region)
        w.sync()
        n_lines = int(total.item())
        lines = torch.empty(max(n_lines, 1) * 28, dtype=torch.uint8, device="cuda:0")
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        times = []
        for k in range(3 + reps):
            ev0.record(stream)
            w.debug_lines_device(lines.data_ptr(), n_lines, total.data_ptr(), flags, region)
            ev1.record(stream)
            ev1.synchronize()
            if k >= 3:
                times.append(ev0.elapsed_time(ev1) * 1e3)
        us = float(np.median(times))
        out = {"case": name, "entities": n, "lines": n_lines, "MB_written": round(n_lines * 28 / 1e6, 1),
               "us_median": round(us, 1), "us_min": round(float(np.min(times)), 1), "GBps_written": round(n_lines * 28 / (us * 1e-6) / 1e9, 1)}
        print(json.dumps(out), flush=True)
        return out


def main():
    torch.cuda.set_device(0)
    case("1M boxes", 1 << 20, False)
    case("4M boxes", 1 << 22, False, reps=10)
    case("100k capsules", 100_000, True)
    case("1M boxes, region of ~1000", 1 << 20, False, region=((-31.0, 0.0, -31.0), (31.0, 10.0, 31.0)))
    case("contacts of 100k resting crates", 100_000, False, flags=W.DEBUG_CONTACTS, plane=True, rest=True)


if __name__ == "__main__":
    main()
