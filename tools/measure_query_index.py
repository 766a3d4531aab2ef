#!/usr/bin/env python3
"""What the query index (include/bge_world.h "Query index") costs and saves, beside the all-bodies pass in the same process.

Run on an MI355X:  python tools/measure_query_index.py [n_bodies] [cell_edge]
Scene: that of tools/measure_characters.py — n_bodies (default 1 M) boxes and capsules mixed, resting on the plane
over 2,000 x 2,000 units, with n_bodies / 8 Static flat slabs; 1,024 characters of radius 0.4 walking 0.03 .. 0.06 a step.  The
index runs with cell_edge (default 4: the largest box of the scene has a bounding radius of 1.74) and min_work = 0.
Every figure is the median of five regions between HIP events on the world's stream after two warm-up regions; the routes alternate
off / on / off in one process on one world, and the off figures carry the max - min of their regions (`spread`).
  update_us        one World.characters_update(dt, 1): off, on, off again
  update2_us       one World.characters_update(dt, 2), index on: update2 - update is a step without the build, and
  build_us         update - (update2 - update) the build alone, by difference
  casts            World.sphere_cast_device of 1, 64, 1,024, 4,096 and 65,536 casts like a character's (radius 0.4, 0.05 .. 0.5 long,
                   level), both routes, and the stats of the indexed call
  first_win        the smallest measured size at which the indexed route is ahead, and the size before it
  characters_100k  one update of 100,000 characters, both routes
  bar              on beats off at 1,024 characters by more than three times the spread of the off regions
Writes the JSON line to stdout.  Not a test, and not part of bench.py.
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

REPS = 5


def regions(stream, call):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for k in range(2 + REPS):
        ev0.record(stream)
        call()
        ev1.record(stream)
        ev1.synchronize()
        if k >= 2:
            times.append(ev0.elapsed_time(ev1) * 1e3)
    return times


def figure(times):
    return {"us": round(float(np.median(times)), 1), "spread": round(float(max(times) - min(times)), 1)}


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
    edge = float(sys.argv[2]) if len(sys.argv) > 2 else 4.0
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
        dt = 1.0 / 60.0
        radius, skin, probe, height = 0.4, 0.01, 0.3, 0.5
        row = {"bodies": n, "slabs": n_slabs, "cell_edge": edge, "regions": REPS}

        def index(on):
            w.set_query_index(on, cell_edge=edge, min_work=0)

        def characters(nc):
            p = np.stack([rng.uniform(-1000, 1000, nc), np.full(nc, radius + skin + 0.005), rng.uniform(-1000, 1000, nc)], 1)
            az = rng.uniform(0, 2 * np.pi, nc)
            walk = np.stack([np.cos(az), np.sin(az)], 1) * rng.uniform(0.03, 0.06, nc)[:, None]
            index(False)
            w.characters_create(W.make_characters(p, radius, skin, height, 0.7071068, probe))
            w.characters_update(dt, 3)
            w.characters_set_input(W.make_character_inputs(walk[:, 0], walk[:, 1]))
            out = {}
            for name, on, steps in (("off", False, 1), ("on", True, 1), ("on2", True, 2), ("off_again", False, 1)):
                index(on)
                out[name] = figure(regions(stream, lambda: w.characters_update(dt, steps)))
                if on and steps == 1:
                    out["stats"] = w.query_index_stats()
            index(False)
            return out

        c = characters(1024)
        row["characters"] = 1024
        row["update_us"] = {k: c[k] for k in ("off", "on", "off_again")}
        row["update2_us"] = c["on2"]
        row["build_us"] = round(c["on"]["us"] - (c["on2"]["us"] - c["on"]["us"]), 1)
        row["update_stats"] = c["stats"]
        off_us = min(c["off"]["us"], c["off_again"]["us"])
        off_spread = max(c["off"]["spread"], c["off_again"]["spread"])
        row["ratio_off_over_on"] = round(off_us / c["on"]["us"], 2)
        row["bar"] = {"off_minus_on_us": round(off_us - c["on"]["us"], 1), "three_spreads_us": round(3 * off_spread, 1),
                      "met": bool(off_us - c["on"]["us"] > 3 * off_spread)}

        casts = {}
        sizes = (1, 64, 1024, 4096, 65536)
        for m in sizes:
            o = np.stack([rng.uniform(-1000, 1000, m), np.full(m, radius + skin), rng.uniform(-1000, 1000, m)], 1)
            az = rng.uniform(0, 2 * np.pi, m)
            d = np.stack([np.cos(az), np.zeros(m), np.sin(az)], 1)
            rec = torch.from_numpy(W.make_sphere_casts(o, d, rng.uniform(0.05, 0.5, m), np.full(m, radius), np.full(m, 0xFFFFFFFF, np.uint32)).view(np.uint8)).to("cuda:0")
            hits = torch.zeros(m * 40, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            one = {}
            for name, on in (("off", False), ("on", True), ("off_again", False)):
                index(on)
                one[name] = figure(regions(stream, lambda: w.sphere_cast_device(rec, hits)))
                if on:
                    st = w.query_index_stats()
                    one["far"], one["wide"] = st["queries_far"], st["bodies_wide"]
            casts[str(m)] = one
        index(False)
        row["casts"] = casts
        wins = [m for m in sizes if casts[str(m)]["on"]["us"] < min(casts[str(m)]["off"]["us"], casts[str(m)]["off_again"]["us"])]
        first = wins[0] if wins else None
        row["first_win"] = {"casts": first, "size_before": None if first is None or first == sizes[0] else sizes[sizes.index(first) - 1],
                            "n_slots": total}
        if os.environ.get("MEASURE_100K", "1") != "0":
            big = characters(100000)
            row["characters_100k"] = {"update_us": {k: big[k] for k in ("off", "on", "off_again")}, "stats": big["stats"]}
        else:
            row["characters_100k"] = "not measured"
        print(json.dumps(row))


if __name__ == "__main__":
    main()
