"""What crowd separation costs.  One process, one JSON line:

  * characters_update(dt, 1) at 1 M characters standing on the plane at about two overlaps each, with the crowd off and on;
  * the Separate stage alone: the crowd query over the same positions and radii (the stage's launches plus the r_max reduction,
    which the character path takes from the descs instead);
  * the crowd query alone through the hashed grid (BGE_CROWD_GRID_MIN=1) and through all pairs at n = 256, 4 k, 64 k and 1 M, and
    at the powers of two between 32 and 16 k for the crossover that the default of BGE_CROWD_GRID_MIN rests on.

    python tools/measure_crowd.py [--n 1000000] [--no-pairs-1m] [--crossover-only]

Every figure is the median of five regions; a region is `calls` calls between two events on the world's stream, after a warm-up of
the same shape.  All pairs at 1 M is 10^12 pair tests: one call per region and two regions."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import banggameengine_amd as B  # noqa: E402
from banggameengine_amd import world as W  # noqa: E402

DT = 1.0 / 60.0
RADIUS = 0.5
REGIONS = 5
GRID, PAIRS = "1", str(1 << 31)


def standing(n, rng):
    """n centres on y = radius + skin, uniform over a square sized for two overlaps each: density * pi * (2 r)^2 = 2."""
    side = float(np.sqrt(n * np.pi * (2 * RADIUS) ** 2 / 2.0))
    p = np.zeros((n, 3), np.float32)
    p[:, 0], p[:, 2] = rng.uniform(0, side, n), rng.uniform(0, side, n)
    p[:, 1] = RADIUS + 0.01
    return p


def regions(stream, fn, calls, n_regions=REGIONS, warmup=2):
    """Median, min and max over the regions of the time of one call, in ms."""
    for _ in range(warmup):
        fn()
    stream.synchronize()
    ms = []
    for _ in range(n_regions):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(calls):
            fn()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b) / calls)
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)), calls=calls, regions=n_regions)


def query_figures(w, stream, n, rng, pairs=True):
    spheres = W.make_crowd_spheres(standing(n, rng), RADIUS)
    d_spheres = torch.from_numpy(spheres.view(np.uint8).copy()).to("cuda:0")
    d_hits = torch.zeros(32 * n, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    out = dict(n=n)
    answers = {}
    for name, env in (("grid", GRID), ("pairs", PAIRS)):
        if name == "pairs" and not pairs:
            continue
        os.environ["BGE_CROWD_GRID_MIN"] = env
        huge = name == "pairs" and n > 100_000
        calls = 1 if huge else max(1, min(200, 4_000_000 // n)) if name == "grid" else max(1, min(200, int(2e10 / (float(n) * n))))
        out[name] = regions(stream, lambda: w.crowd_query_device(d_spheres, d_hits), calls, 2 if huge else REGIONS, 1 if huge else 2)
        w.sync()
        answers[name] = d_hits.cpu().numpy().tobytes()
    if len(answers) == 2:
        out["same_bytes"] = answers["grid"] == answers["pairs"]
    hits = np.frombuffer(answers["grid"], W.CROWD_HIT_DTYPE)
    out["mean_overlaps"] = float(hits["n_overlaps"].mean())
    os.environ.pop("BGE_CROWD_GRID_MIN", None)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--no-pairs-1m", action="store_true")
    ap.add_argument("--crossover-only", action="store_true", help="only the two paths at 32 .. 16384 spheres")
    args = ap.parse_args()
    rng = np.random.default_rng(4232)
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    out = dict(n_characters=args.n)
    sizes = (32, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384)
    if args.crossover_only:
        with B.World(device=0, stream=stream.cuda_stream) as w:
            print(json.dumps(dict(crossover=[query_figures(w, stream, n, rng) for n in sizes])))
        return
    with B.World(device=0, stream=stream.cuda_stream) as w:
        w.set_topology(np.full(1, W.NO_PARENT, np.uint32))
        w.upload_trs(np.zeros((1, 3), np.float32), np.zeros((1, 3), np.float32), np.ones((1, 3)))
        w.upload_bodies(np.uint8([W.BODY_NONE]), None, np.uint8([0]), np.float32([[0.5, 0.5, 0.5]]), np.uint32([1]), np.uint32([0xFFFFFFFF]))
        w.set_ground_plane(True)
        w.tick(flags=W.TICK_ALL | W.TICK_BROADPHASE)
        pos = standing(args.n, rng)
        descs = W.make_characters(pos, RADIUS)
        calls = max(1, min(20, 4_000_000 // args.n))
        for name, on in (("update_off", False), ("update_on", True), ("update_off_again", False)):
            w.characters_create(descs)
            if on:
                w.characters_crowd(True)
            out[name] = regions(stream, lambda: w.characters_update(DT, 1), calls)
            if on:
                h = w.characters_crowd_hits()
                out["pushed_after"] = int(((h["flags"] & W.CROWD_PUSHED) != 0).sum())
        out["separate_by_difference_ms"] = out["update_on"]["median_ms"] - out["update_off"]["median_ms"]
        w.characters_create(descs[:1])
        sep = query_figures(w, stream, args.n, np.random.default_rng(4232), pairs=False)
        out["separate_alone"] = sep["grid"]
        out["mean_overlaps"] = sep["mean_overlaps"]
        out["query"] = [query_figures(w, stream, n, rng, pairs=not (args.no_pairs_1m and n > 100_000)) for n in (256, 4096, 65536, 1_000_000)]
        out["crossover"] = [query_figures(w, stream, n, rng) for n in sizes]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
