"""What impulses and the characters' push cost.  One process per part, one JSON object, written to
profiles/impulses_measure.json (parts given on the command line are merged into what the file holds):

  apply   apply_impulses_device for 1 k, 100 k and 1 M records spread over 1 M free bodies, and for 100 k records on ONE body (the
          serial run of k_imp_apply), every kind mixed;
  push    characters_update(dt, 1) with push off, on and off again at 1,024 and 100,000 characters on the query-index
          measurement's world (1 M bodies and 125 k slabs, index on), walking;
  epoch   the tick that follows an impulse call (one CENTRAL record) against the same tick without one, on the 1 M flat headline
          scene: the price of moving both epochs on for every wave instead of the body's own;
  bench   bench.py --gpus 1 run in child processes, alternating another build of the library (--parent-lib, through
          BGE_WORLD_LIB) with the in-tree one: the headline does not use any of this and must tie.

    python tools/measure_impulses.py apply push epoch
    python tools/measure_impulses.py bench --parent-lib /path/to/libbge_world.so [--bench-runs 4]

The apply figures are the median of five regions between events on the world's stream after two warm-up regions; push and epoch
INTERLEAVE their variants (off / on, alone / after a call: seven rounds after two warm-up rounds, every round runs every variant
once) and also give the median of the per-round differences.  The max - min of the regions stands beside every figure (`spread`)."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "impulses_measure.json")
REPS = 5
DT = 1.0 / 60.0


def regions(stream, call, before=None):
    import torch
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for k in range(2 + REPS):
        if before:
            before()
        ev0.record(stream)
        call()
        ev1.record(stream)
        ev1.synchronize()
        if k >= 2:
            times.append(ev0.elapsed_time(ev1) * 1e3)
    return times


def interleaved(stream, variants, rounds=7, warmup=2):
    """variants: (name, prepare or None, call).  Every round runs each variant once, in order — prepare() outside the timed region,
    call() inside it — so that a drift of the session reaches all variants alike.  name -> the times of the rounds after the warm-up."""
    import torch
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {name: [] for name, _, _ in variants}
    for k in range(warmup + rounds):
        for name, prepare, call in variants:
            if prepare:
                prepare()
            stream.synchronize()
            ev0.record(stream)
            call()
            ev1.record(stream)
            ev1.synchronize()
            if k >= warmup:
                times[name].append(ev0.elapsed_time(ev1) * 1e3)
    return times


def figure(times):
    import numpy as np
    return {"us": round(float(np.median(times)), 1), "spread": round(float(max(times) - min(times)), 1), "regions": len(times)}


def flat_world(w, n):
    """The headline scene: n flat Dynamic bodies, ticked so that they exist and fall."""
    from banggameengine_amd import synth
    wl = synth.config("flat1m", n=n)
    w.load(wl)
    w.tick()
    w.set_velocities(wl.vel)
    w.tick(ticks=4)
    return wl


def part_apply(n_bodies):
    import numpy as np
    import torch
    import banggameengine_amd as B
    from banggameengine_amd import world as W
    rng = np.random.default_rng(4251)
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    out = {"bodies": n_bodies}
    with B.World(device=0, stream=stream.cuda_stream) as w, torch.cuda.stream(stream):
        flat_world(w, n_bodies)

        def batch(n, one_body):
            ent = np.full(n, 12345 % n_bodies, np.uint32) if one_body else rng.integers(0, n_bodies, n).astype(np.uint32)
            kind = rng.choice(np.uint32([W.IMPULSE_AT_POINT, W.IMPULSE_CENTRAL, W.IMPULSE_TORQUE]), n)
            rec = W.make_impulses(ent, rng.uniform(-1e-3, 1e-3, (n, 3)), rng.uniform(-0.5, 0.5, (n, 3)), kind)
            d = torch.from_numpy(rec.view(np.uint8).copy()).to("cuda:0")
            status = torch.zeros(n, dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()
            f = figure(regions(stream, lambda: w.apply_impulses_device(d, status)))
            w.sync()
            f["applied"] = int((status.cpu().numpy() & 1).sum())
            return f

        for n in (1000, 100_000, 1_000_000):
            out[f"{n}_spread_over_the_bodies"] = batch(n, False)
        out["100000_on_one_body"] = batch(100_000, True)
    return out


def part_push(n_bodies):
    import numpy as np
    import torch
    import banggameengine_amd as B
    from banggameengine_amd import world as W
    rng = np.random.default_rng(3)
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    n, n_slabs = n_bodies, n_bodies // 8
    out = {"bodies": n, "slabs": n_slabs, "query_index": "on, cell_edge 4, min_work 0", "force": 30.0}
    with B.World(device=0, stream=stream.cuda_stream) as w, torch.cuda.stream(stream):
        # the world of tools/measure_query_index.py
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
        w.set_query_index(True, cell_edge=4.0, min_work=0)
        radius, skin, probe, height = 0.4, 0.01, 0.3, 0.5
        for nc in (1024, 100_000):
            p = np.stack([rng.uniform(-1000, 1000, nc), np.full(nc, radius + skin + 0.005), rng.uniform(-1000, 1000, nc)], 1)
            az = rng.uniform(0, 2 * np.pi, nc)
            walk = np.stack([np.cos(az), np.sin(az)], 1) * rng.uniform(0.03, 0.06, nc)[:, None]
            w.characters_create(W.make_characters(p, radius, skin, height, 0.7071068, probe))
            w.characters_update(DT, 3)
            w.characters_set_input(W.make_character_inputs(walk[:, 0], walk[:, 1]))
            update = lambda: w.characters_update(DT, 1)
            t = interleaved(stream, [("off", lambda: w.characters_push(False), update), ("on", lambda: w.characters_push(True, 30.0), update)])
            one = {"off": figure(t["off"]), "on": figure(t["on"])}
            one["pushing_in_the_last_step"] = int((w.characters_push_records()["entity"] != W.RAY_NO_ENTITY).sum())
            one["push_by_difference_us"] = round(one["on"]["us"] - one["off"]["us"], 1)
            one["push_by_paired_difference_us"] = figure([b - a for a, b in zip(t["off"], t["on"])])
            out[str(nc)] = one
    return out


def part_epoch(n_bodies):
    import numpy as np
    import torch
    import banggameengine_amd as B
    from banggameengine_amd import world as W
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    out = {"bodies": n_bodies}
    with B.World(device=0, stream=stream.cuda_stream) as w, torch.cuda.stream(stream):
        flat_world(w, n_bodies)
        rec = torch.from_numpy(W.make_impulses([7], [(1e-6, 0.0, 0.0)]).view(np.uint8).copy()).to("cuda:0")
        torch.cuda.synchronize()
        kick = lambda: w.apply_impulses_device(rec)
        settle = lambda: w.tick()  # (the tick after an impulse call earns the per-wave words back: the next one is the ordinary case)

        def kicked():
            settle()
            kick()

        t = interleaved(stream, [("tick_alone", settle, lambda: w.tick()), ("tick_after_an_impulse_call", kicked, lambda: w.tick()),
                                 ("four_ticks_alone", settle, lambda: w.tick(ticks=4)),
                                 ("four_ticks_after_an_impulse_call", kicked, lambda: w.tick(ticks=4)), ("the_impulse_call_itself", settle, kick)])
        for name, times in t.items():
            out[name] = figure(times)
        out["epoch_bump_by_paired_difference_us"] = figure([b - a for a, b in zip(t["tick_alone"], t["tick_after_an_impulse_call"])])
        out["epoch_bump_four_ticks_by_paired_difference_us"] = figure([b - a for a, b in zip(t["four_ticks_alone"], t["four_ticks_after_an_impulse_call"])])
    return out


def part_bench(parent_lib, runs, steps, warmup):
    """bench.py in child processes, parent's library and the in-tree one in turn; the margin is the parent's own spread."""
    def one(lib):
        env = dict(os.environ)
        env.pop("BGE_WORLD_LIB", None)
        if lib:
            env["BGE_WORLD_LIB"] = lib
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                           env=env, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError(f"bench.py failed ({r.returncode}): {r.stdout[-2000:]}{r.stderr[-2000:]}")
        line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        return {"value": line["value"], "unit": line["unit"], "ms_per_step": line["ms_per_step"],
                "kernel_ms_per_launch": line.get("roofline", {}).get("kernel_ms_per_launch")}

    out = {"steps": steps, "warmup": warmup, "parent": [], "this": []}
    for _ in range(runs):
        out["parent"].append(one(parent_lib))
        out["this"].append(one(None))
    for who in ("parent", "this"):
        v = sorted(r["value"] for r in out[who])
        out[who + "_median"] = (v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2
        out[who + "_min"], out[who + "_max"] = v[0], v[-1]
    out["margin_the_parents_own_spread"] = out["parent_max"] - out["parent_min"]
    out["tie"] = bool(out["this_median"] >= out["parent_median"] - out["margin_the_parents_own_spread"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parts", nargs="+", choices=["apply", "push", "epoch", "bench"])
    ap.add_argument("--bodies", type=int, default=1_000_000)
    ap.add_argument("--parent-lib")
    ap.add_argument("--bench-runs", type=int, default=4)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    result = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            result = json.load(f)
    for part in args.parts:
        if part == "apply":
            result["apply"] = part_apply(args.bodies)
        elif part == "push":
            result["push"] = part_push(args.bodies)
        elif part == "epoch":
            result["epoch_bump"] = part_epoch(args.bodies)
        else:
            if not args.parent_lib:
                ap.error("bench needs --parent-lib")
            result["bench"] = part_bench(args.parent_lib, args.bench_runs, args.steps, args.warmup)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")
        print(json.dumps({part: result["epoch_bump" if part == "epoch" else part]}), flush=True)


if __name__ == "__main__":
    main()
