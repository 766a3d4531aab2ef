#!/usr/bin/env python3
"""Cost of the character trigger events (bge_world_characters_watch_triggers) inside one step of a character set.

Run on an MI355X:  python tools/measure_char_triggers.py [n_bodies]
Scene: that of tools/measure_characters.py — n_bodies (default 1 M) boxes and capsules mixed, resting on the plane over 2,000 x 2,000
units, with n_bodies / 8 Static flat slabs added — plus 1,000 trigger volumes (boxes of half extents 1 .. 3, yawed, mask = the
characters' group), each centred within 2 units of one of the characters so that about as many pairs overlap as there are
characters.  1,024 characters as there (radius 0.4, skin 0.01, step_height 0.5, probe 0.3, walking 0.03 .. 0.06 a step), with a layer
mask that leaves the triggers' layer out so that a volume is no obstacle.
Timed with HIP events on the world's stream (warm-up first, then the median of the repeats), in one process on one world,
alternating so that drift shows:
  off_us   one World.characters_update(dt, 1) with the watch off
  on_us    the same with the watch on: one more copy and four more launches (1,024 x 1,000 box tests)
The expectation is on_us - off_us of a few launches' worth against a step of about 13 ms.  Not a test, and not part of bench.py.
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
    n_slabs, n_trig, nc = n // 8, 1000, 1024
    rng = np.random.default_rng(3)
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    with B.World(device=0, stream=stream.cuda_stream) as w, torch.cuda.stream(stream):
        total = n + n_slabs + n_trig
        w.set_topology(np.full(total, W.NO_PARENT, np.uint32))
        size = rng.uniform(0.2, 1.0, (n, 3)).astype(np.float32)
        shape = rng.integers(0, 2, n).astype(np.uint8)
        btype = rng.choice([W.BODY_STATIC, W.BODY_DYNAMIC, W.BODY_KINEMATIC], n, p=[0.34, 0.5, 0.16]).astype(np.uint8)
        rest = np.where(shape == 1, size[:, 0] + size[:, 1], np.maximum(size[:, 1], 0.01))
        pos = np.stack([rng.uniform(-1000, 1000, n), rest, rng.uniform(-1000, 1000, n)], 1).astype(np.float32)
        top = rng.uniform(0.1, 0.6, n_slabs)
        s_size = np.stack([rng.uniform(0.5, 2.0, n_slabs), top / 2, rng.uniform(0.5, 2.0, n_slabs)], 1).astype(np.float32)
        s_pos = np.stack([rng.uniform(-1000, 1000, n_slabs), top / 2, rng.uniform(-1000, 1000, n_slabs)], 1).astype(np.float32)
        radius, skin, probe, height, dt, reps = 0.4, 0.01, 0.3, 0.5, 1.0 / 60.0, 7
        p = np.stack([rng.uniform(-1000, 1000, nc), np.full(nc, radius + skin + 0.005), rng.uniform(-1000, 1000, nc)], 1)
        az = rng.uniform(0, 2 * np.pi, nc)
        walk = np.stack([np.cos(az), np.sin(az)], 1) * rng.uniform(0.03, 0.06, nc)[:, None]
        t_size = rng.uniform(1.0, 3.0, (n_trig, 3)).astype(np.float32)
        t_pos = (p[np.arange(n_trig) % nc] + np.stack([rng.uniform(-2, 2, n_trig), np.zeros(n_trig), rng.uniform(-2, 2, n_trig)], 1)).astype(np.float32)
        euler = np.zeros((total, 3), np.float32)
        euler[n:, 1] = rng.uniform(-np.pi, np.pi, n_slabs + n_trig)
        w.upload_trs(np.concatenate([pos, s_pos, t_pos]), euler, np.ones((total, 3), np.float32))
        w.upload_bodies(np.concatenate([btype, np.full(n_slabs, W.BODY_STATIC, np.uint8), np.full(n_trig, W.BODY_NONE, np.uint8)]), None,
                        np.concatenate([shape, np.zeros(n_slabs + n_trig, np.uint8)]), np.concatenate([size, s_size, t_size]))
        t_entity = np.arange(n + n_slabs, total, dtype=np.uint32)
        w.upload_triggers(t_entity, np.zeros(n_trig, np.uint8), t_size, np.full(n_trig, 4, np.uint32), np.full(n_trig, 2, np.uint32),
                          np.zeros(n_trig, np.uint8), np.ones(n_trig, np.uint8))
        w.set_ground_plane(True)
        w.set_sleeping(0.8, 1.0, 0.05)
        w.tick(flags=W.TICK_ALL, ticks=30)
        w.tick(flags=W.TICK_ALL | W.TICK_BROADPHASE)  # poses the ghosts
        w.trigger_events()
        listed = int(w.trigger_boxes(t_entity)[1].sum())
        w.characters_create(W.make_characters(p, radius, skin, height, 0.7071068, probe, layer_mask=0xFFFFFFFF & ~4))
        w.characters_update(dt, 3)
        w.characters_set_input(W.make_character_inputs(walk[:, 0], walk[:, 1]))
        row = {"bodies": n, "slabs": n_slabs, "triggers": n_trig, "listed": listed, "characters": nc}
        off, on, events = [], [], []
        for _ in range(2):
            w.characters_unwatch_triggers()
            off.append(timed_device(stream, lambda: w.characters_update(dt, 1), reps))
            w.characters_watch_triggers()
            on.append(timed_device(stream, lambda: w.characters_update(dt, 1), reps))
            ev = w.characters_trigger_events()
            events.append([int((ev[:, 0] == k).sum()) for k in range(3)])
        row["off_us"], row["on_us"] = off, on
        row["on_minus_off_us"] = [round(b - a, 2) for a, b in zip(off, on)]
        row["events_enter_stay_exit"] = events
        row["remembered_pairs"] = int(len(w.characters_trigger_overlaps()))
        s = w.characters_state()
        row["steps_run"] = int(s["steps"][0])
        row["grounded"] = int(((s["flags"] & W.CHAR_GROUNDED) != 0).sum())
        print(json.dumps(row))


if __name__ == "__main__":
    main()
