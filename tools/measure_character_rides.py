"""What character platform riding costs: characters_update(dt, 2) at 100,000 characters on the step field of
tests/refmodel/step_cases.py, the median of 20 calls timed with events on the world's stream, with riding off or on.

    python tools/measure_character_rides.py off
    python tools/measure_character_rides.py on
    BGE_WORLD_LIB=/path/to/the/parent's/libbge_world.so python tools/measure_character_rides.py off

One process per figure; prints one JSON line.  The world does not move, so with riding on the two extra launches run their
cheapest path past the anchor test (the pose is compared and found equal): what is measured is the launches and the record
traffic, which is what every call pays."""
from __future__ import annotations

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import banggameengine_amd as B  # noqa: E402
from banggameengine_amd import world as W  # noqa: E402
from refmodel.character_cases import CHAR_SEED, DT, INPUT_SEED, character_batch, input_script  # noqa: E402
from refmodel.rays import ALL  # noqa: E402
from refmodel.step_cases import FIELD_SEED, StepField  # noqa: E402

N, CALLS, WARMUP, STEPS = 100_000, 20, 3, 2


def main():
    riding = sys.argv[1:] == ["on"]
    if sys.argv[1:] not in (["on"], ["off"]):
        raise SystemExit(__doc__)
    field = StepField(np.random.default_rng(FIELD_SEED))
    descs, heading = character_batch(np.random.default_rng(CHAR_SEED), N, field)
    inputs = input_script(np.random.default_rng(INPUT_SEED), heading, 1)[0]
    inputs["buttons"] = 0
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    with B.World(device=0, stream=stream.cuda_stream) as w:
        n = field.n
        w.set_topology(np.full(n, W.NO_PARENT, np.uint32))
        w.upload_trs(field.pos, field.euler, np.ones((n, 3)))
        types = np.full(n, W.BODY_STATIC, np.uint8)
        types[field.ghosts] = W.BODY_NONE
        w.upload_bodies(types, None, field.capsule.astype(np.uint8), field.size, np.full(n, 1, np.uint32), np.full(n, ALL, np.uint32))
        w.set_ground_plane(True)
        w.tick(flags=W.TICK_ALL | W.TICK_BROADPHASE)
        w.characters_create(descs)
        if riding:
            w.characters_ride()
        w.characters_set_input(inputs)
        for _ in range(WARMUP):
            w.characters_update(DT, STEPS)
        w.sync()
        ms = []
        for _ in range(CALLS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            w.characters_update(DT, STEPS)
            b.record(stream)
            b.synchronize()
            ms.append(a.elapsed_time(b))
        state = w.characters_state()
        out = dict(library=os.environ.get("BGE_WORLD_LIB", "in-tree"), riding=riding,
                   median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)),
                   grounded=int(((state["flags"] & W.CHAR_GROUNDED) != 0).sum()))
        if riding:
            out["anchored"] = int((w.characters_rides()["entity"] != W.RAY_NO_ENTITY).sum())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
