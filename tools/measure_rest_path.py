"""The all-asleep state of configs[1] on the ground plane: boxes land, rest, fall asleep, then `--ticks` ticks
are timed (wall clock around one synchronised batch).  Prints one JSON line.  Meant to be run plainly, under
`rocprofv3 --kernel-trace --stats`, or under `rocprofv3 --pmc FETCH_SIZE` / `--pmc WRITE_SIZE` (separate passes): the last
`--ticks` dispatches of k_tick are then the asleep ones.  BGE_REST_PATH=0 and BGE_WORLD_LIB give the A/B."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entities", type=int, default=1_000_000)
    ap.add_argument("--ticks", type=int, default=100)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    import banggameengine_amd as B
    from banggameengine_amd import synth
    from banggameengine_amd.world import FIXED_DT, GRAVITY
    wl = synth.config("flat1m", n=args.entities)
    rng = np.random.default_rng(11)
    wl.pos[:, 1] = (0.9 + rng.uniform(0.0, 0.3, wl.n)).astype(np.float32)  # bench.py measure_ground_config's scene
    with B.World(stream=torch.cuda.current_stream().cuda_stream) as w:
        w.load(wl)
        w.set_ground_plane(True)
        w.tick(dt=FIXED_DT, gravity=GRAVITY, flags=B.TICK_ALL, ticks=610)  # landing, resting, falling asleep
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        w.tick(dt=FIXED_DT, gravity=GRAVITY, flags=B.TICK_ALL, ticks=args.ticks)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / args.ticks * 1e3
        st, _ = w.download_activation()
    print(json.dumps({"label": args.label, "entities": wl.n, "ticks": args.ticks, "asleep_ms_per_step": ms, "asleep": int((st == 2).sum()),
                      "rest_path": os.environ.get("BGE_REST_PATH", "on"), "lib": os.environ.get("BGE_WORLD_LIB", "in-tree")}))


if __name__ == "__main__":
    main()
