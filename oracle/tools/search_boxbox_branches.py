"""Seeded search for the branches of the box-box narrowphase that tests/refmodel/boxbox_cases.py lists as UNREACHABLE.

    python oracle/tools/search_boxbox_branches.py [pairs=1000000] [seed=1]

Half of the pairs are random poses, half are boxes laid nearly face on face (B's orientation plus quarter turns plus a perturbation of
0, 1e-7 .. 1e-1 rad) — the second half is where clips degenerate.  Every pair is bisected along a random direction until its deepest
point lies at 0.01 (or, for a quarter of them, at 1e-6: touching).  Counted over ALL detector calls of the bisection, not only the last:
clip counts, the cull's a = 1e18 branch, depth > breaking, the d <= 0.0001 branch under an edge code, edge axes skipped.
DESIGN.md 6b records the result."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from oracle import pyoracle as po  # noqa: E402


def main(pairs=1_000_000, seed=1, chunk=100_000):
    rng = np.random.default_rng(seed)
    clip = np.zeros(9, np.int64)
    guard = skipped = parallel = calls = 0
    most_skips = 0
    for lo_i in range(0, pairs, chunk):
        n = min(chunk, pairs - lo_i)
        scale = rng.choice([0.1, 1.0, 1.0, 1.0, 100.0], n)[:, None]
        ha, hb = rng.uniform(0.1, 0.5, (n, 3)) * scale, rng.uniform(0.1, 0.5, (n, 3)) * scale
        eb = rng.uniform(-np.pi, np.pi, (n, 3))
        ea = rng.uniform(-np.pi, np.pi, (n, 3))
        flat = rng.random(n) < 0.5
        turn = rng.integers(0, 4, (n, 3)) * (np.pi / 2)
        wobble = rng.choice([0.0, 1e-7, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1], n)[:, None] * rng.uniform(-1, 1, (n, 3))
        ea = np.where(flat[:, None], eb + turn + wobble, ea)
        d = rng.normal(size=(n, 3))
        d /= np.linalg.norm(d, axis=1)[:, None]
        centre = rng.choice([0.0, 0.0, 1e3, 1e4], n)[:, None] * rng.uniform(-1, 1, (n, 3))
        pen = np.where(rng.random(n) < 0.25, 1e-6, 0.01)
        lo, hi = np.zeros(n), np.linalg.norm(ha, axis=1) + np.linalg.norm(hb, axis=1) + 1.0
        for _ in range(32):
            mid = 0.5 * (lo + hi)
            t = po.boxbox_detect(centre + d * mid[:, None], ea, ha, centre, eb, hb)
            calls += n
            face = (t.code >= 1) & (t.code <= 6) & (t.n_clip >= 0)
            clip += np.bincount(t.n_clip[face], minlength=9)[:9]
            guard += int((t.culled == 2).sum())
            skipped += int((t.action == po.ACT_SKIPPED).sum())
            parallel += int(((t.edge_parallel == 1) & (t.code > 6) & (t.n_out > 0)).sum())
            most_skips = max(most_skips, max(bin(int(m)).count("1") for m in np.unique(t.skip_mask)))
            deep = (t.n_out > 0) & (t.depth.min(1) < -pen)
            lo, hi = np.where(deep, mid, lo), np.where(deep, hi, mid)
    print(f"pairs {pairs}  detector calls {calls}")
    print("clip counts 0..8 over face codes:", clip.tolist())
    print("cullPoints2 a = 1e18 branch:", guard)
    print("depth > breaking (point skipped):", skipped)
    print("d <= 0.0001 with an edge code winning:", parallel)
    print("most edge axes skipped in one call:", most_skips)


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:3]))
