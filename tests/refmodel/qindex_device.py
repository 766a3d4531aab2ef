"""The GPU side of the query-index comparisons: the same world asked with the index off (the reference) and on, byte for byte, and
the stats that show the indexed call did go through the index."""
from __future__ import annotations

import numpy as np


def answer_bytes(a):
    """Any answer of a World query (dict of arrays, record array, list of those) as nested bytes."""
    if isinstance(a, dict):
        return {k: answer_bytes(v) for k, v in a.items()}
    if isinstance(a, (list, tuple)):
        return [answer_bytes(v) for v in a]
    return np.ascontiguousarray(a).tobytes()


def off_and_on(w, fn, **desc):
    """fn() with the index off, then on (min_work = 0 unless given), then off again: (off answer, on answer, stats of the on call).
    The on call must have built the index."""
    desc.setdefault("min_work", 0)
    w.set_query_index(False)
    builds = w.query_index_stats()["builds"]
    off = fn()
    st = w.query_index_stats()
    assert st["built"] == 0 and st["builds"] == builds, "the index was built while it was off"
    w.set_query_index(True, **desc)
    on = fn()
    st = w.query_index_stats()
    w.set_query_index(False)
    assert st["built"] == 1 and st["builds"] > builds, f"the indexed call fell back to the all-bodies pass: {st}"
    return off, on, st


def members(sc):
    """How many bodies of a refmodel.device.Scene the index holds: in the world, and visible to some query (mask != 0)"""
    live = sc.bodies_in_world()
    return int(((sc.mask[live] != 0) & (sc.layer[live] != 0)).sum())


def assert_same(off, on, what=""):
    a, b = answer_bytes(off), answer_bytes(on)
    if isinstance(a, dict):
        assert sorted(a) == sorted(b), what
        for k in a:
            assert_same(off[k], on[k], f"{what}.{k}")
    elif isinstance(a, list):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(off, on)):
            assert_same(x, y, f"{what}[{i}]")
    else:
        assert a == b, f"{what}: the indexed answer differs from the all-bodies answer"
