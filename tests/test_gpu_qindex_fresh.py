"""A stale query index is the defect the design invites: the index is rebuilt by every public call that queries (include/bge_world.h
"Query index", rule 6), so after ANY edit of the world the indexed answers must equal the all-bodies answers of the same world at
the same moment.  One LayoutScene (shuffled slots, slots beyond the entity count, ghosts) goes through the history of
test_gpu_query_layouts.py; after each step all five answers are asked with the index off and on."""
from __future__ import annotations

import numpy as np
import pytest

from banggameengine_amd import world as W

from refmodel.layout_cases import N, N_GROWN, N_SHRUNK, Edits, relayout_topology
from refmodel.device import ask
from refmodel.layout_device import LayoutScene, check_members
from refmodel.qindex_device import answer_bytes, assert_same, members, off_and_on

pytestmark = pytest.mark.gpu


def test_every_edit_reaches_the_index():
    sc = LayoutScene()
    try:
        ed = Edits(sc.parent, sc.ht, np.sort(sc.trig))
        sc.tick(6)
        batches = sc.batches("layout")
        seen = []

        def same(step, expect_change=True):
            off, on, st = off_and_on(sc.w, lambda: ask(sc.w, batches))
            assert_same(off, on, step)
            check_members(sc, on)
            assert st["bodies_indexed"] + st["bodies_wide"] == members(sc), (step, st)
            if seen and expect_change:
                assert answer_bytes(on) != seen[-1], f"{step}: the edit changed no answer, the step tests nothing"
            seen.append(answer_bytes(on))
            return st

        first = same("query")
        sc.tick(1)  # dynamic bodies move
        same("tick")
        # a fifth of the bodies are put elsewhere; the tick brings them there
        live = sc.bodies_in_world()
        pos = sc.w.download_pose()[0]
        sc.w.upload_trs(pos[100:500] + np.float32([[3.0, 0.5, -2.0]]), first=100)
        sc.tick(1)
        same("upload_trs + tick")
        # bodies uploaded again are absent until the next tick
        e0 = int(live[1])
        sc.w.upload_bodies(sc.type[e0:e0 + 40], None, sc.shape[e0:e0 + 40], sc.size[e0:e0 + 40], sc.layer[e0:e0 + 40], sc.mask[e0:e0 + 40], first=e0)
        sc.fresh[e0:e0 + 40] = True
        st = same("upload_bodies")
        assert st["bodies_indexed"] + st["bodies_wide"] < first["bodies_indexed"] + first["bodies_wide"]
        sc.remove(ed.removed)
        same("BODY_NONE")
        sc.grow(ed)
        assert sc.w.n == N_GROWN
        same("grow, before the tick", expect_change=False)
        sc.tick(1)
        st = same("grow")
        assert np.isin(np.arange(N, N_GROWN), sc.bodies_in_world()).all()
        old = W.flatten_topology(sc.parent, sc.ht)[0]
        sc.set_topology(relayout_topology(sc.parent), sc.ht)
        has = sc.ht.astype(bool)
        assert (W.flatten_topology(sc.parent, sc.ht)[0][has] != old[has]).any(), "the re-layout moved no slot"
        same("re-layout", expect_change=False)  # (test_a_relayout_changes_no_answer: no byte may change)
        assert seen[-1] == seen[-2], "the re-layout changed an answer"
        sc.drop_above(N_SHRUNK)
        same("dropped")
        sc.shrink(N_SHRUNK, ed)
        same("shrink", expect_change=False)
        sc.tick(1)
        same("shrink + tick")
    finally:
        sc.close()
