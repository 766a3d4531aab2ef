"""Characters through the query index (include/bge_world.h "Query index"): 200 characters on the step field, 12 steps, with
riding, the crowd and the trigger watch on.  Every record the character set keeps — states, ride records, crowd records, trigger
events — must keep its bytes with the index on, a call of 8 steps must equal 8 calls of one, and the stats must show ONE build per
bge_world_characters_update call, whatever the number of passes in it."""
from __future__ import annotations

import numpy as np
import pytest

from refmodel.step_cases import FIELD_SEED, StepField
from refmodel.character_cases import CHAR_SEED, DT, INPUT_SEED, character_batch, input_script
from refmodel.step_device import field_world
from refmodel.qindex_device import assert_same

pytestmark = pytest.mark.gpu

N_CHARS, N_STEPS = 200, 12


class Shared:
    def __init__(self):
        self.field = StepField(np.random.default_rng(FIELD_SEED))
        self.w = field_world(self.field)
        self.descs, heading = character_batch(np.random.default_rng(CHAR_SEED), N_CHARS, self.field)
        self.script = input_script(np.random.default_rng(INPUT_SEED), heading, N_STEPS)

    def walk(self, on, calls, one_input=False):
        """The set created anew and walked through the script; calls: steps per characters_update call; one_input: the first
        input stays for the whole walk.  Everything the set keeps, after every call."""
        w = self.w
        w.set_query_index(on, min_work=0)
        w.characters_create(self.descs)
        w.characters_ride()
        w.characters_crowd(True, 0.05)
        w.characters_watch_triggers()
        out, step = [], 0
        builds = w.query_index_stats()["builds"]
        for k in calls:
            if step == 0 or not one_input:
                w.characters_set_input(self.script[step])
            w.characters_update(DT, k)
            step += k
            st = w.query_index_stats()
            assert st["built"] == int(on)
            if on:
                builds += 1
                assert st["builds"] == builds, f"{st['builds'] - builds + 1} builds in one characters_update call of {k} steps"
                assert st["queries_indexed"] > 0 and st["bodies_indexed"] > 0, st
            out.append(dict(state=w.characters_state(), rides=w.characters_rides(), crowd=w.characters_crowd_hits(),
                            events=w.characters_trigger_events()))
        w.set_query_index(False)
        return out, st


@pytest.fixture(scope="module")
def shared():
    s = Shared()
    yield s
    s.w.close()


def test_twelve_steps_keep_every_byte(shared):
    off, _ = shared.walk(False, [1] * N_STEPS)
    on, st = shared.walk(True, [1] * N_STEPS)
    print(f"last call: {st}")
    assert_same(off, on, "characters")
    moved = off[-1]["state"]["position"] - off[0]["state"]["position"]
    assert (np.abs(moved).max(axis=1) > 0.05).sum() > N_CHARS // 2, "the characters hardly move: the walk tests nothing"
    assert sum(int((o["crowd"]["flags"] != 0).sum()) for o in off) > 0, "no character was ever pushed: the crowd tests nothing"


def test_one_call_of_eight_steps_equals_eight_calls(shared):
    """(one input for the whole walk: the first step consumes its JUMP edges either way)"""
    once, _ = shared.walk(True, [8], one_input=True)
    eight, _ = shared.walk(True, [1] * 8, one_input=True)
    ref, _ = shared.walk(False, [8], one_input=True)
    for k in ("state", "rides", "crowd"):
        assert_same(once[-1][k], eight[-1][k], f"8 steps in one call and 8 calls: {k}")
        assert_same(ref[-1][k], once[-1][k], f"8 steps in one call, index off and on: {k}")
