"""Sphere penetration and recovery, step moves, characters and character triggers on worlds whose slot order differs from their entity
order (include/bge_world.h "Sphere penetration and recovery", "Sphere step moves", "Characters", "Character trigger events").

The flat worlds of the four features' own tests have slot_of_entity = entity_of_slot = the identity, no padding slots and no slot
index beyond the entity count: a library that reported a slot for an entity, read the winner's pose at the entity's index, or scanned
n_entities slots would pass them all.  test_gpu_query_layouts.py closed that for rays, sphere casts, overlaps and plain moves;
this file does it for what came after, and for the host state these features keep across bge_world_set_topology (the staleness of
the device trigger arrays, the queries' ghost list, the character-trigger bitmaps by trigger row, the boxes posed from a trigger's
slot).

Two kinds of world:
  * the layout scene of refmodel/layout_cases.py through its edit history, for penetration and recovery.  The penetration hits go
    through the checks of test_gpu_sphere_recover.py (refmodel/device.py: the device's own overlap exactly; signed_ref in float64 on
    the device's poses at the tolerances of refmodel/tolerances.py as imported), the recoveries equal recover_ref over the device's
    own penetration query byte for byte, and every entity named is in the world;
  * the step field and the trigger walk embedded among pad entities that shuffle their slots (embedded_topology).  Bodies and ghosts
    are posed from the local TRS at their slot, a hierarchy does not move them, and ties and object codes go by entity index: the
    embedded world must answer every call byte for byte as the flat world of the same entities does.  No tolerance is involved.

test_layout_movers_cpu.py asserts that the recipes shuffle what they are meant to shuffle, that the reference alone clears the caps and
floors used here, and that the checkers reject the three mistakes named above."""
from __future__ import annotations

import numpy as np
import pytest

import banggameengine_amd as B
from banggameengine_amd import world as W
from banggameengine_amd.world import make_character_inputs, make_characters

from refmodel.rays import ALL, RAY_BODY
from refmodel.recover import record_valid, recover_ref
from refmodel.step_moves import compose_ref, step_ref
from refmodel.step_cases import FIELD_SEED, STEPPER_SEED, StepField, check_step_coverage, step_coverage, stepper_batch
from refmodel.characters import fresh_state
from refmodel.character_cases import CHAR_SEED, DT, INPUT_SEED, N_CHARS, N_STEPS, character_batch, character_coverage, check_character_coverage, input_script
from refmodel.char_triggers import ENTER, EXIT, STAY, pairs_of
from refmodel.char_trigger_cases import NOBODY, THROUGH_EVENTS, THROUGH_X, Walk, check_coverage, coverage, run_reference
from refmodel.char_trigger_cases import N_CALLS, N_CHARS as WALK_CHARS, N_TRIGGERS as WALK_TRIGGERS
from refmodel.layout_cases import (FIELD_PAD, HAND_PARENT, HAND_POS, N, N_GROWN, N_MOVERS, N_SHRUNK, PEN_FLOORS, PHASES, WALK_PAD, Edits, embedded_topology,
                                   layout_numbers, relayout_topology)
from refmodel.device import (FLAGS, check_penetration_against_overlap, check_penetrations, device_caster, penetration, recover)
from refmodel.layout_device import LayoutScene, check_members
from refmodel.step_device import device_mover, field_world, step_move
from refmodel.character_device import run_script
from refmodel.char_trigger_device import one_call, run_walk, trigger_world

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------------------------------------ penetration and recovery


def differing(got, want):
    return [i for i in range(len(want)) if got[i].tobytes() != want[i].tobytes()]


def penetrations(sc, recs):
    """Both answers to a phase's records, with every entity they name checked against what is in the world."""
    ans = dict(penetration=penetration(sc.w, recs), recover=recover(sc.w, recs))
    check_members(sc, ans, need_bodies=PEN_FLOORS["bodies named"])
    return ans


def beyond_the_entity_count(sc, ans):
    """How many body winners of the penetration query sit at a slot >= the entity count (and how many entities are off their index)."""
    slot, has = W.flatten_topology(sc.parent, sc.ht)[0], sc.ht.astype(bool)
    pen = ans["penetration"]
    winners = pen["entity"][pen["kind"] == RAY_BODY]
    far = int((slot[winners] >= sc.n).sum())
    print(f"{int((slot[has] != np.arange(sc.n)[has]).sum())} of {int(has.sum())} entities off their index; {far} of {len(winners)} body winners at slots "
          f">= the entity count {sc.n}")
    return far


def compare_penetrations(sc, recs, ans=None):
    """The whole comparison of a phase: the device's own overlap exactly, the float64 reference on what is in the world, and the
    recovery against the rule over the device's own penetration query, byte for byte.  Returns (the answers, how many body winners
    sit at a slot beyond the entity count)."""
    ans = penetrations(sc, recs) if ans is None else ans
    check_penetration_against_overlap(sc.w, recs, ans["penetration"], (PEN_FLOORS["penetrated"], PEN_FLOORS["outside"]))
    check_penetrations(sc.objects(), recs, np.array([record_valid(m) for m in recs]), ans["penetration"])
    want = recover_ref(lambda s: penetration(sc.w, s), recs)
    bad = differing(ans["recover"], want)
    assert not bad, f"{len(bad)} of {len(recs)} recoveries differ, first {bad[0]}: {ans['recover'][bad[0]]} vs {want[bad[0]]}"
    return ans, beyond_the_entity_count(sc, ans)


def test_penetration_and_recovery_on_the_layout_scene_and_after_a_relayout():
    sc = LayoutScene()
    try:
        sc.tick(6)
        recs = sc.spheres("layout")
        before, far = compare_penetrations(sc, recs)
        assert far >= 1, "no winner at a slot beyond the entity count: the scan's length is not tested"
        got = before["recover"]
        assert all((got["n_pushes"] == k).any() for k in range(W.RECOVER_ROUNDS + 1)) and ((got["flags"] & W.RECOVER_STUCK) != 0).any()
        # a re-layout without a tick changes no byte of either answer
        old = W.flatten_topology(sc.parent, sc.ht)[0]
        sc.set_topology(relayout_topology(sc.parent), sc.ht)
        new, has = W.flatten_topology(sc.parent, sc.ht)[0], sc.ht.astype(bool)
        print(f"re-layout: {int((new[has] != old[has]).sum())} of {int(has.sum())} slots moved")
        assert (new[has] != old[has]).sum() >= 0.5 * has.sum()
        after = penetrations(sc, recs)
        for name in before:
            assert after[name].tobytes() == before[name].tobytes(), f"{name} changed with the layout"
        # ghosts are posed from the new slots now
        sc.tick(2)
        compare_penetrations(sc, recs)
    finally:
        sc.close()


@pytest.mark.parametrize("upto", PHASES[1:])
def test_penetration_and_recovery_between_edits(upto):
    """The history of test_gpu_query_layouts.py::test_edits_between_ticks, run to the phase `upto`: every phase passed is asked its
    records and every entity named must be in the world; the last phase's answers go through the whole comparison."""
    sc = LayoutScene()
    try:
        ed = Edits(sc.parent, sc.ht, np.sort(sc.trig))
        sc.tick(6)

        def phase(name):
            recs = sc.spheres(name)
            ans = penetrations(sc, recs)
            if name == upto:
                compare_penetrations(sc, recs, ans)
            return name == upto

        n_before = len(sc.bodies_in_world())
        sc.remove(ed.removed)
        assert len(sc.bodies_in_world()) == n_before - len(ed.removed)
        if phase("removed"):
            return
        sc.grow(ed)
        assert sc.w.n == N_GROWN and not np.isin(np.arange(N, N_GROWN), sc.bodies_in_world()).any()
        if phase("grown, before the tick"):
            return
        sc.tick(1)
        assert np.isin(np.arange(N, N_GROWN), sc.bodies_in_world()).all()
        if phase("grown"):
            return
        # the triggers and bodies of the dropped entities go first; the re-uploaded ghosts wait for the next tick
        recs = sc.spheres("grown")
        sc.drop_above(N_SHRUNK)
        assert len(sc.trig) == len(ed.trig_shrunk) and len(sc.ghosts_in_world()) == 0
        ans = penetrations(sc, recs)
        assert not (ans["penetration"]["kind"] == W.RAY_TRIGGER).any() and not (ans["recover"]["hit_kind"] == W.RAY_TRIGGER).any()
        sc.shrink(N_SHRUNK, ed)
        penetrations(sc, recs)
        sc.tick(1)
        assert len(sc.ghosts_in_world()) == len(ed.trig_shrunk)
        assert phase("shrunk")
    finally:
        sc.close()


# ------------------------------------------------------------------------------------------------ the embedded step field


class Fields:
    """The step field as a flat world and embedded among FIELD_PAD pad entities, both ticked once."""

    def __init__(self):
        self.field = StepField(np.random.default_rng(FIELD_SEED))
        self.parent, self.ht = embedded_topology(self.field.n, FIELD_PAD)
        nums, slot = layout_numbers(self.parent, self.ht, self.field.n)
        print(f"the step field embedded: {nums}")
        assert nums["off"] >= 0.9 * self.field.n and nums["far"] >= 1 and nums["slots"] > nums["transforms"]
        self.flat = field_world(self.field)
        try:
            self.emb = field_world(self.field, topology=(self.parent, self.ht))
        except Exception:
            self.flat.close()
            raise
        info = self.emb.info()
        assert self.emb.n == nums["entities"] and info["n_slots"] == nums["slots"]

    def relayout(self):
        """Re-lays the embedded world out; the number of own slots that moved."""
        old = layout_numbers(self.parent, self.ht, self.field.n)[1]
        self.parent = relayout_topology(self.parent)
        self.emb.set_topology(self.parent, self.ht)
        nums, new = layout_numbers(self.parent, self.ht, self.field.n)
        moved = int((new != old).sum())
        print(f"re-laid out: {nums}; {moved} own slots moved")
        assert moved >= 0.5 * self.field.n and nums["far"] >= 1
        return moved

    def close(self):
        self.flat.close()
        self.emb.close()


def test_step_moves_on_the_embedded_field_equal_the_flat_world_byte_for_byte():
    f = Fields()
    try:
        moves = stepper_batch(np.random.default_rng(STEPPER_SEED), N_MOVERS, f.field)
        want = step_move(f.flat, moves)

        def same(when):
            got = step_move(f.emb, moves)
            bad = differing(got, want)
            assert not bad, f"{when}: {len(bad)} of {len(moves)} differ from the flat world, first {bad[0]}: {got[bad[0]]} vs {want[bad[0]]}"
            return got

        got = same("embedded")
        trace = {}
        ref = step_ref(device_caster(f.emb), moves, trace)
        assert not differing(got, ref), "the rule over the embedded world's own casts"
        assert not differing(got, compose_ref(device_caster(f.emb), moves, got, device_mover(f.emb))), "the composition of public calls"
        check_step_coverage(step_coverage(got, trace))
        # the hits name own entities, some of them at slots beyond the entity count
        slot = layout_numbers(f.parent, f.ht, f.field.n)[1]
        named = got["hit_entity"][got["hit_kind"] == RAY_BODY]
        assert (named < f.field.n).all()
        far = int((slot[named] >= f.emb.n).sum())
        print(f"{len(named)} last hits on bodies, {far} of them at slots >= the entity count {f.emb.n}")
        assert far >= 1
        f.relayout()
        same("after the re-layout, before a tick")
        f.emb.tick(flags=FLAGS)
        same("after the re-layout and a tick")
    finally:
        f.close()


def test_characters_on_the_embedded_field_equal_the_flat_world_after_every_step():
    f = Fields()
    try:
        descs, heading = character_batch(np.random.default_rng(CHAR_SEED), N_CHARS, f.field)
        script = input_script(np.random.default_rng(INPUT_SEED), heading, N_STEPS)
        want = run_script(f.flat, descs, script, DT)
        got = run_script(f.emb, descs, script, DT)
        for k in range(N_STEPS):
            bad = differing(got[k], want[k])
            assert not bad, f"step {k}: {len(bad)} of {N_CHARS} differ from the flat world, first {bad[0]}: {got[k][bad[0]]} vs {want[k][bad[0]]}"
        check_character_coverage(character_coverage(fresh_state(descs), got))
        # the bodies stood on and run into are own entities, some of them at slots beyond the entity count
        slot = layout_numbers(f.parent, f.ht, f.field.n)[1]
        named = np.concatenate([s[e][s[k] == RAY_BODY] for s in got for k, e in (("ground_kind", "ground_entity"), ("hit_kind", "hit_entity"))])
        assert (named < f.field.n).all()
        far = int((slot[named] >= f.emb.n).sum())
        print(f"{len(named)} bodies named by the states, {far} of them at slots >= the entity count {f.emb.n}")
        assert far >= 1
        # the same run with the embedded world re-laid out, grown and shrunk under the characters: the set is not the entities'
        w = f.emb
        w.characters_create(descs)
        n = w.n
        for k, inp in enumerate(script):
            if k == 4:
                before = w.characters_state().tobytes()
                f.relayout()
                assert w.characters_state().tobytes() == before, "set_topology changed a character"
            if k == 6:  # 64 more entities without bodies, half of them under own entities
                before = w.characters_state().tobytes()
                parent = np.concatenate([f.parent, np.full(64, W.NO_PARENT, np.uint32)])
                parent[n:n + 32] = np.arange(32)
                w.set_topology(parent, np.concatenate([f.ht, np.ones(64, np.uint8)]))
                assert w.n == n + 64 and w.characters_state().tobytes() == before
            if k == 7:
                w.set_topology(f.parent, f.ht)
                assert w.n == n
            w.characters_set_input(inp)
            w.characters_update(DT, 1)
            bad = differing(w.characters_state(), want[k])
            assert not bad, f"step {k} of the edited run: {len(bad)} of {N_CHARS} differ from the flat world, first {bad[0]}"
    finally:
        f.close()


def test_a_character_set_made_before_the_topology_outlives_it():
    """bge_world_characters_create "may be called before bge_world_set_topology": the set does not belong to the entities."""
    field = StepField(np.random.default_rng(FIELD_SEED))
    descs, _ = character_batch(np.random.default_rng(CHAR_SEED), 65, field)
    w = B.World(device=0)
    try:
        w.characters_create(descs)
        before = w.characters_state().tobytes()
        assert before == fresh_state(descs).tobytes()
        for topology in (embedded_topology(field.n, FIELD_PAD), (np.full(3, W.NO_PARENT, np.uint32), None)):
            w.set_topology(*topology)
            assert w.characters_state_device()[1] == 65 and w.characters_state().tobytes() == before
    finally:
        w.close()


# ------------------------------------------------------------------------------------------------ the embedded trigger walk


def test_character_triggers_on_the_embedded_walk_equal_the_rule_and_the_flat_world():
    walk = Walk()
    parent, ht = embedded_topology(WALK_TRIGGERS, WALK_PAD)
    nums, slot = layout_numbers(parent, ht, WALK_TRIGGERS)
    print(f"the walk embedded: {nums}")
    assert nums["off"] >= 0.9 * WALK_TRIGGERS and nums["far"] >= 1 and nums["slots"] > nums["transforms"]
    flat = trigger_world(walk)
    emb = None
    try:
        emb = trigger_world(walk, topology=(parent, ht))
        assert emb.n == nums["entities"] and emb.info()["n_slots"] == nums["slots"]
        flat_boxes, flat_listed = flat.trigger_boxes(walk.entity)
        boxes, listed = emb.trigger_boxes(walk.entity)
        assert listed.all() and listed.tobytes() == flat_listed.tobytes() and boxes.tobytes() == flat_boxes.tobytes()
        want = run_walk(flat, walk, WALK_CHARS)
        got = run_walk(emb, walk, WALK_CHARS)
        ref = run_reference(walk, boxes, listed, [pos for _, pos, _ in got])
        for call in range(N_CALLS):
            (ev, pos, pairs), (rev, prev), (fev, fpos, fpairs) = got[call], ref[call], want[call]
            assert ev.shape == rev.shape and np.array_equal(ev, rev), (call, len(ev), len(rev))
            assert np.array_equal(pairs, pairs_of(prev, walk.entity)), call
            assert np.array_equal(ev, fev) and pos.tobytes() == fpos.tobytes() and np.array_equal(pairs, fpairs), call
        check_coverage(coverage(walk, boxes, [pos for _, pos, _ in got], [ev for ev, _, _ in got]))
        far = np.nonzero(slot >= emb.n)[0]
        met = sum(int(np.isin(ev[:, 1], far).sum()) for ev, _, _ in got)
        print(f"{len(far)} triggers at slots >= the entity count {emb.n}; {met} events name one of them")
        assert met >= 1
        # the same walk with the world re-laid out under the watch, between two calls and without a tick
        emb.characters_create(walk.descs)
        emb.characters_watch_triggers(walk.group, walk.cmask)
        for call in range(N_CALLS):
            if call == 6:
                held = emb.characters_trigger_events(), emb.characters_trigger_overlaps()
                parent2 = relayout_topology(parent)
                emb.set_topology(parent2, ht)
                moved = int((layout_numbers(parent2, ht, WALK_TRIGGERS)[1] != slot).sum())
                print(f"re-laid out under the watch: {moved} of {WALK_TRIGGERS} triggers' slots moved")
                assert moved >= 0.5 * WALK_TRIGGERS
                assert np.array_equal(emb.characters_trigger_events(), held[0]) and np.array_equal(emb.characters_trigger_overlaps(), held[1])
                now = emb.trigger_boxes(walk.entity)
                assert now[0].tobytes() == boxes.tobytes() and now[1].all()
            if call == 9:  # ... and a tick later: the boxes are posed from the new slots
                emb.tick(flags=FLAGS)
                now = emb.trigger_boxes(walk.entity)
                assert now[0].tobytes() == boxes.tobytes() and now[1].all()
            ev, pos, pairs = one_call(emb, walk, call, WALK_CHARS)
            fev, fpos, fpairs = want[call]
            assert np.array_equal(ev, fev) and pos.tobytes() == fpos.tobytes() and np.array_equal(pairs, fpairs), f"call {call} of the re-laid-out walk"
    finally:
        flat.close()
        if emb is not None:
            emb.close()


# ------------------------------------------------------------------------------------------------ the frozen ghost, hand-worked


def test_a_trigger_that_lost_its_transform_keeps_its_frozen_box_for_the_characters():
    """The topology of test_gpu_query_layouts.py::test_transform_loss_hand_worked: the trigger on entity 2 (half extents 1, at
    (5, 2, 0), child of entity 7, which is listed after it).  Character 0 (radius 0.5: the box +-0.52 about its centre) is warped
    along x through the volume (fed box +-1.02 about its centre: inside for |x| <= 1.54); character 1 waits 100 away."""
    w = B.World(device=0)
    try:
        ht = np.array([1, 1, 1, 0, 1, 1, 1, 1], np.uint8)
        slot = W.flatten_topology(HAND_PARENT, ht)[0]
        assert slot[2] != 2 and slot[2] >= len(ht), "slot order equals entity order: the scene tests nothing"
        w.set_topology(HAND_PARENT, ht)
        w.upload_trs(HAND_POS, np.zeros((8, 3)), np.ones((8, 3)))
        types = np.uint8([W.BODY_STATIC, W.BODY_STATIC, W.BODY_NONE, W.BODY_STATIC, W.BODY_NONE, W.BODY_STATIC, W.BODY_NONE, W.BODY_NONE])
        w.upload_bodies(types, None, np.zeros(8, np.uint8), np.full((8, 3), 0.5, np.float32), np.full(8, 1, np.uint32), np.full(8, ALL, np.uint32))
        w.upload_triggers(np.uint32([2]), None, np.float32([[1, 1, 1]]), np.uint32([4]), np.uint32([ALL]), np.uint8([0]), np.uint8([1]))
        w.set_ground_plane(False)
        w.tick(flags=FLAGS)
        cx, cy, cz = (float(v) for v in HAND_POS[2])
        w.characters_create(make_characters([[cx + THROUGH_X[-1], cy, cz], [cx + 100.0, cy, cz]], radius=0.5, gravity=0.0, layer_mask=NOBODY))
        w.characters_watch_triggers()
        w.characters_set_input(make_character_inputs(np.zeros(2), 0.0))

        def put(char, x, z=cz):
            w.characters_warp([char], [[x, cy, z]])
            w.characters_update(DT, 1)
            return w.characters_trigger_events().tolist()

        def through():
            """The warp sequence ends outside the volume, then character 0 is put at its centre: the remembered pair."""
            lists = [put(0, cx + x) for x in THROUGH_X]
            assert lists == [[[t, 2, 0] for t in types_] for types_ in THROUGH_EVENTS], lists
            assert len(w.characters_trigger_overlaps()) == 0
            assert put(0, cx) == [[ENTER, 2, 0]] and w.characters_trigger_overlaps().tolist() == [[2, 0]]

        through()
        box, listed = w.trigger_boxes([2])
        assert listed.tolist() == [True] and np.allclose(box[0], [cx - 1.02, cy - 1.02, cz - 1.02, cx + 1.02, cy + 1.02, cz + 1.02], atol=1e-5, rtol=0)
        # entity 2 loses its Transform: the same six floats, still listed, the pair kept, the same events
        lost = ht.copy()
        lost[2] = 0
        w.set_topology(HAND_PARENT, lost)
        for when in ("before a tick", "after a tick"):
            now = w.trigger_boxes([2])
            assert now[1].tolist() == [True] and now[0].tobytes() == box.tobytes(), when
            assert w.characters_trigger_overlaps().tolist() == [[2, 0]], when
            assert put(0, cx) == [[STAY, 2, 0]], when
            assert put(0, cx + THROUGH_X[-1]) == [[EXIT, 2, 0]], when
            through()
            w.tick(flags=FLAGS)
        # the Transform comes back 20 away: after one tick the box stands there.  Character 0 still stands at the old place
        w.set_topology(HAND_PARENT, ht)
        assert W.flatten_topology(HAND_PARENT, ht)[0][2] != 2
        w.upload_trs(np.float32([[cx, cy, cz + 20]]), np.zeros((1, 3)), np.ones((1, 3)), first=2)
        w.tick(flags=FLAGS)
        now = w.trigger_boxes([2])
        assert now[1].tolist() == [True] and np.allclose(now[0][0], box[0] + np.float32([0, 0, 20, 0, 0, 20]), atol=1e-5, rtol=0)
        assert w.characters_trigger_overlaps().tolist() == [[2, 0]]
        assert put(1, cx, cz + 20) == [[ENTER, 2, 1], [EXIT, 2, 0]]
        assert w.characters_trigger_overlaps().tolist() == [[2, 1]]
    finally:
        w.close()
