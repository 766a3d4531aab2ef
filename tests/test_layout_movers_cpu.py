"""Penetration, recovery, step moves, characters and character triggers on worlds whose slot order differs from their entity order,
without a GPU: the recipes test_gpu_layout_movers.py runs on the device, with the conditions that make its comparisons mean
something.  What is asserted here are conditions on the recipes and on the float64 reference, never on the library's answers:

  * the two embedded topologies (the step field's 500 bodies among 530 pad entities, the walk's 70 triggers among 210) and their
    re-layouts are acyclic, put at least 90 % of the own entities off their index, leave padding slots, put an own entity at a slot
    beyond the entity count, and the re-layout moves at least half of the own slots;
  * on every phase's in-world set the penetration batch stays inside check_caps on the reference alone, its recoveries are of every
    sort, and it names the bodies check_members asks for: a GPU failure cannot hide behind the caps;
  * the checkers have teeth: three wrong answers made from the reference's right ones (a slot reported for an entity, the winner's
    pose read at the wrong index, the slots beyond the entity count not scanned) are rejected."""
from __future__ import annotations

import collections
import types

import numpy as np
import pytest

from refmodel.rays import RAY_BODY, RAY_GROUND, RAY_TRIGGER, World64
from refmodel.recover import classify, pen_of, record_valid, recover_ref, signed_ref
from refmodel.recover_cases import check_caps, check_penetrations
from refmodel.records import RECOVER_ROUNDS, RECOVER_STUCK
from refmodel.spheres import SphereRef
from refmodel.moves import caster_of
from refmodel.step_moves import step_ref
from refmodel.step_cases import FIELD_SEED, STEPPER_SEED, StepField, check_step_coverage, step_coverage, stepper_batch
from refmodel.char_trigger_cases import N_TRIGGERS as WALK_TRIGGERS
from refmodel.layout_cases import (FIELD_PAD, N, N_MOVERS, N_SPHERES, PEN_FLOORS, PHASES, WALK_PAD, Edits, acyclic, check_members, embedded_topology, in_world,
                                   joined, layout_numbers, layout_topology, penetration_batches, relayout_topology, scene_reference, subset)

# ------------------------------------------------------------------------------------------------ conditions on the recipes

# (own entities, pad) -> what the recipe gave when it was written: entities, slots, own entities off their index, own entities at a
# slot >= the entity count, own slots the re-layout moves.  Printed beside what it gives now; the floors below are what is asserted.
EMBEDDED = {(500, FIELD_PAD): (1030, 1280, 498, 32, 428), (WALK_TRIGGERS, WALK_PAD): (280, 512, 70, 31, 65)}


@pytest.mark.parametrize("n_own,n_pad", list(EMBEDDED))
def test_the_embedded_topologies_shuffle_the_own_entities(n_own, n_pad):
    assert n_own == (StepField(np.random.default_rng(FIELD_SEED)).n if n_pad == FIELD_PAD else WALK_TRIGGERS)
    parent, ht = embedded_topology(n_own, n_pad)
    parent2 = relayout_topology(parent)
    assert len(parent) == n_own + n_pad and ht[:n_own].all() and not ht[n_own:].all()
    assert acyclic(parent) and acyclic(parent2)
    first, slot = layout_numbers(parent, ht, n_own)
    second, slot2 = layout_numbers(parent2, ht, n_own)
    moved = int((slot2 != slot).sum())
    print(f"{n_own} + {n_pad}: {first}; re-laid out: {second}; the re-layout moves {moved} own slots; when written: {EMBEDDED[n_own, n_pad]}")
    for nums in (first, second):
        assert nums["off"] >= 0.9 * n_own, nums
        assert nums["slots"] > nums["transforms"], nums  # padding slots exist
        assert nums["far"] >= 1, nums                    # an own entity at a slot index that is no entity index
    assert moved >= 0.5 * n_own


# ------------------------------------------------------------------------------------------------ conditions on the reference


def phase_world(phase):
    """(the float64 world of a phase: the scene before its first tick cut to the phase's in-world set, its bodies, its ghosts, the
    phase's recover records), as test_query_layouts_cpu.py builds its worlds."""
    w64, pos, trig = scene_reference()
    parent, ht = layout_topology(N, trig)
    ed = Edits(parent, ht, trig)
    bodies, ghosts = in_world(phase, ht, trig, ed)
    world = subset(joined(w64, ed.world64()), np.concatenate([bodies, ghosts]))
    assert len(world.entity) == len(bodies) + len(ghosts)
    recs = penetration_batches(phase, np.concatenate([pos, ed.pos])[bodies], pos[ghosts])
    return world, bodies, ghosts, recs


@pytest.mark.parametrize("phase", PHASES)
def test_reference_alone_stays_inside_the_penetration_caps_of_every_phase(phase):
    world, bodies, ghosts, recs = phase_world(phase)
    n_valid = n_pen = n_skipped = n_axis = n_outside = 0
    kinds = collections.Counter()
    for m in recs:
        if not record_valid(m):
            continue
        n_valid += 1
        cands, winner_clear, normal_clear = classify(world, m)
        if cands and cands[0].depth >= 0:
            n_pen += 1
            n_skipped += not normal_clear
            n_outside += cands[0].sd > 0
            if winner_clear:
                kinds[cands[0].kind] += 1
            n_axis += normal_clear and cands[0].kind != RAY_GROUND and np.isfinite(cands[0].gap)
    print(f"{phase}:", end=" ")
    check_caps(n_valid, n_pen, n_skipped, kinds, n_axis)
    assert n_valid == N_SPHERES - len(range(36, N_SPHERES, 37))
    # the floors test_gpu_layout_movers.py hands check_penetration_against_overlap and check_members: about half of what the
    # reference alone finds in the leanest phase
    pen = pen_of(world)(as_spheres(recs))
    got = recover_ref(pen_of(world), recs)
    named = int((pen["kind"] == RAY_BODY).sum() + (got["hit_kind"] == RAY_BODY).sum())
    print(f"{phase}: {n_pen} penetrated, {n_outside} winners with the centre outside the shape, {named} bodies named by the penetration and the recovery")
    assert n_pen >= 1.5 * PEN_FLOORS["penetrated"] and n_outside >= 1.5 * PEN_FLOORS["outside"] and named >= 1.5 * PEN_FLOORS["bodies named"]
    # the recoveries are of every sort: 0 .. RECOVER_ROUNDS pushes, and one that stays stuck
    pushes = collections.Counter(got["n_pushes"][[record_valid(m) for m in recs]].tolist())
    stuck = int(((got["flags"] & RECOVER_STUCK) != 0).sum())
    print(f"{phase}: recoveries by pushes {dict(sorted(pushes.items()))}, {stuck} stuck")
    assert all(pushes[k] >= 1 for k in range(RECOVER_ROUNDS + 1)) and stuck >= 1
    assert all((got["hit_kind"] == k).any() for k in (RAY_BODY, RAY_TRIGGER, RAY_GROUND))


def test_the_257_steppers_clear_the_step_floors_on_the_reference_alone():
    """test_sphere_step_cpu.py shows it for the 513 movers of the flat comparison; the embedded field is asked the smallest batch
    that crosses a workgroup, drawn from the same seed, and its coverage is checked against the same floors."""
    field = StepField(np.random.default_rng(FIELD_SEED))
    moves = stepper_batch(np.random.default_rng(STEPPER_SEED), N_MOVERS, field)
    trace = {}
    got = step_ref(caster_of(SphereRef(field.world64()).sweep_all), moves, trace)
    check_step_coverage(step_coverage(got, trace))


def as_spheres(recs):
    from banggameengine_amd.world import make_spheres
    return make_spheres(recs["position"], recs["radius"], recs["layer_mask"])


# ------------------------------------------------------------------------------------------------ teeth


class Members:
    """What check_members reads of a scene, for the "layout" phase of the reference."""

    def __init__(self, bodies, ghosts):
        self.n, self.w = N, types.SimpleNamespace(n=N)
        self._bodies, self._ghosts = bodies, ghosts

    def bodies_in_world(self):
        return self._bodies

    def ghosts_in_world(self):
        return self._ghosts


def one_object(world, shape_of, pose_of):
    """The object shape_of of the world, alone, standing where its object pose_of stands."""
    out = World64([], False)
    for k in ("kind", "entity", "group", "omask", "capsule", "dims"):
        setattr(out, k, getattr(world, k)[[shape_of]])
    out.origin, out.basis = world.origin[[pose_of]], world.basis[[pose_of]]
    out._derive()
    return out


def rejected(check, *args):
    try:
        check(*args)
    except AssertionError as e:
        print("rejected:", str(e)[:160])
        return True
    return False


def test_the_checkers_reject_the_three_layout_mistakes():
    world, bodies, ghosts, recs = phase_world("layout")
    _, _, trig = scene_reference()
    parent, ht = layout_topology(N, trig)
    from banggameengine_amd.world import flatten_topology
    slot = flatten_topology(parent, ht)[0].astype(np.int64)
    sc = Members(bodies, ghosts)
    valid = np.array([record_valid(m) for m in recs])
    right = pen_of(world)(as_spheres(recs))
    check_members(sc, {"penetration": right}, need_bodies=PEN_FLOORS["bodies named"] // 2)
    check_penetrations(world, recs, valid, right)
    has_entity = (right["kind"] == RAY_BODY) | (right["kind"] == RAY_TRIGGER)
    index_of = {int(e): k for k, e in enumerate(world.entity)}

    # 1: a slot reported as an entity
    wrong = right.copy()
    wrong["entity"][has_entity] = slot[right["entity"][has_entity]]
    assert (wrong["entity"] != right["entity"]).sum() >= 0.9 * has_entity.sum()
    assert rejected(check_members, sc, {"penetration": wrong}, PEN_FLOORS["bodies named"] // 2)
    assert rejected(check_penetrations, world, recs, valid, wrong)

    # 2: the winner's point and normal from the pose of the entity whose index is the winner's slot
    wrong, n_reposed = right.copy(), 0
    for i in np.nonzero(has_entity)[0]:
        e = int(right["entity"][i])
        if int(slot[e]) in index_of:
            other = one_object(world, index_of[e], index_of[int(slot[e])])
            h = signed_ref(other, recs["position"][i], recs["radius"][i], recs["layer_mask"][i], slack=1e9)[0]
            wrong["point"][i], wrong["normal"][i] = h.point, h.normal
            n_reposed += 1
    print(f"{n_reposed} of {int(has_entity.sum())} winners posed from the entity at their slot's index")
    assert n_reposed >= 0.5 * has_entity.sum()
    check_members(sc, {"penetration": wrong}, need_bodies=PEN_FLOORS["bodies named"] // 2)  # (the entities are right: this one is the float64 comparison's)
    assert rejected(check_penetrations, world, recs, valid, wrong)

    # 3: the slots at and beyond the entity count not scanned
    near = world.entity[slot[world.entity] < N]
    assert 0 < len(world.entity) - len(near) < 0.1 * len(world.entity)
    wrong = pen_of(subset(world, near))(as_spheres(recs))
    lost = np.nonzero(has_entity & (slot[np.where(has_entity, right["entity"], 0)] >= N))[0]
    print(f"{len(world.entity) - len(near)} objects at slots >= {N}; {len(lost)} winners among them")
    assert len(lost) >= 1 and all(wrong[i].tobytes() != right[i].tobytes() for i in lost)
    assert rejected(check_penetrations, world, recs, valid, wrong)
