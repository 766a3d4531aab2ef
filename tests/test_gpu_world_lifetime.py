"""A closed world gives back everything it took (csrc/bge_device_buffer.hpp, DESIGN.md "Who owns device memory").

One cycle opens a World, drives every feature that allocates, and closes it.  bge_device_memory() must then read (0, 0) exactly, and
the device's free memory must not drop over repeated cycles by more than the runtime's own growth plus one allocation granule: the
first check catches a buffer of any size that is left off the owner, the second one an allocation that bypasses the owner."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import banggameengine_amd as B
from banggameengine_amd import world as W

pytestmark = pytest.mark.gpu

DT = W.FIXED_DT
N, N_GROWN = 1024, 1500            # four tiles of 256 slots; the second topology makes every carried array and both entity arrays grow
N_TRIGGERS, N_CHARS, N_KEYS = 70, 64, 8   # more ghosts than BGE_TRIGGER_GRID_MIN's default of 64: the grid answers for them
HOLDER, FROZEN, LEAF = 80, 81, 82  # a bodiless entity, its child and grandchild: depth 2; the child is a frozen root once HOLDER loses its Transform
FLAGS = B.TICK_ALL | B.TICK_BROADPHASE | B.TICK_AABBS | B.TICK_NORMAL_MATRICES
RECORD_WORDS = 12                  # a routed broadphase record: 48 bytes


def scene(n):
    """Rows of boxes 0.95 apart along x (neighbours overlap: pairs, dynamic contacts, islands), resting near the plane."""
    i = np.arange(n)
    pos = np.stack([(i % 32) * 0.95, np.full(n, 0.52), (i // 32) * 1.5], axis=1).astype(np.float32)
    body = np.full(n, B.BODY_DYNAMIC, np.uint8)
    body[:N_TRIGGERS] = B.BODY_NONE            # the trigger volumes' entities
    body[N_TRIGGERS:HOLDER] = B.BODY_STATIC    # obstacles for the static contacts
    body[HOLDER:LEAF + 1] = B.BODY_NONE
    parent = np.full(n, B.NO_PARENT, np.uint32)
    parent[FROZEN], parent[LEAF] = HOLDER, FROZEN
    return parent, pos, body


def cycle(with_comm=False):
    """Open, use everything that allocates, close.  Returns what bge_device_memory() read while the world was open (None where the
    library has no such entry point: the same body measures the commit before it)."""
    parent, pos, body = scene(N)
    zeros, ones = np.zeros((N, 3), np.float32), np.ones((N, 3), np.float32)
    w = B.World(device=0)
    try:
        w.set_topology(parent)
        w.upload_trs(pos, zeros, ones)
        w.upload_bodies(body, np.ones(N, np.float32), np.zeros(N, np.uint8), np.full((N, 3), 0.5, np.float32), np.full(N, 1, np.uint32),
                        np.full(N, 0xFFFFFFFF, np.uint32))
        w.set_ground_plane(True)
        w.set_static_contacts(True)
        w.set_dynamic_contacts(True)
        trig = np.arange(N_TRIGGERS, dtype=np.uint32)
        w.upload_triggers(trig, np.zeros(N_TRIGGERS, np.uint8), np.full((N_TRIGGERS, 3), 0.8, np.float32), np.full(N_TRIGGERS, 4, np.uint32),
                          np.full(N_TRIGGERS, 0xFFFFFFFF, np.uint32), np.zeros(N_TRIGGERS, np.uint8), np.ones(N_TRIGGERS, np.uint8))
        w.profile_enable(2)
        if with_comm:
            w.comm_init(1, 0, B.World.comm_unique_id(), N)
        for _ in range(2):
            w.tick(dt=DT, flags=FLAGS | (B.TICK_GATHER_ROOTS if with_comm else 0))
        for _ in range(2):
            w.step_simulation(DT, 4, DT, flags=FLAGS)
        w.trigger_events()
        w.profile_read()
        w.pairs()

        # one rank of the sharded broadphase: route, pack, search what was "received"
        w.set_global_ids(np.arange(N, dtype=np.uint32))
        counts = w.bp_route(0, np.zeros(2, np.float32))
        n_records = int(counts.sum())
        send = torch.empty(max(n_records, 1) * RECORD_WORDS, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        w.bp_pack(send.data_ptr())
        w.bp_find(send.data_ptr() if n_records else 0, n_records, 0, -np.inf, np.inf)
        w.sync()
        w.pairs()
        del send

        w.set_query_index(True, min_work=0)
        origins = pos[100:164] + np.float32([0.1, 4.0, 0.1])
        down = np.tile(np.float32([0, -1, 0]), (len(origins), 1))
        w.raycast(origins, down)
        w.raycast_all(origins, down)
        w.sphere_cast(origins, down, radius=0.3)
        w.sphere_cast_all(origins, down, radius=0.3)
        w.overlap_sphere(pos[100:164], 0.7)
        w.sphere_penetration(pos[100:164], 0.7)
        w.sphere_move(origins, down * 2, radius=0.3)
        w.sphere_step_move(origins, down * 2, radius=0.3, step_height=0.3)
        w.sphere_recover(pos[100:164], radius=0.7)

        w.characters_create(W.make_characters(pos[200:200 + N_CHARS] + np.float32([0.0, 1.5, 0.0]), radius=0.3))
        w.characters_ride(True)
        w.characters_crowd(True, max_push=0.1)
        w.characters_push(True, force=10.0)
        w.characters_watch_triggers()
        w.characters_set_input(W.make_character_inputs(np.full(N_CHARS, 0.05, np.float32), 0.0))
        w.characters_update(DT, 1)
        w.characters_trigger_events()
        w.characters_state()

        w.crowd_query(W.make_crowd_spheres(pos[300:400], 0.6))
        w.apply_impulses(np.arange(500, 520), np.tile(np.float32([0, 1, 0]), (20, 1)))
        w.debug_lines()
        w.upload_bounds(zeros, np.full((N, 3), 0.5, np.float32))
        w.visible(None)
        w.upload_draw_keys(np.arange(N, dtype=np.uint32) % N_KEYS)
        w.draw_batches(None, N_KEYS)

        # the second topology: more entities, and HOLDER without its Transform (its clean child keeps its matrix: a frozen root)
        parent2, pos2, body2 = scene(N_GROWN)
        has_transform = np.ones(N_GROWN, np.uint8)
        has_transform[HOLDER] = 0
        w.set_topology(parent2, has_transform)
        w.upload_trs(pos2[N:], np.zeros((N_GROWN - N, 3), np.float32), np.ones((N_GROWN - N, 3), np.float32), first=N)
        w.upload_bodies(body2[N:], first=N)
        w.tick(dt=DT, flags=FLAGS)
        w.sync()
        return B.device_memory() if hasattr(B, "device_memory") else None
    finally:
        w.close()


def test_a_closed_world_holds_nothing():
    """Exact: (0, 0) before the first world, more while one is open, (0, 0) after close(), three times over (the first cycle with a
    one-rank communicator, whose ring buffers are the library's too); two worlds at once add up, and each takes only its share along."""
    assert B.device_memory() == (0, 0)
    for k in range(3):
        blocks, nbytes = cycle(with_comm=k == 0)
        print(f"cycle {k}: {blocks} blocks, {nbytes} bytes while open; after close {B.device_memory()}")
        assert blocks > 100 and nbytes > N * 64 * 2   # (the world matrices alone are 64 bytes a slot)
        assert B.device_memory() == (0, 0), k

    parent, pos, body = scene(N)

    def small(n):
        w = B.World(device=0)
        w.set_topology(parent[:n] if n < HOLDER else parent)
        w.upload_trs(pos[:w.n], np.zeros((w.n, 3), np.float32), np.ones((w.n, 3), np.float32))
        w.tick(dt=DT)
        w.sync()
        return w

    a = small(64)
    alone = B.device_memory()
    assert alone[0] > 0 and alone[1] > 0
    b = small(N)
    both = B.device_memory()
    assert both[0] > alone[0] and both[1] > alone[1]
    a.close()
    assert B.device_memory() == (both[0] - alone[0], both[1] - alone[1])
    a = small(64)
    assert B.device_memory() == both        # (the same calls allocate the same)
    b.close()
    assert B.device_memory() == alone
    a.close()
    assert B.device_memory() == (0, 0)


# What the same five cycles lose at the commit before the buffers owned themselves (7f97c30, whose release_all() freed every
# buffer by a hand-kept list): PARENT_LOSS bytes of free device memory, the HIP runtime's own growth.  GRANULE: the drop of free
# memory when a fresh process allocates one byte.  Both measured on an MI355X.
PARENT_LOSS = 0
GRANULE = 2 << 20


def test_nothing_bypasses_the_owner():
    """Free device memory after two warm-up cycles (code objects, the runtime's pools) and after three more.  No communicator here:
    what RCCL allocates for itself is not the library's and does not come back with the world."""
    for _ in range(2):
        cycle()
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    for _ in range(3):
        cycle()
    torch.cuda.synchronize()
    after = torch.cuda.mem_get_info()[0]
    print(f"free device memory: {before} before, {after} after three cycles: lost {before - after} bytes")
    assert before - after <= PARENT_LOSS + GRANULE
