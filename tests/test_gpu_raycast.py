"""Ray queries on the device (include/bge_world.h bge_world_raycast*) against the float64 reference of test_raycast_cpu.py.

Tolerances: the reference takes the device's own binary32 poses (download_pose / download_bodies) and binary32
ray inputs, so what differs is the kernel's binary32 arithmetic — a rotation into the body frame, one slab division or a
quadratic solved about the point of closest approach.  Bounds: fraction 1e-5 relative + 1e-6 absolute; point 2e-5 per unit of
coordinate magnitude; normal 1e-4 per component plus 2e-6 x (|origin|_1 + |direction * max_distance|_1) / (the hit shape's
smallest half extent or radius) — the entry point is only known to a few binary32 ulp of the ray's magnitudes, and the normal
of a small capsule turns by that error over its radius (measured: 1.3e-3 for a ray from ~700 units at a small capsule)."""
from __future__ import annotations

import math
import os
import subprocess

import numpy as np
import pytest

import banggameengine_amd as B
from banggameengine_amd import world as W

from test_raycast_cpu import RAY_BODY, RAY_GROUND, RAY_MISS, RAY_TRIGGER, NO_ENTITY, Obj, World64, quat_from_euler, random_rays

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F_REL, F_ABS, P_REL, N_ABS, N_SCALE = 1e-5, 1e-6, 2e-5, 1e-4, 2e-6
FLAGS = W.TICK_ALL | W.TICK_BROADPHASE


class Scene:
    """A world plus what the reference needs to rebuild its objects."""

    def __init__(self, n, rng, n_triggers=0, spread=30.0, plane=True, parent=None, has_transform=None):
        self.n = n
        self.w = B.World(device=0)
        self.w.set_topology(np.full(n, W.NO_PARENT, np.uint32) if parent is None else parent, has_transform)
        pos = np.stack([rng.uniform(-spread, spread, n), rng.uniform(0.3, 6.0, n), rng.uniform(-spread, spread, n)], 1)
        self.w.upload_trs(pos, rng.uniform(-math.pi, math.pi, (n, 3)), np.ones((n, 3)))
        self.type = rng.choice([W.BODY_STATIC, W.BODY_DYNAMIC, W.BODY_KINEMATIC], n, p=[0.3, 0.5, 0.2]).astype(np.uint8)
        self.trig = np.zeros(0, np.int64)
        if n_triggers:
            self.trig = rng.choice(n, n_triggers, replace=False)
            self.type[self.trig] = W.BODY_NONE
        self.shape = rng.integers(0, 2, n).astype(np.uint8)
        self.size = rng.uniform(0.1, 1.5, (n, 3)).astype(np.float32)
        self.layer = (1 << rng.integers(0, 4, n)).astype(np.uint32)
        self.mask = rng.choice(np.array([0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0x3, 0], np.uint32), n)
        self.w.upload_bodies(self.type, None, self.shape, self.size, self.layer, self.mask)
        self.plane = plane
        self.w.set_ground_plane(plane)
        self.t_active = np.ones(len(self.trig), np.uint8)
        self.t_oneshot = np.zeros(len(self.trig), np.uint8)
        if len(self.trig):
            self.upload_triggers()

    def upload_triggers(self):
        self.w.upload_triggers(self.trig, self.shape[self.trig], self.size[self.trig], self.layer[self.trig], self.mask[self.trig],
                               self.t_oneshot, self.t_active)

    def tick(self, k=1):
        for _ in range(k):
            self.ghost_pose = self.w.download_pose()  # ghosts are posed from the Transforms as they are before the step
            self.w.tick(flags=FLAGS)

    def dims(self):
        """Per entity: the box's half extents with margin or the capsule's (radius, half height, radius), as the library holds them."""
        h = np.maximum(self.size, np.float32(0.01))
        m0 = np.float32(0.04)
        safe = (np.float32(0.1) * h.min(axis=1))[:, None]
        inner = h - m0
        box = np.where(safe < m0, ((inner + m0) - safe) + safe, inner + m0).astype(np.float32)
        cap = np.stack([h[:, 0], np.maximum(self.size[:, 1], np.float32(0)), h[:, 0]], 1)
        return np.where(self.shape[:, None] == 1, cap, box)

    def bodies_in_world(self):
        return np.nonzero(self.type != W.BODY_NONE)[0]

    def ghosts_in_world(self):
        return self.trig[self.t_active.astype(bool)]

    def objects(self):
        """The reference's world: every body at the pose the device holds, every active ghost at its posed pose."""
        pos, _ = self.w.download_pose()
        quat = self.w.download_bodies()["quat"].astype(np.float64)
        dims = self.dims()
        live, ghosts = self.bodies_in_world(), self.ghosts_in_world()
        gp, ge = self.ghost_pose
        gq = np.array([quat_from_euler(ge[e].astype(np.float64)) for e in ghosts]).reshape(-1, 4)
        ent = np.concatenate([live, ghosts])
        kind = np.concatenate([np.full(len(live), RAY_BODY), np.full(len(ghosts), RAY_TRIGGER)])
        return World64.from_arrays(kind, ent, self.layer[ent], self.mask[ent], self.shape[ent] == 1, dims[ent],
                                   np.concatenate([pos[live], gp[ghosts]]), np.concatenate([quat[live], gq]), self.plane)

    def close(self):
        self.w.close()


def check_against_reference(ref, o, d, md, mask, got, need_hits=50):
    checked = hits = 0
    err_f = err_p = err_n = 0.0
    for i in range(len(o)):
        if not ref.clear(o[i], d[i], md[i], mask[i]):
            continue
        checked += 1
        want = ref.cast_all(o[i], d[i], md[i], mask[i])
        if not want:
            assert got["kind"][i] == RAY_MISS and got["entity"][i] == NO_ENTITY, f"ray {i}: hit where the reference misses"
            continue
        f, code, kind, ent, n = want[0]
        assert (got["kind"][i], got["entity"][i]) == (kind, ent), f"ray {i}: {got['kind'][i]}/{got['entity'][i]} != {kind}/{ent}"
        hits += 1
        gf = float(got["fraction"][i])
        assert abs(gf - f) <= F_REL * f + F_ABS, f"ray {i}: fraction {gf} vs {f}"
        p = o[i].astype(np.float64) + (d[i] * md[i]).astype(np.float64) * f
        assert np.all(np.abs(got["point"][i] - p) <= P_REL * (1.0 + np.abs(p))), f"ray {i}: point {got['point'][i]} vs {p}"
        # the entry point carries binary32 rounding of the ray's magnitudes; the normal turns by that over the shape's size
        n_tol = N_ABS + N_SCALE * float(np.abs(o[i]).sum() + np.abs(d[i] * md[i]).sum()) / ref.min_dim(code)
        assert np.all(np.abs(got["normal"][i] - n) <= n_tol), f"ray {i}: normal {got['normal'][i]} vs {n}"
        assert got["distance"][i] == np.float32(got["fraction"][i] * md[i])
        err_f = max(err_f, abs(gf - f) / max(f, 1e-6))
        err_p = max(err_p, float(np.max(np.abs(got["point"][i] - p) / (1.0 + np.abs(p)))))
        err_n = max(err_n, float(np.max(np.abs(got["normal"][i] - n))))
    assert checked >= 0.5 * len(o) and hits >= need_hits, (checked, hits)
    print(f"checked {checked} of {len(o)} rays, {hits} hits; max rel err f {err_f:.2e}, point {err_p:.2e}, normal {err_n:.2e}")
    return hits


def check_all_hits(ref, o, d, md, mask, got, allh):
    """All hits: per-ray sets in (f, code) order, offsets, and the first one is the closest hit (got: the closest hits of the
    same rays, or of a batch these rays begin)."""
    off = allh["offsets"].astype(np.int64)
    assert off[0] == 0 and np.all(np.diff(off) >= 0) and off[-1] == len(allh["kind"])
    for i in range(len(o)):
        want = ref.cast_all(o[i], d[i], md[i], mask[i])
        seg = slice(off[i], off[i + 1])
        if ref.clear(o[i], d[i], md[i], mask[i]):
            got_set = sorted(zip(allh["kind"][seg].tolist(), allh["entity"][seg].tolist()))
            assert got_set == sorted((h[2], h[3]) for h in want), f"ray {i}"
        fr = allh["fraction"][seg]
        assert np.all(np.diff(fr) >= 0)
        if off[i + 1] > off[i]:
            for k in ("kind", "entity", "fraction", "distance"):
                assert allh[k][off[i]] == got[k][i], (i, k)
            assert np.array_equal(allh["point"][off[i]], got["point"][i]) and np.array_equal(allh["normal"][off[i]], got["normal"][i])
        else:
            assert got["kind"][i] == RAY_MISS


@pytest.mark.parametrize("n,seed", [(2000, 1), (20000, 2)])
def test_random_scene_closest_and_all(n, seed):
    rng = np.random.default_rng(seed)
    sc = Scene(n, rng, n_triggers=12)
    try:
        sc.tick(6)
        ref = sc.objects()
        pos, _ = sc.w.download_pose()
        o, d, md, mask = random_rays(rng, 3000, pos)
        got = sc.w.raycast(o, d, md, mask)
        check_against_reference(ref, o, d, md, mask, got)
        assert (got["kind"] == RAY_BODY).any() and (got["kind"] == RAY_MISS).any()
        sub = slice(0, 256)
        check_all_hits(ref, o[sub], d[sub], md[sub], mask[sub], got, sc.w.raycast_all(o[sub], d[sub], md[sub], mask[sub]))
    finally:
        sc.close()


def test_determinism_device_entry_and_batch_of_one():
    import torch
    rng = np.random.default_rng(5)
    sc = Scene(8000, rng, n_triggers=8)
    try:
        sc.tick(3)
        pos, _ = sc.w.download_pose()
        o, d, md, mask = random_rays(rng, 4096, pos)
        a = sc.w.raycast(o, d, md, mask)
        b = sc.w.raycast(o, d, md, mask)
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k
        rays = W.make_rays(o, d, md, mask)
        rt = torch.from_numpy(rays.view(np.uint8)).to("cuda:0")
        ht = torch.zeros(len(rays) * 40, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        sc.w.raycast_device(rt, ht)
        sc.w.sync()
        hd = ht.cpu().numpy().view(W.RAY_HIT_DTYPE)
        for k in a:
            assert np.ascontiguousarray(hd[k]).tobytes() == a[k].tobytes(), k
        for i in (0, 17, 4095):
            one = sc.w.raycast(o[i:i + 1], d[i:i + 1], md[i:i + 1], mask[i:i + 1])
            for k in a:
                assert one[k][0].tobytes() == a[k][i].tobytes(), (i, k)
        # raycast_all: a cap that is too small is BGE_ERR_INVALID with the true total
        import ctypes as C
        lib = B.lib()
        total = C.c_uint64(0)
        r8 = rays[:64].copy()
        assert lib.bge_world_raycast_all(sc.w._h, 64, r8.ctypes.data_as(C.c_void_p), None, 0, None, C.byref(total)) == 0
        assert total.value > 1
        hits = np.zeros(int(total.value), W.RAY_HIT_DTYPE)
        assert lib.bge_world_raycast_all(sc.w._h, 64, r8.ctypes.data_as(C.c_void_p), hits.ctypes.data_as(C.c_void_p), total.value - 1,
                                         None, C.byref(total)) == -1
        assert total.value == len(hits)
        assert lib.bge_world_raycast(sc.w._h, 0, None, None) == 0  # n_rays = 0 is a no-op
    finally:
        sc.close()


def _world(n=4):
    w = B.World(device=0)
    w.set_topology(np.full(n, W.NO_PARENT, np.uint32))
    return w


def test_directed_plane_filters_and_no_hit_inputs():
    w = _world(2)
    try:
        # a Static box "Ground" 50 x 1 x 50 at y = -0.01, layer 1; a Dynamic box far away that falls asleep on the plane
        w.upload_trs(np.float32([[0, -0.01, 0], [80, 0.5, 0]]), np.zeros((2, 3)), np.ones((2, 3)))
        w.upload_bodies(np.uint8([W.BODY_STATIC, W.BODY_DYNAMIC]), None, np.uint8([0, 0]), np.float32([[50, 1, 50], [0.5, 0.5, 0.5]]),
                        np.uint32([1, 1]), np.uint32([0xFFFFFFFF, 0xFFFFFFFF]))
        w.set_ground_plane(True)
        w.tick(flags=FLAGS, ticks=400)  # > 2 s: the resting box sleeps
        state, _ = w.download_activation()
        assert state[1] == 2  # ISLAND_SLEEPING
        down = (0, -1, 0)
        h = w.raycast([[0, 10, 0]], [down], 200.0, 1)
        assert h["kind"][0] == RAY_BODY and h["entity"][0] == 0
        assert abs(h["point"][0][1] - 0.99) < 1e-5 and abs(h["distance"][0] - 9.01) < 1e-4 and h["normal"][0][1] == 1.0
        # the sleeping body is hit
        h = w.raycast([[80, 10, 0]], [down], 200.0, 1)
        assert h["kind"][0] == RAY_BODY and h["entity"][0] == 1
        # mask 1 never sees the plane; mask 2 beside the Ground box: the plane, no entity, +y; from below: -y
        h = w.raycast([[100, 10, 0], [100, 10, 0], [100, -3, 0], [100, 1, 0]], [down, down, (0, 1, 0), (1, 0, 0)], 200.0, [1, 2, 2, 2])
        assert h["kind"].tolist() == [RAY_MISS, RAY_GROUND, RAY_GROUND, RAY_MISS]
        assert h["entity"][1] == NO_ENTITY and h["normal"][1].tolist() == [0, 1, 0] and h["normal"][2].tolist() == [0, -1, 0]
        assert h["distance"][1] == np.float32(10.0) and h["fraction"][2] == np.float32(3 / 200)
        # inputs that see nothing: max distance <= 0, mask 0, zero direction, NaN
        nan = float("nan")
        h = w.raycast([[0, 10, 0]] * 5 + [[nan, 10, 0]], [down, down, down, (0, 0, 0), (0, nan, 0), down], [0.0, -5.0, 200, 200, 200, 200],
                      [1, 1, 0, 1, 1, 1])
        assert h["kind"].tolist() == [RAY_MISS] * 6 and h["entity"].tolist() == [NO_ENTITY] * 6
        assert not h["fraction"].any() and not h["point"].any()
        # inside-start rule: from inside the Ground box the ray does not hit it (the plane, mask 2, still is)
        h = w.raycast([[0, 0.5, 0], [0, 0.5, 0]], [down, down], 200.0, [1, 3])
        assert h["kind"][0] == RAY_MISS and h["kind"][1] == RAY_GROUND
        # object mask 0: never hit
        w.upload_bodies(np.uint8([W.BODY_STATIC]), None, None, np.float32([[50, 1, 50]]), np.uint32([1]), np.uint32([0]))
        w.tick(flags=FLAGS)
        assert w.raycast([[0, 10, 0]], [down], 200.0, 1)["kind"][0] == RAY_MISS
    finally:
        w.close()


def test_uploaded_and_removed_bodies_are_not_in_the_world():
    w = _world(3)
    try:
        w.upload_trs(np.float32([[0, 2, 0], [5, 2, 0], [10, 2, 0]]), np.zeros((3, 3)), np.ones((3, 3)))
        w.upload_bodies(np.uint8([W.BODY_STATIC, W.BODY_STATIC, W.BODY_NONE]))
        w.tick(flags=FLAGS)
        o, d = [[0, 10, 0], [5, 10, 0], [10, 10, 0]], [(0, -1, 0)] * 3
        assert w.raycast(o, d, 100.0, 1)["kind"].tolist() == [RAY_BODY, RAY_BODY, RAY_MISS]
        # body 1 removed, body 2 uploaded: neither is in the world before the next tick
        w.upload_bodies(np.uint8([W.BODY_NONE, W.BODY_STATIC]), first=1)
        assert w.raycast(o, d, 100.0, 1)["kind"].tolist() == [RAY_BODY, RAY_MISS, RAY_MISS]
        w.tick(flags=FLAGS)
        h = w.raycast(o, d, 100.0, 1)
        assert h["kind"].tolist() == [RAY_BODY, RAY_MISS, RAY_BODY] and h["entity"][2] == 2
    finally:
        w.close()


def test_triggers_layers_activity_one_shots_and_posed_pose():
    w = _world(4)
    try:
        # 0: trigger layer 4 at x = 0; 1: trigger layer 8 at x = 5, one-shot; 2: trigger at x = 10, inactive; 3: a Dynamic box
        # that falls into trigger 1 (one-shot fires)
        w.upload_trs(np.float32([[0, 2, 0], [5, 2, 0], [10, 2, 0], [5, 2.5, 0]]), np.zeros((4, 3)), np.ones((4, 3)))
        w.upload_bodies(np.uint8([W.BODY_NONE, W.BODY_NONE, W.BODY_NONE, W.BODY_DYNAMIC]), mask=np.uint32([0, 0, 0, 0xFFFFFFFF]))
        w.upload_triggers(np.uint32([0, 1, 2]), None, np.float32([[1, 1, 1]] * 3), np.uint32([4, 8, 4]), None,
                          np.uint8([0, 1, 0]), np.uint8([1, 1, 0]))
        o = [[0, 10, 0], [0, 10, 0], [10, 10, 0], [0, -3, 0]]
        d = [(0, -1, 0)] * 3 + [(0, 1, 0)]
        # never posed: nothing
        assert w.raycast(o, d, 100.0, [4, 1, 4, 4])["kind"].tolist() == [RAY_MISS] * 4
        w.tick(flags=FLAGS)  # the box overlaps trigger 1: the one-shot fires in this tick
        h = w.raycast(o, d, 100.0, [4, 1, 4, 4])
        assert h["kind"].tolist() == [RAY_TRIGGER, RAY_MISS, RAY_MISS, RAY_TRIGGER] and h["entity"][0] == 0
        assert abs(h["point"][0][1] - 3.0) < 1e-5 and h["normal"][0].tolist() == [0, 1, 0] and h["normal"][3].tolist() == [0, -1, 0]
        assert not w.trigger_active([1])[0]
        h = w.raycast([[5, 10, 0.9]], [(0, -1, 0)], 100.0, 8)  # the fired one-shot: gone
        assert h["kind"][0] == RAY_MISS
        # move trigger 0's entity: the ghost stays where the last tick posed it until the next tick
        w.upload_trs(np.float32([[0, 2, 20]]), first=0)
        assert w.raycast([[0, 10, 0]], [(0, -1, 0)], 100.0, 4)["kind"][0] == RAY_TRIGGER
        assert w.raycast([[0, 10, 20]], [(0, -1, 0)], 100.0, 4)["kind"][0] == RAY_MISS
        w.tick(flags=FLAGS)
        assert w.raycast([[0, 10, 0]], [(0, -1, 0)], 100.0, 4)["kind"][0] == RAY_MISS
        h = w.raycast([[0, 10, 20]], [(0, -1, 0)], 100.0, 4)
        assert h["kind"][0] == RAY_TRIGGER and h["entity"][0] == 0
    finally:
        w.close()


def test_adapter_hud_ray_on_demo_scene(tmp_path):
    cpp = os.path.join(ROOT, "tests", "cpp")
    lib = os.path.join(ROOT, "banggameengine_amd")
    exe = str(tmp_path / "raycast_demo_scene")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unused-parameter", "-o", exe,
                           os.path.join(cpp, "raycast_demo_scene.cpp"), f"-L{lib}", "-lbge_world", f"-Wl,-rpath,{lib}",
                           "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "demo_scene_reference_format.json")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "all checks passed" in r.stdout


def test_full_size_million_bodies():
    rng = np.random.default_rng(11)
    n = 1 << 20
    sc = Scene(n, rng, spread=500.0)
    try:
        sc.tick(2)
        pos, _ = sc.w.download_pose()
        o, d, md, mask = random_rays(rng, 4096, pos, spread=500.0)
        got = sc.w.raycast(o, d, md, mask)
        pick = rng.choice(4096, 256, replace=False)
        ref = sc.objects()
        check_against_reference(ref, o[pick], d[pick], md[pick], mask[pick], {k: v[pick] for k, v in got.items()}, need_hits=30)
    finally:
        sc.close()
