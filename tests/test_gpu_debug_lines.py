"""The debug overlay on the device (include/bge_world.h bge_world_debug_lines*) against the float64 reference of
refmodel/debug_lines.py.

Tolerance: the reference takes the device's own binary32 poses (download_pose / download_bodies), ghost poses as
recorded before the tick and the dimensions the library holds, so what differs is the kernel's binary32 arithmetic — a rotation
of a local point plus the origin.  Bound: the point tolerance of the ray tests, P_REL = 2e-5 per unit of coordinate magnitude,
the magnitude being |origin|_inf + the shape's bounding radius.  Colours and counts are exact; the shapes section is compared
line by line IN ORDER over 100 % of the lines."""
from __future__ import annotations

import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import banggameengine_amd as B
from banggameengine_amd import world as W

from refmodel.tolerances import P_REL
from refmodel.rays import quat_from_euler
from refmodel.debug_lines import COL_CONTACT, CONTACTS, DYNAMIC, GHOST, KINEMATIC, SHAPES, STATIC, Obj, basis_of, debug_lines_ref, in_region
from refmodel.device import FLAGS, Scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KIND = {W.BODY_STATIC: STATIC, W.BODY_DYNAMIC: DYNAMIC, W.BODY_KINEMATIC: KINEMATIC}


class DebugScene(Scene):
    """The ray tests' random scene with a chosen share of capsules, an optional hierarchy, and the list of bodies that are in the
    world (uploaded before the last tick, not removed)."""

    def __init__(self, n, rng, n_triggers=0, spread=30.0, plane=True, capsule_p=0.5, parent=None):
        self.n = n
        self.w = B.World(device=0)
        self.w.set_topology(np.full(n, W.NO_PARENT, np.uint32) if parent is None else parent)
        pos = np.stack([rng.uniform(-spread, spread, n), rng.uniform(0.3, 6.0, n), rng.uniform(-spread, spread, n)], 1)
        self.w.upload_trs(pos, rng.uniform(-math.pi, math.pi, (n, 3)), np.ones((n, 3)))
        self.type = rng.choice([W.BODY_STATIC, W.BODY_DYNAMIC, W.BODY_KINEMATIC, W.BODY_NONE], n, p=[0.3, 0.4, 0.2, 0.1]).astype(np.uint8)
        self.trig = np.zeros(0, np.int64)
        if n_triggers:
            self.trig = np.sort(rng.choice(n, n_triggers, replace=False))
            self.type[self.trig] = W.BODY_NONE
        self.shape = (rng.random(n) < capsule_p).astype(np.uint8)
        self.size = rng.uniform(0.1, 1.5, (n, 3)).astype(np.float32)
        self.layer = (1 << rng.integers(0, 4, n)).astype(np.uint32)
        self.mask = rng.choice(np.array([0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0x3, 0], np.uint32), n)
        self.w.upload_bodies(self.type, None, self.shape, self.size, self.layer, self.mask)
        self.plane = plane
        self.w.set_ground_plane(plane)
        self.t_active = np.ones(len(self.trig), np.uint8)
        self.t_oneshot = np.zeros(len(self.trig), np.uint8)
        self.in_world = self.type != W.BODY_NONE
        if len(self.trig):
            self.upload_triggers()

    def ref_objects(self, only=None):
        """Obj list in the specified order: bodies in the world by entity index, then live ghosts in trigger order."""
        pos, _ = self.w.download_pose()
        quat = self.w.download_bodies()["quat"].astype(np.float64)
        dims = self.dims()
        objs, ents = [], []
        bodies = np.nonzero(self.in_world)[0] if only is None else only[self.in_world[only]]
        for e in bodies:
            objs.append(Obj(KIND[int(self.type[e])], pos[e], quat[e], self.shape[e] == 1, dims[e]))
            ents.append(int(e))
        if only is None and len(self.trig):
            gp, ge = self.ghost_pose
            live = self.w.trigger_active(self.trig) & self.t_active.astype(bool)
            for e in self.trig[live]:
                objs.append(Obj(GHOST, gp[e], quat_from_euler(ge[e].astype(np.float64)), self.shape[e] == 1, dims[e]))
                ents.append(int(e))
        return objs, ents


def line_tolerance(objs, plane, region=None):
    """Per line of the shapes section: P_REL x (|origin|_inf + bounding radius)."""
    tol = [np.full(12, P_REL * (25.0 * math.sqrt(2.0)))] if plane else []
    for o in objs:
        if not in_region(region, o.origin):
            continue
        radius = o.dims[0] + o.dims[1] if o.capsule else float(np.linalg.norm(o.dims))
        tol.append(np.full(o.n_lines(), P_REL * (float(np.abs(o.origin).max()) + radius)))
    return np.concatenate(tol) if tol else np.zeros(0)


def assert_shapes_equal(got, want, tol, what):
    assert len(got) == len(want) == len(tol), f"{what}: {len(got)} lines, reference {len(want)}"
    assert np.array_equal(got["abgr"], want["abgr"]), f"{what}: colours differ"
    err = np.maximum(np.abs(got["from"] - want["from"]).max(axis=1), np.abs(got["to"] - want["to"]).max(axis=1)) if len(got) else np.zeros(0)
    worst = float((err / np.maximum(tol, 1e-30)).max()) if len(got) else 0.0
    print(f"{what}: {len(got)} lines, worst error {float(err.max()) if len(got) else 0.0:.3e}, {worst:.3f} of the tolerance")
    bad = np.nonzero(err > tol)[0]
    assert len(bad) == 0, f"{what}: line {bad[0]} off by {err[bad[0]]:.3e} (tolerance {tol[bad[0]]:.3e}); got {got[bad[0]]}, want {want[bad[0]]}"


def check_scene(sc, what):
    objs, _ = sc.ref_objects()
    want = debug_lines_ref(objs, sc.plane, flags=SHAPES)
    got = sc.w.debug_lines(W.DEBUG_SHAPES)
    boxes = sum(1 for o in objs if not o.capsule)
    assert len(got) == 12 * boxes + 120 * (len(objs) - boxes) + (12 if sc.plane else 0)
    assert_shapes_equal(got, want, line_tolerance(objs, sc.plane), what)
    return objs, got


def _fire_one_shot(sc, rng):
    """trigger 0 inactive; trigger 1 a one-shot with a Dynamic box put right on it (it fires in the first tick)."""
    sc.t_active[0] = 0
    sc.t_oneshot[1] = 1
    sc.upload_triggers()
    body = int(np.nonzero(sc.type == W.BODY_DYNAMIC)[0][0])
    pos, _ = sc.w.download_pose()
    sc.w.upload_trs(pos[sc.trig[1]][None], first=body)
    sc.mask[body] = 0xFFFFFFFF
    sc.shape[body] = 0
    sc.w.upload_bodies(sc.type[body:body + 1], None, sc.shape[body:body + 1], sc.size[body:body + 1], sc.layer[body:body + 1],
                       sc.mask[body:body + 1], first=body)
    sc.mask[sc.trig[1]] = 0xFFFFFFFF
    sc.upload_triggers()


@pytest.mark.parametrize("n,seed,plane", [(600, 1, True), (3000, 2, False)])
def test_random_scene_shapes_in_order(n, seed, plane):
    rng = np.random.default_rng(seed)
    sc = DebugScene(n, rng, n_triggers=10, plane=plane)
    try:
        _fire_one_shot(sc, rng)
        sc.tick(4)
        assert not sc.w.trigger_active(sc.trig[1:2])[0], "the one-shot did not fire"
        objs, got = check_scene(sc, f"random scene n={n}")
        kinds = {o.kind for o in objs}
        assert kinds == {STATIC, DYNAMIC, KINEMATIC, GHOST}
        assert sum(o.kind == GHOST for o in objs) == 8  # ten triggers, one inactive, one fired
        assert any(o.capsule for o in objs) and any(not o.capsule for o in objs)
    finally:
        sc.close()


def test_hierarchy_uploaded_and_removed_bodies():
    rng = np.random.default_rng(3)
    n = 1500
    parent = np.full(n, W.NO_PARENT, np.uint32)
    kids = rng.choice(np.arange(1, n), n // 2, replace=False)
    parent[kids] = (rng.random(len(kids)) * kids).astype(np.uint32)  # a parent of lower index: chains of several levels
    slot, _, _, _ = W.flatten_topology(parent)
    assert not np.array_equal(slot, np.arange(n)), "slot order equals entity order: the scene tests nothing"
    sc = DebugScene(n, rng, n_triggers=4, parent=parent)
    try:
        sc.tick(3)
        check_scene(sc, "hierarchy")
        # bodies uploaded after the last tick and removed bodies are not in the world
        up = np.arange(100, 150)
        sc.w.upload_bodies(sc.type[up], None, sc.shape[up], sc.size[up], sc.layer[up], sc.mask[up], first=100)
        sc.w.upload_bodies(np.full(50, W.BODY_NONE, np.uint8), first=200)
        before = int(sc.in_world.sum())
        sc.in_world[100:150] = False
        sc.in_world[200:250] = False
        assert int(sc.in_world.sum()) < before - 60
        check_scene(sc, "uploaded / removed")
        sc.type[200:250] = W.BODY_NONE
        sc.in_world = sc.type != W.BODY_NONE
        sc.tick(1)
        check_scene(sc, "after the next tick")
    finally:
        sc.close()


def _contact_scene():
    """Crates resting on the plane, on Static boxes and on each other."""
    pos, typ, size, yaw = [], [], [], []
    for k in range(6):  # platforms (Static), a crate on each
        pos += [[10.0 + 6.0 * k, 0.5, 3.0 * k], [10.0 + 6.0 * k + 0.3 * (k % 3), 1.502, 3.0 * k]]
        typ += [W.BODY_STATIC, W.BODY_DYNAMIC]
        size += [[2.0, 0.5, 2.0], [0.5, 0.5, 0.5]]
        yaw += [0.07 * k, 0.3 + 0.11 * k]
    for k in range(6):  # crates on the plane
        pos += [[-4.0 * k, 0.402 + 0.05 * k, -20.0]]
        typ += [W.BODY_DYNAMIC]
        size += [[0.5, 0.4 + 0.05 * k, 0.5]]
        yaw += [0.13 * k]
    for k in range(6):  # towers of two on the plane, aligned (they stand)
        pos += [[-4.0 * k, 0.502, 20.0], [-4.0 * k, 1.504, 20.0]]
        typ += [W.BODY_DYNAMIC, W.BODY_DYNAMIC]
        size += [[0.5, 0.5, 0.5], [0.5, 0.5, 0.5]]
        yaw += [0.17 * k, 0.17 * k]
    n = len(pos)
    w = B.World(device=0)
    w.set_topology(np.full(n, W.NO_PARENT, np.uint32))
    euler = np.zeros((n, 3), np.float32)
    euler[:, 1] = yaw
    w.upload_trs(np.float32(pos), euler, np.ones((n, 3)))
    w.upload_bodies(np.uint8(typ), None, np.zeros(n, np.uint8), np.float32(size))
    return w, n


def _contact_reference(w, n):
    """(pointOnB, normal) from the three contact downloads and the device's poses."""
    pos, _ = w.download_pose()
    quat = w.download_bodies()["quat"].astype(np.float64)
    out = []
    npl, ppl = w.download_contacts()
    for e in range(n):
        for j in range(npl[e]):
            out.append((np.array([ppl[e, j, 4], 0.0, ppl[e, j, 6]], np.float64), (0.0, 1.0, 0.0)))
    nb, bh, bp = w.download_box_contacts()
    for e in range(n):
        for k in range(nb[e]):
            b = int(bh[e, k, 0])
            for j in range(bh[e, k, 1]):
                pt = bp[e, k, j].astype(np.float64)
                out.append((basis_of(quat[b]) @ pt[3:6] + pos[b].astype(np.float64), pt[6:9]))
    hdr, pts = w.download_dynamic_pairs()
    for k in range(len(hdr)):
        b = int(hdr[k, 1])
        for j in range(hdr[k, 2]):
            pt = pts[k, j].astype(np.float64)
            out.append((basis_of(quat[b]) @ pt[3:6] + pos[b].astype(np.float64), pt[6:9]))
    return out, (int(npl.sum()), int(bh[:, :, 1][bh[:, :, 0] != 0xFFFFFFFF].sum()), int(hdr[:, 2].sum()) if len(hdr) else 0)


def _sorted(lines):
    key = np.concatenate([lines["from"], lines["to"]], axis=1)
    return lines[np.lexsort(key.T[::-1])]


def test_contact_section_matches_the_downloads():
    w, n = _contact_scene()
    try:
        w.set_ground_plane(True)
        w.set_static_contacts(True)
        w.set_dynamic_contacts(True)
        w.tick(flags=W.TICK_ALL, ticks=90)
        contacts, (n_plane, n_box, n_pair) = _contact_reference(w, n)
        print(f"contact points: plane {n_plane}, obstacle {n_box}, pairs {n_pair}")
        assert n_plane >= 12 and n_box >= 6 and n_pair >= 6, "the scene holds too few manifolds to test anything"
        want = debug_lines_ref([], False, contacts, CONTACTS)
        got = w.debug_lines(W.DEBUG_CONTACTS)
        assert len(got) == n_plane + n_box + n_pair == len(want)
        assert set(got["abgr"].tolist()) == {COL_CONTACT}
        g, r = _sorted(got), _sorted(want)
        # sorted on the host: a point's neighbours in the order are > 1e-3 apart here, the errors ~1e-6, so the orders agree
        tol = P_REL * (np.abs(r["from"]).max(axis=1) + 1.0)
        err = np.maximum(np.abs(g["from"] - r["from"]).max(axis=1), np.abs(g["to"] - r["to"]).max(axis=1))
        print(f"contacts: worst error {err.max():.3e}, {float((err / tol).max()):.3f} of the tolerance")
        assert np.all(err <= tol), (g[err > tol][:3], r[err > tol][:3])
        # flags: the two halves of ALL; two calls return the same multiset
        both = w.debug_lines(W.DEBUG_ALL)
        shapes = w.debug_lines(W.DEBUG_SHAPES)
        assert len(both) == len(shapes) + len(got)
        assert both[:len(shapes)].tobytes() == shapes.tobytes()
        assert _sorted(both[len(shapes):]).tobytes() == _sorted(got).tobytes()
        assert _sorted(w.debug_lines(W.DEBUG_CONTACTS)).tobytes() == _sorted(got).tobytes()
        # region: contacts by their `from` point
        region = ((-30.0, -1.0, -25.0), (5.0, 5.0, -15.0))
        gr = w.debug_lines(W.DEBUG_CONTACTS, region)
        keep = np.array([in_region(region, f) for f in got["from"]])
        assert 0 < keep.sum() < len(got) and _sorted(gr).tobytes() == _sorted(got[keep]).tobytes()
        # the three switches off: the section is empty
        w.set_ground_plane(False)
        w.set_static_contacts(False)
        w.set_dynamic_contacts(False)
        assert len(w.debug_lines(W.DEBUG_CONTACTS)) == 0
        assert len(w.debug_lines(W.DEBUG_ALL)) == len(shapes) - 12
    finally:
        w.close()


def test_region_with_an_entity_on_the_boundary():
    rng = np.random.default_rng(7)
    sc = DebugScene(2000, rng, n_triggers=6)
    try:
        sc.tick(2)
        objs, _ = sc.ref_objects()
        # region_min.x and region_max.x ARE the x of two bodies' origins: both are in (closed box)
        a, b = objs[10].origin.astype(np.float32), objs[40].origin.astype(np.float32)
        region = (np.minimum(a, b) - np.float32([0, 5, 8]), np.maximum(a, b) + np.float32([0, 5, 8]))
        want = debug_lines_ref(objs, sc.plane, flags=SHAPES, region=region)
        inside = [o for o in objs if in_region(region, o.origin)]
        assert objs[10] in inside and objs[40] in inside and len(inside) < len(objs)
        got = sc.w.debug_lines(W.DEBUG_SHAPES, region)
        assert_shapes_equal(got, want, line_tolerance(objs, sc.plane, region), "region")
        nan = float("nan")
        for bad in (((nan, 0, 0), (5, 5, 5)), ((0, 0, 0), (5, 5, nan)), ((5, 0, 0), (-5, 9, 9))):
            only_plane = sc.w.debug_lines(W.DEBUG_ALL, bad)
            assert len(only_plane) == 12 and only_plane.tobytes() == got[:12].tobytes()
    finally:
        sc.close()


def test_count_cap_device_entry_and_determinism():
    import torch
    rng = np.random.default_rng(9)
    sc = DebugScene(5000, rng, n_triggers=5, plane=False)  # (no plane, no contacts: the whole list is the shapes section)
    try:
        sc.tick(3)
        a = sc.w.debug_lines()
        b = sc.w.debug_lines()
        assert len(a) > 5000 and a.tobytes() == b.tobytes()
        lib = B.lib()
        total = C.c_uint64(0)
        assert lib.bge_world_debug_lines(sc.w._h, None, None, 0, C.byref(total)) == 0  # desc = NULL: ALL, whole world
        assert total.value == len(a)
        # cap = total - 1: BGE_ERR_INVALID, *total right, and the guard record behind cap untouched
        buf = np.zeros(len(a), W.DEBUG_LINE_DTYPE)
        buf.view(np.uint8)[:] = 0xA5
        total = C.c_uint64(0)
        assert lib.bge_world_debug_lines(sc.w._h, None, buf.ctypes.data_as(C.c_void_p), len(a) - 1, C.byref(total)) == -1
        assert total.value == len(a)
        assert np.all(buf.view(np.uint8)[-28:] == 0xA5)
        # the device entry: same bytes, same total; a guard record behind cap stays
        lines = torch.full(((len(a) + 1) * 28,), 0xA5, dtype=torch.uint8, device="cuda:0")
        tot = torch.zeros(1, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        sc.w.debug_lines_device(lines.data_ptr(), len(a), tot.data_ptr())
        sc.w.sync()
        host = lines.cpu().numpy()
        assert int(tot.item()) == len(a)
        assert host[:len(a) * 28].tobytes() == a.tobytes() and np.all(host[len(a) * 28:] == 0xA5)
        # a cap in the middle of the list: nothing beyond it is written, total still counts everything
        cap = len(a) // 2 + 1
        lines.fill_(0xA5)
        torch.cuda.synchronize()
        sc.w.debug_lines_device(lines.data_ptr(), cap, tot.data_ptr())
        sc.w.sync()
        host = lines.cpu().numpy()
        assert int(tot.item()) == len(a)
        assert host[:cap * 28].tobytes() == a[:cap].tobytes() and np.all(host[cap * 28:] == 0xA5)
        # a 4-byte aligned, not 16-byte aligned destination
        lines.fill_(0xA5)
        torch.cuda.synchronize()
        sc.w.debug_lines_device(lines.data_ptr() + 4, len(a), tot.data_ptr())
        sc.w.sync()
        host = lines.cpu().numpy()
        assert host[4:4 + len(a) * 28].tobytes() == a.tobytes() and np.all(host[:4] == 0xA5) and np.all(host[4 + len(a) * 28:] == 0xA5)
    finally:
        sc.close()


def test_empty_world_is_not_an_error():
    w = B.World(device=0)
    try:
        w.set_topology(np.full(4, W.NO_PARENT, np.uint32))
        w.upload_trs(np.zeros((4, 3)), np.zeros((4, 3)), np.ones((4, 3)))
        w.tick(flags=FLAGS)
        assert len(w.debug_lines()) == 0
    finally:
        w.close()


def test_the_query_changes_nothing():
    def run(query):
        rng = np.random.default_rng(21)
        sc = DebugScene(4000, rng, n_triggers=6)
        try:
            sc.tick(3)
            before = (sc.w.download_world().tobytes(), sc.w.download_pose()[0].tobytes(), sc.w.download_pose()[1].tobytes(),
                      sc.w.download_bodies()["quat"].tobytes(), sc.w.download_bodies()["linvel"].tobytes())
            if query:
                sc.w.debug_lines()
                sc.w.debug_lines(W.DEBUG_SHAPES, ((-5, 0, -5), (5, 5, 5)))
                after = (sc.w.download_world().tobytes(), sc.w.download_pose()[0].tobytes(), sc.w.download_pose()[1].tobytes(),
                         sc.w.download_bodies()["quat"].tobytes(), sc.w.download_bodies()["linvel"].tobytes())
                assert before == after
            sc.tick(2)
            return sc.w.download_world().tobytes(), sc.w.download_pose()[0].tobytes(), sc.w.download_bodies()["quat"].tobytes()
        finally:
            sc.close()

    assert run(True) == run(False)


def test_adapter_overlay_on_demo_scene(tmp_path):
    cpp = os.path.join(ROOT, "tests", "cpp")
    lib = os.path.join(ROOT, "banggameengine_amd")
    exe = str(tmp_path / "debug_demo_scene")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unused-parameter", "-o", exe,
                           os.path.join(cpp, "debug_demo_scene.cpp"), f"-L{lib}", "-lbge_world", f"-Wl,-rpath,{lib}",
                           "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "demo_scene_reference_format.json")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "all checks passed" in r.stdout
    assert "[PhysicsDebug] overlay ON" in r.stdout and "[PhysicsDebug] overlay OFF" in r.stdout


def test_full_size_million_bodies():
    rng = np.random.default_rng(11)
    n = 1 << 20
    sc = DebugScene(n, rng, spread=500.0, capsule_p=0.01)
    try:
        sc.tick(2)
        per = np.where(sc.in_world, np.where(sc.shape == 1, 120, 12), 0).astype(np.int64)
        first = 12 + np.concatenate([[0], np.cumsum(per)[:-1]])  # the count prefix locates an entity's lines
        got = sc.w.debug_lines(W.DEBUG_SHAPES)
        assert len(got) == 12 + int(per.sum())
        pick = np.sort(rng.choice(n, 2000, replace=False))
        objs, ents = sc.ref_objects(only=pick)
        want = debug_lines_ref(objs, False, flags=SHAPES)
        sel = np.concatenate([np.arange(first[e], first[e] + per[e]) for e in ents])
        assert_shapes_equal(got[sel], want, line_tolerance(objs, False), "1 M bodies, 2000 sampled")
    finally:
        sc.close()
