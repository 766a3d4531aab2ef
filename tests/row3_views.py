"""Every way of observing the world matrices, for tests/test_gpu_row3_defer.py and its child processes (no test in here).

A tick may leave the translation row of a flat body unstored (DESIGN.md §4.1 "Deferred translation row"); whoever reads a matrix
composes it or has it stored first.  `observe` gathers what each reader returns, `expect` what the oracle's matrices make of it."""
from __future__ import annotations

import ctypes as C

import numpy as np

import banggameengine_amd as B
from banggameengine_amd import synth
from banggameengine_amd._capi import lib
from banggameengine_amd.world import ARRAY_ROOT_WORLDS, ARRAY_WORLD, NO_PARENT

from refmodel.visible import visible_ref32

F = np.float32
N_KEYS = 3
# a frustum that contains every body of these scenes (|x|, |y|, |z| <= 1e4), and one plane that cuts them: y >= CUT_Y
EVERYTHING = np.array([[1, 0, 0, 1e4], [-1, 0, 0, 1e4], [0, 1, 0, 1e4], [0, -1, 0, 1e4], [0, 0, 1, 1e4], [0, 0, -1, 1e4]], F)
CUT_Y = 125.0
CUT = np.array([[0, 1, 0, -CUT_Y]], F)


def hip():
    for name in ("libamdhip64.so", "libamdhip64.so.7", "libamdhip64.so.6", "/opt/rocm/lib/libamdhip64.so"):
        try:
            h = C.CDLL(name)
            h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            return h
        except OSError:
            continue
    raise RuntimeError("HIP runtime library not found")


def read_device(ptr, shape, dtype=F):
    out = np.empty(shape, dtype)
    assert hip().hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0  # device -> host
    return out


def scene(n, seed=0):
    """n flat Dynamic bodies of mass 1, far above y = 0, falling faster than the sleeping threshold (0.8 m/s) from the start."""
    wl = synth.config("flat1m", n=n)
    wl.pos[:, 1] += F(100.0)
    rng = np.random.default_rng(300 + seed)
    vel = wl.vel.copy()
    vel[:, 1] = rng.uniform(-3.0, -1.0, n).astype(F)
    return wl, vel


def render_setup(w, n):
    """Unit boxes as bounds and a draw key per entity."""
    w.upload_bounds(np.zeros((n, 3), F), np.full((n, 3), 0.5, F))
    w.upload_draw_keys((np.arange(n) % N_KEYS).astype(np.uint32))


def shuffled(n, seed=5):
    return np.random.default_rng(seed).permutation(n).astype(np.uint32)


def download_world_indexed(w, idx):
    idx = np.ascontiguousarray(idx, np.uint32)
    out = np.empty((len(idx), 16), F)
    if len(idx):
        B._capi.check(lib().bge_world_download_world_indexed(w._h, len(idx), idx.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
    return out


def observe(w, n, idx, n_roots, render=True):
    """download_world, download_world_indexed(idx), the visible list and the draw batches of EVERYTHING, the list of CUT, pack_roots."""
    out = {"world": w.download_world(), "indexed": download_world_indexed(w, idx)}
    if render:
        vis = w.visible(EVERYTHING)
        out["visible_entities"], out["visible_world"] = vis["entities"], vis["world"]
        cut = w.visible(CUT)
        out["cut_entities"], out["cut_world"] = cut["entities"], cut["world"]
        bat = w.draw_batches(EVERYTHING, N_KEYS)
        out["batches"], out["batch_entities"], out["batch_world"] = bat["batches"], bat["entities"], bat["world"]
    w.pack_roots()
    w.sync()
    ptr, count = w.device_array(ARRAY_ROOT_WORLDS)
    assert count == n_roots
    out["roots"] = read_device(ptr, (n_roots, 16))
    return out


def expect(ref_world, idx, parent, render=True):
    """What `observe` must return when the matrices are ref_world (entity order) and every Transform is clean."""
    n = len(ref_world)
    out = {"world": ref_world, "indexed": ref_world[idx]}
    if render:
        ent = np.arange(n, dtype=np.uint32)
        out["visible_entities"], out["visible_world"] = ent, ref_world
        cut = np.flatnonzero(visible_ref32(ref_world, np.zeros((n, 3), F), np.full((n, 3), 0.5, F), CUT)).astype(np.uint32)
        out["cut_entities"], out["cut_world"] = cut, ref_world[cut]
        key = ent % N_KEYS
        order = np.lexsort((ent, key)).astype(np.uint32)
        counts = np.bincount(key, minlength=N_KEYS).astype(np.uint32)
        first = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.uint32)
        out["batches"] = np.stack([first, counts], axis=1)
        out["batch_entities"], out["batch_world"] = order, ref_world[order]
    out["roots"] = ref_world[np.asarray(parent) == NO_PARENT]
    return out


def assert_same(got, want, what):
    assert got.keys() == want.keys()
    for k in want:
        g, x = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.shape == x.shape, f"{k} ({what}): shape {g.shape}, want {x.shape}"
        if g.tobytes() != x.tobytes():
            gw, xw = g.view(np.uint32).ravel(), x.view(np.uint32).ravel()
            bad = np.flatnonzero(gw != xw)
            raise AssertionError(f"{k} ({what}): {len(bad)} of {gw.size} words differ, first at flat index {bad[:5].tolist()}: "
                                 f"got {g.ravel()[bad[0]]!r} want {x.ravel()[bad[0]]!r}")


def raw_world(w, n_slots):
    """The bytes behind BGE_ARRAY_WORLD (slot order).  Asking for the pointer pins the world: no tick defers a row after it."""
    w.sync()
    ptr, count = w.device_array(ARRAY_WORLD)
    assert count == n_slots
    return read_device(ptr, (n_slots, 16))
