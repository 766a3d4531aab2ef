"""Draw batches (include/bge_world.h bge_world_draw_batches*): the grouping restated in numpy, hand-worked cases, the exported
symbols, the C99 view of the header and the C++20 compile of the adapter's members.

The GPU tests (test_gpu_draw_batches.py) compare the device's batches and record order with draw_batches_ref() exactly."""
from __future__ import annotations

import os
import subprocess

import numpy as np

import banggameengine_amd as B
from banggameengine_amd import _capi
from banggameengine_amd import world as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_KEY = 0xFFFFFFFF


def draw_batches_ref(visible_mask, keys, n_keys):
    """batches (n_keys, 2) uint32 = (first_instance, instance_count) per key, and the entity indices in record order: the
    visible entities whose key is below n_keys, sorted by (key, entity index)."""
    visible_mask = np.asarray(visible_mask, bool)
    keys = np.asarray(keys, np.uint32)
    assert visible_mask.shape == keys.shape and keys.ndim == 1
    entity = np.nonzero(visible_mask & (keys < np.uint32(min(n_keys, 2 ** 32 - 1))) & (n_keys > 0))[0].astype(np.uint32)
    key = keys[entity]
    order = np.lexsort((entity, key))
    entity, key = entity[order], key[order]
    count = np.bincount(key, minlength=n_keys).astype(np.uint64)
    first = np.concatenate([[0], np.cumsum(count)[:-1]]).astype(np.uint64) if n_keys else count
    batches = np.stack([first, count], axis=1).astype(np.uint32).reshape(n_keys, 2)
    return batches, entity


def _check(mask, keys, n_keys, batches, entities):
    b, e = draw_batches_ref(mask, keys, n_keys)
    assert b.dtype == np.uint32 and e.dtype == np.uint32 and b.shape == (n_keys, 2)
    assert b.tolist() == batches, b.tolist()
    assert e.tolist() == entities, e.tolist()


def test_empty_batches_at_the_front_in_the_middle_and_at_the_back():
    #          e: 0  1  2  3  4  5
    keys = [2, 4, 2, 1, 4, 2]
    _check(np.ones(6, bool), keys, 7, [[0, 0], [0, 1], [1, 3], [4, 0], [4, 2], [6, 0], [6, 0]], [3, 0, 2, 5, 1, 4])
    # an invisible entity leaves its batch and shifts the ones behind it
    _check(np.array([1, 1, 0, 1, 1, 1], bool), keys, 7, [[0, 0], [0, 1], [1, 2], [3, 0], [3, 2], [5, 0], [5, 0]], [3, 0, 5, 1, 4])
    # nothing visible: every batch is (0, 0)
    _check(np.zeros(6, bool), keys, 3, [[0, 0], [0, 0], [0, 0]], [])


def test_all_entities_in_one_key():
    _check(np.ones(5, bool), [0] * 5, 1, [[0, 5]], [0, 1, 2, 3, 4])
    _check(np.ones(5, bool), [3] * 5, 5, [[0, 0], [0, 0], [0, 0], [0, 5], [5, 0]], [0, 1, 2, 3, 4])


def test_keys_descending_with_entity_index():
    _check(np.ones(4, bool), [3, 2, 1, 0], 4, [[0, 1], [1, 1], [2, 1], [3, 1]], [3, 2, 1, 0])
    _check(np.ones(6, bool), [2, 2, 1, 1, 0, 0], 3, [[0, 2], [2, 2], [4, 2]], [4, 5, 2, 3, 0, 1])  # ties keep entity order


def test_a_key_equal_to_n_keys_and_no_draw_key_are_left_out():
    _check(np.ones(5, bool), [0, 2, 1, 3, NO_KEY], 2, [[0, 1], [1, 1]], [0, 2])
    _check(np.ones(3, bool), [NO_KEY] * 3, 65536, [[0, 0]] * 65536, [])
    b, e = draw_batches_ref(np.ones(4, bool), [65535, 65536, 0, NO_KEY], 65536)
    assert e.tolist() == [2, 0] and b[0].tolist() == [0, 1] and b[65535].tolist() == [1, 1] and int(b[:, 1].sum()) == 2


def test_exported_symbols_are_present_and_declared():
    lib = B.lib()
    for name in ("bge_world_upload_draw_keys", "bge_world_upload_draw_keys_indexed", "bge_world_draw_batches",
                 "bge_world_draw_batches_device"):
        assert getattr(lib, name) is not None
        assert name in _capi.SYMBOLS and getattr(lib, name).argtypes == _capi.SYMBOLS[name][1]
    for name in ("upload_draw_keys", "draw_batches", "draw_batches_device"):
        assert callable(getattr(B.World, name))
    assert W.NO_DRAW_KEY == NO_KEY and W.DRAW_MAX_KEYS == 65536


def test_c99_view_of_the_header(tmp_path):
    exe = str(tmp_path / "abi_check_batches")
    lib = os.path.join(ROOT, "banggameengine_amd")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "abi_check_batches.c"), f"-L{lib}", "-lbge_world", f"-Wl,-rpath,{lib}",
                           "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "batches abi ok" in r.stdout


def test_adapter_members_compile_against_reference_shapes(tmp_path):
    subprocess.check_call(["g++", "-std=c++20", "-O0", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-c",
                           os.path.join(ROOT, "tests", "cpp", "batches_reference_shapes.cpp"), "-o", str(tmp_path / "batches_reference_shapes.o")])
