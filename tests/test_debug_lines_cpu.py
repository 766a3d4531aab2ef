"""The debug overlay's specification (include/bge_world.h bge_world_debug_lines*) as a float64 reference, with hand-worked cases,
plus the C99 view of the record and the C++20 compile of the adapter's overlay members.

debug_lines_ref() is written from the description of the reference's drawer (BulletDebugDrawer: DrawBox, DrawCapsule,
DrawStaticPlane, drawContactPoint; PhysicsSystem::CollectDebugLines for the colours): the GPU tests compare the device's lines
with it."""
from __future__ import annotations

import numpy as np

from abi import build_and_run_c99, compile_reference_shapes
from refmodel.debug_lines import (COL_CONTACT, COL_DYNAMIC, COL_STATIC, COL_TRIGGER, CONTACTS, DYNAMIC, GHOST, KINEMATIC, SHAPES, STATIC, Obj,
                                  debug_lines_ref)

# ---------------------------------------------------------------- hand-worked cases

def test_unit_box_at_the_origin():
    got = debug_lines_ref([Obj(DYNAMIC, (0, 0, 0), dims=(1, 1, 1))], plane=False)
    c = [(-1, -1, -1), (1, -1, -1), (1, 1, -1), (-1, 1, -1), (-1, -1, 1), (1, -1, 1), (1, 1, 1), (-1, 1, 1)]
    want = [(c[a], c[b]) for a, b in [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)]]
    assert len(got) == 12
    assert np.array_equal(got["from"], np.array([w[0] for w in want], np.float64))
    assert np.array_equal(got["to"], np.array([w[1] for w in want], np.float64))
    assert set(got["abgr"].tolist()) == {COL_DYNAMIC}


def test_box_rotated_a_quarter_turn_about_y():
    h = np.sqrt(0.5)
    got = debug_lines_ref([Obj(STATIC, (10, 0, 0), quat=(0, h, 0, h), dims=(2, 1, 0.5))], plane=False)
    # +90 degrees about y takes local x to world -z and local z to world x: corner 0 (-2, -1, -0.5) -> (-0.5, -1, 2)
    assert np.allclose(got["from"][0], (10 - 0.5, -1, 2), atol=1e-12)
    assert np.allclose(got["to"][0], (10 - 0.5, -1, -2), atol=1e-12)      # corner 1 (2, -1, -0.5)
    assert np.allclose(got["to"][8], (10 + 0.5, -1, 2), atol=1e-12)       # edge 0-4: corner 4 (-2, -1, 0.5)
    assert set(got["abgr"].tolist()) == {COL_STATIC}


def test_upright_capsule():
    got = debug_lines_ref([Obj(KINEMATIC, (0, 0, 0), capsule=True, dims=(0.5, 1.0, 0.5))], plane=False)
    assert len(got) == 120
    ring = got[:72]
    for k in range(24):
        top, bottom, side = ring[3 * k], ring[3 * k + 1], ring[3 * k + 2]
        for rec, y in ((top, 1.0), (bottom, -1.0)):
            for p in (rec["from"], rec["to"]):
                assert abs(p[1] - y) < 1e-12 and abs(np.hypot(p[0], p[2]) - 0.5) < 1e-7
        assert np.array_equal(side["from"], top["from"]) and np.array_equal(side["to"], bottom["from"])
        assert np.allclose(top["to"], ring[3 * ((k + 1) % 24)]["from"], atol=1e-6)  # the ring closes
    # the ring starts on the basis' Z column and turns towards its X column
    assert np.allclose(ring[0]["from"], (0, 1, 0.5), atol=1e-12) and np.allclose(ring[3 * 6]["from"], (0.5, 1, 0), atol=1e-7)
    hemi = got[72:]
    assert np.allclose(hemi[0]["from"], (0, 1, 0.5), atol=1e-12)   # top, Z-column plane
    assert np.allclose(hemi[1]["from"], (0, -1, -0.5), atol=1e-12)  # bottom, mirrored
    assert np.allclose(hemi[2]["from"], (0.5, 1, 0), atol=1e-12)   # top, X-column plane
    for k in range(4):
        assert np.allclose(hemi[44 + k]["to"], (0, 1.5 if k % 2 == 0 else -1.5, 0), atol=1e-7)
    assert set(got["abgr"].tolist()) == {COL_DYNAMIC}  # Kinematic is NOT static-coloured


def test_plane_constants():
    got = debug_lines_ref([], plane=True)
    assert len(got) == 12 and set(got["abgr"].tolist()) == {COL_STATIC}
    c = [(-25, 0, 25), (-25, 0, -25), (25, 0, -25), (25, 0, 25)]
    for i in range(4):
        assert np.array_equal(got["from"][i], c[i]) and np.array_equal(got["to"][i], c[(i + 1) % 4])
    assert np.allclose(got["from"][4], (-15, 0, 25), atol=1e-5) and np.allclose(got["to"][4], (-15, 0, -25), atol=1e-5)
    assert np.allclose(got["from"][5], (-25, 0, 15), atol=1e-5) and np.allclose(got["to"][5], (25, 0, 15), atol=1e-5)
    assert np.allclose(got["from"][10], (15, 0, 25), atol=1e-5) and np.allclose(got["from"][11], (-25, 0, -15), atol=1e-5)


def test_colours_and_contact_lines():
    objs = [Obj(STATIC, (0, 0, 0)), Obj(DYNAMIC, (2, 0, 0)), Obj(KINEMATIC, (4, 0, 0)), Obj(GHOST, (6, 0, 0))]
    contacts = [((1, 0, 1), (0, 2, 0)), ((0, 1, 0), (0, 0, 0)), ((0, 0, 0), (3, 0, 4))]
    got = debug_lines_ref(objs, True, contacts)
    assert len(got) == 12 + 48 + 3
    assert [int(got["abgr"][12 * k]) for k in range(5)] == [COL_STATIC, COL_STATIC, COL_DYNAMIC, COL_DYNAMIC, COL_TRIGGER]
    tail = got[60:]
    assert set(tail["abgr"].tolist()) == {COL_CONTACT}
    assert np.allclose(tail["to"][0], (1, 0.25, 1)) and np.allclose(tail["to"][1], (0, 1.25, 0))  # normalised; degenerate -> +y
    assert np.allclose(tail["to"][2], (0.15, 0, 0.2))
    # the two flags are the two halves
    assert np.array_equal(debug_lines_ref(objs, True, contacts, SHAPES), got[:60])
    assert np.array_equal(debug_lines_ref(objs, True, contacts, CONTACTS), got[60:])


def test_region_rule():
    objs = [Obj(DYNAMIC, (1, 2, 3)), Obj(DYNAMIC, (1.5, 2, 3)), Obj(GHOST, (0, 0, 0), capsule=True)]
    contacts = [((1, 0, 3), (0, 1, 0)), ((9, 0, 9), (0, 1, 0))]
    got = debug_lines_ref(objs, True, contacts, region=((0, 0, 0), (1, 2, 3)))  # origin exactly on region_max is in
    assert len(got) == 12 + 12 + 120 + 1
    assert np.array_equal(got[12:24], debug_lines_ref(objs[:1], False))
    nan = float("nan")
    for bad in (((nan, 0, 0), (5, 5, 5)), ((0, 0, 0), (5, nan, 5)), ((2, 0, 0), (1, 5, 5))):
        got = debug_lines_ref(objs, True, contacts, region=bad)
        assert len(got) == 12 and np.array_equal(got, debug_lines_ref([], True))  # only the plane


# ---------------------------------------------------------------- the C and C++ views

def test_c99_record_layout(tmp_path):
    build_and_run_c99(tmp_path, "abi_check_debug.c", "debug abi ok")


def test_adapter_overlay_members_compile_against_reference_shapes(tmp_path):
    compile_reference_shapes(tmp_path, "debug_reference_shapes.cpp")
