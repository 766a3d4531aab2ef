"""Thin numpy face of the C ABI (include/bge_world.h).  One method per entry point; no logic of its own."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from ._capi import CullDesc, DebugDesc, WorldDesc, WorldInfo, check, lib

NO_PARENT = 0xFFFFFFFF
BODY_STATIC, BODY_DYNAMIC, BODY_KINEMATIC, BODY_NONE = 0, 1, 2, 255
SHAPE_BOX, SHAPE_CAPSULE = 0, 1
TICK_PHYSICS, TICK_TRANSFORMS, TICK_BROADPHASE, TICK_ALL, TICK_GATHER_ROOTS, TICK_NORMAL_MATRICES, TICK_AABBS = 1, 2, 4, 3, 8, 16, 32
TICK_BULLET_BASIS = 64
ARRAY_WORLD, ARRAY_ROOT_WORLDS, ARRAY_SLOT_OF_ENTITY, ARRAY_POSITION, ARRAY_PAIRS = 0, 1, 2, 3, 4

# ray queries (bge_world_raycast*): the C records as numpy dtypes
RAY_MISS, RAY_BODY, RAY_TRIGGER, RAY_GROUND = 0, 1, 2, 3
RAY_NO_ENTITY = 0xFFFFFFFF
RAY_DTYPE = np.dtype([("origin", "<f4", (3,)), ("direction", "<f4", (3,)), ("max_distance", "<f4"), ("layer_mask", "<u4")])
RAY_HIT_DTYPE = np.dtype([("kind", "<u4"), ("entity", "<u4"), ("fraction", "<f4"), ("distance", "<f4"), ("point", "<f4", (3,)),
                          ("normal", "<f4", (3,))])
assert RAY_DTYPE.itemsize == 32 and RAY_HIT_DTYPE.itemsize == 40


def make_rays(origins, directions, max_distance=200.0, layer_mask=0xFFFFFFFF):
    """bge_ray records: origins / directions (n, 3); max_distance and layer_mask a scalar or one value per ray."""
    o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(directions, np.float32).reshape(-1, 3)
    if len(o) != len(d):
        raise ValueError(f"{len(o)} origins, {len(d)} directions")
    rays = np.zeros(len(o), RAY_DTYPE)
    rays["origin"] = o
    rays["direction"] = d
    rays["max_distance"] = np.broadcast_to(np.asarray(max_distance, np.float32), (len(o),))
    rays["layer_mask"] = np.broadcast_to(np.asarray(layer_mask, np.uint64).astype(np.uint32), (len(o),))
    return rays


def _device_records(records, results, records_name, results_name, record_bytes, result_bytes):
    """The count of whole records in a device tensor, after checking that the result tensor has room for as many."""
    nb = records.numel() * records.element_size()
    if nb % record_bytes:
        raise ValueError(f"{records_name} holds {nb} bytes, not a whole number of {record_bytes}-byte records")
    n = nb // record_bytes
    if results.numel() * results.element_size() < result_bytes * n:
        raise ValueError(f"{results_name} has room for {results.numel() * results.element_size()} bytes, {result_bytes * n} needed")
    if not (records.is_cuda and results.is_cuda and records.is_contiguous() and results.is_contiguous()):
        raise ValueError(f"{records_name} and {results_name} must be contiguous device tensors")
    return n


def _hit_fields(h):
    return {"kind": h["kind"].copy(), "entity": h["entity"].copy(), "fraction": h["fraction"].copy(),
            "distance": h["distance"].copy(), "point": h["point"].copy(), "normal": h["normal"].copy()}


# sphere queries (bge_world_sphere_cast*, bge_world_overlap_sphere): their records; a cast's hit is a RAY_HIT_DTYPE record
SPHERE_CAST_DTYPE = np.dtype([("origin", "<f4", (3,)), ("direction", "<f4", (3,)), ("max_distance", "<f4"), ("radius", "<f4"),
                              ("layer_mask", "<u4"), ("reserved", "<u4")])
SPHERE_DTYPE = np.dtype([("center", "<f4", (3,)), ("radius", "<f4"), ("layer_mask", "<u4")])
OVERLAP_HIT_DTYPE = np.dtype([("kind", "<u4"), ("entity", "<u4"), ("distance", "<f4")])
assert SPHERE_CAST_DTYPE.itemsize == 40 and SPHERE_DTYPE.itemsize == 20 and OVERLAP_HIT_DTYPE.itemsize == 12


def make_sphere_casts(origins, directions, max_distance=200.0, radius=0.5, layer_mask=0xFFFFFFFF):
    """bge_sphere_cast records: make_rays() plus the radius, a scalar or one value per cast."""
    rays = make_rays(origins, directions, max_distance, layer_mask)
    casts = np.zeros(len(rays), SPHERE_CAST_DTYPE)
    for k in ("origin", "direction", "max_distance", "layer_mask"):
        casts[k] = rays[k]
    casts["radius"] = np.broadcast_to(np.asarray(radius, np.float32), (len(rays),))
    return casts


def make_spheres(centers, radius, layer_mask=0xFFFFFFFF):
    """bge_sphere records: centers (n, 3); radius and layer_mask a scalar or one value per sphere."""
    c = np.ascontiguousarray(centers, np.float32).reshape(-1, 3)
    spheres = np.zeros(len(c), SPHERE_DTYPE)
    spheres["center"] = c
    spheres["radius"] = np.broadcast_to(np.asarray(radius, np.float32), (len(c),))
    spheres["layer_mask"] = np.broadcast_to(np.asarray(layer_mask, np.uint64).astype(np.uint32), (len(c),))
    return spheres


# sphere moves (bge_world_sphere_move*): bge_move_flags and the two records
MOVE_SLIDES = 4
MOVE_INVALID, MOVE_GROUNDED, MOVE_OUT_OF_SLIDES, MOVE_PROBE_HIT = 1, 2, 4, 8
SPHERE_MOVE_DTYPE = np.dtype([("position", "<f4", (3,)), ("displacement", "<f4", (3,)), ("radius", "<f4"), ("skin", "<f4"),
                              ("probe_distance", "<f4"), ("min_ground_ny", "<f4"), ("layer_mask", "<u4"), ("reserved", "<u4")])
SPHERE_MOVE_RESULT_DTYPE = np.dtype([("position", "<f4", (3,)), ("remaining", "<f4", (3,)), ("flags", "<u4"), ("n_hits", "<u4"),
                                     ("hit_kind", "<u4"), ("hit_entity", "<u4"), ("hit_normal", "<f4", (3,)), ("ground_kind", "<u4"),
                                     ("ground_entity", "<u4"), ("ground_distance", "<f4"), ("ground_normal", "<f4", (3,)),
                                     ("reserved", "<u4")])
assert SPHERE_MOVE_DTYPE.itemsize == 48 and SPHERE_MOVE_RESULT_DTYPE.itemsize == 80


def make_sphere_moves(positions, displacements, radius=0.5, skin=0.01, probe_distance=0.0, min_ground_ny=0.7071068, layer_mask=0xFFFFFFFF):
    """bge_sphere_move records: positions / displacements (n, 3); every other argument a scalar or one value per mover."""
    p = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(displacements, np.float32).reshape(-1, 3)
    if len(p) != len(d):
        raise ValueError(f"{len(p)} positions, {len(d)} displacements")
    moves = np.zeros(len(p), SPHERE_MOVE_DTYPE)
    moves["position"] = p
    moves["displacement"] = d
    for k, v in (("radius", radius), ("skin", skin), ("probe_distance", probe_distance), ("min_ground_ny", min_ground_ny)):
        moves[k] = np.broadcast_to(np.asarray(v, np.float32), (len(p),))
    moves["layer_mask"] = np.broadcast_to(np.asarray(layer_mask, np.uint64).astype(np.uint32), (len(p),))
    return moves


# sphere step moves (bge_world_sphere_step_move*): the two further flag bits and the records, which are the move's with step_height
# and step_rise where those have their reserved words
MOVE_STEP_TRIED, MOVE_STEPPED = 16, 32
SPHERE_STEP_MOVE_DTYPE = np.dtype([("position", "<f4", (3,)), ("displacement", "<f4", (3,)), ("radius", "<f4"), ("skin", "<f4"),
                                   ("probe_distance", "<f4"), ("min_ground_ny", "<f4"), ("layer_mask", "<u4"), ("step_height", "<f4")])
SPHERE_STEP_RESULT_DTYPE = np.dtype([("position", "<f4", (3,)), ("remaining", "<f4", (3,)), ("flags", "<u4"), ("n_hits", "<u4"),
                                     ("hit_kind", "<u4"), ("hit_entity", "<u4"), ("hit_normal", "<f4", (3,)), ("ground_kind", "<u4"),
                                     ("ground_entity", "<u4"), ("ground_distance", "<f4"), ("ground_normal", "<f4", (3,)),
                                     ("step_rise", "<f4")])
assert SPHERE_STEP_MOVE_DTYPE.itemsize == 48 and SPHERE_STEP_RESULT_DTYPE.itemsize == 80


def make_sphere_step_moves(positions, displacements, radius=0.5, skin=0.01, probe_distance=0.0, min_ground_ny=0.7071068, layer_mask=0xFFFFFFFF,
                           step_height=0.0):
    """bge_sphere_step_move records: make_sphere_moves() with step_height, a scalar or one value per mover."""
    plain = make_sphere_moves(positions, displacements, radius, skin, probe_distance, min_ground_ny, layer_mask)
    moves = plain.view(SPHERE_STEP_MOVE_DTYPE)
    moves["step_height"] = np.broadcast_to(np.asarray(step_height, np.float32), (len(moves),))
    return moves


# sphere penetration and recovery (bge_world_sphere_penetration*, bge_world_sphere_recover*): bge_recover_flags and the records; the
# penetration query's input is a SPHERE_DTYPE record
RECOVER_ROUNDS = 4
RECOVER_INVALID, RECOVER_MOVED, RECOVER_STUCK = 1, 2, 4
PENETRATION_HIT_DTYPE = np.dtype([("kind", "<u4"), ("entity", "<u4"), ("depth", "<f4"), ("point", "<f4", (3,)), ("normal", "<f4", (3,)),
                                  ("reserved", "<u4")])
SPHERE_RECOVER_DTYPE = np.dtype([("position", "<f4", (3,)), ("radius", "<f4"), ("skin", "<f4"), ("layer_mask", "<u4"), ("reserved", "<u4")])
SPHERE_RECOVER_RESULT_DTYPE = np.dtype([("position", "<f4", (3,)), ("pushed", "<f4", (3,)), ("flags", "<u4"), ("n_pushes", "<u4"),
                                        ("hit_kind", "<u4"), ("hit_entity", "<u4"), ("hit_normal", "<f4", (3,)), ("hit_depth", "<f4"),
                                        ("remaining_depth", "<f4"), ("reserved", "<u4")])
assert PENETRATION_HIT_DTYPE.itemsize == 40 and SPHERE_RECOVER_DTYPE.itemsize == 28 and SPHERE_RECOVER_RESULT_DTYPE.itemsize == 64


def make_sphere_recovers(positions, radius=0.5, skin=0.01, layer_mask=0xFFFFFFFF):
    """bge_sphere_recover records: positions (n, 3); every other argument a scalar or one value per sphere."""
    p = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
    records = np.zeros(len(p), SPHERE_RECOVER_DTYPE)
    records["position"] = p
    records["radius"] = np.broadcast_to(np.asarray(radius, np.float32), (len(p),))
    records["skin"] = np.broadcast_to(np.asarray(skin, np.float32), (len(p),))
    records["layer_mask"] = np.broadcast_to(np.asarray(layer_mask, np.uint64).astype(np.uint32), (len(p),))
    return records


# characters (bge_world_characters_*): bge_character_flags, bge_character_buttons and the three records
CHAR_INVALID, CHAR_GROUNDED, CHAR_JUMPED, CHAR_LANDED, CHAR_HEAD_BUMP = 1, 2, 4, 8, 16
CHAR_RECOVERED, CHAR_STUCK, CHAR_STEPPED, CHAR_OUT_OF_SLIDES = 32, 64, 128, 256
CHAR_BUTTON_JUMP = 1
# character trigger events (bge_world_characters_watch_triggers ..): bge_character_trigger_event_type and the watch's flag
CHAR_TRIGGER_ENTER, CHAR_TRIGGER_STAY, CHAR_TRIGGER_EXIT = 0, 1, 2
CHAR_TRIGGER_STAY_EVENTS = 1
CHARACTER_DESC_DTYPE = np.dtype([("position", "<f4", (3,)), ("radius", "<f4"), ("skin", "<f4"), ("step_height", "<f4"), ("min_ground_ny", "<f4"),
                                 ("probe_distance", "<f4"), ("gravity", "<f4"), ("jump_speed", "<f4"), ("fall_speed", "<f4"), ("layer_mask", "<u4")])
CHARACTER_INPUT_DTYPE = np.dtype([("walk_x", "<f4"), ("walk_z", "<f4"), ("buttons", "<u4"), ("reserved", "<u4")])
CHARACTER_STATE_DTYPE = np.dtype([("position", "<f4", (3,)), ("vertical_velocity", "<f4"), ("flags", "<u4"), ("ground_kind", "<u4"),
                                  ("ground_entity", "<u4"), ("ground_normal", "<f4", (3,)), ("hit_kind", "<u4"), ("hit_entity", "<u4"),
                                  ("hit_normal", "<f4", (3,)), ("step_rise", "<f4"), ("recovered", "<f4", (3,)), ("steps", "<u4")])
assert CHARACTER_DESC_DTYPE.itemsize == 48 and CHARACTER_INPUT_DTYPE.itemsize == 16 and CHARACTER_STATE_DTYPE.itemsize == 80
# character platform riding (bge_world_characters_ride ..): bge_character_ride_mode, bge_character_ride_flags and the record
CHAR_RIDE_ON, CHAR_RIDE_DYNAMIC = 1, 2
CHAR_RIDE_CARRIED, CHAR_RIDE_LOST = 1, 2
CHARACTER_RIDE_DTYPE = np.dtype([("flags", "<u4"), ("entity", "<u4"), ("anchor_position", "<f4", (3,)), ("anchor_rotation", "<f4", (4,)),
                                 ("carried", "<f4", (3,)), ("turn", "<f4", (4,))])
assert CHARACTER_RIDE_DTYPE.itemsize == 64
# crowd separation (bge_world_crowd_query*, bge_world_characters_crowd ..): bge_crowd_flags, bge_character_crowd_mode and the records
CROWD_INVALID, CROWD_PUSHED, CROWD_CLAMPED = 1, 2, 4
CHAR_CROWD_ON = 1
CROWD_SPHERE_DTYPE = np.dtype([("center", "<f4", (3,)), ("radius", "<f4"), ("group", "<u4"), ("mask", "<u4")])
CROWD_HIT_DTYPE = np.dtype([("flags", "<u4"), ("other", "<u4"), ("n_overlaps", "<u4"), ("depth", "<f4"), ("push", "<f4", (3,)),
                            ("reserved", "<u4")])
assert CROWD_SPHERE_DTYPE.itemsize == 24 and CROWD_HIT_DTYPE.itemsize == 32
# impulses and the characters' push (bge_world_apply_impulses*, bge_world_characters_push ..): bge_impulse_flags, bge_impulse_status,
# bge_character_push_mode and the records
IMPULSE_AT_POINT, IMPULSE_CENTRAL, IMPULSE_TORQUE, IMPULSE_WORLD_POINT = 0, 1, 2, 4
IMPULSE_APPLIED, IMPULSE_WOKE, IMPULSE_INVALID, IMPULSE_NO_BODY = 1, 2, 4, 8
CHAR_PUSH_ON = 1
IMPULSE_DTYPE = np.dtype([("entity", "<u4"), ("flags", "<u4"), ("impulse", "<f4", (3,)), ("point", "<f4", (3,))])
CHARACTER_PUSH_DESC_DTYPE = np.dtype([("flags", "<u4"), ("force", "<f4"), ("max_normal_y", "<f4"), ("body_mask", "<u4")])
assert IMPULSE_DTYPE.itemsize == 32 and CHARACTER_PUSH_DESC_DTYPE.itemsize == 16
# the query index (bge_world_set_query_index, bge_world_query_index_stats): bge_query_index_desc, bge_query_index_stats
QUERY_INDEX_MIN_WORK_DEFAULT = 1 << 30
QUERY_INDEX_DESC_DTYPE = np.dtype([("mode", "<u4"), ("cell_edge", "<f4"), ("max_cells", "<u4"), ("reserved", "<u4"), ("min_work", "<u8")])
QUERY_INDEX_STATS_DTYPE = np.dtype([("built", "<u4"), ("table_size", "<u4"), ("bodies_indexed", "<u8"), ("bodies_wide", "<u8"),
                                    ("queries_indexed", "<u8"), ("queries_far", "<u8"), ("cell_edge", "<f4"), ("reserved", "<u4"),
                                    ("builds", "<u8"), ("reserved2", "<u8")])
assert QUERY_INDEX_DESC_DTYPE.itemsize == 24 and QUERY_INDEX_STATS_DTYPE.itemsize == 64


def make_crowd_spheres(centers, radius=0.5, group=1, mask=0xFFFFFFFF):
    """bge_crowd_sphere records: centers (n, 3); every other argument a scalar or one value per sphere."""
    c = np.ascontiguousarray(centers, np.float32).reshape(-1, 3)
    spheres = np.zeros(len(c), CROWD_SPHERE_DTYPE)
    spheres["center"] = c
    spheres["radius"] = np.broadcast_to(np.asarray(radius, np.float32), (len(c),))
    spheres["group"] = np.broadcast_to(np.asarray(group, np.uint64).astype(np.uint32), (len(c),))
    spheres["mask"] = np.broadcast_to(np.asarray(mask, np.uint64).astype(np.uint32), (len(c),))
    return spheres


def make_impulses(entity, impulse, point=None, kind=None, world_point=False):
    """bge_impulse records: entity (n,), impulse (n, 3); point (n, 3) or None (zeros); kind and world_point a scalar or one value
    per record.  kind = None: IMPULSE_AT_POINT where a point is given, IMPULSE_CENTRAL otherwise."""
    if kind is None:
        kind = IMPULSE_CENTRAL if point is None else IMPULSE_AT_POINT
    e = np.atleast_1d(np.asarray(entity, np.uint64)).astype(np.uint32)
    records = np.zeros(len(e), IMPULSE_DTYPE)
    records["entity"] = e
    records["impulse"] = np.ascontiguousarray(impulse, np.float32).reshape(-1, 3)
    if point is not None:
        records["point"] = np.ascontiguousarray(point, np.float32).reshape(-1, 3)
    flags = np.broadcast_to(np.asarray(kind, np.uint32), (len(e),)).copy()
    flags |= np.where(np.broadcast_to(np.asarray(world_point, bool), (len(e),)), IMPULSE_WORLD_POINT, 0).astype(np.uint32)
    records["flags"] = flags
    return records


def make_characters(positions, radius=0.5, skin=0.01, step_height=0.35, min_ground_ny=0.7071068, probe_distance=0.1, gravity=9.81, jump_speed=5.0,
                    fall_speed=29.43, layer_mask=0xFFFFFFFF):
    """bge_character_desc records: positions (n, 3); every other argument a scalar or one value per character."""
    p = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
    descs = np.zeros(len(p), CHARACTER_DESC_DTYPE)
    descs["position"] = p
    for k, v in (("radius", radius), ("skin", skin), ("step_height", step_height), ("min_ground_ny", min_ground_ny),
                 ("probe_distance", probe_distance), ("gravity", gravity), ("jump_speed", jump_speed), ("fall_speed", fall_speed)):
        descs[k] = np.broadcast_to(np.asarray(v, np.float32), (len(p),))
    descs["layer_mask"] = np.broadcast_to(np.asarray(layer_mask, np.uint64).astype(np.uint32), (len(p),))
    return descs


def make_character_inputs(walk_x, walk_z, jump=False):
    """bge_character_input records: the level displacement of one step per character, and whether the JUMP edge is set."""
    x = np.atleast_1d(np.asarray(walk_x, np.float32))
    inputs = np.zeros(len(x), CHARACTER_INPUT_DTYPE)
    inputs["walk_x"] = x
    inputs["walk_z"] = np.broadcast_to(np.asarray(walk_z, np.float32), (len(x),))
    inputs["buttons"] = np.where(np.broadcast_to(np.asarray(jump, bool), (len(x),)), CHAR_BUTTON_JUMP, 0)
    return inputs


# debug overlay (bge_world_debug_lines*): bge_debug_flags and the 28-byte line record
DEBUG_SHAPES, DEBUG_CONTACTS, DEBUG_ALL = 1, 2, 3
DEBUG_LINE_DTYPE = np.dtype([("from", "<f4", (3,)), ("to", "<f4", (3,)), ("abgr", "<u4")])
assert DEBUG_LINE_DTYPE.itemsize == 28


def _debug_desc(flags, region):
    """bge_debug_desc: region = None (the whole world) or (min xyz, max xyz)."""
    d = DebugDesc(C.sizeof(DebugDesc), int(flags), 0 if region is None else 1)
    if region is not None:
        mn, mx = (np.asarray(r, np.float32).reshape(3) for r in region)
        d.region_min = (C.c_float * 3)(*mn.tolist())
        d.region_max = (C.c_float * 3)(*mx.tolist())
    return d


# frustum culling (bge_world_visible*): bge_cull_desc from an (n, 4) array of inward-pointing planes (a, b, c, d), n <= 16
CULL_MAX_PLANES = 16
# draw batches (bge_world_draw_batches*): the key of an entity that has none, and the largest n_keys
NO_DRAW_KEY = 0xFFFFFFFF
DRAW_MAX_KEYS = 65536


def _cull_desc(planes):
    pl = np.zeros((0, 4), np.float32) if planes is None else np.ascontiguousarray(planes, np.float32).reshape(-1, 4)
    d = CullDesc(C.sizeof(CullDesc), len(pl))
    n = min(len(pl), CULL_MAX_PLANES)  # (a longer list keeps its count: the library refuses it)
    C.memmove(d.planes, pl.ctypes.data, 16 * n)
    return d


def frustum_planes(viewproj, homogeneous_depth=False):
    """Host-only: the six planes (6, 4) of a view-projection matrix in the bx row-vector convention, in the order w+x, w-x, w+y,
    w-y, near (z, or w+z with homogeneous_depth), w-z (bge_frustum_planes)."""
    m = np.ascontiguousarray(viewproj, np.float32).reshape(16)
    out = np.empty((6, 4), np.float32)
    check(lib().bge_frustum_planes(_p(m), int(bool(homogeneous_depth)), _p(out)))
    return out


# fixed step and gravity of the reference (assets/config/physics.json:2-3)
FIXED_DT = float(np.float32(0.0083333333))
GRAVITY = (0.0, -9.81, 0.0)


def _arr(a, dtype, shape_tail=None):
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=dtype)
    if shape_tail is not None and a.ndim == 2 and a.shape[1] != shape_tail:
        raise ValueError(f"expected (*, {shape_tail}) array, got {a.shape}")
    return a


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class World:
    """A device-resident mirror of one reference ``Scene`` (see include/bge_world.h)."""

    def __init__(self, device: int = -1, stream: int | None = None, pair_capacity: int = 0):
        self._h = C.c_void_p()
        desc = WorldDesc(C.sizeof(WorldDesc), device, C.c_void_p(stream) if stream else None, pair_capacity)
        check(lib().bge_world_create(C.byref(desc), C.byref(self._h)))
        self.n = 0

    def close(self):
        if self._h:
            lib().bge_world_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- topology and components
    def set_topology(self, parent, has_transform=None):
        parent = _arr(parent, np.uint32)
        ht = _arr(has_transform, np.uint8)
        self.n = len(parent)
        check(lib().bge_world_set_topology(self._h, self.n, _p(parent), _p(ht)))
        return self

    def upload_trs(self, pos=None, euler=None, scale=None, first=0):
        pos, euler, scale = (_arr(a, np.float32, 3) for a in (pos, euler, scale))
        count = next(len(a) for a in (pos, euler, scale) if a is not None)
        check(lib().bge_world_upload_trs(self._h, first, count, _p(pos), _p(euler), _p(scale)))

    def upload_trs_indexed(self, entity_index, pos=None, euler=None, scale=None):
        """Sparse form of upload_trs: row i belongs to entity entity_index[i] (bge_world_upload_trs_indexed)."""
        idx = _arr(entity_index, np.uint32)
        pos, euler, scale = (_arr(a, np.float32, 3) for a in (pos, euler, scale))
        check(lib().bge_world_upload_trs_indexed(self._h, len(idx), _p(idx), _p(pos), _p(euler), _p(scale)))

    def mark_dirty(self, first=0, count=None):
        check(lib().bge_world_mark_dirty(self._h, first, self.n - first if count is None else count))

    def upload_bodies(self, body_type, mass=None, shape=None, size=None, layer=None, mask=None, first=0):
        t = _arr(body_type, np.uint8)
        check(lib().bge_world_upload_bodies(self._h, first, len(t), _p(t), _p(_arr(mass, np.float32)),
                                            _p(_arr(shape, np.uint8)), _p(_arr(size, np.float32, 3)),
                                            _p(_arr(layer, np.uint32)), _p(_arr(mask, np.uint32))))

    def set_velocities(self, linvel=None, angvel=None, first=0):
        l, a = _arr(linvel, np.float32, 3), _arr(angvel, np.float32, 3)
        count = len(l) if l is not None else len(a)
        check(lib().bge_world_set_velocities(self._h, first, count, _p(l), _p(a)))

    # -- tick
    def tick(self, dt=FIXED_DT, gravity=GRAVITY, flags=TICK_ALL, ticks=1):
        g = (C.c_float * 3)(*gravity)
        check(lib().bge_world_tick_many(self._h, ticks, dt, g, flags))

    def step_simulation(self, dt, max_sub_steps=4, fixed_step=FIXED_DT, gravity=GRAVITY, flags=TICK_PHYSICS) -> int:
        """Bullet's stepSimulation(dt, max_sub_steps, fixed_step) around the world's ticks; returns the sub-steps due."""
        g = (C.c_float * 3)(*gravity)
        n = C.c_int(0)
        check(lib().bge_world_step_simulation(self._h, float(dt), int(max_sub_steps), float(fixed_step), g, flags, C.byref(n)))
        return int(n.value)

    def set_ground_plane(self, enabled=True):
        """The reference's static plane y = 0 with Bullet's contact handling (include/bge_world.h)."""
        check(lib().bge_world_set_ground_plane(self._h, int(enabled)))

    def upload_friction(self, friction, first=0):
        fr = _arr(friction, np.float32)
        check(lib().bge_world_upload_friction(self._h, first, len(fr), _p(fr)))

    def set_static_contacts(self, enabled=True):
        """Dynamic boxes collide with the Static / Kinematic box colliders of the scene (bge_world.h)."""
        check(lib().bge_world_set_static_contacts(self._h, int(enabled)))

    def upload_restitution(self, restitution, first=0):
        r = _arr(restitution, np.float32)
        check(lib().bge_world_upload_restitution(self._h, first, len(r), _p(r)))

    def set_dynamic_contacts(self, enabled=True):
        """Dynamic boxes collide with each other: a persistent manifold per pair, simulation islands of several bodies
        (bge_world_set_dynamic_contacts)."""
        check(lib().bge_world_set_dynamic_contacts(self._h, int(enabled)))

    def download_dynamic_pairs(self):
        """(hdr, points): hdr[k] = lower entity index, higher entity index, points of the k-th pair of Dynamic boxes in the pair
        cache (ascending); points[k, j] = localA.xyz, localB.xyz, normalWorldOnB.xyz, distance, appliedImpulse, appliedImpulseLateral1."""
        total = C.c_uint64(0)
        check(lib().bge_world_download_dynamic_pairs(self._h, 0, None, None, C.byref(total)))
        n = int(total.value)
        hdr = np.zeros((max(n, 1), 3), np.uint32)
        pts = np.zeros((max(n, 1), 4, 12), np.float32)
        if n:
            check(lib().bge_world_download_dynamic_pairs(self._h, n, _p(hdr), _p(pts), C.byref(total)))
        return hdr[:n], pts[:n]

    def download_box_contacts(self, first=0, count=None):
        """(n_manifolds[count], header[count, 4, 2] = (other entity, points), points[count, 4, 4, 12]) — ascending other entity."""
        count = self.n - first if count is None else count
        n = np.zeros(count, np.uint8)
        hdr = np.zeros((count, 4, 2), np.uint32)
        pts = np.zeros((count, 4, 4, 12), np.float32)
        check(lib().bge_world_download_box_contacts(self._h, first, count, _p(n), _p(hdr), _p(pts)))
        return n, hdr, pts

    def download_contacts(self, first=0, count=None):
        """(n, points): n[i] contact points of body i with the ground; points[i, k] = localA.xyz, appliedImpulse, localB.x, distance, localB.z, lateral."""
        count = self.n - first if count is None else count
        n = np.zeros(count, np.uint8)
        pts = np.zeros((count, 4, 8), np.float32)
        check(lib().bge_world_download_contacts(self._h, first, count, _p(n), _p(pts)))
        return n, pts

    def reset_clock(self):
        check(lib().bge_world_reset_clock(self._h))

    def sync(self):
        check(lib().bge_world_sync(self._h))

    def profile_enable(self, mode=1):
        """0 off, 1 one event pair per tick() call, 2 one pair per tick (see include/bge_world.h)."""
        check(lib().bge_world_profile_enable(self._h, int(mode)))

    def profile_read(self):
        """(summed tick-kernel milliseconds, ticks) since the last read; synchronises the stream."""
        ms, n = C.c_double(0), C.c_uint64(0)
        check(lib().bge_world_profile_read(self._h, C.byref(ms), C.byref(n)))
        return float(ms.value), int(n.value)

    # -- results
    def download_world(self, first=0, count=None, out=None):
        count = self.n - first if count is None else count
        out = np.empty((count, 16), np.float32) if out is None else out
        check(lib().bge_world_download_world(self._h, first, count, _p(out)))
        return out

    def download_normal(self, first=0, count=None):
        count = self.n - first if count is None else count
        out = np.empty((count, 16), np.float32)
        check(lib().bge_world_download_normal(self._h, first, count, _p(out)))
        return out

    def download_pose(self, first=0, count=None):
        count = self.n - first if count is None else count
        pos, euler = np.empty((count, 3), np.float32), np.empty((count, 3), np.float32)
        check(lib().bge_world_download_pose(self._h, first, count, _p(pos), _p(euler)))
        return pos, euler

    def download_bodies(self, first=0, count=None):
        count = self.n - first if count is None else count
        v, w, q, bb = (np.empty((count, k), np.float32) for k in (3, 3, 4, 6))
        check(lib().bge_world_download_bodies(self._h, first, count, _p(v), _p(w), _p(q), _p(bb)))
        return dict(linvel=v, angvel=w, quat=q, aabb=bb)

    def download_dirty(self, first=0, count=None):
        count = self.n - first if count is None else count
        d = np.empty(count, np.uint8)
        check(lib().bge_world_download_dirty(self._h, first, count, _p(d)))
        return d.astype(bool)

    def download_activation(self, first=0, count=None):
        """(state, time): bge_activation per entity (0 none, 1 ACTIVE_TAG, 2 ISLAND_SLEEPING, 3 WANTS_DEACTIVATION,
        4 DISABLE_DEACTIVATION) and Bullet's m_deactivationTime."""
        count = self.n - first if count is None else count
        st, tm = np.empty(count, np.uint8), np.empty(count, np.float32)
        check(lib().bge_world_download_activation(self._h, first, count, _p(st), _p(tm)))
        return st, tm

    def set_sleeping(self, linear=0.8, angular=1.0, seconds=2.0):
        check(lib().bge_world_set_sleeping(self._h, linear, angular, seconds))

    # -- sharded broadphase (global pair set across worlds / ranks)
    def set_global_ids(self, ids, first=0):
        ids = _arr(ids, np.uint32)
        check(lib().bge_world_set_global_ids(self._h, first, len(ids), _p(ids)))

    def aabb_bounds(self):
        mn, mx = np.empty(3, np.float32), np.empty(3, np.float32)
        n = C.c_uint64(0)
        check(lib().bge_world_aabb_bounds(self._h, _p(mn), _p(mx), C.byref(n)))
        return mn, mx, int(n.value)

    def axis_histogram(self, axis, lo, hi, bins=4096):
        hist = np.zeros(bins, np.uint64)
        check(lib().bge_world_axis_histogram(self._h, axis, lo, hi, bins, _p(hist)))
        return hist

    def bp_route(self, axis, cuts):
        """cuts: nranks + 1 slab boundaries (the outer two are ignored).  Returns records per destination slab."""
        cuts = _arr(cuts, np.float32)
        counts = np.zeros(len(cuts) - 1, np.uint64)
        check(lib().bge_world_bp_route(self._h, axis, len(cuts) - 1, _p(cuts), _p(counts)))
        return counts

    def bp_pack(self, send_device_ptr):
        check(lib().bge_world_bp_pack(self._h, C.c_void_p(send_device_ptr)))

    def bp_find(self, records_device_ptr, n_records, axis, window_lo, window_hi):
        check(lib().bge_world_bp_find(self._h, C.c_void_p(records_device_ptr), n_records, axis, window_lo, window_hi))

    def bp_exchange(self, axis=2):
        check(lib().bge_world_bp_exchange(self._h, axis))

    def dirty_count(self) -> int:
        v = C.c_uint64(0)
        check(lib().bge_world_dirty_count(self._h, C.byref(v)))
        return int(v.value)

    def pairs(self, cap=None):
        """Sorted (a, b) entity-index pairs of the last BROADPHASE tick."""
        total = C.c_uint64(0)
        cap = int(cap or max(1024, 8 * self.n))
        buf = np.empty((cap, 2), np.uint32)
        check(lib().bge_world_pairs(self._h, _p(buf), cap, C.byref(total)))
        if total.value > cap:
            raise _capi.BgeError(-1, f"{total.value} pairs found but the host buffer holds {cap}")
        out = buf[: total.value]
        order = np.lexsort((out[:, 1], out[:, 0]))
        return out[order].copy()

    def pair_count(self) -> int:
        total = C.c_uint64(0)
        check(lib().bge_world_pairs(self._h, None, 0, C.byref(total)))
        return int(total.value)

    # -- trigger volumes
    def upload_triggers(self, entity_index, shape=None, size=None, layer=None, mask=None, one_shot=None, active=None, keep_order=False):
        """The world processes its triggers in the order of the uploaded array (bge_world.h); unless keep_order is set the set is
        sent in ascending entity order — the order the oracle's ProcessTriggerEvents walks (oracle/physics_ref.h)."""
        e = _arr(entity_index, np.uint32)
        if not keep_order and len(e) > 1:
            order = np.argsort(e, kind="stable")
            pick = lambda a: None if a is None else np.asarray(a)[order]
            e, shape, size, layer, mask, one_shot, active = e[order], pick(shape), pick(size), pick(layer), pick(mask), pick(one_shot), pick(active)
        check(lib().bge_world_upload_triggers(self._h, len(e), _p(e), _p(_arr(shape, np.uint8)), _p(_arr(size, np.float32, 3)),
                                              _p(_arr(layer, np.uint32)), _p(_arr(mask, np.uint32)),
                                              _p(_arr(one_shot, np.uint8)), _p(_arr(active, np.uint8))))

    def trigger_events(self):
        """(type, trigger entity, other entity) rows since the last call, sorted; type 0 Enter, 1 Stay, 2 Exit."""
        total = C.c_uint64(0)
        check(lib().bge_world_trigger_events(self._h, None, 0, C.byref(total)))
        out = np.empty((int(total.value), 3), np.uint32)
        check(lib().bge_world_trigger_events(self._h, _p(out), len(out), C.byref(total)))
        return out[np.lexsort((out[:, 2], out[:, 1], out[:, 0]))].copy() if len(out) else out

    def trigger_active(self, entity_index):
        e = _arr(entity_index, np.uint32)
        out = np.empty(len(e), np.uint8)
        check(lib().bge_world_trigger_active(self._h, len(e), _p(e), _p(out)))
        return out.astype(bool)

    def set_trigger_stay_events(self, enabled=True):
        """Stay records in trigger_events() (the reference's behaviour, the default) or Enter / Exit only (bge_world.h)."""
        check(lib().bge_world_set_trigger_stay_events(self._h, int(bool(enabled))))

    def trigger_diff_stats(self):
        """(ticks whose Enter / Exit difference was taken on the device, ticks that took it on the host, Stay events left out)."""
        a, b, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        check(lib().bge_world_trigger_diff_stats(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def trigger_query_stats(self):
        """(ghosts that walked the broadphase grid, ghosts tested against every body) in the last tick."""
        a, b = C.c_uint32(0), C.c_uint32(0)
        check(lib().bge_world_trigger_query_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    # -- multi-GPU support / device-resident consumers
    # -- ray queries (PhysicsSystem::Raycast / RaycastAll for a batch; include/bge_world.h states what a ray sees)
    def raycast(self, origins, directions, max_distance=200.0, layer_mask=0xFFFFFFFF):
        """Closest hit per ray: dict of numpy arrays kind, entity, fraction, distance, point (n, 3), normal (n, 3).
        max_distance and layer_mask take a scalar or one value per ray."""
        rays = make_rays(origins, directions, max_distance, layer_mask)
        hits = np.zeros(len(rays), RAY_HIT_DTYPE)
        check(lib().bge_world_raycast(self._h, len(rays), _p(rays), _p(hits)))
        return _hit_fields(hits)

    def raycast_all(self, origins, directions, max_distance=200.0, layer_mask=0xFFFFFFFF):
        """Every hit per ray: the arrays of raycast() over all hits plus offsets (n + 1): ray i's hits are
        [offsets[i], offsets[i + 1]), in (fraction, object code) order."""
        rays = make_rays(origins, directions, max_distance, layer_mask)
        total = C.c_uint64(0)
        offsets = np.zeros(len(rays) + 1, np.uint64)
        check(lib().bge_world_raycast_all(self._h, len(rays), _p(rays), None, 0, _p(offsets), C.byref(total)))
        hits = np.zeros(max(int(total.value), 1), RAY_HIT_DTYPE)
        check(lib().bge_world_raycast_all(self._h, len(rays), _p(rays), _p(hits), len(hits), _p(offsets), C.byref(total)))
        out = _hit_fields(hits[:int(total.value)])
        out["offsets"] = offsets
        return out

    def raycast_device(self, rays, hits):
        """Closest hit per ray between device tensors: rays holds n bge_ray records (32 bytes each, e.g. a uint8 / float32 /
        int32 tensor made from make_rays()), hits room for n bge_ray_hit records (40 bytes each).  Enqueued on the world's
        stream without synchronisation: call sync() (or order the stream yourself) before reading hits."""
        nb = rays.numel() * rays.element_size()
        if nb % 32:
            raise ValueError(f"rays holds {nb} bytes, not a whole number of 32-byte records")
        n = nb // 32
        if hits.numel() * hits.element_size() < 40 * n:
            raise ValueError(f"hits has room for {hits.numel() * hits.element_size()} bytes, {40 * n} needed")
        if not (rays.is_cuda and hits.is_cuda and rays.is_contiguous() and hits.is_contiguous()):
            raise ValueError("rays and hits must be contiguous device tensors")
        check(lib().bge_world_raycast_device(self._h, n, C.c_void_p(rays.data_ptr()), C.c_void_p(hits.data_ptr())))

    # -- sphere queries (not in the reference; include/bge_world.h states what a sphere touches and where)
    def sphere_cast(self, origins, directions, max_distance=200.0, radius=0.5, layer_mask=0xFFFFFFFF):
        """Closest touch per sphere cast: the dict raycast() returns; point is the contact point on the shape, normal points
        from it to the sphere's centre.  max_distance, radius and layer_mask take a scalar or one value per cast."""
        casts = make_sphere_casts(origins, directions, max_distance, radius, layer_mask)
        hits = np.zeros(len(casts), RAY_HIT_DTYPE)
        check(lib().bge_world_sphere_cast(self._h, len(casts), _p(casts), _p(hits)))
        return _hit_fields(hits)

    def sphere_cast_all(self, origins, directions, max_distance=200.0, radius=0.5, layer_mask=0xFFFFFFFF):
        """Every touch per cast: the arrays of sphere_cast() over all hits plus offsets (n + 1), as raycast_all()."""
        casts = make_sphere_casts(origins, directions, max_distance, radius, layer_mask)
        total = C.c_uint64(0)
        offsets = np.zeros(len(casts) + 1, np.uint64)
        check(lib().bge_world_sphere_cast_all(self._h, len(casts), _p(casts), None, 0, _p(offsets), C.byref(total)))
        hits = np.zeros(max(int(total.value), 1), RAY_HIT_DTYPE)
        check(lib().bge_world_sphere_cast_all(self._h, len(casts), _p(casts), _p(hits), len(hits), _p(offsets), C.byref(total)))
        out = _hit_fields(hits[:int(total.value)])
        out["offsets"] = offsets
        return out

    def sphere_cast_device(self, casts, hits):
        """Closest touch per cast between device tensors: casts holds n bge_sphere_cast records (40 bytes each, e.g. a uint8
        tensor made from make_sphere_casts()), hits room for n bge_ray_hit records (40 bytes each).  Enqueued on the world's
        stream without synchronisation, as raycast_device()."""
        nb = casts.numel() * casts.element_size()
        if nb % 40:
            raise ValueError(f"casts holds {nb} bytes, not a whole number of 40-byte records")
        n = nb // 40
        if hits.numel() * hits.element_size() < 40 * n:
            raise ValueError(f"hits has room for {hits.numel() * hits.element_size()} bytes, {40 * n} needed")
        if not (casts.is_cuda and hits.is_cuda and casts.is_contiguous() and hits.is_contiguous()):
            raise ValueError("casts and hits must be contiguous device tensors")
        check(lib().bge_world_sphere_cast_device(self._h, n, C.c_void_p(casts.data_ptr()), C.c_void_p(hits.data_ptr())))

    def overlap_sphere(self, centers, radius, layer_mask=0xFFFFFFFF):
        """Every object within radius of each centre: dict of kind, entity, distance (0 inside the shape) over all hits plus
        offsets (n + 1); sphere i's objects are [offsets[i], offsets[i + 1]), bodies by entity, then ghosts, then the plane."""
        spheres = make_spheres(centers, radius, layer_mask)
        total = C.c_uint64(0)
        offsets = np.zeros(len(spheres) + 1, np.uint64)
        check(lib().bge_world_overlap_sphere(self._h, len(spheres), _p(spheres), None, 0, _p(offsets), C.byref(total)))
        hits = np.zeros(max(int(total.value), 1), OVERLAP_HIT_DTYPE)
        check(lib().bge_world_overlap_sphere(self._h, len(spheres), _p(spheres), _p(hits), len(hits), _p(offsets), C.byref(total)))
        hits = hits[:int(total.value)]
        return {"kind": hits["kind"].copy(), "entity": hits["entity"].copy(), "distance": hits["distance"].copy(), "offsets": offsets}

    # -- sphere moves (not in the reference; include/bge_world.h states the rule: collide, slide, probe for ground)
    def sphere_move(self, positions, displacements, radius=0.5, skin=0.01, probe_distance=0.0, min_ground_ny=0.7071068,
                    layer_mask=0xFFFFFFFF):
        """One collide-and-slide move per sphere: a SPHERE_MOVE_RESULT_DTYPE array (position, remaining, flags, n_hits, the last
        hit of the slides, the ground probe's hit).  Every argument but the first two takes a scalar or one value per mover."""
        moves = make_sphere_moves(positions, displacements, radius, skin, probe_distance, min_ground_ny, layer_mask)
        results = np.zeros(len(moves), SPHERE_MOVE_RESULT_DTYPE)
        check(lib().bge_world_sphere_move(self._h, len(moves), _p(moves), _p(results)))
        return results

    def sphere_move_device(self, moves, results):
        """The same between device tensors: moves holds n bge_sphere_move records (48 bytes each, e.g. a uint8 tensor made from
        make_sphere_moves()), results room for n bge_sphere_move_result records (80 bytes each).  Enqueued on the world's stream
        without synchronisation, as raycast_device()."""
        nb = moves.numel() * moves.element_size()
        if nb % 48:
            raise ValueError(f"moves holds {nb} bytes, not a whole number of 48-byte records")
        n = nb // 48
        if results.numel() * results.element_size() < 80 * n:
            raise ValueError(f"results has room for {results.numel() * results.element_size()} bytes, {80 * n} needed")
        if not (moves.is_cuda and results.is_cuda and moves.is_contiguous() and results.is_contiguous()):
            raise ValueError("moves and results must be contiguous device tensors")
        check(lib().bge_world_sphere_move_device(self._h, n, C.c_void_p(moves.data_ptr()), C.c_void_p(results.data_ptr())))

    # -- sphere step moves (not in the reference; include/bge_world.h states the rule: the move, stepping up over low obstacles)
    def sphere_step_move(self, positions, displacements, radius=0.5, skin=0.01, probe_distance=0.0, min_ground_ny=0.7071068,
                         layer_mask=0xFFFFFFFF, step_height=0.0):
        """One step move per sphere: a SPHERE_STEP_RESULT_DTYPE array (the fields of sphere_move() and step_rise; MOVE_STEP_TRIED and
        MOVE_STEPPED in flags).  Every argument but the first two takes a scalar or one value per mover."""
        moves = make_sphere_step_moves(positions, displacements, radius, skin, probe_distance, min_ground_ny, layer_mask, step_height)
        results = np.zeros(len(moves), SPHERE_STEP_RESULT_DTYPE)
        check(lib().bge_world_sphere_step_move(self._h, len(moves), _p(moves), _p(results)))
        return results

    def sphere_step_move_device(self, moves, results):
        """The same between device tensors: moves holds n bge_sphere_step_move records (48 bytes each, e.g. a uint8 tensor made from
        make_sphere_step_moves()), results room for n bge_sphere_step_result records (80 bytes each).  Enqueued on the world's
        stream without synchronisation, as sphere_move_device()."""
        nb = moves.numel() * moves.element_size()
        if nb % 48:
            raise ValueError(f"moves holds {nb} bytes, not a whole number of 48-byte records")
        n = nb // 48
        if results.numel() * results.element_size() < 80 * n:
            raise ValueError(f"results has room for {results.numel() * results.element_size()} bytes, {80 * n} needed")
        if not (moves.is_cuda and results.is_cuda and moves.is_contiguous() and results.is_contiguous()):
            raise ValueError("moves and results must be contiguous device tensors")
        check(lib().bge_world_sphere_step_move_device(self._h, n, C.c_void_p(moves.data_ptr()), C.c_void_p(results.data_ptr())))

    # -- sphere penetration and recovery (not in the reference; include/bge_world.h states the signed distance and the rule)
    def sphere_penetration(self, centers, radius, layer_mask=0xFFFFFFFF):
        """The object that reaches deepest into each sphere: dict of numpy arrays kind, entity, depth, point (n, 3), normal (n, 3);
        kind RAY_MISS where nothing touches the sphere.  radius and layer_mask take a scalar or one value per sphere."""
        spheres = make_spheres(centers, radius, layer_mask)
        hits = np.zeros(len(spheres), PENETRATION_HIT_DTYPE)
        check(lib().bge_world_sphere_penetration(self._h, len(spheres), _p(spheres), _p(hits)))
        return {k: hits[k].copy() for k in ("kind", "entity", "depth", "point", "normal")}

    def sphere_penetration_device(self, spheres, hits):
        """The same between device tensors: spheres holds n bge_sphere records (20 bytes each, e.g. a uint8 tensor made from
        make_spheres()), hits room for n bge_penetration_hit records (40 bytes each).  Enqueued on the world's stream without
        synchronisation, as raycast_device()."""
        n = _device_records(spheres, hits, "spheres", "hits", 20, 40)
        check(lib().bge_world_sphere_penetration_device(self._h, n, C.c_void_p(spheres.data_ptr()), C.c_void_p(hits.data_ptr())))

    def sphere_recover(self, positions, radius=0.5, skin=0.01, layer_mask=0xFFFFFFFF):
        """Pushes each sphere out of what it touches or penetrates, in at most RECOVER_ROUNDS pushes: a
        SPHERE_RECOVER_RESULT_DTYPE array (position, pushed, flags, n_pushes, the last push's hit, remaining_depth).  Every
        argument but the first takes a scalar or one value per sphere.  Per frame: recover, then sphere_move()."""
        records = make_sphere_recovers(positions, radius, skin, layer_mask)
        results = np.zeros(len(records), SPHERE_RECOVER_RESULT_DTYPE)
        check(lib().bge_world_sphere_recover(self._h, len(records), _p(records), _p(results)))
        return results

    def sphere_recover_device(self, records, results):
        """The same between device tensors: records holds n bge_sphere_recover records (28 bytes each, e.g. a uint8 tensor made
        from make_sphere_recovers()), results room for n bge_sphere_recover_result records (64 bytes each).  Enqueued on the
        world's stream without synchronisation, as raycast_device()."""
        n = _device_records(records, results, "records", "results", 28, 64)
        check(lib().bge_world_sphere_recover_device(self._h, n, C.c_void_p(records.data_ptr()), C.c_void_p(results.data_ptr())))

    # -- characters (an extension; include/bge_world.h "Characters" states the rule: recover, gravity and jump, step move, ground snap)
    def characters_create(self, descs):
        """Replaces the world's character set: descs is a CHARACTER_DESC_DTYPE array (make_characters()); an empty one removes
        the set.  Characters start at their desc's position, not grounded, at rest."""
        descs = np.ascontiguousarray(descs, CHARACTER_DESC_DTYPE)
        check(lib().bge_world_characters_create(self._h, len(descs), _p(descs) if len(descs) else None))

    def characters_set_input(self, inputs, first=0):
        """inputs: a CHARACTER_INPUT_DTYPE array (make_character_inputs()) for characters first .., or a contiguous device tensor
        holding such records (16 bytes each), which is copied on the world's stream without synchronisation."""
        if hasattr(inputs, "data_ptr"):
            nb = inputs.numel() * inputs.element_size()
            if nb % 16:
                raise ValueError(f"inputs holds {nb} bytes, not a whole number of 16-byte records")
            if not (inputs.is_cuda and inputs.is_contiguous()):
                raise ValueError("inputs must be a contiguous device tensor")
            check(lib().bge_world_characters_set_input_device(self._h, first, nb // 16, C.c_void_p(inputs.data_ptr())))
            return
        inputs = np.ascontiguousarray(inputs, CHARACTER_INPUT_DTYPE)
        check(lib().bge_world_characters_set_input(self._h, first, len(inputs), _p(inputs)))

    def characters_warp(self, index, positions):
        """Puts the characters index[k] at positions[k], at rest and not grounded."""
        index = np.ascontiguousarray(np.atleast_1d(index), np.uint32)
        positions = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
        if len(index) != len(positions):
            raise ValueError(f"{len(index)} indices, {len(positions)} positions")
        check(lib().bge_world_characters_warp(self._h, len(index), _p(index), _p(positions)))

    def characters_update(self, dt, steps=1):
        """Enqueues `steps` steps of length dt for every character on the world's stream; nothing is read back."""
        check(lib().bge_world_characters_update(self._h, float(dt), int(steps)))

    def characters_state(self, first=0, count=None):
        """The states of characters first .. first + count (all of them by default) as a CHARACTER_STATE_DTYPE array.
        Synchronises the world's stream."""
        if count is None:
            count = self.characters_state_device()[1] - first
        states = np.zeros(max(count, 0), CHARACTER_STATE_DTYPE)
        check(lib().bge_world_characters_download(self._h, first, count, _p(states) if count > 0 else None))
        return states

    def characters_state_device(self):
        """(device pointer, n) of the resident bge_character_state[n]; (0, 0) without characters."""
        ptr, n = C.c_void_p(), C.c_uint64()
        check(lib().bge_world_characters_state_device(self._h, C.byref(ptr), C.byref(n)))
        return int(ptr.value or 0), int(n.value)

    # -- character platform riding (include/bge_world.h "Character platform riding" states the rule)
    def characters_ride(self, on=True, dynamic=False):
        """Switches riding on (characters move with the Static or Kinematic body they stand on; with dynamic=True with a Dynamic
        one too) or off.  Switching on while it is on changes only the flags and keeps the anchors."""
        if dynamic and not on:
            raise ValueError("dynamic=True needs on=True")
        check(lib().bge_world_characters_ride(self._h, (CHAR_RIDE_ON if on else 0) | (CHAR_RIDE_DYNAMIC if dynamic else 0)))

    def characters_rides(self, first=0, count=None):
        """The ride records of characters first .. first + count (all of them by default) as a CHARACTER_RIDE_DTYPE array.
        Synchronises the world's stream."""
        if count is None:
            count = self.characters_state_device()[1] - first
        rides = np.zeros(max(count, 0), CHARACTER_RIDE_DTYPE)
        check(lib().bge_world_characters_rides(self._h, first, count, _p(rides) if count > 0 else None))
        return rides

    def characters_rides_device(self):
        """(device pointer, n) of the resident bge_character_ride[n]; (0, 0) while riding is off."""
        ptr, n = C.c_void_p(), C.c_uint64()
        check(lib().bge_world_characters_rides_device(self._h, C.byref(ptr), C.byref(n)))
        return int(ptr.value or 0), int(n.value)

    # -- crowd separation (include/bge_world.h "Crowd separation" states the rule)
    def crowd_query(self, spheres, max_push=0.0):
        """Every sphere of the batch against every other: spheres is a CROWD_SPHERE_DTYPE array (make_crowd_spheres()); a
        CROWD_HIT_DTYPE array comes back (flags, the deepest overlapping sphere, the number of overlaps, its depth, the level push
        away from it).  max_push > 0 limits the push.  Uses nothing of the world but its stream."""
        spheres = np.ascontiguousarray(spheres, CROWD_SPHERE_DTYPE)
        hits = np.zeros(len(spheres), CROWD_HIT_DTYPE)
        check(lib().bge_world_crowd_query(self._h, len(spheres), _p(spheres) if len(spheres) else None, float(max_push),
                                          _p(hits) if len(spheres) else None))
        return hits

    def crowd_query_device(self, spheres, hits, max_push=0.0):
        """The same between device tensors: spheres holds n bge_crowd_sphere records (24 bytes each, e.g. a uint8 tensor made from
        make_crowd_spheres()), hits room for n bge_crowd_hit records (32 bytes each).  Enqueued on the world's stream without
        synchronisation, as raycast_device()."""
        n = _device_records(spheres, hits, "spheres", "hits", 24, 32)
        check(lib().bge_world_crowd_query_device(self._h, n, C.c_void_p(spheres.data_ptr()), float(max_push), C.c_void_p(hits.data_ptr())))

    def characters_crowd(self, on=True, max_push=0.0, group=None, mask=None):
        """Switches crowd separation on (every step of characters_update() begins by pushing overlapping characters apart) or off.
        group, mask: one value per character or a scalar (default 1 and 0xffffffff).  Calling it again replaces them and max_push."""
        if not on:
            check(lib().bge_world_characters_crowd(self._h, 0, 0.0, 0, None, None))
            return
        n = self.characters_state_device()[1]
        pick = lambda a: None if a is None else np.ascontiguousarray(np.broadcast_to(np.asarray(a, np.uint64).astype(np.uint32), (n,)))
        g, m = pick(group), pick(mask)
        check(lib().bge_world_characters_crowd(self._h, CHAR_CROWD_ON, float(max_push), n, None if g is None else _p(g),
                                               None if m is None else _p(m)))

    def characters_crowd_hits(self, first=0, count=None):
        """The crowd records of characters first .. first + count (all of them by default) as the last update call's last step
        left them: a CROWD_HIT_DTYPE array.  Synchronises the world's stream."""
        if count is None:
            count = self.characters_state_device()[1] - first
        hits = np.zeros(max(count, 0), CROWD_HIT_DTYPE)
        check(lib().bge_world_characters_crowd_hits(self._h, first, count, _p(hits) if count > 0 else None))
        return hits

    def characters_crowd_hits_device(self):
        """(device pointer, n) of the resident bge_crowd_hit[n]; (0, 0) while the crowd is off."""
        ptr, n = C.c_void_p(), C.c_uint64()
        check(lib().bge_world_characters_crowd_hits_device(self._h, C.byref(ptr), C.byref(n)))
        return int(ptr.value or 0), int(n.value)

    # -- impulses and the characters' push (include/bge_world.h "Impulses" and "Character push" state the rule)
    def apply_impulses(self, entity, impulse=None, point=None, kind=None, world_point=False, want_status=False):
        """Applies impulses to Dynamic bodies as Bullet's applyImpulse / applyCentralImpulse / applyTorqueImpulse + activate() would,
        record after record: entity (n,), impulse (n, 3), point (n, 3) or None; kind = IMPULSE_AT_POINT / CENTRAL / TORQUE (None:
        AT_POINT with a point, CENTRAL without).  entity may also be a ready IMPULSE_DTYPE array (make_impulses()), the other
        arguments are then ignored.  want_status: the status word per record comes back (IMPULSE_APPLIED, ...)."""
        if isinstance(entity, np.ndarray) and entity.dtype == IMPULSE_DTYPE:
            records = np.ascontiguousarray(entity)
        else:
            records = make_impulses(entity, impulse, point, kind, world_point)
        status = np.zeros(len(records), np.uint32) if want_status else None
        check(lib().bge_world_apply_impulses(self._h, len(records), _p(records) if len(records) else None,
                                             _p(status) if want_status and len(records) else None))
        return status

    def apply_impulses_device(self, records, status=None):
        """The same between device tensors: records holds n bge_impulse records (32 bytes each, e.g. a uint8 tensor made from
        make_impulses()), status (optional) room for n 32-bit words.  Enqueued on the world's stream without synchronisation, as
        raycast_device()."""
        n = _device_records(records, records if status is None else status, "records", "status", 32, 0 if status is None else 4)
        check(lib().bge_world_apply_impulses_device(self._h, n, C.c_void_p(records.data_ptr()),
                                                    None if status is None else C.c_void_p(status.data_ptr())))

    def characters_push(self, on=True, force=0.0, max_normal_y=0.5, body_mask=0xFFFFFFFF):
        """Switches the characters' push on (every step of characters_update() ends by pushing the Dynamic body the character
        walked into with `force` newtons over the step, level, away from the character) or off.  Hits steeper than max_normal_y
        (|hit_normal.y|) and bodies whose group misses body_mask are not pushed.  Calling it again replaces the settings."""
        d = np.zeros(1, CHARACTER_PUSH_DESC_DTYPE)
        if on:
            d[0] = (CHAR_PUSH_ON, force, max_normal_y, body_mask)
        check(lib().bge_world_characters_push(self._h, _p(d)))

    def characters_push_records(self, first=0, count=None):
        """The push records of characters first .. first + count (all of them by default) as the last update call's last step
        left them: an IMPULSE_DTYPE array.  Synchronises the world's stream."""
        if count is None:
            count = self.characters_state_device()[1] - first
        records = np.zeros(max(count, 0), IMPULSE_DTYPE)
        check(lib().bge_world_characters_push_records(self._h, first, count, _p(records) if count > 0 else None))
        return records

    def characters_push_records_device(self):
        """(device pointer, n) of the resident bge_impulse[n]; (0, 0) while push is off."""
        ptr, n = C.c_void_p(), C.c_uint64()
        check(lib().bge_world_characters_push_records_device(self._h, C.byref(ptr), C.byref(n)))
        return int(ptr.value or 0), int(n.value)

    # -- the query index (include/bge_world.h "Query index" states the rule)
    def set_query_index(self, on=True, cell_edge=0.0, max_cells=0, min_work=None):
        """Switches the query index on or off: with it, the body pass of every query (and of the moves, recoveries and character
        steps made of them) visits only the bodies near the query instead of all of them.  Every answer keeps its bytes.
        cell_edge = 0 and max_cells = 0: chosen by the library; min_work: calls with n_queries * n_slots below it take the
        all-bodies pass (None: the library's default, 0: every call goes through the index)."""
        d = np.zeros(1, QUERY_INDEX_DESC_DTYPE)
        d["mode"] = 1 if on else 0
        d["cell_edge"] = cell_edge
        d["max_cells"] = max_cells
        d["min_work"] = QUERY_INDEX_MIN_WORK_DEFAULT if min_work is None else int(min_work)
        check(lib().bge_world_set_query_index(self._h, _p(d)))

    def query_index_stats(self):
        """What the last call that queried did with the index: a dict of the fields of bge_query_index_stats (built, table_size,
        bodies_indexed, bodies_wide, queries_indexed, queries_far, cell_edge, builds).  Synchronises the world's stream."""
        s = np.zeros(1, QUERY_INDEX_STATS_DTYPE)
        check(lib().bge_world_query_index_stats(self._h, _p(s)))
        return {k: (float(s[k][0]) if k == "cell_edge" else int(s[k][0])) for k in s.dtype.names if not k.startswith("reserved")}

    # -- character trigger events (include/bge_world.h "Character trigger events" states the rule and the order of the list)
    def characters_watch_triggers(self, group=None, mask=None, stay=True, event_capacity=0):
        """Turns on Enter / Stay / Exit of the characters against the trigger volumes, made by every characters_update() call.
        group, mask: one value per character or a scalar (default 2 and 0xffffffff).  With no characters the watch is off."""
        n = self.characters_state_device()[1]
        pick = lambda a: None if a is None else np.ascontiguousarray(np.broadcast_to(np.asarray(a, np.uint64).astype(np.uint32), (n,)))
        g, m = pick(group), pick(mask)
        check(lib().bge_world_characters_watch_triggers(self._h, n, _p(g), _p(m), CHAR_TRIGGER_STAY_EVENTS if stay else 0, int(event_capacity)))

    def characters_unwatch_triggers(self):
        """Turns the watch off (bge_world_characters_watch_triggers with n = 0): the remembered pairs and the list are forgotten."""
        check(lib().bge_world_characters_watch_triggers(self._h, 0, None, None, 0, 0))

    def characters_trigger_events(self):
        """(type, trigger entity, character index) rows of the last characters_update() call in the list's own order (the order
        is part of the rule, so nothing is sorted); type 0 Enter, 1 Stay, 2 Exit.  Synchronises the world's stream."""
        total = C.c_uint64(0)
        check(lib().bge_world_characters_trigger_events(self._h, None, 0, C.byref(total)))
        out = np.empty((int(total.value), 3), np.uint32)
        check(lib().bge_world_characters_trigger_events(self._h, _p(out), len(out), C.byref(total)))
        return out

    def characters_trigger_events_device(self):
        """(device pointer of the records, device pointer of the 4-byte count, capacity in records); (0, 0, 0) with the watch
        off.  count may exceed capacity; reads must be ordered after the world's stream."""
        ev, cnt, cap = C.c_void_p(), C.c_void_p(), C.c_uint64()
        check(lib().bge_world_characters_trigger_events_device(self._h, C.byref(ev), C.byref(cnt), C.byref(cap)))
        return int(ev.value or 0), int(cnt.value or 0), int(cap.value)

    def characters_trigger_overlaps(self):
        """The remembered (trigger entity, character index) pairs as a (k, 2) uint32 array, by trigger array order, then character."""
        total = C.c_uint64(0)
        check(lib().bge_world_characters_trigger_overlaps(self._h, 0, None, C.byref(total)))
        out = np.empty((int(total.value), 2), np.uint32)
        check(lib().bge_world_characters_trigger_overlaps(self._h, len(out), _p(out), C.byref(total)))
        return out

    def characters_set_trigger_overlaps(self, pairs):
        """Replaces the remembered set by (trigger entity, character index) pairs."""
        pairs = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
        check(lib().bge_world_characters_set_trigger_overlaps(self._h, len(pairs), _p(pairs) if len(pairs) else None))

    def trigger_boxes(self, entity_index):
        """(boxes (k, 6) float32: min xyz, max xyz; listed (k,) bool) of the triggers on these entities as the queries' ghost list
        has them; an entity that is not a listed trigger gets the empty box (+inf, -inf)."""
        e = np.ascontiguousarray(np.atleast_1d(entity_index), np.uint32)
        boxes = np.empty((len(e), 6), np.float32)
        listed = np.empty(len(e), np.uint8)
        check(lib().bge_world_trigger_boxes(self._h, len(e), _p(e), _p(boxes), _p(listed)))
        return boxes, listed.astype(bool)

    # -- debug overlay (PhysicsSystem::GetDebugLines; include/bge_world.h states what is drawn and in which order)
    def debug_lines(self, flags=DEBUG_ALL, region=None):
        """The overlay's lines as a structured array (from, to: 3 x f4; abgr: u4): the shapes section in its fixed order, then
        the contact lines.  region = (min xyz, max xyz) keeps the bodies / ghosts / contact points inside that closed box."""
        desc = _debug_desc(flags, region)
        total = C.c_uint64(0)
        check(lib().bge_world_debug_lines(self._h, C.byref(desc), None, 0, C.byref(total)))
        lines = np.zeros(int(total.value), DEBUG_LINE_DTYPE)
        if len(lines):
            check(lib().bge_world_debug_lines(self._h, C.byref(desc), _p(lines), len(lines), C.byref(total)))
        return lines[:int(total.value)]

    def debug_lines_device(self, lines_ptr, cap, total_ptr, flags=DEBUG_ALL, region=None):
        """The same into device memory: lines_ptr = room for cap 28-byte records, total_ptr = one uint64 (device pointers, e.g.
        tensor.data_ptr()).  Enqueued on the world's stream without synchronisation; lines beyond cap are counted, not written."""
        desc = _debug_desc(flags, region)
        check(lib().bge_world_debug_lines_device(self._h, C.byref(desc), C.c_void_p(lines_ptr) if lines_ptr else None, int(cap),
                                                 C.c_void_p(total_ptr)))

    # -- frustum culling (include/bge_world.h states the rule and the order)
    def upload_bounds(self, center, half, first=0, entity_index=None):
        """Model-space bounds (centre, half extents; (n, 3) each) of a range of entities, or of entity_index[i] per row."""
        c, h = _arr(center, np.float32, 3), _arr(half, np.float32, 3)
        if len(c) != len(h):
            raise ValueError(f"{len(c)} centres, {len(h)} half extents")
        if entity_index is None:
            check(lib().bge_world_upload_bounds(self._h, first, len(c), _p(c), _p(h)))
        else:
            idx = _arr(entity_index, np.uint32)
            check(lib().bge_world_upload_bounds_indexed(self._h, len(idx), _p(idx), _p(c), _p(h)))

    def visible_count(self, planes=None) -> int:
        desc = _cull_desc(planes)
        total = C.c_uint64(0)
        check(lib().bge_world_visible(self._h, C.byref(desc), None, None, None, 0, C.byref(total)))
        return int(total.value)

    def visible(self, planes=None, want_world=True, want_normal=False):
        """The visible entities in ascending entity index: dict of "entities" (n,) uint32 and, when asked for, "world" and
        "normal" (n, 16) — row k of each belongs to entities[k]."""
        desc = _cull_desc(planes)
        n = self.visible_count(planes)
        ent = np.empty(n, np.uint32)
        wm = np.empty((n, 16), np.float32) if want_world else None
        nm = np.empty((n, 16), np.float32) if want_normal else None
        total = C.c_uint64(0)
        if n or want_normal:  # (a missing normal-matrix tick is reported even when nothing is visible)
            check(lib().bge_world_visible(self._h, C.byref(desc), _p(ent), _p(wm), _p(nm), n, C.byref(total)))
        out = {"entities": ent}
        if want_world:
            out["world"] = wm
        if want_normal:
            out["normal"] = nm
        return out

    def visible_device(self, planes, entities_ptr, world_ptr, normal_ptr, cap, total_ptr):
        """The same between device pointers (0 / None leaves an output out): room for cap records each, total_ptr one uint64.
        Enqueued on the world's stream without synchronisation; records beyond cap are counted, not written."""
        desc = _cull_desc(planes)
        vp = lambda a: C.c_void_p(a) if a else None
        check(lib().bge_world_visible_device(self._h, C.byref(desc), vp(entities_ptr), vp(world_ptr), vp(normal_ptr), int(cap),
                                             C.c_void_p(total_ptr)))

    # -- draw batches (include/bge_world.h states membership and order)
    def upload_draw_keys(self, keys, first=0, entity_index=None):
        """Draw key (uint32, the caller's id of a mesh + material) of a range of entities, or of entity_index[i] per row."""
        k = _arr(keys, np.uint32).reshape(-1)
        if entity_index is None:
            check(lib().bge_world_upload_draw_keys(self._h, first, len(k), _p(k)))
        else:
            idx = _arr(entity_index, np.uint32).reshape(-1)
            if len(idx) != len(k):
                raise ValueError(f"{len(idx)} indices, {len(k)} keys")
            check(lib().bge_world_upload_draw_keys_indexed(self._h, len(idx), _p(idx), _p(k)))

    def draw_batches(self, planes, n_keys, want_world=True, want_normal=False):
        """The visible entities whose key is below n_keys, sorted by (key, entity index): dict of "batches" (n_keys, 2) uint32
        (first_instance, instance_count per key), "entities" (n,) uint32 and, when asked for, "world" and "normal" (n, 16)."""
        desc = _cull_desc(planes)
        n_keys = int(n_keys)
        total = C.c_uint64(0)
        check(lib().bge_world_draw_batches(self._h, C.byref(desc), n_keys, None, None, None, None, 0, C.byref(total)))
        n = int(total.value)
        batches = np.zeros((n_keys, 2), np.uint32)
        ent = np.empty(n, np.uint32)
        wm = np.empty((n, 16), np.float32) if want_world else None
        nm = np.empty((n, 16), np.float32) if want_normal else None
        check(lib().bge_world_draw_batches(self._h, C.byref(desc), n_keys, _p(batches), _p(ent), _p(wm), _p(nm), n, C.byref(total)))
        out = {"batches": batches, "entities": ent}
        if want_world:
            out["world"] = wm
        if want_normal:
            out["normal"] = nm
        return out

    def draw_batches_device(self, planes, n_keys, batches_ptr, entities_ptr, world_ptr, normal_ptr, cap, total_ptr):
        """The same between device pointers (0 / None leaves an output out): n_keys batches, room for cap records each, total_ptr
        one uint64.  Enqueued on the world's stream without synchronisation; records beyond cap are counted, not written."""
        desc = _cull_desc(planes)
        vp = lambda a: C.c_void_p(a) if a else None
        check(lib().bge_world_draw_batches_device(self._h, C.byref(desc), int(n_keys), vp(batches_ptr), vp(entities_ptr), vp(world_ptr),
                                                  vp(normal_ptr), int(cap), C.c_void_p(total_ptr)))

    def pack_roots(self, dst_device_ptr: int | None = None):
        check(lib().bge_world_pack_roots(self._h, C.c_void_p(dst_device_ptr) if dst_device_ptr else None))

    # native RCCL collective (see include/bge_world.h)
    @staticmethod
    def comm_unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        check(lib().bge_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, nranks: int, rank: int, unique_id: bytes, rows_per_rank: int):
        buf = C.create_string_buffer(unique_id, 128)
        check(lib().bge_world_comm_init(self._h, nranks, rank, buf, rows_per_rank))

    def gather_roots(self) -> int:
        """Pack this rank's roots and enqueue the frame's all-gather; returns the device pointer of the table."""
        ptr = C.c_void_p()
        check(lib().bge_world_gather_roots(self._h, C.byref(ptr)))
        return int(ptr.value or 0)

    def download_gathered(self, nranks: int, rows_per_rank: int):
        out = np.empty((nranks, rows_per_rank, 16), np.float32)
        check(lib().bge_world_download_gathered(self._h, _p(out), out.size))
        return out

    def comm_wait(self):
        check(lib().bge_world_comm_wait(self._h))

    def comm_set_mode(self, mode: int):
        """0 = ncclAllGather, 1 = direct send/recv per peer (include/bge_world.h)."""
        check(lib().bge_world_comm_set_mode(self._h, int(mode)))

    def comm_destroy(self):
        check(lib().bge_world_comm_destroy(self._h))

    def device_array(self, which: int):
        ptr, n = C.c_void_p(), C.c_uint64(0)
        check(lib().bge_world_device_array(self._h, which, C.byref(ptr), C.byref(n)))
        return int(ptr.value or 0), int(n.value)

    def info(self) -> dict:
        inf = WorldInfo()
        check(lib().bge_world_get_info(self._h, C.byref(inf)))
        return inf.as_dict()

    # -- convenience used by tests and the bench: build a whole synthetic workload
    def load(self, wl, with_bodies=True):
        self.set_topology(wl.parent)
        self.upload_trs(wl.pos, wl.euler, wl.scale)
        if with_bodies:
            self.upload_bodies(wl.body_type)
        return self


class PinnedArray:
    """numpy view of page-locked host memory (bge_host_alloc); keep the object alive as long as the array is used."""

    def __init__(self, shape, dtype=np.float32):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self._p = C.c_void_p()
        check(lib().bge_host_alloc(n, C.byref(self._p)))
        buf = (C.c_char * max(n, 1)).from_address(self._p.value)
        self.array = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def __del__(self):
        try:
            if self._p:
                lib().bge_host_free(self._p)
                self._p = C.c_void_p()
        except Exception:
            pass


def device_memory():
    """(allocations, bytes) the library holds in this process over all worlds (bge_device_memory); (0, 0) once every world is closed."""
    allocations, nbytes = C.c_uint64(), C.c_uint64()
    lib().bge_device_memory(C.byref(allocations), C.byref(nbytes))
    return int(allocations.value), int(nbytes.value)


def balanced_cuts(hist, lo, hi, nranks):
    """Host-only: slab boundaries at the k/nranks quantiles of an (all-reduced) axis histogram."""
    hist = _arr(hist, np.uint64)
    cuts = np.zeros(nranks + 1, np.float32)
    check(lib().bge_balanced_cuts(_p(hist), len(hist), lo, hi, nranks, _p(cuts)))
    return cuts


def flatten_topology(parent, has_transform=None):
    """Host-only: the slot / level / pass the library would give each entity, plus layout info."""
    parent = _arr(parent, np.uint32)
    ht = _arr(has_transform, np.uint8)
    n = len(parent)
    slot = np.empty(n, np.uint32)
    level = np.empty(n, np.uint8)
    pas = np.empty(n, np.uint32)
    inf = WorldInfo()
    check(lib().bge_flatten_topology(n, _p(parent), _p(ht), _p(slot), _p(level), _p(pas), C.byref(inf)))
    return slot, level, pas, inf.as_dict()


def partition_subtrees(parent, nranks, has_transform=None):
    """Host-only: rank of every entity (whole subtrees per rank) and the node count per rank."""
    parent = _arr(parent, np.uint32)
    ht = _arr(has_transform, np.uint8)
    n = len(parent)
    rank = np.empty(n, np.uint32)
    load = np.empty(nranks, np.uint64)
    check(lib().bge_partition_subtrees(n, _p(parent), _p(ht), nranks, _p(rank), _p(load)))
    return rank, load
