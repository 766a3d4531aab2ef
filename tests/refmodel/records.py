"""The C records and flag words of include/bge_world.h that the references fill in, restated as numpy dtypes so that the model
layers need nothing of the product package (test_tree_layout_cpu.py holds them equal to banggameengine_amd.world's)."""
from __future__ import annotations

import numpy as np

RAY_HIT_DTYPE = np.dtype([("kind", "<u4"), ("entity", "<u4"), ("fraction", "<f4"), ("distance", "<f4"), ("point", "<f4", (3,)),
                          ("normal", "<f4", (3,))])
SPHERE_CAST_DTYPE = np.dtype([("origin", "<f4", (3,)), ("direction", "<f4", (3,)), ("max_distance", "<f4"), ("radius", "<f4"),
                              ("layer_mask", "<u4"), ("reserved", "<u4")])
SPHERE_DTYPE = np.dtype([("center", "<f4", (3,)), ("radius", "<f4"), ("layer_mask", "<u4")])

MOVE_SLIDES = 4
MOVE_INVALID, MOVE_GROUNDED, MOVE_OUT_OF_SLIDES, MOVE_PROBE_HIT = 1, 2, 4, 8
SPHERE_MOVE_RESULT_DTYPE = np.dtype([("position", "<f4", (3,)), ("remaining", "<f4", (3,)), ("flags", "<u4"), ("n_hits", "<u4"),
                                     ("hit_kind", "<u4"), ("hit_entity", "<u4"), ("hit_normal", "<f4", (3,)), ("ground_kind", "<u4"),
                                     ("ground_entity", "<u4"), ("ground_distance", "<f4"), ("ground_normal", "<f4", (3,)),
                                     ("reserved", "<u4")])

RECOVER_ROUNDS = 4
RECOVER_INVALID, RECOVER_MOVED, RECOVER_STUCK = 1, 2, 4
PENETRATION_HIT_DTYPE = np.dtype([("kind", "<u4"), ("entity", "<u4"), ("depth", "<f4"), ("point", "<f4", (3,)), ("normal", "<f4", (3,)),
                                  ("reserved", "<u4")])
SPHERE_RECOVER_RESULT_DTYPE = np.dtype([("position", "<f4", (3,)), ("pushed", "<f4", (3,)), ("flags", "<u4"), ("n_pushes", "<u4"),
                                        ("hit_kind", "<u4"), ("hit_entity", "<u4"), ("hit_normal", "<f4", (3,)), ("hit_depth", "<f4"),
                                        ("remaining_depth", "<f4"), ("reserved", "<u4")])
