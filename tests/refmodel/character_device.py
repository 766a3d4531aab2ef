"""The GPU side of the character comparisons: the device's penetration query and the public World.sphere_recover /
World.sphere_step_move in the forms char_ref expects, and a character set driven step by step with every state kept."""
from __future__ import annotations

import ctypes as C

import numpy as np

from banggameengine_amd import world as W

from .step_device import STEP_FIELDS


def device_pen(w):
    """SPHERE_DTYPE[n] -> PENETRATION_HIT_DTYPE[n] through World.sphere_penetration."""
    def pen_fn(spheres):
        h = w.sphere_penetration(spheres["center"], spheres["radius"], spheres["layer_mask"])
        hits = np.zeros(len(spheres), W.PENETRATION_HIT_DTYPE)
        for k, v in h.items():
            hits[k] = v
        return hits
    return pen_fn


def public_batches(w):
    """The two batches of char_ref as the public calls: recover_fn, step_fn."""
    return dict(recover_fn=lambda rec: w.sphere_recover(rec["position"], rec["radius"], rec["skin"], rec["layer_mask"]),
                step_fn=lambda mv: w.sphere_step_move(*(mv[k] for k in STEP_FIELDS)))


def run_script(w, descs, script, dt):
    """Creates the set, then one update of one step per input of the script: the states after every step."""
    w.characters_create(descs)
    history = []
    for inp in script:
        w.characters_set_input(inp)
        w.characters_update(dt, 1)
        history.append(w.characters_state())
    return history


def read_device_into(tensor, ptr):
    """Copies tensor's size in bytes from the device pointer ptr into the device tensor (hipMemcpy, device to device)."""
    for name in ("libamdhip64.so", "libamdhip64.so.7", "libamdhip64.so.6", "/opt/rocm/lib/libamdhip64.so"):
        try:
            hip = C.CDLL(name)
            break
        except OSError:
            continue
    else:
        raise RuntimeError("HIP runtime library not found")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(tensor.data_ptr(), ptr, tensor.numel() * tensor.element_size(), 3) == 0
