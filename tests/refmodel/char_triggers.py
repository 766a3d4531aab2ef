"""The rule of include/bge_world.h "Character trigger events" in plain numpy: the character box in binary32 exactly as the rule
writes it, the closed-interval overlap, the two-sided filter, and the Enter / Stay / Exit difference in the rule's order."""
from __future__ import annotations

import numpy as np

ENTER, STAY, EXIT = 0, 1, 2
CHAR_GROUP, CHAR_MASK = 2, 0xFFFFFFFF  # what NULL filter arrays mean
THRESHOLD = np.float32(0.02)


def char_boxes(pos, radius):
    """(cmin, cmax), each (n, 3) float32: (p - r) - 0.02f and (p + r) + 0.02f, one rounding per operation."""
    p = np.asarray(pos, np.float32).reshape(-1, 3)
    r = np.asarray(radius, np.float32).reshape(-1, 1)
    cmin = ((p - r).astype(np.float32) - THRESHOLD).astype(np.float32)
    cmax = ((p + r).astype(np.float32) + THRESHOLD).astype(np.float32)
    return cmin, cmax


def geometric_overlap(boxes, pos, radius):
    """(T, n) bool: on every axis tmin <= cmax and tmax >= cmin."""
    b = np.asarray(boxes, np.float32).reshape(-1, 6)
    cmin, cmax = char_boxes(pos, radius)
    return ((b[:, None, 0:3] <= cmax[None]) & (b[:, None, 3:6] >= cmin[None])).all(axis=2)


def filter_pass(layer, mask, group, cmask):
    """(T, n) bool: (trigger.layer & char.mask) != 0 and (char.group & trigger.mask) != 0."""
    layer, mask = np.asarray(layer, np.uint32)[:, None], np.asarray(mask, np.uint32)[:, None]
    group, cmask = np.asarray(group, np.uint32)[None], np.asarray(cmask, np.uint32)[None]
    return ((layer & cmask) != 0) & ((group & mask) != 0)


def char_trigger_ref(boxes, listed, layer, mask, pos, radius, group, cmask, prev, stay, entity=None):
    """One update call.  boxes (T, 6), listed (T,), layer and mask (T,) of the triggers in the order of the uploaded array; pos
    (n, 3), radius, group and cmask (n,) of the characters; prev (T, n) bool, the remembered matrix.  Returns (events (k, 3) uint32
    rows of (type, trigger, character) in the list's order, the new remembered matrix).  trigger is entity[t], or t itself."""
    prev = np.asarray(prev, bool)
    T, n = prev.shape
    listed = np.asarray(listed, bool)
    cur = geometric_overlap(boxes, pos, radius) & filter_pass(layer, mask, group, cmask)
    rows, after = [], prev.copy()
    for t in range(T):
        if not listed[t]:
            continue  # not tested, no event, remembered as it was
        name = t if entity is None else int(entity[t])
        for c in np.nonzero(cur[t])[0]:
            if prev[t, c]:
                if stay:
                    rows.append((STAY, name, c))
            else:
                rows.append((ENTER, name, c))
        for c in np.nonzero(prev[t] & ~cur[t])[0]:
            rows.append((EXIT, name, c))
        after[t] = cur[t]
    return np.array(rows, np.uint32).reshape(-1, 3), after


def pairs_of(remembered, entity=None):
    """The remembered matrix as (trigger, character) rows, by trigger array order and then by character."""
    t, c = np.nonzero(np.asarray(remembered, bool))
    return np.stack([t if entity is None else np.asarray(entity)[t], c], axis=1).astype(np.uint32).reshape(-1, 2)
