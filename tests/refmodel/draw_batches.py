"""The reference of the draw batches (include/bge_world.h bge_world_draw_batches*): the grouping restated in numpy."""
from __future__ import annotations

import numpy as np

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
