"""The tolerances of the comparisons between the device and the float64 reference: the one place they are stated.

The reference takes the device's own binary32 poses (download_pose / download_bodies) and binary32 query inputs, so what differs
is the kernel's binary32 arithmetic — a rotation into the body frame, one slab division or a quadratic solved about the point of
closest approach.  Bounds: fraction 1e-5 relative + 1e-6 absolute; point 2e-5 per unit of coordinate magnitude; normal 1e-4 per
component plus 2e-6 x (|origin|_1 + |direction * max_distance|_1) / (the hit shape's smallest half extent or radius) — the entry
point is only known to a few binary32 ulp of the ray's magnitudes, and the normal of a small capsule turns by that error over its
radius (measured: 1.3e-3 for a ray from ~700 units at a small capsule)."""
from __future__ import annotations

import numpy as np

F_REL, F_ABS, P_REL, N_ABS, N_SCALE = 1e-5, 1e-6, 2e-5, 1e-4, 2e-6
NEVER_INSIDE_MARGIN = np.float32(1e-3)  # by how much a mover that started clear may end inside something

# Histogram of the sharded broadphase (bge_world_axis_histogram, refmodel/slabs.hist_sandwich).  The device forms the bin of a min
# corner x as t = (x - lo) * (1 / ((hi - lo) / bins)) in five binary32 roundings (hi - lo, the division by bins, the reciprocal,
# x - lo, the product), each relative 2^-24 = u, on quantities no larger than hi - lo once carried back to x: the bin edge the
# device sees lies within 5 u (hi - lo) of the exact one.  The sandwich allows d = HIST_EDGE_ULPS u (hi - lo), the next power of
# two above that bound; the factor follows from this count, not from what a device returned.
HIST_EDGE_ULPS = 8

# The box-box narrowphase against its float64 model (refmodel/boxbox64): the largest deviation of the ORACLE's answers from the model over
# the whole case set of refmodel/boxbox_cases, every figure taken relative to the pair's scale, is BOXBOX_MEASURED (DESIGN.md 6b has the
# figure per check).  The margin of 4 is for the summation orders a compiler's fast-math mode may choose differently (the reference was
# built with one); it comes from that argument, not from what a device returned.
BOXBOX_MEASURED = 6.5e-7
BOXBOX_REL = 4 * BOXBOX_MEASURED
