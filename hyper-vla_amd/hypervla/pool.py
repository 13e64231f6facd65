"""Episode pool (include/hvla.h `hvla_weights_alloc` / `hvla_generate_slots` / `hvla_step_slots` / `hvla_ensemble_slots`):
host-side checks of a slot map before it reaches the device.

A pool is a weight arena of `capacity` slots.  Episodes join it (`HyperVLA.assign_tasks`) and leave it at any time, and a step
runs any subset of its slots (`HyperVLA.sample_actions(..., slots=...)`).  The kernels skip a slot outside [0, capacity), so a
bad index never touches memory outside the arena; but a skipped row leaves its outputs unwritten, and duplicate slots would race
on one row.  So every slot map goes through :func:`check_slots` first."""
from __future__ import annotations

import numpy as np


def check_slots(slots, capacity: int) -> np.ndarray:
    """`slots` (a sequence, numpy array or torch tensor of integers) as a contiguous int32 [K] array; raises ValueError when it is
    empty, not one-dimensional, longer than `capacity`, has an entry outside [0, capacity) or names a slot twice, and TypeError
    when its entries are not integers."""
    if hasattr(slots, "detach"):                          # a torch tensor (on any device)
        slots = slots.detach().cpu().numpy()
    a = np.asarray(slots)
    if a.ndim != 1:
        raise ValueError(f"slots must be one-dimensional, got shape {a.shape}")
    if a.size == 0:
        raise ValueError("slots is empty: a pooled call needs at least one slot")
    if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer):
        raise TypeError(f"slots must be integers, got {a.dtype}")
    capacity = int(capacity)
    if a.size > capacity:
        raise ValueError(f"{a.size} slots for a pool of {capacity}")
    lo, hi = int(a.min()), int(a.max())
    if lo < 0 or hi >= capacity:
        raise ValueError(f"slot {lo if lo < 0 else hi} outside [0, {capacity})")
    if np.unique(a).size != a.size:
        vals, counts = np.unique(a, return_counts=True)
        raise ValueError(f"slots named more than once: {vals[counts > 1].tolist()}")
    return np.ascontiguousarray(a, dtype=np.int32)
