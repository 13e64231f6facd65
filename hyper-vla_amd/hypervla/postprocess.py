"""`InferenceWrapper.postprocess` for the slots of an episode pool, on the device (include/hvla.h `hvla_post_*`).

Each slot keeps the caller-side state of the episode it runs -- the temporal-ensemble history, the call count and the google_robot
sticky gripper -- together with its own policy setup, so one pool can mix `libero`, `widowx_bridge` and `google_robot` episodes.  One
launch post-processes every stepped slot: un-normalisation, temporal ensemble (temperature 0), euler -> axis-angle and the gripper
rule of its setup, in f64 and in the host's operation order (data/utils/hypervla_interface.py:219-299).  raw_action and the env
action's translation are bitwise the host's, the rotation is within 1 f32 ulp of it and the gripper is exact."""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple, Union

import numpy as np

from . import _native
from .interface import action_statistics
from .pool import check_slots

SETUP_CODES = {"libero": _native.HVLA_SETUP_LIBERO, "widowx_bridge": _native.HVLA_SETUP_WIDOWX_BRIDGE,
               "google_robot": _native.HVLA_SETUP_GOOGLE_ROBOT}


def table_row(policy_setup: str, stats: Dict, normalization_type: str) -> _native.hvla_post_row:
    """The `hvla_post_row` of one policy setup with its action statistics: the exact f64 operands `InferenceWrapper.unnormalize`
    uses.  For BOUNDS the second vector is ``p99 - p01 + 1e-8`` evaluated as that expression evaluates it (in the statistics' own
    dtype), widened to f64 -- the kernel then computes ``(a + 1) * p1 / 2 + p01`` literally."""
    if policy_setup not in SETUP_CODES:                  # 'metaworld' included: the reference's branch cannot run (1-D [:, -1])
        raise ValueError(f"Unknown policy setup: {policy_setup}")
    s = stats
    if normalization_type in ("normal", "NORMAL"):
        kind = _native.HVLA_NORM_NORMAL
        mask = np.asarray(s.get("mask", np.ones_like(s["mean"], dtype=bool)), bool)
        p0, p1 = s["mean"], s["std"]
    elif normalization_type in ("bounds", "BOUNDS"):
        kind = _native.HVLA_NORM_BOUNDS
        mask = np.asarray(s.get("mask", np.ones_like(s["p01"], dtype=bool)), bool)
        p0, p1 = s["p01"], s["p99"] - s["p01"] + 1e-8
    else:
        raise ValueError(f"Unknown normalization type: {normalization_type}")
    D = _native.HVLA_POST_DIM
    p0, p1 = (np.asarray(v).astype(np.float64) for v in (p0, p1))
    if mask.shape != (D,) or p0.shape != (D,) or p1.shape != (D,):
        raise ValueError(f"action statistics must have {D} entries, got mask {mask.shape}, {p0.shape}, {p1.shape}")
    row = _native.hvla_post_row()
    row.normalization, row.setup = kind, SETUP_CODES[policy_setup]
    row.p0[:], row.p1[:], row.mask[:] = p0.tolist(), p1.tolist(), mask.astype(np.uint8).tolist()
    return row


class DevicePostprocessor:
    """Post-processing state for `capacity` slots (`hvla_post_create`), freed on garbage collection.

    `assign(slots, policy_setup, action_ensemble)` starts fresh episodes in those slots (what `InferenceWrapper.reset` does to its
    own state); `step(actions, slots)` post-processes one prediction per slot.  The table row of a policy setup is built from the
    model's statistics (`interface.action_statistics`) the first time a slot is assigned to it; the device table is only replaced
    when a new setup arrives, so a loop of `step` calls after the last new setup can be captured in a hipGraph."""

    def __init__(self, model, capacity: int):
        import torch
        capacity = int(capacity)
        if not 1 <= capacity <= model.max_batch:
            raise ValueError(f"capacity {capacity} outside [1, max_batch={model.max_batch}]")
        self.model, self.capacity = model, capacity
        self._h = None
        self._h = model._ctx.post_create(capacity, model._stream())
        self._rows: Dict[str, int] = {}
        self._host_rows: List[_native.hvla_post_row] = []
        self._table = torch.empty(0, dtype=torch.uint8, device=model.device)

    def __del__(self):
        try:
            if self._h is not None:
                self.model._ctx.post_free(self._h)
                self._h = None
        except Exception:
            pass

    def row_of(self, policy_setup: str) -> int:
        """Table row of `policy_setup`, built (and the device table extended) on first use."""
        import torch
        if policy_setup in self._rows:
            return self._rows[policy_setup]
        if policy_setup not in SETUP_CODES:
            raise ValueError(f"Unknown policy setup: {policy_setup}")
        stats, kind = action_statistics(self.model, policy_setup)
        self._host_rows.append(table_row(policy_setup, stats, kind))
        blob = b"".join(bytes(r) for r in self._host_rows)
        self._table = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(self.model.device)
        self._rows[policy_setup] = len(self._host_rows) - 1
        return self._rows[policy_setup]

    def assign(self, slots, policy_setup: Union[str, Sequence[str]], action_ensemble: Union[bool, Sequence[bool]] = True) -> None:
        """Fresh episodes in `slots` (`hvla_post_assign`): slot slots[k] runs `policy_setup` (one setup for all, or one per slot)
        with the temporal ensemble on or off (likewise).  Other slots keep their state."""
        import torch
        s = check_slots(slots, self.capacity)
        K = len(s)
        setups = [policy_setup] * K if isinstance(policy_setup, str) else list(policy_setup)
        if len(setups) != K:
            raise ValueError(f"{len(setups)} policy setups for {K} slots")
        ens = [bool(action_ensemble)] * K if np.ndim(action_ensemble) == 0 else [bool(e) for e in action_ensemble]
        if len(ens) != K:
            raise ValueError(f"{len(ens)} action_ensemble flags for {K} slots")
        rows = np.array([self.row_of(p) for p in setups], np.int32)
        dev = self.model.device
        sd, rd = torch.as_tensor(s).to(dev), torch.as_tensor(rows).to(dev)
        ed = torch.as_tensor(np.array(ens, np.uint8)).to(dev)
        self.model._ctx.post_assign(self._h, sd.data_ptr(), K, rd.data_ptr(), ed.data_ptr(), self.model._stream())

    def step(self, actions, slots) -> Tuple:
        """One `InferenceWrapper.postprocess` per slot (`hvla_post_step`): actions [K, horizon, 7] (row k the prediction of slot
        slots[k]) -> (raw_action, env_action), f64 [K, 7] each.  Numpy in -> numpy out, torch in -> torch out."""
        import torch
        m = self.model
        g = m.geometry
        s = check_slots(slots, self.capacity)
        K = len(s)
        as_torch = isinstance(actions, torch.Tensor)
        shape = tuple(actions.shape) if hasattr(actions, "shape") else np.shape(actions)
        D = _native.HVLA_POST_DIM
        if tuple(shape) != (K, g.horizon, D):
            raise ValueError(f"actions must be [{K}, {g.horizon}, {D}], got {tuple(shape)}")
        if not self._host_rows:
            raise RuntimeError("no slot has been assigned a policy setup yet: call assign() first")
        act = m._dev(actions, torch.float32)
        sd = torch.as_tensor(s).to(m.device)
        raw = torch.empty(K, D, dtype=torch.float64, device=m.device)
        env = torch.empty(K, D, dtype=torch.float64, device=m.device)
        m._ctx.post_step(self._h, sd.data_ptr(), K, act.data_ptr(), self._table.data_ptr(), len(self._host_rows), raw.data_ptr(),
                         env.data_ptr(), m._stream())
        if as_torch:
            return raw, env
        torch.cuda.current_stream(m.device).synchronize()
        return raw.cpu().numpy(), env.cpu().numpy()

