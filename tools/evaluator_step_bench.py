"""Evaluator step with host vs device post-processing (README geometry, synthetic weights): BatchEvaluator.run_episodes over a toy
vector env of E in-process simulators with a fixed 224 x 224 frame, once with postprocess="host" (one InferenceWrapper.postprocess
per running episode) and once with postprocess="device" (one hvla_post_step launch).  Every episode runs exactly `steps` steps, so
all E slots step at every timestep.  Model seconds per step = (model seconds of a `steps`-step run - those of a 1-step run) /
(steps - 1): the pool creation, the first-frame encoding and the task assignment cancel.  One JSON line per E.

    python tools/evaluator_step_bench.py [E ...]        (default: 64 256)"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "hyper-vla_amd"), ROOT]

SIZE = 224


class ToyEnv:
    """Frames depend on (seed, t) only; never succeeds, truncates after `limit` steps."""

    def __init__(self, limit):
        self.limit, self.seed, self.t = limit, 0, 0

    def _frame(self):
        return np.random.default_rng(1000 * self.seed + self.t).integers(0, 256, (SIZE, SIZE, 3), dtype=np.uint8)

    def reset(self, seed=0, **kw):
        self.seed, self.t = seed, 0
        return self._frame(), {}

    def get_language_instruction(self):
        return f"move block {self.seed}"

    def step(self, action):
        self.t += 1
        return self._frame(), 0.0, False, self.t >= self.limit, {}


def main(envs=(64, 256), steps=41, setup="google_robot"):
    import functools

    from hypervla.config import FULL
    from hypervla.evaluate import BatchEvaluator, DummyVectorEnv
    from hypervla.model import HyperVLA
    from hypervla.synthetic import synthetic_instructions
    g = FULL
    m = HyperVLA.from_synthetic(g, max_batch=max(envs))
    for E in envs:
        base = synthetic_instructions(E, g)["language_instruction"]

        def tokenize(instrs):
            idx = [int(s.split()[-1]) for s in instrs]
            return {k: np.asarray(v)[idx] for k, v in base.items()}

        def model_seconds(mode, n):
            venv = DummyVectorEnv([functools.partial(ToyEnv, n) for _ in range(E)], (SIZE, SIZE, 3))
            ev = BatchEvaluator(m, policy_setup=setup, pred_action_horizon=g.horizon, action_ensemble=True, postprocess=mode)
            r = ev.run_episodes(venv, tokenize, E, max_steps=n, reset_kwargs_for=lambda i: {"seed": i})
            assert r["rows_stepped"] == E * n, r["rows_stepped"]
            return r["model_seconds"]

        out = {"E": E, "steps": steps, "policy_setup": setup}
        for mode in ("host", "device"):
            model_seconds(mode, 2)                                   # warm-up: allocations, first launches
            one, full = model_seconds(mode, 1), model_seconds(mode, steps)
            out[f"{mode}_ms_per_step"] = round(1e3 * (full - one) / (steps - 1), 3)
        out["saved_ms_per_step"] = round(out["host_ms_per_step"] - out["device_ms_per_step"], 3)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main(tuple(int(a) for a in sys.argv[1:]) or (64, 256))
