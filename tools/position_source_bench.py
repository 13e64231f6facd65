"""The fine-tune step of `bench.py --finetune --train-encoder` with the DINOv2 position table trained through its interpolation
(DESIGN.md section 13): the same model, inputs, warm-up and timed loop, once with the baked table as the parameter (source off,
what bench.py runs) and once with a hub-shaped 37 x 37 source (source on: two more launches in the step, two in the apply).

    python tools/position_source_bench.py --batch 32 --steps 20 --warmup 3

Prints one JSON line: ms per step of both, their difference, and the two kernels alone (HIP events, median of 50)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "hyper-vla_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch


def timed(ft, args, steps, warmup, dev):
    for _ in range(warmup):
        ft.step(*args)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(steps):
        ft.step(*args)
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=37)
    a = ap.parse_args()
    from hypervla import synthetic as syn
    from hypervla.config import FULL
    from hypervla.model import HyperVLA
    from hypervla.train import FineTuner
    g, B = FULL, a.batch
    model = HyperVLA.from_synthetic(g, position_table_source=syn.synthetic_position_table_hub(g, a.n), max_batch=B)
    dev = model.device
    ins, st = syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g)
    images = torch.as_tensor(syn.synthetic_images(B, g)[:, 0]).to(dev).contiguous()
    args = (ins, st, images, syn.synthetic_action_batch(B, g))
    out = {"batch": B, "steps": a.steps, "warmup": a.warmup, "n": a.n}
    for name, kw in (("off", dict(accept_baked_position_table=True)), ("on", {}), ("off_again", dict(accept_baked_position_table=True))):
        ft = FineTuner(model, B, train_encoder=True, **kw)
        assert (ft.source_n > 0) == (name == "on")
        out[f"ms_per_step_source_{name}"] = round(timed(ft, args, a.steps, a.warmup, dev), 3)
        if name == "on":                                  # the two kernels alone
            ctx, w, grid = model._ctx, ft.interp_w, g.grid
            for label, call in (("interp", lambda: ctx.position_interp(ft.params[ft.tail].data_ptr(), a.n, w.data_ptr(), ft.params[ft.slot].data_ptr(), model._stream())),
                                ("adjoint", lambda: ctx.position_interp_adjoint(ft.grads[ft.slot].data_ptr(), a.n, w.data_ptr(), ft.grads[ft.tail].data_ptr(), model._stream()))):
                us = []
                for _ in range(50):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    call()
                    e1.record()
                    e1.synchronize()
                    us.append(e0.elapsed_time(e1) * 1e3)
                out[f"{label}_us_median"] = round(float(np.median(us)), 2)
        del ft
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
