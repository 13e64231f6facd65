"""The fine-tune step of `bench.py --finetune` (frozen encoder) with the reference's attention entropy / alignment terms off and on
(DESIGN.md section 15): the same model, inputs and timed loop, alternating off / on / off / on so that drift of the box shows up as
a difference between the two runs of the same setting.  Timed with HIP events on the step's stream.

    python tools/attention_loss_bench.py --batch 32 --steps 20 --warmup 3

Prints one JSON line: ms per step of every leg, the means of both settings and their difference (on: two launches of
attention_aux_kernel more per step), and the box's sustained shader clock (hvla_box_probe)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "hyper-vla_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch


def timed(ft, args, kw, steps, warmup, dev):
    for _ in range(warmup):
        ft.step(*args, **kw)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    e0.record()
    for _ in range(steps):
        ft.step(*args, **kw)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    from hypervla import synthetic as syn
    from hypervla.config import FULL
    from hypervla.model import HyperVLA
    from hypervla.train import FineTuner
    g, B = FULL, a.batch
    model = HyperVLA.from_synthetic(g, max_batch=B)
    dev = model.device
    ins, st = syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g)
    images = torch.as_tensor(syn.synthetic_images(B, g)[:, 0]).to(dev).contiguous()
    args = (ins, st, images, syn.synthetic_action_batch(B, g))
    ref = model.reference_attention_map(images)           # the pretrained encoder's map: nothing has been published
    off = FineTuner(model, B)
    on = FineTuner(model, B, attention_entropy=0.01, attention_map_alignment=1.0, num_steps=10 ** 6)
    out = {"batch": B, "steps": a.steps, "warmup": a.warmup, "off_ms": [], "on_ms": []}
    for _ in range(a.rounds):
        out["off_ms"].append(round(timed(off, args, {}, a.steps, a.warmup, dev), 3))
        out["on_ms"].append(round(timed(on, args, dict(reference_attention=ref), a.steps, a.warmup, dev), 3))
    out["off_ms_mean"] = round(float(np.mean(out["off_ms"])), 3)
    out["on_ms_mean"] = round(float(np.mean(out["on_ms"])), 3)
    out["on_minus_off_ms"] = round(out["on_ms_mean"] - out["off_ms_mean"], 3)
    out["on_minus_off_percent"] = round(100.0 * out["on_minus_off_ms"] / out["off_ms_mean"], 3)
    out["metrics_last_step"] = {k: float(v.mean()) for k, v in on.aux_metrics.items()}
    mhz, tflops, _ = model._ctx.box_probe(model._stream())             # what this box sustains: a step time is read against it
    out["box_shader_mhz"], out["box_probe_tflops"] = round(mhz, 1), round(tflops, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
