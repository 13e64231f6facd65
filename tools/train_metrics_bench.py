"""What the training metrics cost: `FineTuner.step` at the README geometry with metrics=False and metrics=True,
the same model, inputs and timed loop, alternating off / on so that drift of the box shows up between two legs of one setting.  Every
step is bracketed by HIP events on its stream; a leg reports the median over its steps (>= 50) after a warm-up.  Then the three
passes the metrics add are timed alone, each as the median of `--passes` event-bracketed calls: hvla_train_metrics(PRE),
hvla_train_metrics(UPDATE) and the snapshot copy, with the bytes each moves and the rate that makes.

    python tools/train_metrics_bench.py --train-encoder --batch 32 --steps 50 --warmup 5

Prints one JSON line."""
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


def events(n):
    return [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]


def median_ms(fn, n, warmup, dev):
    """Median over n calls of fn, each between two events on the current stream; one synchronisation at the end."""
    for _ in range(warmup):
        fn()
    ev = events(n)
    torch.cuda.synchronize(dev)
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize(dev)
    t = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
    return float(np.median(t)), float(t[0]), float(t[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--passes", type=int, default=50)
    ap.add_argument("--train-encoder", action="store_true")
    a = ap.parse_args()
    if a.steps < 50:
        ap.error("--steps >= 50: a leg reports a median")
    from hypervla import _native, synthetic as syn
    from hypervla.config import FULL
    from hypervla.model import HyperVLA
    from hypervla.train import FineTuner
    g, B = FULL, a.batch
    model = HyperVLA.from_synthetic(g, max_batch=B)
    dev = model.device
    ins, st = syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g)
    images = torch.as_tensor(syn.synthetic_images(B, g)[:, 0]).to(dev).contiguous()
    args = (ins, st, images, syn.synthetic_action_batch(B, g))
    off = FineTuner(model, B, train_encoder=a.train_encoder)
    on = FineTuner(model, B, train_encoder=a.train_encoder, metrics=True)
    out = {"geometry": "README (FULL)", "batch": B, "train_encoder": bool(a.train_encoder), "n_params": on.n, "steps": a.steps,
           "warmup": a.warmup, "off_ms": [], "on_ms": []}
    for _ in range(a.rounds):
        out["off_ms"].append(round(median_ms(lambda: off.step(*args), a.steps, a.warmup, dev)[0], 3))
        out["on_ms"].append(round(median_ms(lambda: on.step(*args), a.steps, a.warmup, dev)[0], 3))
    out["off_ms_median"] = round(float(np.median(out["off_ms"])), 3)
    out["on_ms_median"] = round(float(np.median(out["on_ms"])), 3)
    out["on_minus_off_ms"] = round(out["on_ms_median"] - out["off_ms_median"], 3)
    out["on_minus_off_percent"] = round(100.0 * out["on_minus_off_ms"] / out["off_ms_median"], 3)
    # the three passes alone.  PRE reads grads and params (and the frozen mask when there is one), UPDATE params and the snapshot,
    # the copy reads and writes one vector; the small kernels behind the norm pass (finish, rows, loss terms) are inside the PRE time
    on._select()
    n, mask = on.n, 1 if on.frozen is not None else 0
    passes = {"pre": (lambda: on._metrics_call(_native.HVLA_METRICS_PRE), (8 + mask) * n + 4 * B * on.G),
              "update": (lambda: on._metrics_call(_native.HVLA_METRICS_UPDATE), 8 * n),
              "snapshot": (lambda: on.prev_params.copy_(on.params), 8 * n)}
    for name, (fn, nbytes) in passes.items():
        med, lo, hi = median_ms(fn, a.passes, 3, dev)
        out[name] = {"ms_median": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4), "bytes": int(nbytes),
                     "TB_per_s": round(nbytes / (med * 1e-3) / 1e12, 3)}
    out["passes_ms_sum"] = round(sum(out[k]["ms_median"] for k in passes), 4)
    out["info_last_step"] = {k: float(v) for k, v in on.info().items()}
    mhz, tflops, _ = model._ctx.box_probe(model._stream())             # what this box sustains: a step time is read against it
    out["box_shader_mhz"], out["box_probe_tflops"] = round(mhz, 1), round(tflops, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
