"""What `frozen_keys` saves in the fine-tune step: README geometry, image encoder frozen, the same model and
inputs for three configurations of one process on one box -- no frozen_keys, the context encoder frozen (bucket 2 not computed:
no dctx split-K product, no context-encoder backward), the output heads frozen (bucket 1 not computed: no dW_cat, no db_cat; the
optimizer skips 98 % of the vector) -- and the first once more at the end, to show the box's drift.

    python tools/finetune_frozen_bench.py --batch 32 --steps 20 --warmup 3 [--out FILE]

Per configuration: ms per forward_backward and per apply (HIP events on the model's stream round each call, mean over the timed
steps) and the kernel launches of one forward_backward and one apply (torch.profiler's device activity: every kernel of the
process, memsets and copies left out).  With the box's clock (hvla_box_probe).  Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "hyper-vla_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch

CONFIGS = (("none", ()),
           ("context_frozen", ("Transformer_0.*", "task_*", "initial_image_*", "layer_pos_embedding")),
           ("heads_frozen", ("output_head_*",)),
           ("none_again", ()))


def timed(ft, args, steps, warmup, dev):
    for _ in range(warmup):
        ft.forward_backward(*args)
        ft.apply(lr=1e-4)
    torch.cuda.synchronize(dev)
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(steps)]
    for e in ev:
        e[0].record()
        ft.forward_backward(*args)
        e[1].record()
        ft.apply(lr=1e-4)
        e[2].record()
    torch.cuda.synchronize(dev)
    return (sum(e[0].elapsed_time(e[1]) for e in ev) / steps, sum(e[1].elapsed_time(e[2]) for e in ev) / steps)


def launches(call, dev):
    """Kernels one call puts on the device, or None with the reason when the profiler sees no device activity here."""
    from torch.profiler import ProfilerActivity, profile
    try:
        torch.cuda.synchronize(dev)
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            call()
            torch.cuda.synchronize(dev)
        names = [e.name for e in prof.events() if str(e.device_type).endswith("CUDA")]
    except Exception as exc:                          # a measurement tool: say why there is no figure
        return None, f"{type(exc).__name__}: {exc}"
    kernels = [n for n in names if not any(w in n.lower() for w in ("memset", "memcpy", "fillbuffer", "copybuffer"))]
    return (len(kernels), None) if names else (None, "torch.profiler recorded no device activity")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    from hypervla import synthetic as syn
    from hypervla.config import FULL
    from hypervla.model import HyperVLA
    from hypervla.train import FineTuner
    g, B = FULL, a.batch
    model = HyperVLA.from_synthetic(g, max_batch=B)
    dev = model.device
    clock, tflops, _ = model._ctx.box_probe(model._stream())
    ins, st = syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g)
    images = torch.as_tensor(syn.synthetic_images(B, g)[:, 0]).to(dev).contiguous()
    tokens = model.encode_images(images)                   # f32 [B, P, E] on the device: what a frozen-encoder step is given
    args = (ins, st, tokens, syn.synthetic_action_batch(B, g))
    out = {"geometry": "FULL", "batch": B, "steps": a.steps, "warmup": a.warmup, "train_encoder": False,
           "clock_mhz": round(clock), "mfma_tflops": round(tflops, 1), "configs": {}}
    for name, keys in CONFIGS:
        ft = FineTuner(model, B, frozen_keys=keys)
        fb_ms, ap_ms = timed(ft, args, a.steps, a.warmup, dev)
        n_fb, why = launches(lambda: ft.forward_backward(*args), dev)
        n_ap, why2 = launches(lambda: ft.apply(lr=1e-4), dev)
        out["configs"][name] = {"frozen_buckets": ft.frozen_buckets, "frozen_count": ft.frozen_count, "trainable_count": ft.trainable_count,
                                "forward_backward_ms": round(fb_ms, 3), "apply_ms": round(ap_ms, 3),
                                "forward_backward_launches": n_fb, "apply_launches": n_ap}
        if why or why2:
            out["configs"][name]["launches_note"] = why or why2
        del ft
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
