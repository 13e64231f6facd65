"""Fine-tuning share_layer_index=False on one MI355X: ms per FineTuner.step (image encoder frozen: hvla_encode + forward
+ backward + AdamW) at batch B with Geometry.layer_tokens off, on, and on with shared block heads.  The three models and tuners live
in ONE process and ALTERNATE `--rounds` times, so that the box's drift shows next to the difference; synthetic weights,
device-resident inputs, HIP-event timing.  One JSON line per (geometry, round, flavour), then the medians and the spread.

`--gemm`: the batched-GEMM launch timer (hvla_train_profile) around one forward_backward per flavour, with the output heads' bucket
computed and frozen (frozen_keys=("output_head_*",) leaves out dW_h and db_h and nothing else): total GEMM ms, and by difference the
dW_h product -- the plain `bgemm` launch with the flag off, the grouped launch with it on."""
import argparse
import dataclasses
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "hyper-vla_amd"), ROOT]

FLAVOURS = {"off": dict(layer_tokens=False), "on": dict(layer_tokens=True), "on_shared": dict(layer_tokens=True, shared_block_heads=True)}


def _timed(torch, fn, warmup, iters):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def _setup(torch, name, flavour, B, **ft_kw):
    from hypervla import config, synthetic as syn
    from hypervla.model import HyperVLA
    from hypervla.train import FineTuner
    g = dataclasses.replace(getattr(config, name), **FLAVOURS[flavour])
    m = HyperVLA.from_synthetic(g, max_batch=B)
    dev = m.device
    ins, st, batch = syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g), syn.synthetic_action_batch(B, g)
    ins = {"language_instruction": {k: torch.as_tensor(v).to(dev) for k, v in ins["language_instruction"].items()}}
    im = torch.as_tensor(syn.synthetic_images(B, g)[:, 0]).to(dev).contiguous()
    ft = FineTuner(m, B, layer_tokens=g.layer_tokens, **ft_kw)
    return m, ft, (ins, st, im, batch)


def steps(name="FULL", B=32, rounds=5, warmup=3, iters=10):
    import torch
    run = {}
    for fl in FLAVOURS:
        m, ft, args = _setup(torch, name, fl, B)
        run[fl] = (lambda ft=ft, args=args: ft.step(*args, lr=1e-4), m, ft)
    ms = {fl: [] for fl in FLAVOURS}
    for rnd in range(rounds):
        for fl in FLAVOURS:
            ms[fl].append(_timed(torch, run[fl][0], warmup, iters))
            print(json.dumps({"geometry": name, "round": rnd, "layer_tokens": fl, "B": B, "train_encoder": False,
                              "finetune_step_ms": round(ms[fl][-1], 3), "iters": iters}), flush=True)
    med = {fl: statistics.median(v) for fl, v in ms.items()}
    print(json.dumps({"geometry": name, "B": B, **{"finetune_step_ms_%s_median" % fl: round(v, 3) for fl, v in med.items()},
                      "on_over_off": round(med["on"] / med["off"], 4), "on_shared_over_off": round(med["on_shared"] / med["off"], 4),
                      "off_spread": round((max(ms["off"]) - min(ms["off"])) / med["off"], 4)}), flush=True)


def gemm(name="FULL", B=32, reps=5):
    import torch
    for fl in FLAVOURS:
        out = {}
        for what, kw in (("all", {}), ("heads_frozen", dict(frozen_keys=("output_head_*",)))):
            m, ft, args = _setup(torch, name, fl, B, **kw)
            args = (args[0], args[1], m.encode_images(args[2]), args[3])      # forward_backward takes the frozen encoder's tokens
            for _ in range(2):
                ft.forward_backward(*args)
            torch.cuda.synchronize()
            m._ctx.train_profile(True)
            vals = []
            for _ in range(reps):
                ft.forward_backward(*args)
                torch.cuda.synchronize()
                ms, flops, n = m._ctx.train_profile_read()
                vals.append((ms, n))
            m._ctx.train_profile(False)
            out[what] = (statistics.median(v[0] for v in vals), vals[0][1])
        print(json.dumps({"geometry": name, "B": B, "layer_tokens": fl, "gemm_ms_forward_backward": round(out["all"][0], 4),
                          "gemm_launches": out["all"][1], "gemm_ms_heads_frozen": round(out["heads_frozen"][0], 4),
                          "gemm_launches_heads_frozen": out["heads_frozen"][1],
                          "dW_h_product_ms": round(out["all"][0] - out["heads_frozen"][0], 4)}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--geometry", default="FULL")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--gemm", action="store_true")
    a = ap.parse_args()
    if a.gemm:
        gemm(a.geometry, a.batch)
    else:
        steps(a.geometry, B=a.batch, rounds=a.rounds, iters=a.iters)
