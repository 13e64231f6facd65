"""use_differential_transformer on one MI355X: the generated policy alone (policy_from_tokens) at the README geometry
for the three attention flavours -- policy_kernel, policy_kernel_bias (return_attention_map) and policy_kernel_diff -- on synthetic
weights and device-resident Gaussian tokens, HIP-event timing.  The flavours ALTERNATE `--rounds` times in one process on one box,
`--iters` launches per timing after a warm-up, so that the box's drift shows next to the differences; one JSON line per (round, flavour,
B), then per B the medians, the ratio to the base flavour and the base flavour's spread over the rounds."""
import argparse
import dataclasses
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "hyper-vla_amd"), ROOT]

FLAVOURS = {"base": {}, "mask_as_bias": {"mask_as_bias": True}, "differential": {"differential": True}}


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


def main(batches=(256, 1), rounds=5, warmup=5, iters=40):
    import torch
    from hypervla import synthetic as syn
    from hypervla.config import FULL
    from hypervla.model import HyperVLA
    cap = max(batches)
    models = {}
    for name, kw in FLAVOURS.items():
        g = dataclasses.replace(FULL, **kw)
        m = HyperVLA.from_synthetic(g, max_batch=cap)
        ins, st = syn.synthetic_instructions(cap, g), syn.synthetic_initial_state(cap, g)
        li = {k: torch.as_tensor(v).to(m.device) for k, v in ins["language_instruction"].items()}
        pe = torch.as_tensor(st["patch_embeddings"]).to(m.device)
        tok = torch.randn(cap, g.patches, g.enc_dim, generator=torch.Generator().manual_seed(0)).to(m.device)
        models[name] = (m, li, pe, tok)
    res = {}
    for B in batches:
        ws = {name: m.create_tasks(instruction_dict={"language_instruction": {k: v[:B] for k, v in li.items()}},
                                   initial_state={"patch_embeddings": pe[:B]})[0] for name, (m, li, pe, tok) in models.items()}
        for rnd in range(rounds):
            for name, (m, li, pe, tok) in models.items():
                tokB, w = tok[:B].contiguous(), ws[name]
                r = {"round": rnd, "flavour": name, "B": B, "launches": iters,
                     "policy_ms": _timed(torch, lambda: m.policy_from_tokens(tokB, w), warmup, iters)}
                res.setdefault((name, B), []).append(r["policy_ms"])
                print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}), flush=True)
    for B in batches:
        base = res[("base", B)]
        out = {"B": B, "launches_per_flavour": rounds * iters,
               "base_spread": round((max(base) - min(base)) / statistics.median(base), 4)}
        for name in FLAVOURS:
            med = statistics.median(res[(name, B)])
            out[name + "_ms_median"] = round(med, 4)
            out[name + "_over_base"] = round(med / statistics.median(base), 4)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 1])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=40)
    a = ap.parse_args()
    main(tuple(a.batches), rounds=a.rounds, iters=a.iters)
