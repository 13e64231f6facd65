"""hypernet_kwargs.share_layer_index=False on one MI355X: `create_tasks` (context encoder + weight generation, the call
as a caller sees it, its stream synchronisation included) at the README geometry for `layer_tokens` off (ctx_encoder_kernel +
weightgen_kernel), on (ctx_encoder_kernel_tokens + weightgen_tokens_kernel) and on with `shared_block_heads`, on synthetic weights
and device-resident inputs, HIP-event timing.  The flavours ALTERNATE `--rounds` times in one process on one box, `--iters` calls per
timing after a warm-up, so that the box's drift shows next to the differences; one JSON line per (round, flavour, B), then per B the
medians, the ratio to `off` and the spread of `off` over the rounds.  `--flavours off` times the unchanged path alone (it then also
runs on a tree from before the flag, for the comparison with the parent commit on the same box)."""
import argparse
import dataclasses
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "hyper-vla_amd"), ROOT]

FLAVOURS = {"off": {}, "on": {"layer_tokens": True}, "on_shared_heads": {"layer_tokens": True, "shared_block_heads": True}}


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


def main(batches=(256, 1), rounds=5, warmup=5, iters=40, flavours=tuple(FLAVOURS)):
    import torch
    from hypervla import synthetic as syn
    from hypervla.config import FULL
    from hypervla.model import HyperVLA
    cap = max(batches)
    models = {}
    for name in flavours:
        g = dataclasses.replace(FULL, enc_layers=1, **FLAVOURS[name])      # (the image encoder is not run: one layer keeps the load short)
        m = HyperVLA.from_synthetic(g, max_batch=cap)
        ins, st = syn.synthetic_instructions(cap, g), syn.synthetic_initial_state(cap, g)
        li = {k: torch.as_tensor(v).to(m.device) for k, v in ins["language_instruction"].items()}
        pe = torch.as_tensor(st["patch_embeddings"]).to(m.device)
        models[name] = (m, li, pe)
    res = {}
    for B in batches:
        for rnd in range(rounds):
            for name, (m, li, pe) in models.items():
                ins, st = {"language_instruction": {k: v[:B] for k, v in li.items()}}, {"patch_embeddings": pe[:B]}
                r = {"round": rnd, "flavour": name, "B": B, "calls": iters,
                     "create_tasks_ms": _timed(torch, lambda: m.create_tasks(instruction_dict=ins, initial_state=st), warmup, iters)}
                res.setdefault((name, B), []).append(r["create_tasks_ms"])
                print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}), flush=True)
    for B in batches:
        base = res[(flavours[0], B)]
        out = {"B": B, "calls_per_flavour": rounds * iters,
               flavours[0] + "_spread": round((max(base) - min(base)) / statistics.median(base), 4)}
        for name in flavours:
            med = statistics.median(res[(name, B)])
            out[name + "_ms_median"] = round(med, 4)
            out[name + "_over_" + flavours[0]] = round(med / statistics.median(base), 4)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 1])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--flavours", nargs="+", default=list(FLAVOURS), choices=list(FLAVOURS))
    a = ap.parse_args()
    main(tuple(a.batches), rounds=a.rounds, iters=a.iters, flavours=tuple(a.flavours))
