"""return_attention_map on one MI355X: the README geometry with Geometry.mask_as_bias off and on, synthetic weights,
device-resident inputs, HIP-event timing.  Per batch size the policy alone (policy_from_tokens: policy_kernel against
policy_kernel_bias) and the full step (sample_actions from uint8 frames), the two models ALTERNATING `--rounds` times so that the box's
drift shows next to the difference; one JSON line per (round, flag, B), then per B the medians and the on / off ratio.

`--finetune B`: instead, ms per FineTuner.step (image encoder frozen: hvla_encode + forward + backward + AdamW) at batch B with the
flag off, on and off once more; one JSON line per run, then the on / off ratio and the drift of the two off runs."""
import argparse
import dataclasses
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "hyper-vla_amd"), ROOT]


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


def main(batches=(1, 256), rounds=3, warmup=3, iters=20):
    import torch
    from hypervla import synthetic as syn
    from hypervla.config import FULL
    from hypervla.model import HyperVLA
    cap = max(batches)
    models = {}
    for flag in (False, True):
        g = dataclasses.replace(FULL, mask_as_bias=flag)
        m = HyperVLA.from_synthetic(g, max_batch=cap)
        dev = m.device
        ins, st = syn.synthetic_instructions(cap, g), syn.synthetic_initial_state(cap, g)
        li = {k: torch.as_tensor(v).to(dev) for k, v in ins["language_instruction"].items()}
        pe = torch.as_tensor(st["patch_embeddings"]).to(dev)
        im = torch.as_tensor(syn.synthetic_images(cap, g)[:, 0]).to(dev).contiguous()
        tok = torch.randn(cap, g.patches, g.enc_dim, generator=torch.Generator().manual_seed(0)).to(dev)
        models[flag] = (m, li, pe, im, tok)
    res = {}
    for B in batches:
        ws = {}
        for flag, (m, li, pe, im, tok) in models.items():
            ws[flag] = m.create_tasks(instruction_dict={"language_instruction": {k: v[:B] for k, v in li.items()}},
                                      initial_state={"patch_embeddings": pe[:B]})[0]
        for rnd in range(rounds):
            for flag, (m, li, pe, im, tok) in models.items():
                imB, tokB, w = im[:B].contiguous(), tok[:B].contiguous(), ws[flag]
                r = {"round": rnd, "mask_as_bias": flag, "B": B,
                     "policy_ms": _timed(torch, lambda: m.policy_from_tokens(tokB, w), warmup, iters),
                     "step_ms": _timed(torch, lambda: m.sample_actions(imB, None, None, None, w), warmup, iters)}
                res.setdefault((flag, B), []).append(r)
                print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}), flush=True)
    for B in batches:
        out = {"B": B}
        for k in ("policy_ms", "step_ms"):
            off = [r[k] for r in res[(False, B)]]
            on = [r[k] for r in res[(True, B)]]
            out.update({k + "_off_median": round(statistics.median(off), 4), k + "_on_median": round(statistics.median(on), 4),
                        k.replace("_ms", "_on_over_off"): round(statistics.median(on) / statistics.median(off), 4),
                        k + "_off_spread": round((max(off) - min(off)) / statistics.median(off), 4)})
        print(json.dumps(out), flush=True)


def finetune(B, warmup=3, iters=20):
    import torch
    from hypervla import synthetic as syn
    from hypervla.config import FULL
    from hypervla.model import HyperVLA
    from hypervla.train import FineTuner
    ms = []
    for flag in (False, True, False):
        g = dataclasses.replace(FULL, mask_as_bias=flag)
        m = HyperVLA.from_synthetic(g, max_batch=B)
        dev = m.device
        ins, st, batch = syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g), syn.synthetic_action_batch(B, g)
        ins = {"language_instruction": {k: torch.as_tensor(v).to(dev) for k, v in ins["language_instruction"].items()}}
        im = torch.as_tensor(syn.synthetic_images(B, g)[:, 0]).to(dev).contiguous()
        ft = FineTuner(m, B)
        ms.append(_timed(torch, lambda: ft.step(ins, st, im, batch, lr=1e-4), warmup, iters))
        print(json.dumps({"finetune_step_ms": round(ms[-1], 3), "mask_as_bias": flag, "B": B, "train_encoder": False, "iters": iters}),
              flush=True)
        del ft, m
        torch.cuda.empty_cache()
    print(json.dumps({"B": B, "finetune_step_on_over_off": round(ms[1] / (0.5 * (ms[0] + ms[2])), 4),
                      "off_drift": round(ms[2] / ms[0], 4)}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 256])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--finetune", type=int, default=0, metavar="B", help="time FineTuner.step at this batch instead (flag off, on, off)")
    a = ap.parse_args()
    if a.finetune:
        finetune(a.finetune, iters=a.iters)
    else:
        main(tuple(a.batches), rounds=a.rounds, iters=a.iters)
