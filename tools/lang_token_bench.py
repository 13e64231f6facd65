"""use_language_token on one MI355X: the README geometry with the flag off and on, synthetic weights, device-resident
inputs, HIP-event timing.  Per batch size: the policy alone (policy_from_tokens), the full step (sample_actions from uint8 frames) and
create_tasks (context encoder + weight generation, + lang_prefix_kernel with the flag on).  One JSON line per (flag, B), then one per B
with the on / off ratios.  `rocprofv3 --kernel-trace --stats -- python tools/lang_token_bench.py` gives lang_prefix_kernel's own time.

`--finetune B`: instead, ms per FineTuner.step (image encoder frozen: hvla_encode + forward + backward + AdamW) at the README geometry
and batch B with the flag off, on (FineTuner(language_tokens=True): the policy on T + P + 1 = 289 rows instead of 257) and off once
more for the box's drift; one JSON line per run, then the on / off ratio next to (Sx / S)^2, the growth of the attention products."""
import argparse
import dataclasses
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "hyper-vla_amd"), ROOT]


def main(batches=(1, 256), warmup=3, iters=20):
    import torch
    from hypervla import synthetic as syn
    from hypervla.config import FULL
    from hypervla.model import HyperVLA

    def timed(fn):
        for _ in range(warmup):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / iters

    cap = max(batches)
    res = {}
    for flag in (False, True):
        g = dataclasses.replace(FULL, lang_in_policy=flag)
        m = HyperVLA.from_synthetic(g, max_batch=cap)
        dev = m.device
        ins, st = syn.synthetic_instructions(cap, g), syn.synthetic_initial_state(cap, g)
        li = {k: torch.as_tensor(v).to(dev) for k, v in ins["language_instruction"].items()}
        pe = torch.as_tensor(st["patch_embeddings"]).to(dev)
        im = torch.as_tensor(syn.synthetic_images(cap, g)[:, 0]).to(dev).contiguous()
        tok = torch.randn(cap, g.patches, g.enc_dim, generator=torch.Generator().manual_seed(0)).to(dev)
        for B in batches:
            insB = {"language_instruction": {k: v[:B] for k, v in li.items()}}
            stB = {"patch_embeddings": pe[:B]}
            w, _, _ = m.create_tasks(instruction_dict=insB, initial_state=stB)
            imB, tokB = im[:B].contiguous(), tok[:B].contiguous()
            r = {"lang_in_policy": flag, "B": B,
                 "policy_ms": timed(lambda: m.policy_from_tokens(tokB, w)),
                 "step_ms": timed(lambda: m.sample_actions(imB, None, None, None, w)),
                 "create_tasks_ms": timed(lambda: m.create_tasks(instruction_dict=insB, initial_state=stB))}
            res[(flag, B)] = r
            print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}), flush=True)
            del w
        del m
        torch.cuda.empty_cache()
    for B in batches:
        off, on = res[(False, B)], res[(True, B)]
        print(json.dumps({"B": B, **{k.replace("_ms", "_on_over_off"): round(on[k] / off[k], 4)
                                     for k in ("policy_ms", "step_ms", "create_tasks_ms")},
                          "create_tasks_extra_ms": round(on["create_tasks_ms"] - off["create_tasks_ms"], 4)}), flush=True)


def finetune(B, warmup=3, iters=20):
    import torch
    from hypervla import synthetic as syn
    from hypervla.config import FULL
    from hypervla.model import HyperVLA
    from hypervla.train import FineTuner
    ms = []
    for flag in (False, True, False):
        g = dataclasses.replace(FULL, lang_in_policy=flag)
        m = HyperVLA.from_synthetic(g, max_batch=B)
        dev = m.device
        ins, st, batch = syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g), syn.synthetic_action_batch(B, g)
        ins = {"language_instruction": {k: torch.as_tensor(v).to(dev) for k, v in ins["language_instruction"].items()}}
        im = torch.as_tensor(syn.synthetic_images(B, g)[:, 0]).to(dev).contiguous()
        ft = FineTuner(m, B, language_tokens=flag)
        for _ in range(warmup):
            ft.step(ins, st, im, batch, lr=1e-4)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            ft.step(ins, st, im, batch, lr=1e-4)
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / iters)
        print(json.dumps({"finetune_step_ms": round(ms[-1], 3), "lang_in_policy": flag, "B": B, "policy_rows": g.policy_seq,
                          "train_encoder": False, "iters": iters}), flush=True)
        del ft, m
        torch.cuda.empty_cache()
    S, Sx = FULL.seq, FULL.seq + FULL.lang_tokens
    print(json.dumps({"B": B, "finetune_step_on_over_off": round(ms[1] / (0.5 * (ms[0] + ms[2])), 4), "off_drift": round(ms[2] / ms[0], 4),
                      "attention_growth_(Sx/S)^2": round((Sx / S) ** 2, 4)}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 256])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--finetune", type=int, default=0, metavar="B", help="time FineTuner.step at this batch instead (flag off, on, off)")
    a = ap.parse_args()
    if a.finetune:
        finetune(a.finetune, iters=a.iters)
    else:
        main(tuple(a.batches), iters=a.iters)
