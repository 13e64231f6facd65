"""Fine-tuning use_differential_transformer on one MI355X: ms per FineTuner.step (image encoder frozen: hvla_encode +
forward + backward + AdamW) at batch B for MID and the README geometry, with Geometry.differential off and on.  Both models and
both tuners live in ONE process and ALTERNATE `--rounds` times, so that the box's drift shows next to the difference; synthetic
weights, device-resident inputs, HIP-event timing.  One JSON line per (geometry, round, flag), then per geometry the medians, the
on / off ratio and the spread of the flag-off rounds."""
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


def main(names=("MID", "FULL"), B=32, rounds=5, warmup=3, iters=10):
    import torch
    from hypervla import config, synthetic as syn
    from hypervla.model import HyperVLA
    from hypervla.train import FineTuner
    for name in names:
        steps = {}
        for flag in (False, True):
            g = dataclasses.replace(getattr(config, name), differential=flag)
            m = HyperVLA.from_synthetic(g, max_batch=B)
            dev = m.device
            ins, st, batch = syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g), syn.synthetic_action_batch(B, g)
            ins = {"language_instruction": {k: torch.as_tensor(v).to(dev) for k, v in ins["language_instruction"].items()}}
            im = torch.as_tensor(syn.synthetic_images(B, g)[:, 0]).to(dev).contiguous()
            ft = FineTuner(m, B, differential=flag)
            steps[flag] = (lambda ft=ft, ins=ins, st=st, im=im, batch=batch: ft.step(ins, st, im, batch, lr=1e-4), m, ft)
        ms = {False: [], True: []}
        for rnd in range(rounds):
            for flag in (False, True):
                ms[flag].append(_timed(torch, steps[flag][0], warmup, iters))
                print(json.dumps({"geometry": name, "round": rnd, "differential": flag, "B": B, "train_encoder": False,
                                  "finetune_step_ms": round(ms[flag][-1], 3), "iters": iters}), flush=True)
        off, on = statistics.median(ms[False]), statistics.median(ms[True])
        print(json.dumps({"geometry": name, "B": B, "finetune_step_ms_off_median": round(off, 3), "finetune_step_ms_on_median": round(on, 3),
                          "on_over_off": round(on / off, 4), "off_spread": round((max(ms[False]) - min(ms[False])) / off, 4),
                          "on_spread": round((max(ms[True]) - min(ms[True])) / on, 4)}), flush=True)
        del steps
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--geometries", nargs="+", default=["MID", "FULL"])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    main(tuple(a.geometries), B=a.batch, rounds=a.rounds, iters=a.iters)
