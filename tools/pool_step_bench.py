"""Episode pool step against a plain step (README geometry, synthetic weights): sample_actions(slots=K slots of a 256-slot pool)
vs sample_actions of a batch-K arena, K in {1, 64, 256}, device-resident frames, HIP-event timing.  One JSON line per K."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "hyper-vla_amd"), ROOT]


def main(cap=256, ks=(1, 64, 256), warmup=3, iters=10):
    import torch
    from hypervla import synthetic as syn
    from hypervla.config import FULL
    from hypervla.model import HyperVLA
    g = FULL
    m = HyperVLA.from_synthetic(g, max_batch=cap)
    ins, st = syn.synthetic_instructions(cap, g), syn.synthetic_initial_state(cap, g)
    im = torch.as_tensor(syn.synthetic_images(cap, g)[:, 0]).to(m.device).contiguous()
    pool, _, _ = m.create_tasks(instruction_dict=ins, initial_state=st)

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

    rng = np.random.default_rng(0)
    for K in ks:
        slots = np.sort(rng.permutation(cap)[:K])
        img = im[:K].contiguous()
        w, _, _ = m.create_tasks(instruction_dict={"language_instruction": {k: v[:K] for k, v in ins["language_instruction"].items()}},
                                 initial_state={"patch_embeddings": st["patch_embeddings"][:K]})
        plain = timed(lambda: m.sample_actions(img, None, None, None, w))
        pooled = timed(lambda: m.sample_actions(img, None, None, None, pool, slots=slots))
        print(json.dumps({"K": K, "pool": cap, "plain_ms": round(plain, 4), "slots_ms": round(pooled, 4),
                          "ratio": round(pooled / plain, 4)}), flush=True)


if __name__ == "__main__":
    main()
