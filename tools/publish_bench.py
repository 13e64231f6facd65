"""Serving fine-tuned weights: the device route against the host route (README geometry, synthetic weights, train_encoder=True).

  device  FineTuner.publish(host_copy=False): hvla_train_publish packs the flat training vector into the serving buffers in place;
          timed with events on the stream, one event pair per repetition.
  host    what there was before: ft.params.cpu() -> unpack_params -> Context.load_weights on the context that already exists
          (device -> host copy, the single-thread host packer of csrc/serving_layout.h + pack.h, upload); wall clock around the
          synchronous calls, and around hvla_load_weights alone.

Next to each time: the bytes the device route moves (the vector read once, every serving buffer written once) divided by the
time, against this process's device-to-device copy rate (a torch copy of a buffer of the vector's size, read + write counted) and
the box's clock / matrix rate (hvla_box_probe).  Prints per-repetition times and one JSON line; `--out FILE` also writes the text."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "hyper-vla_amd"), ROOT]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 10:
        raise SystemExit("--reps >= 10")
    import torch
    from hypervla.config import FULL, hypernet_param_shapes
    from hypervla.model import HyperVLA
    from hypervla.train import FineTuner, unpack_params
    g = FULL
    m = HyperVLA.from_synthetic(g, max_batch=2)
    ft = FineTuner(m, 2, train_encoder=True)
    dev, lines = m.device, []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    clock, tflops, _ = m._ctx.box_probe(m._stream())
    # bytes of the device route: the vector once, and what hvla_load_weights allocates (every serving buffer) once
    E, Fe, S, C = g.enc_dim, g.enc_mlp, g.seq, g.ctx_dim
    kp = 2 * ((g.patch_in + 63) // 64 * 64)
    n16 = E * kp + g.enc_layers * (4 * E * E + 2 * E * Fe)
    nf = E + S * E + 2 * E + g.enc_layers * (11 * E + Fe)
    n_hyper_wo_heads = sum(int(np.prod(s)) for k, s in hypernet_param_shapes(g).items()
                           if not k.startswith("output_head_") and not k.startswith("encoder_image_encoder_"))
    gtot = m._ctx.num_generated                                 # (+ padding of the packed order, < 1 %)
    written = n_hyper_wo_heads * 4 + gtot * (C * 2 * 2 + 4) + n16 * 2 * 2 + nf * 4
    moved = ft.n * 4 + written

    src = torch.empty(ft.n, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)

    def event_ms(fn, reps):
        out = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1))
        return out

    event_ms(lambda: dst.copy_(src), 3)
    copy = event_ms(lambda: dst.copy_(src), a.reps)
    copy_rate = 2 * ft.n * 4 / (np.median(copy) * 1e-3) / 1e12
    del src, dst

    event_ms(lambda: ft.publish(host_copy=False), 3)
    device = event_ms(lambda: ft.publish(host_copy=False), a.reps)

    def host_route():
        t0 = time.perf_counter()
        flat = ft.params.cpu().numpy()
        params = dict(m._params)
        params.update(unpack_params(g, flat, True))
        t1 = time.perf_counter()
        m._ctx.load_weights({k: params[k] for k in hypernet_param_shapes(g)})
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        load.append((t2 - t1) * 1e3)
        return (t2 - t0) * 1e3

    load = []
    host_route()
    del load[:]
    host = [host_route() for _ in range(a.reps)]

    d, h = float(np.median(device)), float(np.median(host))
    say(f"box: {clock:.0f} MHz under load, {tflops:.0f} TFLOP/s dense fp16 (hvla_box_probe); device-to-device copy of {ft.n * 4 / 1e6:.0f} MB: "
        f"{np.median(copy):.3f} ms = {copy_rate:.2f} TB/s (read + write)")
    say(f"training vector {ft.n} floats ({ft.n * 4 / 1e6:.0f} MB), serving buffers {written / 1e6:.0f} MB: {moved / 1e6:.0f} MB moved per publish")
    say("device route  FineTuner.publish(host_copy=False), ms per repetition: " + " ".join(f"{x:.3f}" for x in device))
    say(f"              median {d:.3f} ms = {moved / (d * 1e-3) / 1e12:.2f} TB/s = {100 * moved / (d * 1e-3) / 1e12 / copy_rate:.0f} % of the copy rate")
    say("host route    params.cpu() -> unpack_params -> load_weights, ms per repetition: " + " ".join(f"{x:.0f}" for x in host))
    say(f"              median {h:.0f} ms = {moved / (h * 1e-3) / 1e9:.2f} GB/s")
    say("              of which hvla_load_weights (host packer + upload), ms: " + " ".join(f"{x:.0f}" for x in load) + f"; median {np.median(load):.0f}")
    say(f"device route is {h / d:.0f} x faster")
    res = dict(geometry="README", train_encoder=True, reps=a.reps, device_ms=round(d, 4), host_ms=round(h, 1), load_ms=round(float(np.median(load)), 1), speedup=round(h / d, 1),
               bytes_moved=int(moved), device_TBps=round(moved / (d * 1e-3) / 1e12, 3), copy_TBps=round(copy_rate, 3),
               clock_mhz=round(clock), mfma_tflops=round(tflops, 1))
    say(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if not d < h:
        raise SystemExit("the device route is not faster than the host route")


if __name__ == "__main__":
    main()
