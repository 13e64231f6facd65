"""CPU: adamw_kernel / adamw_shared_kernel (csrc/train.hip) restated line by line in numpy f32, six updates, against the float64 optax
restatement the GPU test uses (tests/adamw_ref.py) at the GPU test's tolerances -- so those tolerances are known to fit the kernel's
arithmetic before a device is involved, and the mutation `bc2 = 1 - pow(b2, t - 1)` is shown to fail them."""
import numpy as np
import pytest

from adamw_ref import bf16_round, optax_step

f = np.float32


def _kernel_f32(st, hy, t, sq, nh, bc2_t=None):
    """the device's update in f32, statement by statement; -> params, mu (bf16 values), nu, ema"""
    b1, b2, eps, d = f(hy["b1"]), f(hy["b2"]), f(hy["eps"]), f(hy["ema_decay"])
    norm = np.sqrt(f(sq))
    sc = f(1) if norm < f(hy["clip"]) else f(hy["clip"]) / norm
    bc1, bc2 = f(1) - f(np.power(b1, f(t))), f(1) - f(np.power(b2, f(t if bc2_t is None else bc2_t)))
    p, g, mu, nu, ema = (st[k].astype(f) for k in ("p", "g", "mu", "nu", "ema"))
    gi = g * sc
    m = b1 * mu + (f(1) - b1) * gi
    v = b2 * nu + (f(1) - b2) * gi * gi
    upd = (m / bc1) / (np.sqrt(v / bc2) + eps)
    lr = np.full(len(p), f(hy["lr"]), f)
    lr[nh:] = f(hy["base_lr"])
    dec = np.zeros(len(p), f)
    dec[:nh] = np.where(st["mask"][:nh] != 0, f(hy["weight_decay"]) * p[:nh], f(0))
    if len(p) > nh and hy["base_weight_decay"] > 0:
        bwd = f(hy["base_weight_decay"])
        dec[nh:] = np.where(st["mask"][nh:] != 0, bwd * p[nh:], f(0)) - bwd * st["p0"].astype(f)
    pn = p - lr * (upd + dec)
    return pn, bf16_round(m), v, d * ema + (f(1) - d) * pn


@pytest.mark.parametrize("clip,shared", [(1.0, False), (1e6, False), (1.0, True)])
def test_f32_kernel_restatement_meets_the_gpu_test_s_tolerances(clip, shared):
    rng = np.random.default_rng(5)
    nh, n = 60000, 100000 if shared else 60000
    hy = dict(b1=0.9, b2=0.999, eps=1e-8, weight_decay=0.05, clip=clip, ema_decay=0.999, base_weight_decay=0.01, lr=1e-3, base_lr=1e-3)
    p = rng.standard_normal(n).astype(f) * f(0.1)
    state = dict(p=p, mu=np.zeros(n, f), nu=np.zeros(n, f), ema=p.copy(), mask=(rng.random(n) < 0.5).astype(np.uint8), p0=p[nh:].copy())
    tol, gaps = 2e-6, []
    for t in range(1, 7):
        g = (rng.standard_normal(n) * np.exp(rng.standard_normal(n) * 3) * 0.05).astype(f)       # several decades of magnitudes
        st = {k: np.asarray(v, np.float64) if k != "mask" else v for k, v in state.items()}
        st["g"] = g.astype(np.float64)
        sq = f((st["g"] ** 2).sum())
        norm32 = np.sqrt(sq)
        sc = 1.0 if norm32 < f(clip) else float(f(clip) / norm32)
        assert (sc == 1.0) == (clip == 1e6)
        pn, mu, v, ema = _kernel_f32(st, hy, t, sq, nh)
        want = optax_step(st, hy, t, sc, nh)
        np.testing.assert_allclose(pn, want["p"], rtol=0, atol=tol)
        np.testing.assert_allclose(v, want["nu"], rtol=1e-6, atol=1e-37)
        np.testing.assert_allclose(ema, want["ema"], rtol=0, atol=tol)
        lo, hi = bf16_round(want["m"] - want["band"]), bf16_round(want["m"] + want["band"])
        assert ((mu >= np.minimum(lo, hi)) & (mu <= np.maximum(lo, hi))).all()
        assert (mu != bf16_round(want["m"])).mean() <= 1e-3
        if t > 1:
            prev = optax_step(st, hy, t - 1, sc, nh)
            gap = np.abs(pn - prev["p"]).max() - np.abs(pn - want["p"]).max()
            gaps.append(gap)
            assert gap >= 10 * tol, (t, gap)
            # the mutation: bc2 from t - 1 leaves the tolerance
            bad = _kernel_f32(st, hy, t, sq, nh, bc2_t=t - 1)[0]
            assert np.abs(bad - want["p"]).max() > 5 * tol, (t, np.abs(bad - want["p"]).max())
        state.update(p=pn, mu=mu.astype(f), nu=v, ema=ema)
    print("t vs t - 1 gaps:", gaps)
