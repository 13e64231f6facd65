"""float64 restatement of one update of the reference's optimizer chain (shared by tests/test_gpu_train.py and its CPU companion
tests/test_adamw_reference.py)."""
import numpy as np


def bf16_round(x64):
    """float64 -> bfloat16 (round to nearest even) -> float64, through the f32 bit pattern."""
    u = np.asarray(x64, np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


def optax_step(st, hy, t, sc, nh):
    """One update of clip_by_global_norm -> scale_by_adam(mu_dtype=bf16) -> add_decayed_weights(mask) -> -lr in float64
    (octo/utils/train_utils.py:411-426; the shared group of multi_transform with its own lr, decay and the pull towards the
    pretrained leaves, scripts/train.py:465-471) from the state `st` read back from the device; `t` is the count used in the
    bias corrections, `sc` the clip scale.  b1, b2 and the EMA decay are the f32 values the C ABI carries."""
    b1, b2, d = (float(np.float32(hy[k])) for k in ("b1", "b2", "ema_decay"))
    gc = st["g"] * sc
    t1, t2 = b1 * st["mu"], (1 - b1) * gc
    m = t1 + t2
    v = b2 * st["nu"] + (1 - b2) * gc * gc
    upd = (m / (1 - b1 ** t)) / (np.sqrt(v / (1 - b2 ** t)) + hy["eps"])
    dec = np.where(st["mask"][:nh] != 0, hy["weight_decay"] * st["p"][:nh], 0.0)
    want = st["p"].copy()
    want[:nh] = st["p"][:nh] - hy["lr"] * (upd[:nh] + dec)
    if len(want) > nh:
        bwd = hy["base_weight_decay"]
        dec = np.where(st["mask"][nh:] != 0, bwd * st["p"][nh:], 0.0) - (bwd * st["p0"] if bwd > 0 else 0.0)
        want[nh:] = st["p"][nh:] - hy["base_lr"] * (upd[nh:] + (dec if bwd > 0 else 0.0))
    # each f32 rounding of the device's m (g sc, (1 - b1) x, b1 mu, the sum) is within 2^-24 relative of its own result
    band = 2.0 ** -24 * (np.abs(m) + np.abs(t1) + 2 * np.abs(t2))
    return dict(p=want, m=m, band=band, nu=v, ema=d * st["ema"] + (1 - d) * want)
