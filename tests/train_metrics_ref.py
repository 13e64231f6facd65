"""Float64 numpy restatements of every metric of hvla_train_metrics / hvla_loss_terms (include/hvla.h) from plain arrays: what the
reference's training loop logs (scripts/train.py:494-529) and its validation mse (:578-581).  Test infrastructure, like
tests/adamw_ref.py; nothing here reads the device or the library (masked_batch builds the tests' shared action batch)."""
import numpy as np

LOCAL_N = 7                                    # HVLA_METRIC_LOCAL_N: the rank-local block
(TRAINING_LOSS, CONTINUOUS_LOSS, GRIPPER_LOSS, MSE, BASE_PARAMS_NORM, ATTENTION_ENTROPY, ATTENTION_ALIGNMENT) = range(7)
GRAD_NORM, PARAM_NORM, UPDATE_NORM = 7, 8, 9   # + 2 n_tasks
N = 10
BOUND = 2.0 ** -23                             # f64 sums rounded once (2^-24), then one f64 sqrt cast (2^-24)


def masked_batch(g, B=5, rank=0):
    """hypervla.synthetic.synthetic_action_batch with sample 1's timestep mask off and every action of sample 3 masked: both mask
    means are zero there and the 1e-5 floor decides (the seeded batch need not contain either).  Samples 0, 2, 4 keep actions."""
    from hypervla import synthetic as syn
    batch = {k: np.array(v) for k, v in syn.synthetic_action_batch(B, g, rank).items()}
    batch["timestep_pad_mask"][:] = True
    batch["timestep_pad_mask"][1] = False
    batch["action_pad_mask"][3] = False
    batch["action_pad_mask"][[0, 2, 4], :, 0] = True
    return batch


def f64(a):
    return np.asarray(a, np.float64)


def loss_terms(pred, logits, target, timestep_mask, action_mask, max_action, clip_target=True):
    """(continuous [B], gripper [B]) of MixActionHead.loss (action_heads.py:474-522): pred [B, H, ad - 1] the continuous prediction,
    logits [B, H], target [B, H, ad], masks bool [B] and [B, H, ad].  masked_mean(x, m) = mean(x m) / max(mean(m), 1e-5)."""
    pred, logits, a = f64(pred), f64(logits), f64(target)
    if clip_target:
        a = np.clip(a, -max_action, max_action)
    m = (np.asarray(timestep_mask).astype(bool)[:, None, None] & np.asarray(action_mask).astype(bool)).astype(np.float64)
    mc, md = m[..., :-1], m[..., -1]
    ad = a.shape[-1]
    cont = ((pred - a[..., :-1]) ** 2 * mc).mean((1, 2)) / np.maximum(mc.mean((1, 2)), 1e-5) * (ad - 1)
    y = a[..., -1]
    sp = np.log1p(np.exp(-np.abs(logits)))
    bce = y * (np.maximum(-logits, 0.0) + sp) + (1.0 - y) * (np.maximum(logits, 0.0) + sp)
    grip = (bce * md).mean(1) / np.maximum(md.mean(1), 1e-5)
    return cont, grip


def sqerr(actions, target):
    """[B]: sum over (h, a) of (actions - clip(target, -5, 5))^2, unmasked; actions [B, H, ad] with the thresholded gripper column."""
    return ((f64(actions) - np.clip(f64(target), -5.0, 5.0)) ** 2).sum((1, 2))


def mse(actions, target):
    """`validation_action_loss`'s mse (scripts/train.py:580-581) = mean_b sqerr / horizon."""
    return sqerr(actions, target).mean() / np.shape(actions)[1]


def counted(n, frozen=None, slot=None):
    """bool [n]: the elements param_norm counts -- not frozen, not the baked position slot (a slice) while the source is on."""
    keep = np.ones(n, bool)
    if frozen is not None:
        keep &= ~np.asarray(frozen).astype(bool)
    if slot is not None:
        keep[slot] = False
    return keep


def grad_norm(grads):
    return float(np.sqrt((f64(grads) ** 2).sum()))


def param_norm(params, frozen=None, slot=None):
    return float(np.sqrt((f64(params)[counted(len(params), frozen, slot)] ** 2).sum()))


def update_norm(params, prev, slot=None):
    d = (f64(params) - f64(prev))[counted(len(params), None, slot)]
    return float(np.sqrt((d ** 2).sum()))


def encoder_sqsum(params, n_hyper, slot=None):
    """Sum of squares of the shared encoder leaves in a trained-encoder vector: [n_hyper, n) without the baked slot (the source tail
    stands for the table while the source is on)."""
    keep = counted(len(params), None, slot)
    keep[:n_hyper] = False
    return float((f64(params)[keep] ** 2).sum())


def base_params_norm(theta, enc_sq):
    return float(np.sqrt((f64(theta) ** 2).sum(1) + enc_sq).mean())


def task_sums(loss, task_ids, n_tasks):
    """(sums [n_tasks], counts [n_tasks]); an id outside [0, n_tasks) is counted nowhere."""
    loss, ids = f64(loss), np.asarray(task_ids)
    return (np.array([loss[ids == t].sum() for t in range(n_tasks)]), np.array([(ids == t).sum() for t in range(n_tasks)], np.float64))


def rel_err(got, want):
    return abs(float(got) - float(want)) / abs(float(want))
