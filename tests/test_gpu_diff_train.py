"""GPU: fine-tuning a use_differential_transformer model (FineTuner(differential=True), hvla_train_differential) -- one
step of the device against float64 autograd on the restatement (tests/diff_train_ref.py): per-sample loss and every gradient leaf.

Shapes.  MID: S = 65, row stride 68 (row padding; one 64-lane pass plus one lane), two layers, so two different lambda_init.  README
geometry: S = 257, five lane passes, an Sp - S tail of 3, four layers.

Bounds (tests/diff_train_ref.py): per-sample loss rtol 3e-4 / atol 3e-5 (tests/train_parity.py), every leaf max|d| / max(max|ref|,
1e-4 gmax) <= 2e-3 (DESIGN.md §20's fine-tune bound).  They stand because the float32 restatement of the same inputs is under a quarter
of them (tests/test_diff_train_host.py, which also checks on the reference alone that every lambda, subln and projection head is
above the metric's floor, that lambda spreads over a batch by >= 1.0, and that the restatements with lambda frozen at lambda_init and
with plain attention are hundreds of tolerances away).  Inputs: the synthetic checkpoint with the lambda heads x 5, continuous
targets x 0.1; no further sharpening was needed.

Measured on one MI355X (loss error as a fraction of its tolerance / worst leaf; float32 floor in parentheses): MID B = 4 0.058 / 4.1e-4
(0.0023 / 1.8e-5), README geometry B = 2 0.004 / 1.05e-3 (0.0047 / 7.2e-5), MID B = 2 with the trained encoder 0.050 / 1.27e-3
(0.0008 / 3.4e-5); published model: action mean 2.2e-5, max 7.2e-5, logit mean 2.6e-5."""
import ctypes
import functools
import gc

import numpy as np
import pytest

import diff_attention_ref as DR
import diff_train_ref as T
from train_parity import assert_not_vacuous, leaf_errors

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X; torch.cuda.is_available() is False")


def _rows(d, sl):
    return {"language_instruction": {k: np.asarray(v)[sl] for k, v in d["language_instruction"].items()}}


@functools.lru_cache(maxsize=None)
def _reference(name):
    """The float64 reference of a case, computed once and shared."""
    return T.case_reference(name)


def _model(name, max_batch=None):
    from hypervla.model import HyperVLA
    g, B, enc, params, ins, st, x, batch = T.case_inputs(name)
    return HyperVLA.from_synthetic(g, params=params, max_batch=max_batch or B), (g, B, enc, ins, st, x, batch)


def _parity_case(name):
    from hypervla.config import encoder_leaves
    from hypervla.train import FineTuner, unpack_params
    _need_gpu()
    per, grads, lam = _reference(name)
    model, (g, B, enc, ins, st, x, batch) = _model(name)
    ft = FineTuner(model, B, differential=True, train_encoder=enc)
    loss = ft.forward_backward(ins, st, x, batch).clone()
    got_loss = loss.cpu().numpy()
    got = unpack_params(g, ft.grads.cpu().numpy(), train_encoder=enc)
    assert set(got) == set(grads), set(got) ^ set(grads)
    rel, gmax = leaf_errors(got, grads)
    err = np.abs(got_loss - per.numpy())
    tol = T.LOSS_ATOL + T.LOSS_RTOL * np.abs(per.numpy())
    module = [(r, k) for r, k in rel if "DifferentialAttention_0" in k]
    print(f"{name} B={B} S={g.seq} encoder trained={enc}: per-sample loss error max {err.max():.2e} = {(err / tol).max():.3f} of its "
          f"tolerance (loss {per.numpy().min():.3f} .. {per.numpy().max():.3f}); worst leaves {[(f'{r:.2e}', k) for r, k in rel[:4]]}; "
          f"worst module heads {[(f'{r:.2e}', k) for r, k in module[:3]]}")
    above, n = assert_not_vacuous(grads, enc)
    heads = [k for k in grads if k.startswith("output_head_")]
    assert all(float(grads[k].abs().max()) > 1e-4 * gmax for k in heads)              # 100 % of the output heads are above the floor
    assert len(module) == 2 * 9 * g.layers
    np.testing.assert_allclose(got_loss, per.numpy(), rtol=T.LOSS_RTOL, atol=T.LOSS_ATOL)
    assert rel[0][0] <= T.LEAF_TOL, rel[:5]
    if enc:
        assert sum(k.startswith("encoder_image_encoder_") for _, k in rel) == len(encoder_leaves(g))
    # a forward-only step has bitwise the loss of the step (no atomics in the forward pass)
    fwd = ft.forward_backward(ins, st, x, batch, forward_only=True).clone()
    assert torch.equal(fwd, loss)
    del ft, model
    gc.collect()


def test_mid_frozen_encoder():
    """MID, B = 4, encoder frozen."""
    _parity_case("mid")


def test_readme_geometry_frozen_encoder():
    """README geometry, B = 2, encoder frozen."""
    _parity_case("full")


def test_mid_with_the_encoder_trained():
    """MID, B = 2, train_encoder=True: encoder leaves included."""
    _parity_case("mid_enc")


def test_a_sample_alone_is_bitwise_the_sample_in_the_batch_and_runs_repeat():
    """MID: sample 0 alone at B = 1 equals sample 0 of the B = 4 batch in its loss and its dtheta row; two runs of the same step are
    equal in loss, dtheta and theta (the per-episode sums dw and d lambda are reduced in a fixed order, no floating-point atomics)."""
    from hypervla.train import FineTuner
    _need_gpu()
    model, (g, B, enc, ins, st, x, batch) = _model("mid")
    ft = FineTuner(model, B, differential=True)
    loss = ft.forward_backward(ins, st, x, batch).clone()
    dtheta, theta = ft.dtheta.clone(), ft.theta.clone()
    loss2 = ft.forward_backward(ins, st, x, batch).clone()
    assert torch.equal(loss, loss2) and torch.equal(dtheta, ft.dtheta) and torch.equal(theta, ft.theta)
    one = FineTuner(model, 1, differential=True)
    sl = slice(0, 1)
    alone = one.forward_backward(_rows(ins, sl), {"patch_embeddings": np.asarray(st["patch_embeddings"])[sl]}, x[sl],
                                 {k: np.asarray(v)[sl] for k, v in batch.items()}).clone()
    assert torch.equal(alone[0], loss[0]), (float(alone[0]), float(loss[0]))
    # d mean_b loss_b / d theta_0 carries 1 / B: a power of two, so the row of the batch x B is bitwise the row alone
    assert torch.equal(one.dtheta[0], dtheta[0] * B)
    assert float(dtheta[0].abs().max()) > 0


def test_publish_serves_the_trained_differential_model():
    """MID: three step()s with metrics, validate(), publish(), then create_tasks + sample_actions on given frames: within §22's serving
    bounds (action mean 5e-4, max 2e-3, logit mean 2e-3) of diff_attention_ref on the TRAINED parameters; the un-trained parameters'
    restatement is more than ten bounds away, or the test asserts nothing."""
    from hypervla import synthetic as syn
    from hypervla.config import encoder_leaves
    from hypervla.train import FineTuner, unpack_params
    _need_gpu()
    model, (g, B, enc, ins, st, x, batch) = _model("mid")
    im = syn.synthetic_images(B, g)

    def served():
        w, tasks, _ = model.create_tasks(instruction_dict=ins, initial_state=st)
        act, inter = model.sample_actions(im, ins, tasks, None, w)
        return act, inter["gripper_logits"]

    before = served()
    ft = FineTuner(model, B, differential=True, metrics=True)
    ft.publish()
    for a, b in zip(before, served()):
        assert np.array_equal(a, b)                                 # a publish of untouched parameters changes no bit
    losses = [float(ft.step(ins, st, im, batch, lr=2e-3)) for _ in range(3)]
    info = {k: float(v) for k, v in ft.info().items()}
    assert np.isfinite(list(info.values())).all() and info["grad_norm"] > 0 and info["update_norm"] > 0, info
    mse = float(ft.validate(ins, st, im, batch)["mse"])
    assert np.isfinite(mse) and np.isfinite(losses).all()
    ft.publish()
    act, logit = served()
    params0 = T.case_params(g)                                      # (publish() refreshes the model's host copy)
    params = dict(model._params)
    params.update(unpack_params(g, ft.params.cpu().numpy()))
    moved = [k for k in params if "DifferentialAttention_0" in k and not np.array_equal(params[k], params0[k])]
    assert len(moved) == 2 * 9 * g.layers                           # every head of the module moved, the lambda and subln heads among them
    shapes = dict(encoder_leaves(g))
    ract, rlog, _ = DR.sample_actions(params, g, shapes, DR.create_tasks(params, g, ins, st), im)
    oact, olog, _ = DR.sample_actions(params0, g, shapes, DR.create_tasks(params0, g, ins, st), im)
    d, dl = np.abs(act[..., :6] - ract[..., :6]), np.abs(logit - rlog)
    away, away_l = np.abs(oact[..., :6] - ract[..., :6]), np.abs(olog - rlog)
    print("published differential model after 3 steps (losses %s, validation mse %.4f): action MAE %.3e max %.3e, logit mean %.3e; "
          "the un-trained restatement is %.3e (mean) / %.3e (max) away in the actions, %.3e (mean) in the logits"
          % (np.round(losses, 4), mse, d.mean(), d.max(), dl.mean(), away.mean(), away.max(), away_l.mean()))
    assert away.mean() > 10 * 5e-4 and away.max() > 10 * 2e-3 and away_l.mean() > 10 * 2e-3
    assert d.mean() <= 5e-4 and d.max() <= 2e-3 and dl.mean() <= 2e-3


def test_c_entries_on_contexts_of_this_test():
    """hvla_train_differential: refused with a text on a plain context; on a differential context hvla_train_sizes is refused by
    default, succeeds after (ctx, 1) and is refused again after (ctx, 0); values other than 0 / 1 are refused and leave the setting;
    hvla_train_attention_losses with a non-zero coefficient and hvla_train_noise_set with a non-zero rate are refused with a text."""
    from hypervla import _native
    from hypervla.config import MID
    _need_gpu()
    lib = _native.load_library()
    err = lambda c: lib.hvla_last_error(c.h).decode()
    out = (ctypes.c_int64 * 4)()
    plain = _native.Context(MID, max_batch=2)
    assert lib.hvla_train_differential(plain.h, 1) == -1 and "differential_attention" in err(plain)
    assert lib.hvla_train_differential(plain.h, 0) == 0
    assert lib.hvla_train_sizes(plain.h, 2, 0, out) == 0
    plain_sizes = list(out)
    plain.close()
    g = T.case_geometry("mid")
    ctx = _native.Context(g, max_batch=2)
    assert lib.hvla_train_sizes(ctx.h, 2, 0, out) == -1 and "use_differential_transformer" in err(ctx)
    assert lib.hvla_train_publish(ctx.h, None, 0, 0, None) == -1
    assert lib.hvla_train_differential(ctx.h, 1) == 0
    assert lib.hvla_train_sizes(ctx.h, 2, 0, out) == 0
    from hypervla.train import train_param_layout
    from hypervla.config import generated_leaves
    assert out[0] == out[3] == train_param_layout(g)[1] and out[1] == generated_leaves(g)[-1].offset + generated_leaves(g)[-1].size
    assert out[2] > plain_sizes[2]                                  # the 2 H tables and what the backward keeps
    for bad in (2, -1):
        assert lib.hvla_train_differential(ctx.h, bad) == -1 and "0 or 1" in err(ctx)
    assert lib.hvla_train_sizes(ctx.h, 2, 0, out) == 0              # ... and the setting stayed
    att = _native.hvla_train_attention()
    att.struct_size = ctypes.sizeof(_native.hvla_train_attention)
    att.entropy_weight = 0.1
    assert lib.hvla_train_attention_losses(ctx.h, ctypes.byref(att)) == -1 and "differential_attention" in err(ctx)
    att.entropy_weight = 0.0
    assert lib.hvla_train_attention_losses(ctx.h, ctypes.byref(att)) == 0
    with pytest.raises(_native.NativeError, match="differential_attention"):
        ctx.train_noise(seed=1, sample_offset=0, draw=0, policy_dropout=0.1, image_embedding_noise=0.0, context_dropout=0.0, image_dropout=0.0)
    ctx.train_noise(off=True)
    assert lib.hvla_train_differential(ctx.h, 0) == 0
    assert lib.hvla_train_sizes(ctx.h, 2, 0, out) == -1 and "use_differential_transformer" in err(ctx)
    ctx.close()
