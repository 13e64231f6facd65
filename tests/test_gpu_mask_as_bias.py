"""GPU: vit_kwargs.return_attention_map (Geometry.mask_as_bias) -- policy_kernel_bias / policy_kernel_slots_bias and the
train step's softmax_bias_fwd_kernel against the float64 restatement (tests/mask_bias_ref.py).

Serving bounds are those of tests/test_gpu_language_tokens.py: README geometry from given tokens, actions max 1e-3 and gripper logits
1.5e-3; MID end to end from uint8 frames, action mean 5e-4, max 2e-3, head map 1e-3.  On the same inputs the restatement of the masked
model is 5 and more of these tolerances away (tests/test_mask_as_bias_host.py), so a kernel that masked would fail them.

Fine-tune bounds are those of tests/test_gpu_train.py and tests/test_gpu_attention_losses.py: per-sample loss rtol 2e-4 / atol 2e-5,
every leaf max|d| / max(max|ref|, 1e-4 gmax) <= 2e-3 (the policy's key-bias heads, whose true gradient is zero, are held to that floor).

Inputs of the fine-tune cases.  On the synthetic checkpoint as it is, masked against additive moves the per-sample losses by at most
0.09 of 100 tolerances and the hypernetwork gradient by 1 % of its norm (float64, CPU), and scaling the action row of pos_embedding
(factors 0.03 .. 30) does not change that: the action token's first LayerNorm removes the scale.  So the cases sharpen the policy's
attention instead, on the checkpoint alone: every `..._query_{kernel,bias}` output head x 10 (MID; x 2 at the README geometry, whose
four layers need less and get steep sooner: there the f32 step's relative loss error, masked or additive alike, grows from 1e-5 as
the checkpoint is to 1.1e-4 / 1.7e-4 at x 3 and 1e-3 / 8e-4 at x 10, past the tolerance by the input's conditioning alone) and
every `..._value_{kernel,bias}` head x 3 (the generated q and v scale by exactly these factors), and the continuous targets x 0.1
(smaller losses, smaller tolerances).
Each case first asserts on the restatements alone (a) ||g_additive - g_masked|| / ||g_masked|| >= 0.05 over the hypernetwork leaves and
(b) a per-sample loss that moves by >= 100 x its tolerance, 100 x (2e-5 + 2e-4 |loss_b|): the loss check compares the vector of
per-sample losses, so one such sample makes a masked step fail it by that factor.  Measured (moved / (100 tol) per sample; ratio):
    README geometry, B = 2, batch seed 0          0.19, 1.60             0.145
    MID, B = 4, batch seed 2                      0.70, 0.00, 0.04, 1.76 0.134
    MID, B = 4, terms (3, 6000), batch seed 9     0.98, 0.00, 0.01, 1.17 0.056
    MID, B = 2, trained encoder, x 6, seed 0      0.20, 2.24             0.131      (x 10: the loss error is 2.09e-4 relative)
(MID's episode 1 hardly tells the two models apart at any setting tried.)

Measured on one MI355X: README geometry action max 3.8e-5, logit 4.4e-5; MID end to end action max 2.1e-4, head map 2.4e-5; fine-tune
loss error / worst leaf 8.0e-4 / 4.9e-4 (MID), 6.0e-3 / 1.1e-3 (MID with the terms, losses 33.6-39.4: 0.9 of the loss tolerance, a
forward pass without atomics), 4.4e-4 / 8.6e-4 (README geometry), 5.5e-4 / 2.9e-4 (trained encoder)."""
import ctypes
import dataclasses
import gc

import numpy as np
import pytest

import mask_bias_ref as MB
from train_parity import assert_not_vacuous, leaf_errors

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LOSS_RTOL, LOSS_ATOL, LEAF_TOL = 2e-4, 2e-5, 2e-3
QUERY_X, QUERY_X_FULL, QUERY_X_ENC, VALUE_X, TARGET_X = 10.0, 2.0, 6.0, 3.0, 0.1
TERMS = (3.0, 6000.0)
NUM_STEPS = 1000                                        # at step_count 0 the annealed alignment weight is the coefficient itself


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X; torch.cuda.is_available() is False")


def _geo(name):
    from hypervla import config
    return dataclasses.replace(getattr(config, name), mask_as_bias=True)


def _rows(d, sl):
    return {"language_instruction": {k: np.asarray(v)[sl] for k, v in d["language_instruction"].items()}}


# ------------------------------------------------------------------------------------------------------------- serving
@pytest.fixture(scope="module")
def full():
    _need_gpu()
    from hypervla import synthetic as syn
    from hypervla.model import HyperVLA
    g, B = _geo("FULL"), 4
    m = HyperVLA.from_synthetic(g, max_batch=B)
    ins, st = syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g)
    tok = np.random.default_rng(3).standard_normal((B, g.patches, g.enc_dim)).astype(np.float32)
    w, _, _ = m.create_tasks(instruction_dict=ins, initial_state=st)
    act, logit = (t.cpu().numpy() for t in m.policy_from_tokens(tok, w))
    yield dict(g=g, m=m, B=B, ins=ins, st=st, tok=tok, act=act, logit=logit)
    gc.collect()


@pytest.fixture(scope="module")
def mid():
    _need_gpu()
    from hypervla import synthetic as syn
    from hypervla.model import HyperVLA
    g, cap = _geo("MID"), 8
    m = HyperVLA.from_synthetic(g, max_batch=cap)
    yield dict(g=g, m=m, cap=cap, P=syn.synthetic_params(g), ins=syn.synthetic_instructions(cap, g),
               st=syn.synthetic_initial_state(cap, g), im=syn.synthetic_images(cap, g))
    gc.collect()


def test_full_geometry_from_tokens(full):
    """README geometry, B = 4 (policy_kernel_bias<8>): theta in the variant's leaf order, actions and gripper logits."""
    from hypervla.config import generated_leaves
    m, g, B = full["m"], full["g"], full["B"]
    bp = MB.create_tasks(m.params, g, full["ins"], full["st"])
    w, _, _ = m.create_tasks(instruction_dict=full["ins"], initial_state=full["st"])
    theta = w.export()[0].cpu().numpy().astype(np.float64)
    ref = np.concatenate([bp[l.flat_name].reshape(B, -1) for l in generated_leaves(g)], 1)
    assert theta.shape == ref.shape and np.abs(theta - ref).max() <= 1e-4
    ract, rlog, _ = MB.policy(bp, g, full["tok"].astype(np.float64))
    mact, mlog, _ = MB.policy(bp, g, full["tok"].astype(np.float64), "masked")
    d, dl = np.abs(full["act"][..., :6] - ract[..., :6]), np.abs(full["logit"] - rlog)
    dm, dlm = np.abs(full["act"][..., :6] - mact[..., :6]), np.abs(full["logit"] - mlog)
    print("README return_attention_map B=%d from tokens: action max %.3e MAE %.3e, logit max %.3e; against the masked restatement "
          "%.3e, %.3e" % (B, d.max(), d.mean(), dl.max(), dm.max(), dlm.max()))
    assert d.max() <= 1e-3 and dl.max() <= 1.5e-3, (d.max(), dl.max())
    safe = np.abs(rlog) > 2e-3
    assert (full["act"][..., 6][safe] == ract[..., 6][safe]).all()
    assert dm.max() > 4e-3 and dlm.max() > 6e-3                 # 5 tolerances between the restatements, less this side's own error


def test_mid_end_to_end_from_frames_and_head_maps(mid):
    """MID, B = 4 (policy_kernel_bias<2>) from uint8 frames, with the head maps [B, L, H, P]: the action token's row of every layer."""
    from hypervla.config import encoder_leaves
    m, g, B = mid["m"], mid["g"], 4
    ins, st, im = _rows(mid["ins"], slice(0, B)), {"patch_embeddings": mid["st"]["patch_embeddings"][:B]}, mid["im"][:B]
    w, tasks, _ = m.create_tasks(instruction_dict=ins, initial_state=st)
    act, inter = m.sample_actions(im, ins, tasks, np.ones((B, 1)), w, attention_maps=True)
    bp = MB.create_tasks(mid["P"], g, ins, st)
    ract, rlog, head, tok = MB.sample_actions(mid["P"], g, dict(encoder_leaves(g)), bp, im)
    mact, _, mhead = MB.policy(bp, g, tok, "masked")
    d, dl = np.abs(act[..., :6] - ract[..., :6]), np.abs(inter["gripper_logits"] - rlog)
    dh = np.abs(inter["head_attention"] - head)
    print("MID return_attention_map end to end: action MAE %.3e max %.3e, logit max %.3e, head map max %.2e (max weight %.2e); "
          "the masked restatement is %.3e away in the actions, %.2e in the maps"
          % (d.mean(), d.max(), dl.max(), dh.max(), head.max(), np.abs(ract[..., :6] - mact[..., :6]).max(), np.abs(head - mhead).max()))
    assert d.mean() <= 5e-4 and d.max() <= 2e-3 and dl.mean() <= 2e-3, (d.mean(), d.max(), dl.mean())
    assert inter["head_attention"].shape == head.shape == (B, g.layers, g.heads, g.patches)
    assert dh.max() <= 1e-3
    assert np.abs(act[..., :6] - mact[..., :6]).max() > 5 * 2e-3 - 2e-3


def test_batch_of_one_rows_equal_the_batch_s_and_runs_repeat(full):
    m = full["m"]
    for b in range(full["B"]):
        w1, _, _ = m.create_tasks(instruction_dict=_rows(full["ins"], slice(b, b + 1)),
                                  initial_state={"patch_embeddings": full["st"]["patch_embeddings"][b:b + 1]})
        a1, l1 = (t.cpu().numpy() for t in m.policy_from_tokens(full["tok"][b:b + 1], w1))
        assert np.array_equal(a1[0], full["act"][b]) and np.array_equal(l1[0], full["logit"][b]), b
    for _ in range(3):
        w2, _, _ = m.create_tasks(instruction_dict=full["ins"], initial_state=full["st"])
        a2, l2 = (t.cpu().numpy() for t in m.policy_from_tokens(full["tok"], w2))
        assert np.array_equal(a2, full["act"]) and np.array_equal(l2, full["logit"])


def test_pool_scattered_slots_equal_a_full_batch_step(mid):
    """assign_tasks into scattered slots of a pool (policy_kernel_slots_bias): bitwise the rows of a full-batch step, maps included."""
    m, cap = mid["m"], mid["cap"]
    w, tasks, _ = m.create_tasks(instruction_dict=mid["ins"], initial_state=mid["st"])
    act, inter = m.sample_actions(mid["im"], mid["ins"], tasks, None, w, attention_maps=True)
    perm = np.random.default_rng(4).permutation(cap).tolist()
    pool = m.create_pool(cap)
    m.assign_tasks(pool, perm, mid["ins"], mid["st"])             # episode k -> slot perm[k]
    K = 5
    a, it = m.sample_actions(mid["im"][:K], None, None, None, pool, attention_maps=True, slots=perm[:K])
    np.testing.assert_array_equal(a, act[:K])
    for k in ("gripper_logits", "head_attention"):
        np.testing.assert_array_equal(it[k], inter[k][:K])
    a1, _ = m.sample_actions(mid["im"][6:7], None, None, None, pool, slots=[perm[6]])
    np.testing.assert_array_equal(a1[0], act[6])


def test_create_with_v2_with_the_field_zero_is_create():
    """hvla_create(cfg) == hvla_create_with_v2(cfg, {size, 0, 0}): the same bytes on the default geometry, theta, actions and maps."""
    _need_gpu()
    from hypervla import _native, synthetic as syn
    from hypervla.config import MID
    from hypervla.model import HyperVLA
    g, B = MID, 3
    ins, st, im = syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g), syn.synthetic_images(B, g)
    outs = []
    lib = _native.load_library()
    orig = lib.hvla_create
    zero = _native.hvla_policy_options_v2(ctypes.sizeof(_native.hvla_policy_options_v2), 0, 0)
    for route in ("create", "create_with_v2", "create_with_v2 NULL"):
        if route != "create":
            lib.hvla_create = lambda cfg, dev, h: lib.hvla_create_with_v2(cfg, ctypes.byref(zero) if route == "create_with_v2" else None, dev, h)
        try:
            m = HyperVLA.from_synthetic(g, max_batch=4)
        finally:
            lib.hvla_create = orig
        w, t, _ = m.create_tasks(instruction_dict=ins, initial_state=st)
        a, inter = m.sample_actions(im, ins, t, None, w, attention_maps=True)
        outs.append((w.export()[0].cpu().numpy(), a, inter["head_attention"]))
        del w, m
    for other in outs[1:]:
        for x, y in zip(outs[0], other):
            assert np.array_equal(x, y)


def test_the_combination_with_use_language_token_is_refused_with_a_text():
    _need_gpu()
    from hypervla import _native
    from hypervla.config import MID
    lib = _native.load_library()
    ctx = _native.Context(MID, max_batch=1)                       # (a valid hvla_config of this device)
    opt = _native.hvla_policy_options_v2(ctypes.sizeof(_native.hvla_policy_options_v2), 1, 1)
    h = ctypes.c_void_p()
    assert lib.hvla_create_with_v2(ctypes.byref(ctx.cfg), ctypes.byref(opt), 0, ctypes.byref(h)) == -1 and not h.value
    assert b"use_language_token" in lib.hvla_last_error(None)
    ctx.close()


# ------------------------------------------------------------------------------------------------------------- fine-tuning
def _sharpened(params, query_x):
    """The checkpoint with the policy's attention sharpened (module docstring): query heads x query_x, value heads x 3."""
    out = dict(params)
    for k, v in params.items():
        if k.startswith("output_head_") and "Attention_0_query_" in k:
            out[k] = (v * np.float32(query_x)).astype(np.float32)
        elif k.startswith("output_head_") and "Attention_0_value_" in k:
            out[k] = (v * np.float32(VALUE_X)).astype(np.float32)
    return out


def _hyper_norm(grads):
    return np.sqrt(sum(float((v.double() ** 2).sum()) for k, v in grads.items() if not k.startswith("encoder_image_encoder_")))


def _tells_apart(ref, masked):
    """Conditions (a) and (b) of the module docstring on the two restatements: ref / masked = (per, ent, align, grads)."""
    d = {k: ref[3][k] - masked[3][k] for k in ref[3]}
    ratio = _hyper_norm(d) / _hyper_norm(masked[3])
    moved = (ref[0] - masked[0]).abs().numpy()
    need = 100 * (LOSS_ATOL + LOSS_RTOL * ref[0].abs().numpy())
    print(f"restatements: |g_additive - g_masked| / |g_masked| = {ratio:.3f}; losses moved by {moved}, 100 tolerances are {need}")
    assert ratio >= 0.05, ratio
    assert (moved / need).max() >= 1.0, (moved, need)


def _finetune_case(g, B, seed, w=(0.0, 0.0), train_encoder=False, query_x=QUERY_X):
    """One step of a flag-on FineTuner against float64 autograd: per-sample loss, the two terms' metrics, every leaf, the policy's
    key-bias heads, and every sample alone (B = 1) bitwise the sample in the batch."""
    import attention_loss_ref as AR
    from hypervla import synthetic as syn
    from hypervla.config import encoder_leaves, generated_leaves
    from hypervla.model import HyperVLA
    from hypervla.train import FineTuner, unpack_params
    _need_gpu()
    model = HyperVLA.from_synthetic(g, params=_sharpened(syn.synthetic_params(g), query_x), max_batch=B)
    leaves = generated_leaves(g)
    ins, st = syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g)
    batch = syn.synthetic_action_batch(B, g, seed)
    batch["action"][..., :-1] *= TARGET_X
    r = AR.synthetic_reference_map(B, g.patches) if w[1] else None
    if train_encoder:
        x, params, kw = syn.synthetic_images(B, g), model.params, dict(images=syn.synthetic_images(B, g), enc_shapes=dict(encoder_leaves(g)))
        tok = None
    else:
        tok = x = np.random.default_rng(9).standard_normal((B, g.patches, g.enc_dim)).astype(np.float32)
        params, kw = {k: v for k, v in model.params.items() if not k.startswith("encoder_image_encoder_")}, {}
    ref = MB.train_loss_and_grads(params, g, leaves, ins, st, tok, batch, w[0], w[1], r, mode="bias", **kw)
    masked = MB.train_loss_and_grads(params, g, leaves, ins, st, tok, batch, w[0], w[1], r, mode="masked", **kw)
    _tells_apart(ref, masked)
    per, grads = ref[0].numpy(), ref[3]

    tkw = dict(train_encoder=True) if train_encoder else {}
    if w[0] or w[1]:
        tkw.update(attention_entropy=w[0], attention_map_alignment=w[1], num_steps=NUM_STEPS if w[1] else None)
    fkw = dict(reference_attention=r) if w[1] else {}
    ft = FineTuner(model, B, **tkw)
    loss = ft.forward_backward(ins, st, x, batch, **fkw).clone()
    got_loss = loss.cpu().numpy()
    err = np.abs(got_loss - per)
    np.testing.assert_allclose(got_loss, per, rtol=LOSS_RTOL, atol=LOSS_ATOL)
    assert not np.allclose(got_loss, masked[0].numpy(), rtol=LOSS_RTOL, atol=LOSS_ATOL)
    if w[0]:
        np.testing.assert_allclose(ft.aux_metrics["attention_entropy_loss"].cpu().numpy(), ref[1].numpy(), rtol=LOSS_RTOL, atol=LOSS_ATOL)
    if w[1]:
        np.testing.assert_allclose(ft.aux_metrics["attention_alignment_loss"].cpu().numpy(), ref[2].numpy(), rtol=LOSS_RTOL, atol=LOSS_ATOL)
    got = unpack_params(g, ft.grads.cpu().numpy(), train_encoder=train_encoder)
    assert set(got) == set(grads), set(got) ^ set(grads)
    rel, gmax = leaf_errors(got, grads)
    keyb = [(x_, k) for x_, k in rel if k.startswith("output_head_") and "_key_bias/" in k]
    print(f"B={B} S={g.seq} terms={w} encoder trained={train_encoder}: per-sample loss error max {err.max():.2e} (loss {per.min():.3f} .. "
          f"{per.max():.3f}); worst leaves {[(f'{x_:.2e}', k) for x_, k in rel[:4]]}; worst policy key-bias head {keyb[0][0]:.2e}")
    if not (w[0] or w[1]):                                             # (the alignment weight raises gmax, the floor of the metric, over a fifth of the leaves)
        assert_not_vacuous(grads, train_encoder)
    assert len(keyb) == 2 * g.layers and all(float(grads[k].abs().max()) <= 1e-9 * gmax for _, k in keyb)     # true gradient: zero
    assert keyb[0][0] <= LEAF_TOL                                      # i.e. |got| <= 2e-3 x 1e-4 gmax (the step leaves them at zero)
    assert rel[0][0] <= LEAF_TOL, rel[:5]
    if train_encoder:
        assert sum(k.startswith("encoder_image_encoder_") for _, k in rel) == len(encoder_leaves(g))
    # a sample alone has bitwise the loss it has in the batch (the forward pass has no atomics)
    fwd = ft.forward_backward(ins, st, x, batch, forward_only=True, **fkw).clone()
    assert torch.equal(fwd, loss)
    one = FineTuner(model, 1, **tkw)
    for b in range(B):
        sl = slice(b, b + 1)
        kw1 = dict(reference_attention=r[sl]) if w[1] else {}
        alone = one.forward_backward(_rows(ins, sl), {"patch_embeddings": np.asarray(st["patch_embeddings"])[sl]}, x[sl],
                                     {k: np.asarray(v)[sl] for k, v in batch.items()}, forward_only=True, **kw1)
        assert torch.equal(alone[0], loss[b]), (b, float(alone[0]), float(loss[b]))


def test_finetune_mid():
    """MID, B = 4, encoder frozen: S = 65, row stride 68."""
    _finetune_case(_geo("MID"), 4, seed=2)


def test_finetune_mid_with_both_attention_terms():
    """The same with the entropy and alignment terms of DESIGN.md §15 on the action row of the last layer's additive-mask map."""
    _finetune_case(_geo("MID"), 4, seed=9, w=TERMS)


def test_finetune_full_geometry():
    """README geometry, B = 2, encoder frozen: S = 257."""
    _finetune_case(_geo("FULL"), 2, seed=0, query_x=QUERY_X_FULL)


def test_finetune_mid_with_the_encoder_trained():
    """MID, B = 2, train_encoder=True: the patch keys' gradient reaches DINOv2 through the extra key's softmax too."""
    _finetune_case(_geo("MID"), 2, seed=0, train_encoder=True, query_x=QUERY_X_ENC)


def test_publish_serves_the_trained_flag_on_model(mid):
    """One optimizer step of a flag-on FineTuner, publish(), then create_tasks + sample_actions of the same model: within the serving
    bounds of the restatement on the NEW parameters (unpack_params of the vector), and away from the outputs before the step."""
    from hypervla.config import encoder_leaves
    from hypervla.model import HyperVLA
    from hypervla.train import FineTuner, unpack_params
    from hypervla import synthetic as syn
    g, B = mid["g"], 4
    m = HyperVLA.from_synthetic(g, max_batch=B)
    ins, st, im = _rows(mid["ins"], slice(0, B)), {"patch_embeddings": mid["st"]["patch_embeddings"][:B]}, mid["im"][:B]
    batch = syn.synthetic_action_batch(B, g)

    def served():
        w, tasks, _ = m.create_tasks(instruction_dict=ins, initial_state=st)
        act, inter = m.sample_actions(im, ins, tasks, None, w, attention_maps=True)
        return act, inter["gripper_logits"], inter["head_attention"]

    before = served()
    ft = FineTuner(m, B)
    ft.publish()
    for x, y in zip(before, served()):
        assert np.array_equal(x, y)                                 # a publish of untouched parameters changes no bit
    ft.step(ins, st, im, batch, lr=1e-3)
    ft.publish()
    act, logit, hmap = served()
    params = dict(m._params)
    params.update(unpack_params(g, ft.params.cpu().numpy()))
    assert any(not np.array_equal(params[k], mid["P"][k]) for k in params if "CustomMultiHeadDotProductAttention_0" in k)
    bp = MB.create_tasks(params, g, ins, st)
    ract, rlog, head, _ = MB.sample_actions(params, g, dict(encoder_leaves(g)), bp, im)
    d, dl, dh = np.abs(act[..., :6] - ract[..., :6]), np.abs(logit - rlog), np.abs(hmap - head)
    print("published flag-on model: action MAE %.3e max %.3e, logit max %.3e, head map max %.2e; the step moved the actions by %.3e"
          % (d.mean(), d.max(), dl.max(), dh.max(), np.abs(act[..., :6] - before[0][..., :6]).max()))
    assert d.mean() <= 5e-4 and d.max() <= 2e-3 and dl.mean() <= 2e-3 and dh.max() <= 1e-3
    assert np.abs(act[..., :6] - before[0][..., :6]).max() > 2e-3
