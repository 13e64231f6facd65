"""GPU: vit_kwargs.use_differential_transformer (Geometry.differential) -- policy_kernel_diff / policy_kernel_slots_diff
against the float64 restatement of DifferentialAttention (tests/diff_attention_ref.py).

Serving bounds are the project's (tests/test_gpu_mask_as_bias.py, tests/test_gpu_language_tokens.py): README geometry from given
tokens, theta 1e-4, actions max 1e-3, gripper logits 1.5e-3, the gripper bit where |logit| > 2e-3; MID end to end from uint8 frames,
action mean 5e-4, max 2e-3, logit mean 2e-3.  On the same inputs the restatement of the model without the flag is hundreds of
tolerances away and the float32 restatement stays within a quarter of each bound (tests/test_differential_host.py), so the inputs
are well conditioned for the RMSNorm's division and a kernel that ran the plain attention would fail.

The lambda case runs one checkpoint whose lambda heads are x 5 (the generated lambda vectors x 5, their products x 25), so that
exp(sum lambda_q1 lambda_k1) differs across episodes; it first asserts on the restatement that lambda spreads by more than 0.05 over
the B episodes in some layer, else a kernel that used lambda_init alone could pass.

Measured on one MI355X: README geometry theta max 4.0e-6, action max 3.6e-4 / mean 5.2e-5, logit max 2.6e-4 (the plain restatement
4.0 / 2.9 away); lambda heads x 5 (lambda from - 3.4 to 9.7, spread 2.65 in one layer) action max 1.8e-4, logit max 1.5e-4; MID end
to end action mean 1.5e-4 / max 4.4e-4, logit mean 1.5e-4 / max 4.9e-4; a re-imported pytree steps 2.4e-5 / 1.4e-5 from the
generated handle."""
import ctypes
import dataclasses
import gc

import numpy as np
import pytest

import diff_attention_ref as DR

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LAMBDA_X = 5.0


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X; torch.cuda.is_available() is False")


def _geo(name):
    from hypervla import config
    return dataclasses.replace(getattr(config, name), differential=True)


def _rows(d, sl):
    return {"language_instruction": {k: np.asarray(v)[sl] for k, v in d["language_instruction"].items()}}


def _check_serving(act, logit, ract, rlog, what):
    d, dl = np.abs(act[..., :6] - ract[..., :6]), np.abs(logit - rlog)
    print("%s: action max %.3e MAE %.3e, logit max %.3e" % (what, d.max(), d.mean(), dl.max()))
    assert d.max() <= 1e-3 and dl.max() <= 1.5e-3, (d.max(), dl.max())
    safe = np.abs(rlog) > 2e-3
    assert (act[..., 6][safe] == ract[..., 6][safe]).all()
    return d, dl


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
    """README geometry, B = 4 (policy_kernel_diff<8>): theta in the variant's leaf order, actions and gripper logits."""
    from hypervla.config import generated_leaves
    m, g, B = full["m"], full["g"], full["B"]
    bp = DR.create_tasks(m.params, g, full["ins"], full["st"])
    w, _, _ = m.create_tasks(instruction_dict=full["ins"], initial_state=full["st"])
    theta = w.export()[0].cpu().numpy().astype(np.float64)
    ref = np.concatenate([bp[l.flat_name].reshape(B, -1) for l in generated_leaves(g)], 1)
    print("theta max error %.3e" % np.abs(theta - ref).max())
    assert theta.shape == ref.shape == (B, 200_668) and np.abs(theta - ref).max() <= 1e-4
    ract, rlog = DR.policy(bp, g, full["tok"].astype(np.float64))
    pact, plog = DR.policy(bp, g, full["tok"].astype(np.float64), "plain")
    _check_serving(full["act"], full["logit"], ract, rlog, "README use_differential_transformer B=%d from tokens" % B)
    dm, dlm = np.abs(full["act"][..., :6] - pact[..., :6]), np.abs(full["logit"] - plog)
    print("against the plain restatement: action %.3e, logit %.3e" % (dm.max(), dlm.max()))
    assert dm.max() > 4e-3 and dlm.max() > 6e-3                  # farther than 4 tolerances from the model without the flag


def test_mid_end_to_end_from_frames(mid):
    """MID, B = 4 (policy_kernel_diff<2>) from uint8 frames."""
    from hypervla.config import encoder_leaves
    m, g, B = mid["m"], mid["g"], 4
    ins, st, im = _rows(mid["ins"], slice(0, B)), {"patch_embeddings": mid["st"]["patch_embeddings"][:B]}, mid["im"][:B]
    w, tasks, _ = m.create_tasks(instruction_dict=ins, initial_state=st)
    act, inter = m.sample_actions(im, ins, tasks, np.ones((B, 1)), w)
    bp = DR.create_tasks(mid["P"], g, ins, st)
    ract, rlog, tok = DR.sample_actions(mid["P"], g, dict(encoder_leaves(g)), bp, im)
    pact, _ = DR.policy(bp, g, tok, "plain")
    d, dl = np.abs(act[..., :6] - ract[..., :6]), np.abs(inter["gripper_logits"] - rlog)
    print("MID use_differential_transformer end to end: action MAE %.3e max %.3e, logit mean %.3e max %.3e; the plain restatement is "
          "%.3e away" % (d.mean(), d.max(), dl.mean(), dl.max(), np.abs(ract[..., :6] - pact[..., :6]).max()))
    assert d.mean() <= 5e-4 and d.max() <= 2e-3 and dl.mean() <= 2e-3, (d.mean(), d.max(), dl.mean())
    assert np.abs(act[..., :6] - pact[..., :6]).max() > 5 * 2e-3 - 2e-3


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


def test_pool_scattered_slots_and_imported_pytree(mid):
    """assign_tasks into permuted slots of a pool (policy_kernel_slots_diff): bitwise the rows of a full-batch step; import_tasks of
    to_pytree() exports bitwise what the handle it came from exports."""
    m, cap = mid["m"], mid["cap"]
    w, tasks, _ = m.create_tasks(instruction_dict=mid["ins"], initial_state=mid["st"])
    act, inter = m.sample_actions(mid["im"], mid["ins"], tasks, None, w)
    perm = np.random.default_rng(4).permutation(cap).tolist()
    pool = m.create_pool(cap)
    m.assign_tasks(pool, perm, mid["ins"], mid["st"])             # episode k -> slot perm[k]
    K = 5
    a, it = m.sample_actions(mid["im"][:K], None, None, None, pool, slots=perm[:K])
    np.testing.assert_array_equal(a, act[:K])
    np.testing.assert_array_equal(it["gripper_logits"], inter["gripper_logits"][:K])
    a1, _ = m.sample_actions(mid["im"][6:7], None, None, None, pool, slots=[perm[6]])
    np.testing.assert_array_equal(a1[0], act[6])
    tree = w.to_pytree()
    blk = tree["encoder"]["Transformer_0"]["encoderblock_0"]["DifferentialAttention_0"]
    assert sorted(blk) == ["k_proj", "lambda_k1", "lambda_k2", "lambda_q1", "lambda_q2", "out_proj", "q_proj", "subln", "v_proj"]
    w2 = m.import_tasks(tree)
    assert np.array_equal(w2.export()[0].cpu().numpy(), w.export()[0].cpu().numpy())
    # stepping the imported handle: the import re-splits hi + lo, which does not reproduce every bf16 pair of the generated arena
    # (tests/test_gpu_weights_import.py::test_reimported_export_steps_close_to_the_generated_handle, whose bounds these are); an
    # import of the imported handle's own tree is the same arena, bit for bit
    a2, it2 = m.sample_actions(mid["im"], None, None, None, w2)
    d, dl = np.abs(a2[..., :6] - act[..., :6]), np.abs(it2["gripper_logits"] - inter["gripper_logits"])
    print("re-imported pytree against the generated handle: action max %.3e MAE %.3e, logit max %.3e" % (d.max(), d.mean(), dl.max()))
    assert d.mean() <= 2e-4 and d.max() <= 2e-3 and dl.max() <= 2e-3, (d.mean(), d.max(), dl.max())
    w3 = m.import_tasks(w2.to_pytree())
    a3, it3 = m.sample_actions(mid["im"], None, None, None, w3)
    np.testing.assert_array_equal(a3, a2)
    np.testing.assert_array_equal(it3["gripper_logits"], it2["gripper_logits"])


def test_create_with_v3_with_the_field_zero_is_create():
    """hvla_create(cfg) == hvla_create_with_v3(cfg, {size, 0, 0, 0}) == hvla_create_with_v3(cfg, NULL) on MID: theta and actions."""
    _need_gpu()
    from hypervla import _native, synthetic as syn
    from hypervla.config import MID
    from hypervla.model import HyperVLA
    g, B = MID, 3
    ins, st, im = syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g), syn.synthetic_images(B, g)
    outs = []
    lib = _native.load_library()
    orig = lib.hvla_create
    zero = _native.hvla_policy_options_v3(ctypes.sizeof(_native.hvla_policy_options_v3), 0, 0, 0)
    for route in ("create", "create_with_v3", "create_with_v3 NULL"):
        if route != "create":
            lib.hvla_create = lambda cfg, dev, h: lib.hvla_create_with_v3(cfg, ctypes.byref(zero) if route == "create_with_v3" else None, dev, h)
        try:
            m = HyperVLA.from_synthetic(g, max_batch=4)
        finally:
            lib.hvla_create = orig
        w, t, _ = m.create_tasks(instruction_dict=ins, initial_state=st)
        a, inter = m.sample_actions(im, ins, t, None, w)
        outs.append((w.export()[0].cpu().numpy(), a, inter["gripper_logits"]))
        del w, m
    for other in outs[1:]:
        for x, y in zip(outs[0], other):
            assert np.array_equal(x, y)


def test_refused_combinations_and_entries(mid):
    """The two flag combinations return HVLA_E_SHAPE (-1) with a text; hvla_train_step, hvla_train_sizes, hvla_train_publish and the
    head-map export on a differential context return HVLA_E_SHAPE with a text and launch nothing."""
    from hypervla import _native
    from hypervla.config import MID
    lib = _native.load_library()
    plain = _native.Context(MID, max_batch=1)                     # (a valid hvla_config of this device)
    size = ctypes.sizeof(_native.hvla_policy_options_v3)
    for opt, word in ((_native.hvla_policy_options_v3(size, 1, 0, 1), b"use_language_token"),
                      (_native.hvla_policy_options_v3(size, 0, 1, 1), b"attention_mask_as_bias")):
        h = ctypes.c_void_p()
        assert lib.hvla_create_with_v3(ctypes.byref(plain.cfg), ctypes.byref(opt), 0, ctypes.byref(h)) == -1 and not h.value
        assert word in lib.hvla_last_error(None)
    for bad in (_native.hvla_policy_options_v3(size, 0, 0, 2), _native.hvla_policy_options_v3(size - 4, 0, 0, 1)):
        h = ctypes.c_void_p()
        assert lib.hvla_create_with_v3(ctypes.byref(plain.cfg), ctypes.byref(bad), 0, ctypes.byref(h)) == -1 and not h.value
    plain.close()

    ctx = mid["m"]._ctx
    torch.cuda.synchronize()
    ctx.launches()                                                # (reset the counter)
    buf, hyper, out = _native.hvla_train_buffers(), _native.hvla_train_hyper(), (ctypes.c_int64 * 4)()
    one = ctypes.c_void_p(16)                                     # non-null, never read: the entry refuses before it looks
    rc = lib.hvla_train_step(ctx.h, ctypes.byref(buf), one, one, one, one, one, one, one, one, 1, ctypes.byref(hyper), None)
    assert rc == -1 and b"use_differential_transformer" in lib.hvla_last_error(ctx.h)
    assert lib.hvla_train_sizes(ctx.h, 1, 0, out) == -1
    lib.hvla_train_publish.restype = ctypes.c_int
    assert lib.hvla_train_publish(ctx.h, one, ctypes.c_int64(1), 0, None) == -1
    assert lib.hvla_set_attention_outputs(ctx.h, None, one) == -1 and b"head_attention" in lib.hvla_last_error(ctx.h)
    assert lib.hvla_set_attention_outputs(ctx.h, None, None) == 0
    assert ctx.launches() == 0
    w1, _, _ = mid["m"].create_tasks(instruction_dict=_rows(mid["ins"], slice(0, 1)),
                                     initial_state={"patch_embeddings": mid["st"]["patch_embeddings"][:1]})
    with pytest.raises(ValueError, match="use_differential_transformer"):
        mid["m"].sample_actions(mid["im"][:1], None, None, None, w1, attention_maps=True)
    from hypervla.train import FineTuner
    with pytest.raises(ValueError, match="not built; serving is"):
        FineTuner(mid["m"], 1)
    r = mid["m"].reference_attention_map(mid["im"][:2])           # DINOv2's map keeps working
    assert tuple(r.shape) == (2, mid["g"].patches) and bool(torch.isfinite(r).all())


def test_lambda_differs_across_episodes():
    """One checkpoint with the lambda heads x 5, README geometry from given tokens: lambda spreads over the episodes (asserted on the
    restatement first), so lambda_init alone would miss the bounds."""
    _need_gpu()
    from hypervla import synthetic as syn
    from hypervla.model import HyperVLA
    g, B = _geo("FULL"), 4
    P = DR.lambda_scaled(syn.synthetic_params(g), LAMBDA_X)
    ins, st = syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g)
    tok = np.random.default_rng(3).standard_normal((B, g.patches, g.enc_dim)).astype(np.float32)
    bp = DR.create_tasks(P, g, ins, st)
    lam = DR.lambdas(bp, g)
    spread = (lam.max(0) - lam.min(0)).max()
    print("lambda per episode and layer:\n%s\nlargest spread over the episodes %.3f" % (lam, spread))
    assert spread > 0.05
    ract, rlog = DR.policy(bp, g, tok.astype(np.float64))
    m = HyperVLA.from_synthetic(g, params=P, max_batch=B)
    w, _, _ = m.create_tasks(instruction_dict=ins, initial_state=st)
    act, logit = (t.cpu().numpy() for t in m.policy_from_tokens(tok, w))
    _check_serving(act, logit, ract, rlog, "README geometry, lambda heads x %g" % LAMBDA_X)
