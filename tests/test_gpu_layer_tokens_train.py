"""GPU: fine-tuning a share_layer_index=False model (FineTuner(layer_tokens=True), hvla_train_layer_tokens) -- one step
of the device against float64 autograd on the restatement (tests/layer_tokens_torch.py): per-sample loss and every gradient leaf, the
routing of d ctx without the oracle, shared heads as a sum, bits, publish(), metrics, frozen_keys, and the C entries.

Shapes.  MID with layer tokens: S = T + 1 + NL = 20 context rows (two 16-row tiles), NL = 7, G = 81 308 in 6 runs whose last tiles are
partial; B = 5 (odd; more than one wave of the row kernels); the sequence edge S = 48 (four policy layers, 38 language tokens); the
README hypernetwork widths at B = 2; use_language_token (NL = 8) and differential (runs 48 floats longer).  The inputs are
tests/test_layer_tokens_train_host.py's `case_inputs`, which checks on the CPU that the oracle alone passes assert_not_vacuous on them.

Bounds: per-sample loss rtol 3e-4 / atol 3e-5 (tests/train_parity.py); every leaf in train_parity's metric 2e-3 on MID and 3e-3 at the
README widths, as tests/test_gpu_train.py, tests/test_gpu_train_with_language_tokens.py and tests/test_gpu_diff_train.py hold the same
geometries without the flag."""
import ctypes
import dataclasses
import functools
import gc

import numpy as np
import pytest

import layer_tokens_ref as LR
import test_layer_tokens_train_host as H
import train_metrics_ref as MR
from train_parity import FLOOR, LOSS_ATOL, LOSS_RTOL, assert_not_vacuous, leaf_errors

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL = {"own": 2e-3, "shared": 2e-3, "language": 2e-3, "differential": 2e-3, "s48": 2e-3, "readme": 3e-3, "mid_enc": 2e-3}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X; torch.cuda.is_available() is False")


@functools.lru_cache(maxsize=None)
def _reference(name):
    """The float64 reference of a case, computed once and shared: (per, loss, grads, {theta, dtheta, dctx})."""
    keep = {}
    per, loss, grads = H.case_reference(name, keep)
    return per, loss, grads, keep


def _kw(g, enc=False):
    return dict(layer_tokens=True, language_tokens=bool(g.lang_in_policy), differential=bool(g.differential), train_encoder=enc)


@functools.lru_cache(maxsize=None)
def _stepped(name):
    """One forward_backward of a case on the device, shared by the tests that read its buffers."""
    from hypervla.model import HyperVLA
    from hypervla.train import FineTuner
    _need_gpu()
    g, B, enc, params, ins, st, x, batch = H.case_inputs(name)
    model = HyperVLA.from_synthetic(g, params=params, max_batch=B)
    ft = FineTuner(model, B, **_kw(g, enc))
    loss = ft.forward_backward(ins, st, x, batch).clone()
    torch.cuda.synchronize()
    return dict(g=g, B=B, enc=enc, model=model, ft=ft, loss=loss.cpu().numpy(), grads=ft.grads.cpu().numpy().copy(),
                theta=ft.theta.cpu().numpy().copy(), dtheta=ft.dtheta.cpu().numpy().copy(), ins=ins, st=st, x=x, batch=batch)


# ------------------------------------------------------------------------------------------------ the test that fails today
def test_the_switch_exists():
    """Before this feature FineTuner(model, B, layer_tokens=True) was a TypeError and libhvla had no hvla_train_layer_tokens."""
    from hypervla import _native
    s = _stepped("own")
    assert hasattr(_native.load_library(), "hvla_train_layer_tokens")
    assert s["ft"].layer_tokens and np.isfinite(s["loss"]).all()


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("name", ["own", "shared", "language", "differential", "s48", "readme", "mid_enc"])
def test_loss_and_every_gradient_leaf_match_autograd(name):
    from hypervla.train import unpack_params
    per, _, grads, keep = _reference(name)
    s = _stepped(name)
    g, B, enc = s["g"], s["B"], s["enc"]
    if name == "s48":
        assert g.ctx_seq == 48
    assert_not_vacuous(grads, enc)
    got = unpack_params(g, s["grads"], train_encoder=enc)
    assert set(got) == set(grads), set(got) ^ set(grads)
    rel, gmax = leaf_errors(got, grads)
    err = np.abs(s["loss"] - per.numpy())
    tol = LOSS_ATOL + LOSS_RTOL * np.abs(per.numpy())
    dth = np.abs(s["theta"] - keep["theta"].numpy()).max()
    print(f"{name} B={B} S={g.ctx_seq} NL={g.num_layer_tokens} encoder trained={enc}: per-sample loss error max {err.max():.2e} = "
          f"{(err / tol).max():.3f} of its tolerance (loss {per.numpy().min():.3f} .. {per.numpy().max():.3f}); theta max error {dth:.2e}; "
          f"worst leaves {[(f'{r:.2e}', k) for r, k in rel[:4]]}")
    np.testing.assert_allclose(s["loss"], per.numpy(), rtol=LOSS_RTOL, atol=LOSS_ATOL)
    assert rel[0][0] <= TOL[name], rel[:5]
    gc.collect()


# ------------------------------------------------------------------------------------------------ routing without the oracle
def test_token_zero_has_no_gradient():
    """Nobody attends token 0 and no leaf reads it: the gradient of layer_pos_embedding[0] is exactly 0.0 in every element, and no
    other row's is."""
    from hypervla.train import unpack_params
    for name in ("own", "shared"):
        s = _stepped(name)
        lp = unpack_params(s["g"], s["grads"])["layer_pos_embedding"]
        assert lp.shape == (1, s["g"].num_layer_tokens, s["g"].ctx_dim)
        assert (lp[0, 0] == 0.0).all() and (np.abs(lp[0, 1:]).max(1) > 0).all()


@pytest.mark.parametrize("shared", [False, True], ids=["own_heads", "shared_heads"])
def test_dctx_routes_every_run_to_its_token(shared):
    """Heads whose kernel is zero except row 0 = 1 (DESIGN.md §24's routing test): d ctx[b, t, 0] = sum of d theta[b, run(t)] to the
    f32 summation error (run width) 2^-24 sum |d theta|, every d ctx[b, t, c > 0] is exactly 0 and so is token 0's row."""
    from hypervla import synthetic as syn
    from hypervla.model import HyperVLA
    from hypervla.train import FineTuner, token_runs
    _need_gpu()
    g, B = H._geo(shared), 3
    ins, st = syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g)
    P = dict(syn.synthetic_params(g))
    for k in P:
        if k.startswith("output_head_"):
            P[k] = np.zeros_like(P[k])
            if k.endswith("/kernel"):
                P[k][0] = 1.0
    model = HyperVLA.from_synthetic(g, params=P, max_batch=B)
    ft = FineTuner(model, B, layer_tokens=True)
    batch = syn.synthetic_action_batch(B, g)
    tok = np.random.default_rng(9).standard_normal((B, g.patches, g.enc_dim)).astype(np.float32)
    ft.forward_backward(ins, st, tok, batch)
    torch.cuda.synchronize()
    o_ctx, o_dctx, n = model._ctx.train_context_rows(B)
    NL, C = g.num_layer_tokens, g.ctx_dim
    assert n == B * NL * C
    dctx = ft.work[o_dctx:o_dctx + n].cpu().numpy().reshape(B, NL, C)
    dth = ft.dtheta.cpu().numpy().astype(np.float64)
    assert np.abs(dth).max() > 0
    assert (dctx[:, :, 1:] == 0.0).all() and (dctx[:, 0] == 0.0).all()
    worst = 0.0
    for t, w, _, token in token_runs(g):
        want = dth[:, t:t + w].sum(1)
        bound = w * 2.0 ** -24 * np.abs(dth[:, t:t + w]).sum(1)
        d = np.abs(dctx[:, token, 0] - want)
        worst = max(worst, float((d / bound).max()))
        assert (d <= bound).all(), (token, d, bound)
        assert (np.abs(want) > 0).all()
    print("routing %s: worst error %.3f of (run width) 2^-24 sum |d theta|" % ("shared" if shared else "own", worst))
    gc.collect()


# ------------------------------------------------------------------------------------------------ shared heads are a sum
def test_a_shared_head_s_gradient_is_the_sum_over_the_blocks():
    """The own-heads model whose block heads are copies of the shared model's: the shared head's gradient is the sum over the blocks
    of that model's gradients (both on the device), in train_parity's metric at the parity tolerance; every other leaf agrees too."""
    import re
    from hypervla.config import generated_leaves
    from hypervla.model import HyperVLA
    from hypervla.train import FineTuner, unpack_params
    s = _stepped("shared")
    g, B = s["g"], s["B"]
    g_own = dataclasses.replace(g, shared_block_heads=False)
    P = dict(H.case_inputs("shared")[3])
    own = {k: v for k, v in P.items() if not (k.startswith("output_head_") and "encoderblock_" in k)}
    for lf in generated_leaves(g_own):
        for leaf in ("/kernel", "/bias"):
            own[lf.head_name + leaf] = P[lf.shared_head_name + leaf].copy()
    m2 = HyperVLA.from_synthetic(g_own, params=own, max_batch=B)
    ft2 = FineTuner(m2, B, layer_tokens=True)
    loss2 = ft2.forward_backward(s["ins"], s["st"], s["x"], s["batch"]).cpu().numpy()
    assert np.array_equal(loss2, s["loss"])                     # the same theta bits, the same policy
    g2 = unpack_params(g_own, ft2.grads.cpu().numpy())
    summed = {}
    for k, v in g2.items():
        key = re.sub(r"encoderblock_\d+", "encoderblock", k) if k.startswith("output_head_") else k
        summed[key] = summed.get(key, 0) + v.astype(np.float64)
    got = unpack_params(g, s["grads"])
    assert set(summed) == set(got)
    rel, _ = leaf_errors(got, {k: torch.as_tensor(v) for k, v in summed.items()})
    shared = [(r, k) for r, k in rel if k.startswith("output_head_") and re.search(r"encoderblock_(?!\d)", k)]
    assert len(shared) == 2 * sum("encoderblock_0_" in l.flat_name for l in generated_leaves(g))
    print("shared = sum over blocks: worst shared head %.2e, worst leaf %.2e (%s)" % (shared[0][0], rel[0][0], rel[0][1]))
    assert rel[0][0] <= TOL["shared"], rel[:5]
    gc.collect()


# ------------------------------------------------------------------------------------------------ bits
def _rows(ins, st, x, batch, sl):
    return ({"language_instruction": {k: np.asarray(v)[sl] for k, v in ins["language_instruction"].items()}},
            {"patch_embeddings": np.asarray(st["patch_embeddings"])[sl]}, np.asarray(x)[sl], {k: np.asarray(v)[sl] for k, v in batch.items()})


def _run(model, g, B, ins, st, x, batch):
    from hypervla.train import FineTuner
    ft = FineTuner(model, B, **_kw(g))
    loss = ft.forward_backward(ins, st, x, batch).cpu().numpy().copy()
    return loss, ft.theta.cpu().numpy().copy(), ft.dtheta.cpu().numpy().copy()


@pytest.mark.parametrize("name", ["own", "differential"])
def test_a_sample_alone_has_the_bits_it_has_in_a_batch(name):
    """Sample b alone at B = 1 has bitwise the loss and the theta row it has inside B = 5, and two runs of the same step agree in
    them.  The d theta row: the plain policy's LayerNorm and bias gradients are summed by atomics in the order the waves finish
    (DESIGN.md §23), so it is compared bit for bit on the differential flavour, which has none: two runs of B = 5 agree; a row keeps
    its bits when its four neighbours are other episodes; and since 1 / 5 is no power of two the row of B = 1 is held against the
    row inside B = 4, times the exact 4."""
    from hypervla.model import HyperVLA
    _need_gpu()
    g, B, enc, params, ins, st, x, batch = H.case_inputs(name)
    model = HyperVLA.from_synthetic(g, params=params, max_batch=B)
    full = _run(model, g, B, ins, st, x, batch)
    again = _run(model, g, B, ins, st, x, batch)
    assert np.array_equal(full[0], again[0]) and np.array_equal(full[1], again[1])
    for b in (0, B - 1):
        one = _run(model, g, 1, *_rows(ins, st, x, batch, slice(b, b + 1)))
        assert np.array_equal(one[0][0], full[0][b]) and np.array_equal(one[1][0], full[1][b]), b
    if name == "differential":
        assert np.array_equal(full[2], again[2])
        perm = [4, 2, 0, 1, 3]                                   # sample 0 in row 2, among the others in another order
        moved = _run(model, g, B, *_rows(ins, st, x, batch, perm))
        assert np.array_equal(moved[2][2], full[2][0]) and np.array_equal(moved[0][2], full[0][0])
        four = _run(model, g, 4, *_rows(ins, st, x, batch, slice(0, 4)))
        one = _run(model, g, 1, *_rows(ins, st, x, batch, slice(0, 1)))
        assert np.array_equal(four[2][0] * np.float32(4.0), one[2][0])
    gc.collect()


# ------------------------------------------------------------------------------------------------ publish
def _served(m, ins, st):
    w, _, _ = m.create_tasks(instruction_dict=ins, initial_state=st)
    theta, ctx = w.export()
    torch.cuda.synchronize()
    return theta.clone(), ctx.clone()


@pytest.mark.parametrize("shared,ema", [(False, False), (True, False), (True, True)], ids=["own_heads", "shared_heads", "shared_heads_ema"])
def test_publish_serves_what_a_fresh_model_serves(shared, ema):
    """After two optimizer steps publish() leaves the serving buffers those of a fresh model created from the exported parameters:
    create_tasks' theta and context are bitwise equal, and differ from what was served before."""
    from hypervla.model import HyperVLA
    from hypervla.train import FineTuner, unpack_params
    _need_gpu()
    g, B, enc, params, ins, st, x, batch = H.case_inputs("shared" if shared else "own")
    from hypervla import synthetic as syn
    im = syn.synthetic_images(B, g)                                                # step() encodes uint8 frames itself
    m = HyperVLA.from_synthetic(g, params=params, max_batch=B)
    ft = FineTuner(m, B, layer_tokens=True, ema_start_step=0, ema_decay=0.5)
    first = _served(m, ins, st)
    ft.publish()
    same = _served(m, ins, st)
    assert torch.equal(first[0], same[0]) and torch.equal(first[1], same[1])       # un-trained: the load's bits
    for _ in range(2):
        ft.step(ins, st, im, batch, lr=1e-3)
    ft.publish(ema=ema)
    after = _served(m, ins, st)
    vec = (ft.ema if ema else ft.params).cpu().numpy()
    assert not np.array_equal(ft.ema.cpu().numpy(), ft.params.cpu().numpy())
    new = dict(m._params)
    new.update(unpack_params(g, vec))
    fresh = HyperVLA(m.config, new, None, m.dataset_statistics, max_batch=m.max_batch, enc_dtype=m.enc_dtype)
    want = _served(fresh, ins, st)
    for a, b, c in zip(after, want, first):
        assert torch.equal(a, b) and not torch.equal(a, c)
    assert all(np.array_equal(m.params[k], new[k]) for k in new)                    # host_copy: what save_pretrained writes
    gc.collect()


# ------------------------------------------------------------------------------------------------ the other fine-tune features
def test_info_against_the_restatement():
    """metrics=True over the new layout.  The norms on the device's own vectors at tests/test_gpu_train_metrics.py's bound 2^-23, as that
    test holds them; and grad_norm against the restatement fed the ORACLE's gradients: | |g| - |g_ref| | <= |g - g_ref|_2 <=
    tol sqrt(sum_leaf n_leaf m_leaf^2), m_leaf = max(max |ref leaf|, 1e-4 gmax) -- the parity bound of every leaf, summed."""
    from hypervla.model import HyperVLA
    from hypervla.train import FineTuner, pack_params
    _need_gpu()
    g, B, enc, params, ins, st, x, batch = H.case_inputs("shared")
    per, _, grads, _ = _reference("shared")
    m = HyperVLA.from_synthetic(g, params=params, max_batch=B)
    ft = FineTuner(m, B, layer_tokens=True, metrics=True)
    ft.forward_backward(ins, st, x, batch)
    ft.apply(lr=1e-3)
    torch.cuda.synchronize()
    v = ft.metric_vec.cpu().numpy().astype(np.float64)
    dev = {k: getattr(ft, k).cpu().numpy() for k in ("grads", "params", "prev_params", "theta")}
    for slot, want, what in ((MR.GRAD_NORM, MR.grad_norm(dev["grads"]), "grad_norm"), (MR.PARAM_NORM, MR.param_norm(dev["prev_params"]), "param_norm"),
                             (MR.UPDATE_NORM, MR.update_norm(dev["params"], dev["prev_params"]), "update_norm"),
                             (MR.BASE_PARAMS_NORM, MR.base_params_norm(dev["theta"], ft.encoder_sqsum), "base_params_norm")):
        e = MR.rel_err(v[slot], want)
        print(f"{what}: device {v[slot]:.9g} float64 {want:.9g} relative error {e:.2e}")
        assert e <= MR.BOUND, (what, v[slot], want)
    ref_vec = pack_params(g, {k: t.numpy() for k, t in grads.items()})
    gmax = max(float(t.abs().max()) for t in grads.values())
    bound = TOL["shared"] * np.sqrt(sum(t.numel() * max(float(t.abs().max()), FLOOR * gmax) ** 2 for t in grads.values()))
    want = MR.grad_norm(ref_vec)
    print(f"grad_norm against the oracle's gradients: device {v[MR.GRAD_NORM]:.9g} oracle {want:.9g}, |difference| {abs(v[MR.GRAD_NORM] - want):.3e} (bound {bound:.3e})")
    assert abs(v[MR.GRAD_NORM] - want) <= bound
    np.testing.assert_allclose(v[MR.TRAINING_LOSS], float(per.mean()), rtol=LOSS_RTOL, atol=LOSS_ATOL)
    info = ft.info()
    assert float(info["grad_norm"]) == np.float32(v[MR.GRAD_NORM])
    from hypervla import synthetic as syn
    val = ft.validate(ins, st, syn.synthetic_images(B, g), batch)
    assert np.isfinite(float(val["mse"])) and float(val["mse"]) > 0
    gc.collect()


def test_frozen_heads_stay_and_the_loss_decreases():
    """frozen_keys=("output_head_*",) leaves the shared heads (every head) bitwise untouched over two steps while the context
    encoder moves; without it the loss decreases over 5 steps; gradient accumulation runs over the new layout."""
    from hypervla.model import HyperVLA
    from hypervla.train import FineTuner, train_param_layout
    _need_gpu()
    g, B, enc, params, ins, st, x, batch = H.case_inputs("shared")
    m = HyperVLA.from_synthetic(g, params=params, max_batch=B)
    from hypervla import synthetic as syn
    im = syn.synthetic_images(B, g)                                                # step() encodes uint8 frames itself
    at = dict((k, o) for k, o, _ in train_param_layout(g)[0])
    ft = FineTuner(m, B, layer_tokens=True, frozen_keys=("output_head_*",))
    assert ft.frozen_buckets == 2
    p0 = ft.params.clone()
    for _ in range(2):
        ft.step(ins, st, im, batch, lr=1e-3)
    assert torch.equal(ft.params[at["W_cat"]:], p0[at["W_cat"]:]) and not torch.equal(ft.params[:at["W_cat"]], p0[:at["W_cat"]])
    assert torch.equal(ft.grads[at["W_cat"]:], torch.zeros_like(ft.grads[at["W_cat"]:]))
    ft = FineTuner(m, B, layer_tokens=True)
    losses = [float(ft.step(ins, st, im, batch, lr=1e-3)) for _ in range(5)]
    print("losses over 5 steps:", np.round(losses, 4))
    assert losses[-1] < losses[0] and all(np.isfinite(losses))
    fa = FineTuner(m, B, layer_tokens=True, grad_accumulation_steps=2)
    fa.forward_backward(ins, st, x, batch)
    assert fa.apply(lr=1e-3) is False
    fa.forward_backward(ins, st, x, batch)
    assert fa.apply(lr=1e-3) is True
    gc.collect()


# ------------------------------------------------------------------------------------------------ the C entries
def test_c_entries():
    """hvla_train_layer_tokens(ctx, 1) on a model without layer tokens is HVLA_OK and a no-op; without the call every hvla_train_* entry
    that reads the geometry returns HVLA_E_SHAPE with the text it had; values other than 0 / 1 are refused; NULL ctx is HVLA_E_STATE."""
    from hypervla import _native
    from hypervla.config import MID
    from hypervla.train import train_param_layout
    _need_gpu()
    lib = _native.load_library()
    err = lambda c: lib.hvla_last_error(c.h).decode()
    out = (ctypes.c_int64 * 4)()
    for on in (0, 1):
        assert lib.hvla_train_layer_tokens(None, on) == -7
    plain = _native.Context(MID, max_batch=2)
    assert lib.hvla_train_sizes(plain.h, 2, 0, out) == 0
    before = list(out)
    assert lib.hvla_train_layer_tokens(plain.h, 1) == 0
    assert lib.hvla_train_sizes(plain.h, 2, 0, out) == 0 and list(out) == before
    plain.close()
    g = H._geo(True)
    ctx = _native.Context(g, max_batch=2)
    text = "the training path does not build hypernet_kwargs.share_layer_index=False (one layer token per policy module): serving is"
    out6, out3 = (ctypes.c_int64 * 6)(), (ctypes.c_int64 * 3)()
    calls = [lambda: lib.hvla_train_sizes(ctx.h, 2, 0, out), lambda: lib.hvla_train_bucket_ranges(ctx.h, 0, out6),
             lambda: lib.hvla_train_publish(ctx.h, None, 0, 0, None), lambda: lib.hvla_train_context_rows(ctx.h, 2, 0, out3),
             lambda: lib.hvla_train_position_source(ctx.h, 4, None)]
    for call in calls:
        assert call() == -1 and text in err(ctx), err(ctx)
    assert lib.hvla_train_layer_tokens(ctx.h, 1) == 0
    assert lib.hvla_train_sizes(ctx.h, 2, 0, out) == 0
    assert out[0] == out[3] == train_param_layout(g)[1] and out[2] > before[2]
    for bad in (2, -1):
        assert lib.hvla_train_layer_tokens(ctx.h, bad) == -1 and "0 or 1" in err(ctx)
    assert lib.hvla_train_sizes(ctx.h, 2, 0, out) == 0
    assert lib.hvla_train_layer_tokens(ctx.h, 0) == 0
    assert lib.hvla_train_sizes(ctx.h, 2, 0, out) == -1 and text in err(ctx)
    ctx.close()
