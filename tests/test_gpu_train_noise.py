"""GPU: the fine-tune step under hvla_train_noise_set -- the reference's dropout and image-embedding noise from a
counter-based generator that the host restates bit for bit (hypervla.train.philox4x32), so that parity with float64 autograd
(tests/train_noise_ref.py) is as exact as without noise, masks included.  MID geometry, B = 4; rates 0.25 (keep_prob 0.75 is exact),
sigma 0.1.  Bounds: per-sample loss rtol 2e-4 / atol 2e-5 and worst leaf max|d| / max(max|ref|, 1e-4 gmax) <= 2e-3
(tests/test_gpu_train.py); the trained-encoder case at tests/train_parity.py::encoder_case's own (3e-4 / 3e-5, 2e-3).  Measured on
one MI355X: loss errors 0.9e-4 .. 3.6e-4 at losses up to 54, worst leaf 2.6e-4 .. 7.2e-4 (a key bias, held to the floor, every time;
over 48 runs of the all-knobs case at most 1.3e-3)."""
import ctypes as C
import gc

import numpy as np
import pytest

import train_noise_ref as NR
from train_parity import LOSS_ATOL, LOSS_RTOL, assert_not_vacuous, leaf_errors

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

B = 4
RATE, SIGMA, SEED = 0.25, 0.1, 0x5EED0123456789
KNOBS = {"policy": dict(dropout_rate=RATE), "tokens": dict(image_embedding_noise=SIGMA), "context": dict(embedding_dropout_rate=RATE),
         "cls": dict(image_dropout=RATE), "all": dict(dropout_rate=RATE, image_embedding_noise=SIGMA, embedding_dropout_rate=RATE, image_dropout=RATE)}
# The normals: the device evaluates Box-Muller in float32, the restatement in float64.  Measured on an MI355X over 2^16 normals of four
# (seed, sample, draw) settings: max |device - float64| = 1.495e-6; the bound is 4x that, for logf / sincosf last-bit
# differences between library versions.
NORMAL_MEASURED, NORMAL_BOUND = 1.495e-6, 4 * 1.495e-6


def _ref_noise(kw, draw, offset=0, batch=B):
    """train_noise_ref.Noise for FineTuner keywords `kw`."""
    return NR.Noise(batch, policy_dropout=kw.get("dropout_rate", 0.0), image_embedding_noise=kw.get("image_embedding_noise", 0.0),
                    context_dropout=kw.get("embedding_dropout_rate", 0.0), image_dropout=kw.get("image_dropout", 0.0), seed=SEED,
                    sample_offset=offset, draw=draw)


@pytest.fixture(scope="module")
def mid():
    """One MID model with seeded inputs, shared by the module; FineTuners are made per test (they share the model's context)."""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X; torch.cuda.is_available() is False")
    from hypervla import synthetic as syn
    from hypervla.config import MID, generated_leaves
    from hypervla.model import HyperVLA
    g = MID
    model = HyperVLA.from_synthetic(g, max_batch=B)
    ins, st, batch = syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g), syn.synthetic_action_batch(B, g)
    tok = np.random.default_rng(9).standard_normal((B, g.patches, g.enc_dim)).astype(np.float32)
    params = {k: v for k, v in model.params.items() if not k.startswith("encoder_image_encoder_")}
    yield dict(g=g, model=model, ins=ins, st=st, batch=batch, tok=tok, params=params, leaves=generated_leaves(g), im=syn.synthetic_images(B, g))
    gc.collect()


def _tuner(s, **kw):
    from hypervla.train import FineTuner
    return FineTuner(s["model"], B, noise_seed=SEED, **kw)


def _fixed(ft, draw, offset=0, **override):
    """Pin what the tuner tells the context: this draw and sample_offset (FineTuner counts draws and takes the offset from the rank)."""
    def select():
        kw = dict(ft.noise, **override)
        ft.model._ctx.train_noise(seed=ft.noise_seed, sample_offset=offset, draw=draw, **kw)
    ft._select_noise = select


# ---------------------------------------------------------------------------------------------------------------- probe
def test_probe_multipliers_are_the_host_restatement_bitwise(mid):
    from hypervla import train as T
    ctx, g = mid["model"]._ctx, mid["g"]
    S = g.patches + 1
    sites = [(T.NOISE_POLICY_INPUT, 0, S * g.dim, 0.25), (T.NOISE_ATTN_OUT, 1, S * g.dim, 0.25), (T.NOISE_MLP_HIDDEN, 0, S * g.mlp, 0.25),
             (T.NOISE_MLP_HIDDEN, 1, S * g.mlp, 0.25), (T.NOISE_MLP_OUT, 1, S * g.dim, 0.25), (T.NOISE_CONTEXT, 0, g.ctx_dim, 0.1),
             (T.NOISE_IMAGE_CLS, 0, g.enc_dim, 0.5)]
    draw = 7
    ctx.train_noise(policy_dropout=0.25, image_embedding_noise=SIGMA, context_dropout=0.1, image_dropout=0.5, seed=SEED, sample_offset=99, draw=draw)
    try:
        for kind, layer, n, rate in sites:
            for sample in (0, 3, 2 ** 31 + 5):
                for m in (n, n - 3):                                     # also a length that is no multiple of 4
                    out = torch.full((m + 8,), -1.0, dtype=torch.float32, device=mid["model"].device)
                    ctx.train_noise_probe(T.noise_site(kind, layer), sample, m, out.data_ptr(), mid["model"]._stream())
                    got = out.cpu().numpy()
                    want = T.noise_multipliers(rate, SEED, T.noise_site(kind, layer), sample, draw, m)
                    assert (got[m:] == -1.0).all(), (kind, layer, "wrote past n")
                    assert got[:m].tobytes() == want.tobytes(), (kind, layer, sample, m)
                    assert 0 < (want > 0).mean() < 1
    finally:
        ctx.train_noise(off=True)


def test_probe_normals_against_float64(mid):
    from hypervla import train as T
    ctx = mid["model"]._ctx
    n, worst = 2 ** 16, 0.0
    try:
        for seed, sample, draw in ((SEED, 0, 1), (SEED, 5, 1), (SEED, 0, 2), (1, 2 ** 31 + 1, 3)):
            ctx.train_noise(image_embedding_noise=SIGMA, seed=seed, draw=draw)
            out = torch.empty(n, dtype=torch.float32, device=mid["model"].device)
            ctx.train_noise_probe(T.noise_site(T.NOISE_TOKENS), sample, n, out.data_ptr(), mid["model"]._stream())
            want = T.noise_normals(seed, T.noise_site(T.NOISE_TOKENS), sample, draw, n)
            worst = max(worst, float(np.abs(out.cpu().numpy().astype(np.float64) - want).max()))
    finally:
        ctx.train_noise(off=True)
    print(f"normals: max |device - float64| = {worst:.3e} over {4 * n} draws (measured {NORMAL_MEASURED:.1e}, bound {NORMAL_BOUND:.2e})")
    assert worst <= NORMAL_BOUND


# ---------------------------------------------------------------------------------------------------------------- parity
def _parity(g, model, ins, st, obs, batch, kw, tol, rtol, atol, train_encoder=False, **ft_kw):
    from hypervla.config import encoder_leaves, generated_leaves
    from hypervla.train import FineTuner, unpack_params
    ft = FineTuner(model, B, noise_seed=SEED, train_encoder=train_encoder, **kw, **ft_kw)
    got_loss = ft.forward_backward(ins, st, obs, batch).cpu().numpy()
    assert ft.noise_draw == 1
    nz = _ref_noise(kw, draw=ft.noise_draw)
    if train_encoder:
        per, _, grads = NR.train_loss_and_grads(model.params, g, generated_leaves(g), ins, st, None, batch, nz, images=obs,
                                                enc_shapes=dict(encoder_leaves(g)))
    else:
        params = {k: v for k, v in model.params.items() if not k.startswith("encoder_image_encoder_")}
        per, _, grads = NR.train_loss_and_grads(params, g, generated_leaves(g), ins, st, obs, batch, nz)
    got = unpack_params(g, ft.grads.cpu().numpy(), train_encoder=train_encoder)
    assert set(got) == set(grads), set(got) ^ set(grads)
    rel, _ = leaf_errors(got, grads)
    err = np.abs(got_loss - per.numpy())
    print(f"noise {sorted(kw)} enc={int(train_encoder)}: per-sample loss error max {err.max():.2e} (loss {per.numpy().min():.3f} .. {per.numpy().max():.3f}); "
          f"worst relative gradient errors {[(f'{r:.2e}', k) for r, k in rel[:4]]}")
    assert_not_vacuous(grads, train_encoder)
    np.testing.assert_allclose(got_loss, per.numpy(), rtol=rtol, atol=atol)
    assert rel[0][0] <= tol, rel[:5]
    return ft, per.numpy()


@pytest.mark.parametrize("knob", list(KNOBS))
def test_loss_and_every_gradient_leaf_match_autograd(mid, knob):
    """Each knob alone, then all four: the per-sample loss and every leaf of the gradient against float64 autograd with the host's masks
    and normals.  The noise is not a no-op: the loss differs from the noise-free oracle's."""
    from oracle import hvla_ref_torch as ot
    s = mid
    _, per = _parity(s["g"], s["model"], s["ins"], s["st"], s["tok"], s["batch"], KNOBS[knob], 2e-3, 2e-4, 2e-5)
    if "clean" not in s:
        s["clean"] = ot.train_loss_and_grads(s["params"], s["g"], s["leaves"], s["ins"], s["st"], s["tok"], s["batch"])[0].numpy()
    assert np.abs(per - s["clean"]).max() > 1e-3, knob


def test_all_knobs_with_the_encoder_trained(mid):
    """The token noise goes onto the encoder's own output and the gradient passes the addition unchanged: every DINOv2 leaf too."""
    s = mid
    _parity(s["g"], s["model"], s["ins"], s["st"], s["im"], s["batch"], KNOBS["all"], 2e-3, LOSS_RTOL, LOSS_ATOL, train_encoder=True)


def test_all_knobs_with_language_tokens():
    """A use_language_token model: the masks of sites 1, 2 and 4 run over S = T + P + 1 rows."""
    import lang_policy_torch as LT
    from hypervla import synthetic as syn
    from hypervla.model import HyperVLA
    g, b = LT.geometry("T12")
    assert b == B and g.policy_seq == g.lang_tokens + g.patches + 1
    model = HyperVLA.from_synthetic(g, max_batch=B)
    ins, st, batch = syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g), syn.synthetic_action_batch(B, g)
    tok = np.random.default_rng(9).standard_normal((B, g.patches, g.enc_dim)).astype(np.float32)
    _parity(g, model, ins, st, tok, batch, KNOBS["all"], 2e-3, 2e-4, 2e-5, language_tokens=True)


# ---------------------------------------------------------------------------------------------------------------- properties
def _roll(s, k):
    """The batch with row j holding sample (j + k) % B."""
    ix = (np.arange(B) + k) % B
    ins = {"language_instruction": {n: np.asarray(v)[ix] for n, v in s["ins"]["language_instruction"].items()}}
    return ins, {"patch_embeddings": np.asarray(s["st"]["patch_embeddings"])[ix]}, s["tok"][ix], {n: np.asarray(v)[ix] for n, v in s["batch"].items()}


def test_noise_follows_the_global_sample_index_and_the_draw(mid):
    s = mid
    ft = _tuner(s, **KNOBS["all"])
    args = (s["ins"], s["st"], s["tok"], s["batch"])
    _fixed(ft, draw=5)
    base = ft.forward_backward(*args).clone()
    assert torch.equal(ft.forward_backward(*args), base)                  # the same draw: the same bits
    for k in (1, 3):                                                      # row 0 under sample_offset = k is row k under offset 0
        _fixed(ft, draw=5, offset=k)
        rolled = ft.forward_backward(*_roll(s, k)).clone()
        assert torch.equal(rolled[0], base[k]), (k, float(rolled[0]), float(base[k]))
    assert not torch.equal(rolled[1], base[0])                            # k = 3: row 1 is sample 0 again, now under global index 4
    _fixed(ft, draw=6)
    other = ft.forward_backward(*args).clone()
    live = base != 0                                                      # (a sample whose timestep is padding has loss 0 whatever is drawn)
    assert int(live.sum()) >= B - 1 and (other != base)[live].all()       # another draw: another loss, every live sample
    off = _tuner(s)
    clean = off.forward_backward(*args, forward_only=True).clone()
    _fixed(ft, draw=6)
    assert torch.equal(ft.forward_backward(*args, forward_only=True), clean)      # forward_only draws nothing
    assert (other != clean)[live].all()


def test_off_is_off(mid):
    """A context that never set noise, one that set all rates 0 and one that set then cleared it: equal loss bits from a differentiated
    step, equal hvla_train_sizes; a set context reports the larger workspace."""
    from hypervla.model import HyperVLA
    from hypervla.train import FineTuner
    s, g = mid, mid["g"]
    args = (s["ins"], s["st"], s["tok"], s["batch"])
    losses, sizes = [], []
    for how in ("never", "zeros", "cleared"):
        model = HyperVLA.from_synthetic(g, max_batch=B)
        ctx = model._ctx
        if how == "zeros":
            ctx.train_noise(seed=SEED, draw=3, sample_offset=2)
        if how == "cleared":
            ctx.train_noise(policy_dropout=RATE, image_embedding_noise=SIGMA, context_dropout=RATE, image_dropout=RATE, seed=SEED, draw=3)
            big = [ctx.train_sizes(B, enc) for enc in (False, True)]
            ctx.train_noise(off=True)
        sizes.append([ctx.train_sizes(B, enc) for enc in (False, True)])
        ft = FineTuner(model, B)
        if how == "zeros":                                               # (a FineTuner without noise clears the setting: put it back for the step)
            ft._select_noise = lambda: ctx.train_noise(seed=SEED, draw=3, sample_offset=2)
        losses.append(ft.forward_backward(*args).cpu())
    assert sizes[0] == sizes[1] == sizes[2], sizes
    assert torch.equal(losses[0], losses[1]) and torch.equal(losses[0], losses[2])
    E, P = g.enc_dim, g.patches
    assert big[0][2] - sizes[0][0][2] == B * P * E + B * E and big[1][2] - sizes[0][1][2] == B * E
    assert big[0][:2] == sizes[0][0][:2] and big[0][3] == sizes[0][0][3]


def test_refusals_leave_the_previous_setting_in_force(mid):
    from hypervla import _native as N
    s = mid
    ft = _tuner(s, **KNOBS["all"])
    args = (s["ins"], s["st"], s["tok"], s["batch"])
    _fixed(ft, draw=9)
    base = ft.forward_backward(*args).clone()
    ctx = s["model"]._ctx
    ft._select_noise = lambda: None                                       # from here on the context keeps what it has
    good = dict(policy_dropout=RATE, image_embedding_noise=SIGMA, context_dropout=RATE, image_dropout=RATE)
    bad = [dict(struct_size=C.sizeof(N.hvla_train_noise) - 4), dict(struct_size=0), dict(policy_dropout=1.0), dict(policy_dropout=-0.1),
           dict(context_dropout=float("nan")), dict(image_dropout=float("inf")), dict(image_dropout=1.5), dict(image_embedding_noise=-1e-3),
           dict(image_embedding_noise=float("inf")), dict(image_embedding_noise=float("nan"))]
    for change in bad:
        f = dict(good, struct_size=C.sizeof(N.hvla_train_noise), **change) if "struct_size" not in change else dict(good, **change)
        opts = N.hvla_train_noise(f["struct_size"], f["policy_dropout"], f["image_embedding_noise"], f["context_dropout"], f["image_dropout"],
                                  1, 0, 1)
        assert ctx.lib.hvla_train_noise_set(ctx.h, C.byref(opts)) == -1, change          # HVLA_E_SHAPE
        assert N._ERRORS[-1] == "HVLA_E_SHAPE"
    assert torch.equal(ft.forward_backward(*args), base)                  # seed, draw 9 and the four rates are still set
    ctx.train_noise(off=True)


# ---------------------------------------------------------------------------------------------------------------- FineTuner
def test_finetuner_draws_afresh_every_step_and_validates_without_noise(mid):
    s = mid
    ft = _tuner(s, dropout_rate=0.1, image_embedding_noise=0.05, peak_lr=1e-3)
    args = (s["ins"], s["st"], s["im"], s["batch"])
    tok = s["model"].encode_images(s["im"])
    a = ft.forward_backward(s["ins"], s["st"], tok, s["batch"]).clone()
    b = ft.forward_backward(s["ins"], s["st"], tok, s["batch"]).clone()
    assert ft.noise_draw == 2 and int((a != 0).sum()) >= B - 1 and (a != b)[a != 0].all()      # the same batch and parameters, consecutive draws
    v0 = ft.validate(*args)["mse"].clone()
    assert torch.equal(ft.validate(*args)["mse"], v0) and ft.noise_draw == 2
    losses, vals = [], []
    for i in range(10):
        losses.append(float(ft.step(*args, lr=1e-3)))
        vals.append(float(ft.validate(*args)["mse"]))
        assert torch.equal(ft.validate(*args)["mse"].cpu(), torch.tensor(vals[-1]))      # no step between: equal bits
    assert ft.noise_draw == 12 and ft.step_count == 10 and np.isfinite(losses).all() and np.isfinite(vals).all()
    assert len(set(vals)) == 10                                           # ... and only the parameter updates move it
    print("FineTuner with noise: losses", [f"{x:.4f}" for x in losses], "validation mse", [f"{x:.5f}" for x in vals])
