"""GPU parity at the edges of hvla_create's contract (csrc/accept.h): every case stands on one edge of the
set of geometries the library accepts -- the policy kernel's head tile, its MLP tile count, the layer counts its LDS admits, the
context attention's ragged key tiles and narrowest heads, the encoder's widths, patch sizes and GEMM forms -- and is compared stage
by stage with the float64 oracle (oracle/hvla_ref_np.py; tests/lang_policy_ref.py is the same oracle with use_language_token) on the
seeded inputs of hypervla.synthetic.  Tolerances are the table at the top of tests/test_gpu_parity.py, not widened:

  context                      max <= 2e-5
  theta                        max <= 1e-4
  policy from oracle tokens    action MAE <= 1e-4, max <= 1e-3, logits <= 1e-3; the gripper bit where the oracle's |logit| > 2e-3
  tokens                       f16 rms <= 2e-3, max <= 2e-2; bf16 rms <= 1.2e-2
  end to end                   action MAE <= 5e-4, max <= 2e-3 (E = 1024 with bf16 operands: 3 x the float64 emulation of its operand
                               rounding, E1024_BF16_END_TO_END below)

Every case prints its figures before it asserts (DESIGN.md section 16 records one run).  What the contract refuses is asserted too:
HVLA_E_SHAPE at create, never a crash and never a failure at the first launch."""
import functools
import gc

import numpy as np
import pytest

from geometry_cases import ENCODER_P64, ENCODER_P256, _full, _mid

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X; torch.cuda.is_available() is False")


@functools.lru_cache(maxsize=2)
def _oracle(g, B):
    """The float64 reference of one case, computed once: context, theta, patch tokens, actions and logits from those tokens."""
    from hypervla import synthetic as syn
    from hypervla.config import encoder_leaves, generated_leaves
    from oracle import hvla_ref_np as onp
    import lang_policy_ref as LR
    P = syn.synthetic_params(g)
    leaves = generated_leaves(g)
    ins, st, im = syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g), syn.synthetic_images(B, g)
    bp, ctx = onp.create_tasks(P, g, leaves, ins, st)
    theta = np.concatenate([bp[l.flat_name].reshape(B, -1) for l in leaves], 1)
    act, logit, tok = LR.sample_actions(P, g, dict(encoder_leaves(g)), bp, im, ins["language_instruction"]["token_embedding"])
    return dict(P=P, ins=ins, st=st, im=im, ctx=ctx[:, 0], theta=theta, tok=tok, act=act, logit=logit)


# The one case with a bound of its own: bf16 operands at E = 1024 exceed the end-to-end tolerance by operand rounding alone.  The
# float64 emulation of the encoder with every operand site rounded to bf16 and the per-image compensation of the weight rounding
# (`python tests/studies/precision_budget.py --geometry e1024 --episodes 9 --study bias --kind bf16`: this case's geometry, batch and
# inputs) gives action MAE 8.70e-4, max 3.42e-3, mean |d logit| 9.04e-4 against exact float64; the bounds are 3 x those (the factor
# covers what the emulation leaves out: the f32 accumulation order).  Measured on the GPU: 8.16e-4 / 3.28e-3 / 8.66e-4.
E1024_BF16_END_TO_END = (3 * 8.70e-4, 3 * 3.42e-3, 3 * 9.04e-4)


def _check(name, g, B=5, enc_dtype="f16", max_batch=None, end_to_end=(5e-4, 2e-3, 2e-3)):
    """All four stages of one geometry against the oracle; prints the figures, then asserts the module's tolerances.
    end_to_end: (action MAE, action max, mean |d gripper logit|)."""
    _need_gpu()
    from hypervla.model import HyperVLA
    o = _oracle(g, B)
    m = HyperVLA.from_synthetic(g, params=o["P"], max_batch=max_batch or max(8, B), enc_dtype=enc_dtype)
    ad = g.action_dim
    w, tasks, _ = m.create_tasks(instruction_dict=o["ins"], initial_state=o["st"])
    theta, ctx = (t.cpu().numpy().astype(np.float64) for t in w.export())
    assert theta.shape == o["theta"].shape
    d_ctx, d_theta = np.abs(ctx - o["ctx"]).max(), np.abs(theta - o["theta"]).max()
    tok = m.encode_images(o["im"]).cpu().numpy().astype(np.float64)
    dt = tok - o["tok"]
    tok_rms, tok_max = np.sqrt((dt * dt).mean()), np.abs(dt).max()
    act, logit = (t.cpu().numpy() for t in m.policy_from_tokens(o["tok"].astype(np.float32), w))
    dp, dl = np.abs(act[..., :ad - 1] - o["act"][..., :ad - 1]), np.abs(logit - o["logit"])
    act2, inter = m.sample_actions(o["im"], o["ins"], tasks, np.ones((B, 1)), w)
    de = np.abs(act2[..., :ad - 1] - o["act"][..., :ad - 1])
    dle = np.abs(inter["gripper_logits"] - o["logit"])
    print("geometry contract | %s | B %d %s | ctx %.2e | theta %.2e | tokens rms %.2e max %.2e | policy MAE %.2e max %.2e logit %.2e | "
          "end to end MAE %.2e max %.2e logit mean %.2e | smallest oracle |logit| %.1e"
          % (name, B, enc_dtype, d_ctx, d_theta, tok_rms, tok_max, dp.mean(), dp.max(), dl.max(), de.mean(), de.max(), dle.mean(),
             np.abs(o["logit"]).min()))
    del w
    del m
    gc.collect()
    assert act.shape == act2.shape == (B, g.horizon, ad) and logit.shape == (B, g.horizon)
    assert d_ctx <= 2e-5, d_ctx
    assert d_theta <= 1e-4, d_theta
    if enc_dtype == "f16":
        assert tok_rms <= 2e-3 and tok_max <= 2e-2, (tok_rms, tok_max)
    else:
        assert tok_rms <= 1.2e-2, tok_rms
    assert dp.mean() <= 1e-4 and dp.max() <= 1e-3, (dp.mean(), dp.max())
    assert dl.max() <= 1e-3, dl.max()
    safe = np.abs(o["logit"]) > 2e-3
    assert (act[..., ad - 1][safe] == o["act"][..., ad - 1][safe]).all()
    assert np.abs(act[..., :ad - 1]).max() <= g.max_action and set(np.unique(act[..., ad - 1])) <= {0.0, 1.0}
    assert de.mean() <= end_to_end[0] and de.max() <= end_to_end[1], (de.mean(), de.max())
    assert dle.mean() <= end_to_end[2], dle.mean()


# ------------------------------------------------------------------------------------------------ policy kernel + weight generation
# The largest policies the policy kernel's LDS admits at P = 256 (policy_lds_bytes of csrc/accept.h; tests/native/accept_check.cpp
# pins these four numbers to that function): layers at mlp = 128 / mlp at 4 layers, without and with the language prefix's 8 KiB.
MAX_LAYERS, MAX_MLP, MAX_LAYERS_LANG, MAX_MLP_LANG = 7, 768, 4, 256

POLICY_EDGES = {
    "horizon 1": dict(horizon=1),
    "32 head rows (4 x 8)": dict(horizon=4, action_dim=8),
    "horizon 16 x 2": dict(horizon=16, action_dim=2),
    "horizon 8 x 4": dict(horizon=8, action_dim=4),
    "mlp 32 (one hidden tile)": dict(mlp=32, layers=1),
    "mlp 160 (five hidden tiles) x 3 layers": dict(mlp=160, layers=3),
    "language tokens in the policy, 2": dict(lang_in_policy=True, lang_tokens=2),
    "language tokens in the policy, 32": dict(lang_in_policy=True, lang_tokens=32),
}


@pytest.mark.parametrize("edge", sorted(POLICY_EDGES))
@pytest.mark.parametrize("base", ["mid", "full"])
def test_policy_edges(base, edge):
    g = (_mid if base == "mid" else _full)(**POLICY_EDGES[edge])
    _check("%s, %s" % (base, edge), g)


@pytest.mark.parametrize("edge,change", [
    ("most layers at mlp 128", dict(layers=MAX_LAYERS, mlp=128)),
    ("widest mlp at 4 layers", dict(layers=4, mlp=MAX_MLP)),
    ("language: most layers at mlp 128", dict(lang_in_policy=True, layers=MAX_LAYERS_LANG, mlp=128)),
    ("language: widest mlp at 4 layers", dict(lang_in_policy=True, layers=4, mlp=MAX_MLP_LANG)),
])
def test_largest_policies_the_lds_admits(edge, change):
    _check("full, " + edge, _full(**change))


# ------------------------------------------------------------------------------------------------ context encoder
CONTEXT_EDGES = {
    "2 tokens (S = 4)": (dict(lang_tokens=2), 5),
    "38 tokens of 20 (third key tile ragged, one short K chunk)": (dict(lang_tokens=38, lang_dim=20), 5),
    "38 tokens of 20, two episode tiles": (dict(lang_tokens=38, lang_dim=20), 37),
    "14 tokens (S = 16, the last row of the first tile)": (dict(lang_tokens=14), 3),
    "15 tokens, ctx_mlp 48": (dict(lang_tokens=15, ctx_mlp=48), 5),
    "head width 4 (32 / 8), ctx_mlp 16": (dict(ctx_dim=32, ctx_heads=8, ctx_mlp=16), 5),
    "one head of 128": (dict(ctx_dim=128, ctx_heads=1), 5),
    "lang_dim 392 (a second K chunk of 8)": (dict(lang_dim=392), 5),
    "no context layers": (dict(ctx_layers=0), 5),
}


@pytest.mark.parametrize("edge", sorted(CONTEXT_EDGES))
def test_context_edges(edge):
    change, B = CONTEXT_EDGES[edge]
    _check("mid, " + edge, _mid(**{**dict(ctx_layers=2), **change}), B=B, max_batch=40 if B > 8 else None)


# ------------------------------------------------------------------------------------------------ image encoder
@pytest.mark.parametrize("B", [5, 40])
@pytest.mark.parametrize("edge", sorted(ENCODER_P64))
def test_encoder_edges_at_64_patches(edge, B):
    """B = 5: 325 rows, the small-batch forms; B = 40: 2600 rows, past G64_MAXM, the 128 x 128 kernels (P = 64 has no image-aligned tiles)."""
    _check("mid, %s" % edge, _mid(**ENCODER_P64[edge]), B=B, max_batch=40)


@pytest.mark.parametrize("edge", sorted(ENCODER_P256))
def test_encoder_edges_at_256_patches(edge):
    """B = 9: 2313 rows, image-aligned 256-row tiles, a ragged last 64-row block of the small launch in front of each GEMM; two
    encoder layers (fc2 then carries the next layer's norm1) except where the oracle would take more than a few seconds.  The
    same image alone (B = 1) and in a batch of 4, through the small-batch kernels, gets the same tokens bit for bit."""
    _need_gpu()
    from hypervla.model import HyperVLA
    change, dtype = ENCODER_P256[edge]
    g = _full(**{**dict(enc_layers=2), **change})
    _check("full, %s" % edge, g, B=9, enc_dtype=dtype, max_batch=16,
           **(dict(end_to_end=E1024_BF16_END_TO_END) if dtype == "bf16" else {}))
    o = _oracle(g, 9)
    m = HyperVLA.from_synthetic(g, params=o["P"], max_batch=16, enc_dtype=dtype)
    im = o["im"][:, 0]
    nine = m.encode_images(im).cpu()
    for B in (1, 4):
        assert torch.equal(m.encode_images(im[:B]).cpu()[0], nine[0]), B
    assert torch.equal(m.encode_images(np.ascontiguousarray(im[[3, 8, 0]])).cpu()[1], nine[8])


@pytest.mark.parametrize("E,B", [(1024, 64), (512, 128), (256, 256)])
def test_persistent_fused_layernorm_once_per_column_tile_count(E, B):
    """The persistent form of the LayerNorm fused into the 256 x 256 GEMM's epilogue (csrc/plan.h lnx_persistent: B % 8 == 0 and
    B * nbn % 256 == 0 on 256 CUs) with nbn = E / 256 = 4, 2, 1 column tiles per image, at the smallest batch that takes it: the
    first and the last image get, bit for bit, the tokens they get in a batch of 9 (one workgroup per tile).  That these batches
    take the persistent kernels on 256 CUs, and a batch of 9 does not, is pinned on the host (tests/native/plan_check.cpp)."""
    _need_gpu()
    from hypervla import synthetic as syn
    from hypervla.model import HyperVLA
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    if ncu != 256:
        pytest.skip("the persistent fused-LayerNorm launch is planned from the CU count: these batch sizes take it on 256 CUs, this device has %d" % ncu)
    g = _full(enc_dim=E, enc_heads=E // 64, enc_mlp=2 * E)
    m = HyperVLA.from_synthetic(g, max_batch=B)
    im = syn.synthetic_images(B, g)[:, 0]
    big = m.encode_images(im).cpu()
    nine = m.encode_images(np.ascontiguousarray(im[[0, 1, 2, 3, 4, 5, 6, 7, B - 1]])).cpu()
    assert torch.isfinite(big).all()
    assert torch.equal(big[0], nine[0]) and torch.equal(big[B - 1], nine[8])


# ------------------------------------------------------------------------------------------------ what the contract refuses
REFUSED = {
    "one layer past the policy's LDS": lambda: _full(layers=MAX_LAYERS + 1, mlp=128),
    "one hidden tile past the policy's LDS": lambda: _full(layers=4, mlp=MAX_MLP + 32),
    "language: one layer past the policy's LDS": lambda: _full(lang_in_policy=True, layers=MAX_LAYERS_LANG + 1, mlp=128),
    "language: one hidden tile past the policy's LDS": lambda: _full(lang_in_policy=True, layers=4, mlp=MAX_MLP_LANG + 32),
    "language: 33 tokens": lambda: _mid(lang_in_policy=True, lang_tokens=33),
    "33 head rows": lambda: _mid(horizon=3, action_dim=11),
    "no horizon": lambda: _mid(horizon=0),
    "action_dim 1": lambda: _mid(action_dim=1),
    "1 token": lambda: _mid(lang_tokens=1),
    "39 tokens": lambda: _mid(lang_tokens=39),
    "lang_dim 22": lambda: _mid(lang_dim=22),
    "mlp 48": lambda: _mid(mlp=48),
    "enc_dim 1152": lambda: _full(enc_dim=1152, enc_heads=18),
    "ctx_dim 96": lambda: _mid(ctx_dim=96),
    "36 patches": lambda: _mid(image_size=84),
    "context head width 2 (32 / 16)": lambda: _mid(ctx_dim=32, ctx_heads=16),
    "context head width 2 (64 / 32)": lambda: _mid(ctx_dim=64, ctx_heads=32),
    "context head width 1": lambda: _mid(ctx_dim=128, ctx_heads=128),
    "zero policy heads": lambda: _mid(heads=0),
    "zero patch": lambda: _mid(patch=0),
    "zero encoder heads": lambda: _mid(enc_heads=0),
    "zero context heads": lambda: _mid(ctx_heads=0),
    "negative encoder layers": lambda: _mid(enc_layers=-1),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_refused_at_create(what):
    _need_gpu()
    from hypervla import _native
    from hypervla.config import MID
    with pytest.raises(_native.NativeError, match="HVLA_E_SHAPE"):
        _native.Context(REFUSED[what](), 0, 4)
    _native.Context(MID, 0, 4).close()               # a valid model can still be created afterwards, in the same process
