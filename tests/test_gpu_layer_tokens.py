"""GPU: hypernet_kwargs.share_layer_index=False (`Geometry.layer_tokens`) and share_TF_output_head (`shared_block_heads`), DESIGN.md
§24 -- ctx_encoder_kernel_tokens and weightgen_tokens_kernel against the float64 restatement (tests/layer_tokens_ref.py).

Tolerances are the project's own (tests/test_gpu_parity.py): context 2e-5, theta 1e-4, policy from oracle tokens MAE 1e-4 / max 1e-3.
Shapes are the smallest at which each mechanism can break: one, two and three 16-row tiles of the context sequence up to its last row
(S = 48), the three widths of the weight generation (KS = 8, 4, 2), a second, ragged episode tile (B = 33), the README hypernetwork,
and a differential policy, whose arena has tiles that hold two tokens (tests/native/layer_tokens_check.cpp counts them).

Measured on one MI355X: context max 9.3e-8 to 1.6e-7 and theta max 3.5e-6 to 4.3e-6 over all parity cases (README hypernetwork
1.6e-7 / 3.7e-6); routing worst relative error 5.6e-6 against 2^-16 = 1.5e-5, with token gaps of 1.3e-3 and 4.6e-3; policy from the
oracle's tokens on the generated handle action MAE 8.8e-6, max 3.1e-5, logit max 3.1e-5."""
import copy
import ctypes
import dataclasses
import gc

import numpy as np
import pytest

import layer_tokens_ref as LR

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X; torch.cuda.is_available() is False")


def _geo(shared=False, base="MID", **kw):
    from hypervla import config
    return dataclasses.replace(getattr(config, base), layer_tokens=True, shared_block_heads=shared, **kw)


def _rows(ins, st, sl):
    return ({"language_instruction": {k: np.asarray(v)[sl] for k, v in ins["language_instruction"].items()}},
            {"patch_embeddings": np.asarray(st["patch_embeddings"])[sl]})


def _export(w):
    theta, ctx = w.export()
    return theta.cpu().numpy(), ctx.cpu().numpy()


def _parity(g, B, what):
    """create_tasks of a new model of geometry g against the restatement: the context and the whole theta."""
    _need_gpu()
    from hypervla import synthetic as syn
    from hypervla.model import HyperVLA
    m = HyperVLA.from_synthetic(g, max_batch=B)
    ins, st = syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g)
    _, rctx, rtheta = LR.create_tasks(m.params, g, ins, st)
    w, _, _ = m.create_tasks(instruction_dict=ins, initial_state=st)
    theta, ctx = _export(w)
    assert ctx.shape == (B, g.num_layer_tokens, g.ctx_dim) == rctx.shape and theta.shape == rtheta.shape
    assert m._ctx.num_layer_tokens == g.num_layer_tokens
    dc, dt = np.abs(ctx - rctx), np.abs(theta - rtheta)
    print("%s: S = %d, B = %d, context max %.3e, theta max %.3e" % (what, g.ctx_seq, B, dc.max(), dt.max()))
    # token 0 (the shared image encoder's) is computed and exported like the rest; no leaf reads it
    assert dc.max() <= 2e-5, (dc.max(), np.unravel_index(dc.argmax(), dc.shape))
    assert dt.max() <= 1e-4, (dt.max(), np.unravel_index(dt.argmax(), dt.shape))
    return m, theta, rtheta


CASES = {
    "mid_two_row_tiles": (dict(), 3),                                            # S = 20
    "last_row_of_the_second_tile": (dict(lang_tokens=24), 3),                    # S = 32
    "first_row_of_the_third_tile": (dict(lang_tokens=25), 3),                    # S = 33
    "three_row_tiles": (dict(lang_tokens=26), 1),                                # S = 34
    "last_row_of_the_last_tile": (dict(layers=4, lang_tokens=38), 2),            # S = 48
    "ks2": (dict(ctx_dim=32, ctx_heads=2), 3),
    "ks4": (dict(ctx_dim=64), 3),
    "two_episode_tiles": (dict(), 33),
    "language_tokens_in_the_policy": (dict(lang_in_policy=True), 2),             # NL = 8
    "differential": (dict(differential=True), 3),                                # tiles of two tokens
}


@pytest.mark.parametrize("shared", [False, True], ids=["own_heads", "shared_heads"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_parity_with_the_restatement(case, shared):
    kw, B = CASES[case]
    g = _geo(shared, **kw)
    if case == "last_row_of_the_last_tile":
        assert g.ctx_seq == 48
    _parity(g, B, case + (" shared heads" if shared else ""))
    gc.collect()


def test_one_row_more_than_three_tiles_is_refused_at_create():
    _need_gpu()
    from hypervla import _native
    g = _geo(layers=5, lang_tokens=38)
    assert g.ctx_seq == 49
    with pytest.raises(_native.NativeError, match="HVLA_E_SHAPE"):
        _native.Context(g, 0, 2)
    _native.Context(dataclasses.replace(g, layer_tokens=False), 0, 2).close()      # the rows alone refuse it


@pytest.mark.parametrize("shared", [False, True], ids=["own_heads", "shared_heads"])
def test_readme_hypernetwork(shared):
    """FULL(layer_tokens=True): S = 42, G = 201 500, B = 2; generation only, no image-encoder pass."""
    g = _geo(shared, base="FULL")
    assert g.ctx_seq == 42
    _, theta, ref = _parity(g, 2, "README hypernetwork" + (" shared heads" if shared else ""))
    assert theta.shape == (2, 201_500)
    np.testing.assert_allclose(theta.astype(np.float64).sum(1), ref.sum(1), atol=2e-2)
    np.testing.assert_allclose(np.abs(theta.astype(np.float64)).sum(1), np.abs(ref).sum(1), rtol=1e-5)
    gc.collect()


def _routing_params(g, B, ins, st):
    """Synthetic parameters whose heads are zero but for kernel row 0 = 1, from the first seed at which, on the restatement, any
    two of the NL - 1 used tokens differ in channel 0 of the context by more than 1e-3 in every episode."""
    from hypervla import synthetic as syn
    for seed in range(syn.SEED_WEIGHTS, syn.SEED_WEIGHTS + 20):
        P = dict(syn.synthetic_params(g, seed))
        for k in P:
            if k.startswith("output_head_"):
                P[k] = np.zeros_like(P[k])
                if k.endswith("/kernel"):
                    P[k][0] = 1.0
        c0 = LR.context_embedding(P, g, ins["language_instruction"]["token_embedding"], ins["language_instruction"]["attention_mask"],
                                  np.asarray(st["patch_embeddings"])[:, 0])[:, 1:, 0]
        gap = np.abs(c0[:, :, None] - c0[:, None, :]) + 10.0 * np.eye(c0.shape[1])
        if gap.min() > 1e-3:
            return P, gap.min()
    raise AssertionError("no seed separates the tokens")


@pytest.mark.parametrize("kw", [dict(), dict(differential=True), dict(shared=True, lang_in_policy=True)],
                         ids=["mid", "differential", "shared_heads_language"])
def test_every_element_reads_its_own_token(kw):
    """Routing without the restatement's heads: with every head's kernel zero but row 0 = 1 and every bias 0, each element of leaf p
    is ctx[b, token_of(p), 0] to 2^-16 relative (the split-bf16 product of 1 and the context, split again in the matrix region).
    The differential geometry has a tile that holds two tokens; the vector region is covered whole."""
    _need_gpu()
    from hypervla import synthetic as syn
    from hypervla.config import generated_leaves, token_of
    from hypervla.model import HyperVLA
    g, B = _geo(**kw), 3
    ins, st = syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g)
    P, gap = _routing_params(g, B, ins, st)
    m = HyperVLA.from_synthetic(g, params=P, max_batch=B)
    w, _, _ = m.create_tasks(instruction_dict=ins, initial_state=st)
    theta, ctx = _export(w)
    worst = 0.0
    for lf in generated_leaves(g):
        want = ctx[:, token_of(g, lf), 0].astype(np.float64)[:, None]
        got = theta[:, lf.offset:lf.offset + lf.size].astype(np.float64)
        rel = np.abs(got - want) / np.abs(want)
        worst = max(worst, rel.max())
        assert rel.max() <= 2.0 ** -16, (lf.path, rel.max())
    print("routing %s: smallest token gap %.3e, worst relative error %.3e (2^-16 = %.3e)" % (kw, gap, worst, 2.0 ** -16))
    gc.collect()


@pytest.fixture(scope="module")
def mid():
    _need_gpu()
    from hypervla import synthetic as syn
    from hypervla.model import HyperVLA
    g, B = _geo(), 33
    m = HyperVLA.from_synthetic(g, max_batch=B)
    ins, st = syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g)
    w, _, _ = m.create_tasks(instruction_dict=ins, initial_state=st)
    theta, ctx = _export(w)
    yield dict(g=g, m=m, B=B, ins=ins, st=st, w=w, theta=theta, ctx=ctx)
    gc.collect()


def test_an_episode_alone_equals_its_row_and_runs_repeat(mid):
    m = mid["m"]
    for b in (0, 31, 32):                            # the first tile's ends and the ragged second tile's only row
        w1, _, _ = m.create_tasks(**dict(zip(("instruction_dict", "initial_state"), _rows(mid["ins"], mid["st"], slice(b, b + 1)))))
        t1, c1 = _export(w1)
        assert np.array_equal(t1[0], mid["theta"][b]) and np.array_equal(c1[0], mid["ctx"][b]), b
    w2, _, _ = m.create_tasks(instruction_dict=mid["ins"], initial_state=mid["st"])
    t2, c2 = _export(w2)
    assert np.array_equal(t2, mid["theta"]) and np.array_equal(c2, mid["ctx"])


def test_pool_slots_equal_create_tasks(mid):
    m, B = mid["m"], mid["B"]
    perm = np.random.default_rng(5).permutation(B)
    pool = m.create_pool(B)
    K = 20
    ins, st = _rows(mid["ins"], mid["st"], slice(0, K))
    m.assign_tasks(pool, perm[:K].tolist(), ins, st)              # episode k -> slot perm[k]
    theta, ctx = _export(pool)
    assert np.array_equal(theta[perm[:K]], mid["theta"][:K]) and np.array_equal(ctx[perm[:K]], mid["ctx"][:K])
    assert not theta[perm[K:]].any() and not ctx[perm[K:]].any()  # the other slots keep their zeros


def test_save_load_and_copy_round_trip(mid, tmp_path):
    m, B, NL = mid["m"], mid["B"], mid["g"].num_layer_tokens
    path = str(tmp_path / "tasks.npz")
    mid["w"].save(path)
    with np.load(path) as z:
        assert z["context"].shape == (B, NL, mid["g"].ctx_dim)
    theta, ctx = _export(m.load_tasks(path))
    assert np.array_equal(theta, mid["theta"]) and np.array_equal(ctx, mid["ctx"])
    pool = m.create_pool(8)
    m.copy_tasks(pool, [6, 1, 3], mid["w"], [32, 0, 7])
    theta, ctx = _export(pool)
    assert np.array_equal(theta[[6, 1, 3]], mid["theta"][[32, 0, 7]]) and np.array_equal(ctx[[6, 1, 3]], mid["ctx"][[32, 0, 7]])
    # a file whose context width does not fit is refused, like a wrong G; so is a [B, C] context given to import
    bad = str(tmp_path / "bad.npz")
    np.savez(bad, theta=mid["theta"][:2], context=mid["ctx"][:2, 0], G=np.int64(mid["theta"].shape[1]))
    with pytest.raises(ValueError, match="context"):
        m.load_tasks(bad)
    with pytest.raises(ValueError, match="context"):
        m.import_tasks(mid["theta"][:2], context=mid["ctx"][:2, 0])


def test_the_policy_kernels_read_the_arena_the_new_kernel_wrote():
    """MID: policy_from_tokens on the oracle's tokens with the generated handle against oracle.policy on the restated base_params."""
    _need_gpu()
    from hypervla import synthetic as syn
    from hypervla.config import encoder_leaves
    from hypervla.model import HyperVLA
    from oracle import hvla_ref_np as onp
    g, B = _geo(shared=True), 4
    m = HyperVLA.from_synthetic(g, max_batch=B)
    ins, st, im = syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g), syn.synthetic_images(B, g)
    bp, _, _ = LR.create_tasks(m.params, g, ins, st)
    ract, rlog, _, tok = onp.sample_actions(m.params, g, dict(encoder_leaves(g)), bp, im)
    w, _, _ = m.create_tasks(instruction_dict=ins, initial_state=st)
    act, logit = (t.cpu().numpy() for t in m.policy_from_tokens(tok.astype(np.float32), w))
    d = np.abs(act[..., :6] - ract[..., :6])
    print("policy from oracle tokens on the generated handle: action MAE %.3e max %.3e, logit max %.3e" % (d.mean(), d.max(), np.abs(logit - rlog).max()))
    assert d.mean() <= 1e-4 and d.max() <= 1e-3, (d.mean(), d.max())
    # ... and the blocks did receive different weights from their one set of heads
    k = "encoder_Transformer_0_encoderblock_%d_MlpBlock_0_Dense_0_kernel"
    assert np.abs(bp[k % 0] - bp[k % 1]).max() > 1e-3
    gc.collect()


def test_both_new_fields_zero_is_the_v3_context():
    """hvla_create_with_v4 with layer_tokens = shared_block_heads = 0 (and with NULL options): theta, context and actions bit for bit
    those of hvla_create_with_v3."""
    _need_gpu()
    from hypervla import _native, synthetic as syn
    from hypervla.config import MID, hypernet_param_shapes
    g, B = MID, 3
    P = syn.synthetic_params(g)
    ins, st = syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g)
    dev = torch.device("cuda", 0)
    tok = torch.as_tensor(np.asarray(ins["language_instruction"]["token_embedding"], np.float32)).to(dev).contiguous()
    mask = torch.as_tensor(np.asarray(ins["language_instruction"]["attention_mask"], np.int64)).to(dev).contiguous()
    cls = torch.as_tensor(np.ascontiguousarray(np.asarray(st["patch_embeddings"], np.float32)[:, 0])).to(dev).contiguous()
    ptok = torch.as_tensor(np.random.default_rng(2).standard_normal((B, g.patches, g.enc_dim)).astype(np.float32)).to(dev)
    base = _native.Context(g, 0, B)
    lib = base.lib

    def made_by(entry, opts):
        c = copy.copy(base)
        c.h = ctypes.c_void_p()
        rc = entry(ctypes.byref(base.cfg), ctypes.byref(opts) if opts is not None else None, 0, ctypes.byref(c.h))
        assert rc == 0, rc
        return c

    v3 = _native.hvla_policy_options_v3(ctypes.sizeof(_native.hvla_policy_options_v3), 0, 0, 0)
    v4 = _native.hvla_policy_options_v4(ctypes.sizeof(_native.hvla_policy_options_v4), 0, 0, 0, 0, 0)
    out = []
    for c in (made_by(lib.hvla_create_with_v3, v3), made_by(lib.hvla_create_with_v4, v4), made_by(lib.hvla_create_with_v4, None)):
        assert c.num_layer_tokens == 1
        c.load_weights({k: P[k] for k in hypernet_param_shapes(g)})
        w = c.generate(tok.data_ptr(), mask.data_ptr(), cls.data_ptr(), B)
        theta = torch.empty(B, c.num_generated, dtype=torch.float32, device=dev)
        ctx = torch.empty(B, g.ctx_dim, dtype=torch.float32, device=dev)
        act = torch.empty(B, g.horizon, g.action_dim, dtype=torch.float32, device=dev)
        c.weights_export(w, theta.data_ptr(), ctx.data_ptr())
        c.policy(w, ptok.data_ptr(), act.data_ptr(), None, B)
        torch.cuda.synchronize()
        out.append((theta.cpu().numpy(), ctx.cpu().numpy(), act.cpu().numpy()))
        c.weights_free(w)
        c.close()
    for other in out[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(out[0], other))
    # the struct's exact-size rule, and shared heads without layer tokens
    h = ctypes.c_void_p()
    v4.struct_size -= 4
    assert lib.hvla_create_with_v4(ctypes.byref(base.cfg), ctypes.byref(v4), 0, ctypes.byref(h)) == -1 and not h.value
    bad = _native.hvla_policy_options_v4(ctypes.sizeof(_native.hvla_policy_options_v4), 0, 0, 0, 0, 1)
    assert lib.hvla_create_with_v4(ctypes.byref(base.cfg), ctypes.byref(bad), 0, ctypes.byref(h)) == -1 and not h.value
    assert b"shared_block_heads" in lib.hvla_last_error(None)
    base.close()


def test_fine_tuning_is_refused_by_name(mid):
    from hypervla import _native
    from hypervla.train import FineTuner
    with pytest.raises(ValueError, match="share_layer_index"):
        FineTuner(mid["m"], 2)
    with pytest.raises(_native.NativeError, match="HVLA_E_SHAPE.*share_layer_index"):
        mid["m"]._ctx.train_sizes(2)
