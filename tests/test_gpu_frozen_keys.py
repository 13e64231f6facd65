"""GPU: `frozen_keys` (create_optimizer's fnmatch patterns, octo/utils/train_utils.py:242-292) through FineTuner and the C ABI:
what a frozen bucket leaves out of the step, what the masked optimizer leaves alone, and the norm the clip is taken over."""
import numpy as np
import pytest

from adamw_ref import bf16_round as _bf16_round, optax_step as _optax_step

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CONTEXT = ("Transformer_0.*", "task_*", "initial_image_*", "layer_pos_embedding")
HEADS = ("output_head_*",)
BLOCKS = ("Transformer_0.encoderblock_*",)               # part of bucket 2: its gradients are computed, the optimizer ignores them
LAYER0 = ("encoder_image_encoder_encoder_layer_0_*",)


@pytest.fixture(scope="module")
def setup():
    """test_gpu_train's fixture: MID, B = 4, the float64 oracle's gradients on the oracle's own frozen-encoder tokens, once."""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    from hypervla import synthetic as syn
    from hypervla.config import MID, encoder_leaves, generated_leaves
    from hypervla.model import HyperVLA
    from hypervla.train import gradient_buckets
    from oracle import hvla_ref_np as onp, hvla_ref_torch as ot
    g, B = MID, 4
    model = HyperVLA.from_synthetic(g, max_batch=B)
    P = model.params
    ins, st, im = syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g), syn.synthetic_images(B, g)
    batch = syn.synthetic_action_batch(B, g)
    tok = onp.dinov2(P, g, dict(encoder_leaves(g)), onp.normalize_images(im[:, 0]))[:, 1:]
    per, loss, grads = ot.train_loss_and_grads(P, g, generated_leaves(g), ins, st, tok, batch)
    wcat = {name: off for name, off, _ in gradient_buckets(g)}["output_heads"]
    return dict(g=g, B=B, model=model, ins=ins, st=st, im=im, batch=batch, tok=tok.astype(np.float32), wcat=wcat,
                grads={k: v.numpy() for k, v in grads.items()})


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _state(ft):
    return dict(p=ft.params.clone(), mu=ft.mu.clone(), nu=ft.nu.clone(), ema=ft.ema.clone())


def _untouched(ft, before, where):
    """`where`: a slice or a bool mask over the flat vector."""
    return all(_same_bits(getattr(ft, name)[where], before[key][where])
               for name, key in (("params", "p"), ("mu", "mu"), ("nu", "nu"), ("ema", "ema")))


def _worst_leaf(s, ft, pick):
    """test_train_gradients_match_autograd's criterion over the leaves `pick` selects: max |d| of a leaf against
    max(|ref|, 1e-4 gmax), gmax over all leaves of the oracle."""
    from hypervla.train import unpack_params
    got = unpack_params(s["g"], ft.grads.cpu().numpy())
    gmax = max(np.abs(v).max() for v in s["grads"].values())
    worst = sorted(((np.abs(got[k].reshape(ref.shape) - ref).max() / max(np.abs(ref).max(), 1e-4 * gmax), k)
                    for k, ref in s["grads"].items() if pick(k)), reverse=True)
    assert len(worst) > 10
    print("worst relative gradient errors:", [(f"{r:.2e}", k) for r, k in worst[:4]])
    return worst[0]


def test_forward_loss_is_the_same_bits_under_any_mask(setup):
    from hypervla.train import FineTuner
    s = setup
    run = lambda ft: ft.forward_backward(s["ins"], s["st"], s["tok"], s["batch"], forward_only=True).clone()
    plain = FineTuner(s["model"], s["B"])
    assert plain.frozen is None and plain.frozen_buckets == 0 and plain.frozen_count == 0 and plain.trainable_count == plain.n
    want = run(plain)
    for keys in (CONTEXT, HEADS, BLOCKS, ("output_head_encoder_pos_embedding.kernel",), ("*hf_model*",)):
        ft = FineTuner(s["model"], s["B"], frozen_keys=keys)
        assert ft.frozen_count + ft.trainable_count == ft.n and (ft.frozen is None) == (ft.frozen_count == 0)
        assert _same_bits(run(ft), want), keys
    assert _same_bits(run(plain), want)


def test_context_frozen_three_steps(setup):
    from hypervla.train import FineTuner
    s, wcat = setup, setup["wcat"]
    ft = FineTuner(s["model"], s["B"], ema_start_step=0, frozen_keys=CONTEXT)
    assert ft.frozen_buckets == 4 and ft.frozen_count == wcat and bool(ft.frozen[:wcat].all()) and not bool(ft.frozen[wcat:].any())
    before = _state(ft)
    assert not before["mu"].any() and not before["nu"].any()
    ft.forward_backward(s["ins"], s["st"], s["tok"], s["batch"])
    assert not ft.grads[:wcat].any()
    worst = _worst_leaf(s, ft, lambda k: k.startswith("output_head_"))
    assert worst[0] <= 2e-3, worst
    for _ in range(3):
        ft.step(s["ins"], s["st"], s["im"], s["batch"], lr=1e-3)
        assert not ft.grads[:wcat].any()
    assert ft.step_count == 3
    assert _untouched(ft, before, slice(0, wcat))                      # params and ema their initial bits, mu and nu all zero
    assert not ft.mu[:wcat].any() and not ft.nu[:wcat].any()
    assert bool((ft.params[wcat:] != before["p"][wcat:]).any()) and bool(ft.nu[wcat:].any())


def test_heads_frozen_three_steps(setup):
    from hypervla.train import FineTuner
    s, wcat = setup, setup["wcat"]
    ft = FineTuner(s["model"], s["B"], ema_start_step=0, frozen_keys=HEADS)
    assert ft.frozen_buckets == 2 and ft.frozen_count == ft.n_hyper - wcat and bool(ft.frozen[wcat:].all())
    before = _state(ft)
    ft.forward_backward(s["ins"], s["st"], s["tok"], s["batch"])
    assert not ft.grads[wcat:ft.n_hyper].any()
    worst = _worst_leaf(s, ft, lambda k: not k.startswith("output_head_"))       # dtheta and dctx are still computed
    assert worst[0] <= 2e-3, worst
    for _ in range(3):
        ft.step(s["ins"], s["st"], s["im"], s["batch"], lr=1e-3)
        assert not ft.grads[wcat:ft.n_hyper].any()
    assert _untouched(ft, before, slice(wcat, ft.n_hyper))
    assert not ft.mu[wcat:].any() and not ft.nu[wcat:].any()
    assert bool((ft.params[:wcat] != before["p"][:wcat]).any())


@pytest.mark.parametrize("case", ["A-between-the-norms", "B-below-both"])
def test_the_norm_is_over_trainable_elements(setup, case):
    """BLOCKS frozen.  The oracle's gradients give N_train (the norm without the frozen leaves) and N_all; on this fixture
    N_all / N_train = 1.09, asserted >= 1.05 below as a condition on the input.  Case A, clip = sqrt(N_train N_all): the norm
    over trainable elements is below the clip (scale exactly 1), the norm over all elements would be above it.  Case B,
    clip = N_train / 2: the scale is < 1 and taken from the device's sqsum.  Two updates each; tolerances and the sqsum bound are
    test_adamw_six_updates_against_the_optax_chain's (sqsum_frozen_kernel has sqsum_kernel's grid, so its chain of additions).
    The sqsum bound (2.5e-4 relative) separates the two sums, which differ by 19 %, at both updates.  Which side of the clip the
    norm falls on is asserted at the first update, whose parameters are the ones the oracle's norms belong to; at the second the
    scale is whatever the device's sqsum gives, as in that test (one update at lr = 1e-3 moves every trainable weight, and the
    norms with them, by an amount the oracle was not asked about: on this fixture they fall to a fifth)."""
    from fnmatch import fnmatch
    from hypervla.train import FineTuner
    s = setup
    sq = lambda pick: sum(float((v.astype(np.float64) ** 2).sum()) for k, v in s["grads"].items() if pick(k))
    is_frozen = lambda k: fnmatch(k.replace("/", "."), BLOCKS[0])
    n_train, n_all = np.sqrt(sq(lambda k: not is_frozen(k))), np.sqrt(sq(lambda k: True))
    print(f"oracle: N_train {n_train:.4f}, N_all {n_all:.4f}, ratio {n_all / n_train:.4f}")
    assert n_all >= 1.05 * n_train
    clip = float(np.sqrt(n_train * n_all)) if case.startswith("A") else float(n_train / 2)
    ft = FineTuner(s["model"], s["B"], ema_start_step=0, clip=clip, frozen_keys=BLOCKS)
    assert ft.frozen_buckets == 0 and 0 < ft.frozen_count < s["wcat"]
    fz = ft.frozen.bool()
    tr = (~fz).cpu().numpy()
    lr, tol = 1e-3, 2e-6
    hy = dict(ft.hy, lr=lr, base_lr=lr)
    n = ft.n
    chain = -(-n // (1024 * 256)) + 6 + 1024 * 256 // 64 + 1
    r64 = lambda x: x.float().cpu().numpy().astype(np.float64)
    for it in range(2):
        ft.forward_backward(s["ins"], s["st"], s["tok"], s["batch"])
        assert bool(ft.grads[fz].any())                                     # computed and left in grads
        before = _state(ft)
        st = dict(p=r64(ft.params), mu=r64(ft.mu), nu=r64(ft.nu), ema=r64(ft.ema), g=r64(ft.grads), mask=ft.wd_mask.cpu().numpy(), p0=None)
        assert ft.apply(lr=lr) is True
        t = it + 1
        sq_dev = np.float32(ft.sqsum.cpu().numpy()[0])
        sq64 = float((st["g"][tr] ** 2).sum())
        sq64_all = float((st["g"] ** 2).sum())
        rel_sq = abs(float(sq_dev) - sq64) / sq64
        norm32, clip32 = np.sqrt(sq_dev), np.float32(clip)
        sc = 1.0 if norm32 < clip32 else float(clip32 / norm32)
        print(f"{case} update {t}: sqsum {float(sq_dev):.6g}, trainable {sq64:.6g} (rel {rel_sq:.2e}, bound {chain * 2.0 ** -24:.2e}), "
              f"all {sq64_all:.6g}, clip {clip:.6g}, scale {sc:.6g}")
        assert rel_sq <= chain * 2.0 ** -24, (t, rel_sq)
        if t == 1:                                                          # the parameters the oracle's norms were taken at
            if case.startswith("A"):
                assert sc == 1.0 and np.sqrt(sq64_all) > clip               # the norm over all elements would have clipped
            else:
                assert sc < 1.0
        want = _optax_step(st, hy, t, sc, ft.n_hyper)
        got_p, got_mu, got_nu, got_ema = r64(ft.params), r64(ft.mu), r64(ft.nu), r64(ft.ema)
        np.testing.assert_allclose(got_p[tr], want["p"][tr], rtol=0, atol=tol)
        np.testing.assert_allclose(got_ema[tr], want["ema"][tr], rtol=0, atol=tol)
        np.testing.assert_allclose(got_nu[tr], want["nu"][tr], rtol=1e-6, atol=1e-37)
        lo, hi = _bf16_round(want["m"] - want["band"]), _bf16_round(want["m"] + want["band"])
        exact = (got_mu == _bf16_round(want["m"]))[tr]
        within = ((got_mu >= np.minimum(lo, hi)) & (got_mu <= np.maximum(lo, hi)))[tr]
        assert within.all() and (~exact).mean() <= 1e-3, (t, int((~within).sum()), int((~exact).sum()))
        assert _untouched(ft, before, fz)                                   # the frozen elements: the same bits
        assert np.abs(got_p[tr] - st["p"][tr]).max() > 0


@pytest.mark.parametrize("source", [False, True], ids=["baked-table", "position-source"])
def test_encoder_group_leaves_a_frozen_layer_alone(source):
    """train_encoder=True, one DINOv2 layer frozen (adamw_frozen_kernel<true>), two steps; with a position_table_source the position
    leaf is frozen too: its tail and the baked slot derived from it keep their bits."""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    from hypervla import synthetic as syn
    from hypervla.config import MID
    from hypervla.model import HyperVLA
    from hypervla.train import POSITION_LEAF, FineTuner, train_param_layout
    g, B = MID, 2
    kw = dict(position_table_source=syn.synthetic_position_table_hub(g, 9)) if source else {}
    model = HyperVLA.from_synthetic(g, max_batch=B, **kw)
    ins, st, im = syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g), syn.synthetic_images(B, g)
    batch = syn.synthetic_action_batch(B, g)
    keys = LAYER0 + ((POSITION_LEAF,) if source else ())
    ft = FineTuner(model, B, train_encoder=True, ema_start_step=0, frozen_keys=keys)
    assert ft.frozen_buckets == 0 and (ft.source_n == 9) == source
    layout, total = train_param_layout(g, True, ft.source_n)
    rng = lambda prefix: [slice(off, off + int(np.prod(shape))) for name, off, shape in layout if name.startswith(prefix)]
    layer0, layer1 = rng("encoder_image_encoder_encoder_layer_0_"), rng("encoder_image_encoder_encoder_layer_1_")
    assert len(layer0) == len(layer1) == 18 and all(bool(ft.frozen[sl].all()) for sl in layer0)
    expect = sum(sl.stop - sl.start for sl in layer0) + ((ft.slot.stop - ft.slot.start) + (ft.tail.stop - ft.tail.start) if source else 0)
    assert ft.frozen_count == expect
    before = _state(ft)
    for _ in range(2):
        ft.step(ins, st, im, batch, lr=1e-3, base_lr=1e-4)
    assert _untouched(ft, before, ft.frozen.bool())
    for sl in layer0:
        assert _untouched(ft, before, sl)
    assert all(bool((ft.params[sl] != before["p"][sl]).any()) for sl in layer1)          # another layer's leaves moved
    assert bool((ft.params[:ft.n_hyper] != before["p"][:ft.n_hyper]).any())
    if source:
        assert _untouched(ft, before, ft.tail) and _untouched(ft, before, ft.slot)


def test_accumulation_with_the_context_frozen(setup):
    from hypervla.train import FineTuner
    s, wcat = setup, setup["wcat"]
    ft = FineTuner(s["model"], s["B"], grad_accumulation_steps=2, ema_start_step=0, frozen_keys=CONTEXT)
    before = _state(ft)
    ft.forward_backward(s["ins"], s["st"], s["tok"], s["batch"])
    assert ft.apply(lr=1e-3) is False and ft.step_count == 0
    assert _untouched(ft, before, slice(0, ft.n))                       # nothing moved on the first call
    ft.forward_backward(s["ins"], s["st"], s["tok"], s["batch"])
    assert ft.apply(lr=1e-3) is True and ft.step_count == 1
    assert _untouched(ft, before, slice(0, wcat))
    assert bool((ft.params[wcat:] != before["p"][wcat:]).any()) and bool((ft.ema[wcat:] != before["ema"][wcat:]).any())


def test_publish_after_training_the_heads_only(setup):
    from hypervla.model import HyperVLA
    from hypervla.train import FineTuner
    s = setup
    m = HyperVLA.from_synthetic(s["g"], max_batch=s["B"])                # its own model: publish changes what it serves
    theta0, ctx0 = (t.clone() for t in m.create_tasks(instruction_dict=s["ins"], initial_state=s["st"])[0].export())
    ft = FineTuner(m, s["B"], frozen_keys=CONTEXT)
    for _ in range(2):
        ft.step(s["ins"], s["st"], s["im"], s["batch"], lr=1e-3)
    ft.publish()
    theta1, ctx1 = m.create_tasks(instruction_dict=s["ins"], initial_state=s["st"])[0].export()
    assert _same_bits(ctx1, ctx0)                                        # the context encoder is the one that was loaded
    assert bool((theta1 != theta0).any())


def test_all_reduce_skips_the_frozen_bucket(setup, tmp_path, monkeypatch):
    import torch.distributed as dist
    from hypervla.train import FineTuner
    s, wcat = setup, setup["wcat"]
    ft = FineTuner(s["model"], s["B"], frozen_keys=CONTEXT)
    seen = []
    real = dist.all_reduce

    def recording(tensor, *a, **k):
        assert tensor.untyped_storage().data_ptr() == ft.grads.untyped_storage().data_ptr()
        seen.append((tensor.storage_offset(), tensor.numel()))
        return real(tensor, *a, **k)

    dist.init_process_group("nccl", init_method=f"file://{tmp_path}/rdzv", world_size=1, rank=0)
    try:
        monkeypatch.setattr(dist, "all_reduce", recording)
        ft.forward_backward(s["ins"], s["st"], s["tok"], s["batch"])
        ft.all_reduce_gradient(single_rank_too=True)
        torch.cuda.synchronize()
        assert seen == [(wcat, ft.n_hyper - wcat)]                       # the head bucket only
        s["model"]._ctx.train_wait_bucket(2, s["model"]._stream())      # the frozen bucket's event is still recorded
        s["model"]._ctx.train_wait_bucket(1, s["model"]._stream())
        torch.cuda.synchronize()
        assert not ft.grads[:wcat].any() and bool(ft.grads[wcat:].any())
    finally:
        monkeypatch.undo()
        dist.destroy_process_group()


def test_abi_refusals_and_turning_it_off(setup):
    from hypervla import _native
    from hypervla.train import FineTuner, frozen_plan
    s, wcat = setup, setup["wcat"]
    m, B = s["model"], s["B"]
    ctx = m._ctx
    ref = FineTuner(m, B)                                               # never sets a mask
    ref.forward_backward(s["ins"], s["st"], s["tok"], s["batch"])
    ref.apply(lr=1e-3)
    ft = FineTuner(m, B, grad_accumulation_steps=2)                     # (has an accumulator to hand to hvla_train_accumulate)
    ft.forward_backward(s["ins"], s["st"], s["tok"], s["batch"])
    tok, msk, cls, obs, tgt, am, tm = ft._keep
    ptrs = [tok.data_ptr(), msk.data_ptr(), cls.data_ptr(), obs.data_ptr(), None, tgt.data_ptr(), tm.data_ptr(), am.data_ptr()]
    n, n_enc = ctx.train_sizes(B, False)[0], ctx.train_sizes(B, True)[0]
    assert n == ft.n
    plan, flags = frozen_plan(s["g"], CONTEXT)
    mask, mask_enc = torch.as_tensor(plan).cuda(), torch.zeros(n_enc, dtype=torch.uint8, device="cuda")
    try:
        for args in ((mask.data_ptr(), n + 1, 0), (mask.data_ptr(), n - 1, 0), (mask.data_ptr(), 0, 0), (mask_enc.data_ptr(), n_enc, 1),
                     (mask.data_ptr(), n, 8), (mask.data_ptr(), n, -1)):
            with pytest.raises(_native.NativeError, match="HVLA_E_SHAPE"):
                ctx.train_frozen(*args)
        # a mask of the trained encoder's length, calls of the frozen encoder's: refused before any launch
        ctx.train_frozen(mask_enc.data_ptr(), n_enc, 0)
        torch.cuda.synchronize()
        before, g0, a0 = _state(ft), ft.grads.clone(), ft.acc.clone()
        st = m._stream()
        for call in (lambda: ctx.train_step(ft.buf, ptrs, B, ft._hyper(0.0), st),
                     lambda: ctx.train_step(ft.buf, ptrs, B, ft._hyper(0.0, forward_only=True), st),
                     lambda: ctx.train_apply(ft.buf, ft._hyper(1e-3), st),
                     lambda: ctx.train_accumulate(ft.buf, ft.acc.data_ptr(), 0.5, ft._hyper(0.0), st)):
            with pytest.raises(_native.NativeError, match="HVLA_E_STATE"):
                call()
            torch.cuda.synchronize()
            assert _untouched(ft, before, slice(0, n)) and _same_bits(ft.grads, g0) and _same_bits(ft.acc, a0)
        # set for this length, then NULL: the step and the update of a FineTuner that never set one
        ctx.train_frozen(mask.data_ptr(), n, flags)
        ctx.train_frozen(0, 0, 0)
        ctx.train_step(ft.buf, ptrs, B, ft._hyper(0.0), st)
        ctx.train_apply(ft.buf, ft._hyper(1e-3), st)
        torch.cuda.synchronize()
        assert bool(ft.grads[:wcat].any())                               # the context encoder's backward ran
        # test_bucketed_all_reduce_path_on_one_rank's comparison (split-K atomics: not bitwise; Adam's first step is lr sign(g))
        assert float(((ft.params - ref.params).abs() > 1e-5).float().mean()) < 1e-2
        assert bool((ft.params[:wcat] != before["p"][:wcat]).any())
    finally:
        ctx.train_frozen(0, 0, 0)
