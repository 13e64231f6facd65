"""GPU: the reference's attention entropy / alignment terms in the fine-tune step (hvla_train_attention_losses, attention_aux_kernel)
against float64 autograd through tests/attention_loss_ref.py.

Tolerances are those tests/test_gpu_train.py holds the same quantities to: loss rtol 2e-4, atol 2e-5; worst leaf gradient 2e-3 relative
with the 1e-4 gmax floor.

Weights of the cases.  Chosen on the float64 reference alone, so that the terms cannot pass by being negligible; every test asserts
both conditions on the oracle before it looks at the device: (a) ||g_aux - g_0|| / ||g_0|| >= 0.05 over the hypernetwork leaves,
(b) every per-sample loss moves by >= 100 x its tolerance (100 x (2e-5 + 2e-4 |loss_b|)).  Measured on the CPU, per unit weight:
    geometry                        ent_b        align_b         |dg| / |g_0| per unit w_ent, w_align     weights needed (a), (b)
    MID, B = 4, frozen encoder      3.47-3.74    1.14e-3-1.46e-3  4.37e-2, 2.32e-5                         w_ent 1.15, 0.26; w_align 2156, 690
    MID, B = 2, trained encoder     3.39-3.47    1.23e-3-1.27e-3  4.13e-2, 2.35e-5                         w_ent 1.21, 0.29; w_align 2128, 781
    README geometry, B = 2, frozen  4.75-5.01    4.0e-5-9.8e-5    2.35e-2, 8.63e-7                         w_ent 2.13, 0.23; w_align 57 927, 22 489
(align_b is of order 1 / P^2, hence the large alignment weights.)  Used, one term on: MID w_ent = 2 (ratio 0.087; the losses move by
6.9-7.5 where 0.9 is needed), w_align = 4000 (0.093; 4.6-5.8).  With both on the two gradients partly oppose each other -- MID (2, 4000)
gives 0.064 with the frozen and 0.052 with the trained encoder, the README geometry (4, 100 000) 0.057 -- so the both-terms cases use
more: MID (3, 6000): 0.096 frozen, 0.119 with sample 0 masked, 0.078 trained encoder (there the terms also move the DINOv2 leaves'
gradient by 0.067 of its norm), losses move by 17.5-19.6; README geometry (6, 150 000): 0.086, losses move by 36-43 (0.9-1.1 needed)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

MID_W = {"entropy": (2.0, 0.0), "alignment": (0.0, 4000.0), "both": (3.0, 6000.0)}
FULL_W = (6.0, 150000.0)
NUM_STEPS = 1000                                        # at step_count 0 the annealed alignment weight is the coefficient itself


def _tuner(model, B, w, **kw):
    from hypervla.train import FineTuner
    return FineTuner(model, B, attention_entropy=w[0], attention_map_alignment=w[1], num_steps=NUM_STEPS if w[1] else None, **kw)


def _hyper_norm(grads):
    return np.sqrt(sum(float((v.double() ** 2).sum()) for k, v in grads.items() if not k.startswith("encoder_image_encoder_")))


def _conditioned(ref0, ref):
    """The two conditions of the module docstring, on the oracle alone: ref0 = (per, ent, align, grads) with the terms off, ref with them on."""
    d = {k: ref[3][k] - ref0[3][k] for k in ref0[3]}
    ratio = _hyper_norm(d) / _hyper_norm(ref0[3])
    moved = (ref[0] - ref0[0]).abs().numpy()
    need = 100 * (2e-5 + 2e-4 * ref0[0].abs().numpy())
    print(f"oracle: |g_aux - g_0| / |g_0| = {ratio:.3f}; loss moved by {moved} (needed {need})")
    assert ratio >= 0.05, ratio
    assert (moved >= need).all(), (moved, need)


def _check_step(ft, g, args, r, ref, w, train_encoder=False):
    """One step on the device against ref = (per, ent, align, grads) of the oracle: losses, metrics, every leaf, and the forward-only
    losses bitwise reproducible."""
    from hypervla.train import unpack_params
    kw = dict(reference_attention=r) if w[1] else {}
    loss = ft.forward_backward(*args, **kw).clone()
    got_loss = loss.cpu().numpy()
    metrics = {k: v.cpu().numpy().copy() for k, v in ft.aux_metrics.items()}
    print("loss", got_loss, "oracle", ref[0].numpy(), "metrics", metrics)
    np.testing.assert_allclose(got_loss, ref[0].numpy(), rtol=2e-4, atol=2e-5)
    assert set(metrics) == ({"attention_entropy_loss"} if w[0] else set()) | ({"attention_alignment_loss"} if w[1] else set())
    if w[0]:
        np.testing.assert_allclose(metrics["attention_entropy_loss"], ref[1].numpy(), rtol=2e-4, atol=2e-5)
    if w[1]:
        np.testing.assert_allclose(metrics["attention_alignment_loss"], ref[2].numpy(), rtol=2e-4, atol=2e-5)
    got = unpack_params(g, ft.grads.cpu().numpy(), train_encoder=train_encoder)
    grads = ref[3]
    assert set(got) == set(grads), set(got) ^ set(grads)
    gmax = max(float(v.abs().max()) for v in grads.values())
    rel = sorted(((np.abs(got[k].reshape(v.shape) - v.numpy()).max() / max(float(v.abs().max()), 1e-4 * gmax), k) for k, v in grads.items()),
                 reverse=True)
    print("worst relative gradient errors:", [(f"{x:.2e}", k) for x, k in rel[:5]])
    assert rel[0][0] <= 2e-3, rel[:5]
    a = ft.forward_backward(*args, forward_only=True, **kw).clone()
    b = ft.forward_backward(*args, forward_only=True, **kw)
    assert torch.equal(a, b) and torch.equal(a, loss)     # no atomic reduction in the forward pass, the two terms included
    return loss


@pytest.fixture(scope="module")
def mid():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    import attention_loss_ref as ar
    from hypervla import synthetic as syn
    from hypervla.config import MID, encoder_leaves, generated_leaves
    from hypervla.model import HyperVLA
    from oracle import hvla_ref_np as onp
    g, B = MID, 4
    assert (g.patches + 1) % 64 != 0 and (g.patches + 1) % 4 != 0          # S no multiple of 64, and Sp != S
    model = HyperVLA.from_synthetic(g, max_batch=B)
    P, leaves = model.params, generated_leaves(g)
    ins, st, im = syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g), syn.synthetic_images(B, g)
    batch = syn.synthetic_action_batch(B, g)
    tok = onp.dinov2(P, g, dict(encoder_leaves(g)), onp.normalize_images(im[:, 0]))[:, 1:]
    r = ar.synthetic_reference_map(B, g.patches)
    cache = {}

    def oracle(w, batch=batch, key=None):
        k = (w, key)
        if k not in cache:
            cache[k] = ar.train_loss_and_grads_aux(P, g, leaves, ins, st, tok, batch, w[0], w[1], r if w[1] else None)
        return cache[k]

    return dict(g=g, B=B, model=model, ins=ins, st=st, im=im, batch=batch, tok=tok.astype(np.float32), r=r, oracle=oracle)


@pytest.mark.parametrize("case", ["entropy", "alignment", "both"])
def test_mid_terms_against_autograd(mid, case):
    """MID, B = 4, frozen encoder: S = 65 keys (one 64-lane stride plus the action key), row stride Sp = 68."""
    s, w = mid, MID_W[case]
    ref0, ref = s["oracle"]((0.0, 0.0)), s["oracle"](w)
    _conditioned(ref0, ref)
    ft = _tuner(s["model"], s["B"], w)
    _check_step(ft, s["g"], (s["ins"], s["st"], s["tok"], s["batch"]), s["r"], ref, w)


def test_full_geometry_terms_against_autograd():
    """README geometry, B = 2, frozen encoder, synthetic weights and tokens: S = 257 -- a thread of the 256 owns key 0 AND key 256, the
    action key, which counts for the entropy and not for the alignment.  Both terms on."""
    import attention_loss_ref as ar
    from hypervla import synthetic as syn
    from hypervla.config import FULL, generated_leaves
    from hypervla.model import HyperVLA
    g, B, w = FULL, 2, FULL_W
    assert g.patches + 1 == 257
    model = HyperVLA.from_synthetic(g, max_batch=B)
    ins, st = syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g)
    batch = syn.synthetic_action_batch(B, g)
    tok = np.random.default_rng(9).standard_normal((B, g.patches, g.enc_dim)).astype(np.float32)
    r = ar.synthetic_reference_map(B, g.patches)
    params = {k: v for k, v in model.params.items() if not k.startswith("encoder_image_encoder_")}
    ref0 = ar.train_loss_and_grads_aux(params, g, generated_leaves(g), ins, st, tok, batch)
    ref = ar.train_loss_and_grads_aux(params, g, generated_leaves(g), ins, st, tok, batch, w[0], w[1], r)
    _conditioned(ref0, ref)
    _check_step(_tuner(model, B, w), g, (ins, st, tok, batch), r, ref, w)


def test_encoder_trained_terms_against_autograd():
    """train_encoder=True at the smallest geometry tests/test_gpu_train.py's _encoder_case uses (MID), B = 2, both terms on: the gradient
    reaches the shared DINOv2 leaves through the policy's keys; every DINOv2 and hypernetwork leaf against float64 autograd with
    `images` in the graph."""
    import attention_loss_ref as ar
    from hypervla import synthetic as syn
    from hypervla.config import MID, encoder_leaves, generated_leaves
    from hypervla.model import HyperVLA
    g, B, w = MID, 2, MID_W["both"]
    model = HyperVLA.from_synthetic(g, max_batch=B)
    ins, st, im = syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g), syn.synthetic_images(B, g)
    batch = syn.synthetic_action_batch(B, g)
    r = ar.synthetic_reference_map(B, g.patches)
    kw = dict(images=im, enc_shapes=dict(encoder_leaves(g)))
    ref0 = ar.train_loss_and_grads_aux(model.params, g, generated_leaves(g), ins, st, None, batch, **kw)
    ref = ar.train_loss_and_grads_aux(model.params, g, generated_leaves(g), ins, st, None, batch, w[0], w[1], r, **kw)
    _conditioned(ref0, ref)
    enc0 = {k: v for k, v in ref0[3].items() if k.startswith("encoder_image_encoder_")}
    moved = np.sqrt(sum(float(((ref[3][k] - v) ** 2).sum()) for k, v in enc0.items()) / sum(float((v ** 2).sum()) for v in enc0.values()))
    print(f"oracle: the terms move the DINOv2 leaves' gradient by {moved:.3f} of its norm")
    assert moved >= 0.01
    _check_step(_tuner(model, B, w, train_encoder=True), g, (ins, st, im, batch), r, ref, w, train_encoder=True)


def test_off_is_off(mid):
    """Weights zero, and again after hvla_train_attention_losses(ctx, NULL) behind a step with the terms on: the losses of a FineTuner
    built without the arguments, bit for bit; gradients within the existing tolerance of the existing oracle (the split-K weight
    gradients are not bit-reproducible); hvla_train_sizes unchanged throughout."""
    from hypervla.train import FineTuner, unpack_params
    from oracle import hvla_ref_torch as ot
    from hypervla.config import generated_leaves
    s = mid
    g, B, m = s["g"], s["B"], s["model"]
    args = (s["ins"], s["st"], s["tok"], s["batch"])
    per, _, grads = ot.train_loss_and_grads(m.params, g, generated_leaves(g), s["ins"], s["st"], s["tok"], s["batch"])
    sizes = m._ctx.train_sizes(B)
    plain = FineTuner(m, B)
    loss_plain = plain.forward_backward(*args).clone()
    np.testing.assert_allclose(loss_plain.cpu().numpy(), per.numpy(), rtol=2e-4, atol=2e-5)

    def grads_ok(ft):
        got = unpack_params(g, ft.grads.cpu().numpy())
        gmax = max(float(v.abs().max()) for v in grads.values())
        worst = max((np.abs(got[k].reshape(v.shape) - v.numpy()).max() / max(float(v.abs().max()), 1e-4 * gmax), k) for k, v in grads.items())
        assert worst[0] <= 2e-3, worst

    grads_ok(plain)
    zero = FineTuner(m, B, attention_entropy=0.0, attention_map_alignment=0.0)
    assert torch.equal(zero.forward_backward(*args), loss_plain) and zero.aux_metrics == {}
    grads_ok(zero)
    assert m._ctx.train_sizes(B) == sizes
    on = _tuner(m, B, MID_W["both"])
    loss_on = on.forward_backward(*args, reference_attention=s["r"]).clone()
    assert not torch.equal(loss_on, loss_plain)
    assert m._ctx.train_sizes(B) == sizes                              # the terms take no workspace
    assert m._ctx.lib.hvla_train_attention_losses(m._ctx.h, None) == 0
    assert torch.equal(plain.forward_backward(*args), loss_plain)
    grads_ok(plain)
    assert m._ctx.train_sizes(B) == sizes


def test_masks_do_not_touch_the_terms(mid):
    """A sample whose timestep_pad_mask is false: its mix loss is zero, its loss is w_ent ent + w_align align, and what it adds to the
    gradient is the terms' alone (the whole gradient against the oracle on that batch)."""
    s, w = mid, MID_W["both"]
    batch = dict(s["batch"])
    tm = np.array(batch["timestep_pad_mask"]).copy()
    tm[0] = False
    batch["timestep_pad_mask"] = tm
    ref0, ref = s["oracle"]((0.0, 0.0), batch, "masked"), s["oracle"](w, batch, "masked")
    assert float(ref0[0][0]) == 0.0 and float(ref[0][0]) > 0.0
    _conditioned(ref0, ref)
    ft = _tuner(s["model"], s["B"], w)
    loss = _check_step(ft, s["g"], (s["ins"], s["st"], s["tok"], batch), s["r"], ref, w).cpu().numpy()
    want = w[0] * ref[1].numpy()[0] + w[1] * ref[2].numpy()[0]
    np.testing.assert_allclose(loss[0], want, rtol=2e-4, atol=2e-5)
    own = w[0] * ft.aux_metrics["attention_entropy_loss"].cpu().numpy()[0] + w[1] * ft.aux_metrics["attention_alignment_loss"].cpu().numpy()[0]
    np.testing.assert_allclose(loss[0], own, rtol=1e-6)                # the device's own terms, f32 rounding of one multiply-add each


def test_refusals_leave_the_previous_setting(mid):
    """A wrong struct_size, a negative or non-finite weight, a NULL map with a positive alignment weight: HVLA_E_SHAPE each, and the
    setting made before them stays in force."""
    from hypervla import _native
    s = mid
    m, B = s["model"], s["B"]
    args = (s["ins"], s["st"], s["tok"], s["batch"])
    w = MID_W["entropy"]
    ft = _tuner(m, B, w)
    loss_on = ft.forward_backward(*args, forward_only=True).clone()
    plain = _tuner(m, B, (0.0, 0.0))
    loss_plain = plain.forward_backward(*args, forward_only=True).clone()
    assert not torch.equal(loss_on, loss_plain)
    ft._select_attention(None)                                          # the valid setting: entropy on
    lib, h, size = m._ctx.lib, m._ctx.h, ctypes.sizeof(_native.hvla_train_attention)
    rmap = torch.zeros(B, s["g"].patches, device=m.device)
    mk = lambda sz, we, wa, ref: _native.hvla_train_attention(sz, we, wa, ref, None, None)
    for bad in (mk(size - 4, 1.0, 0.0, None), mk(size + 8, 1.0, 0.0, None), mk(0, 1.0, 0.0, None), mk(size, -1.0, 0.0, None),
                mk(size, 1.0, -2.0, rmap.data_ptr()), mk(size, float("nan"), 0.0, None), mk(size, 0.0, float("inf"), rmap.data_ptr()),
                mk(size, 0.0, 3.0, None)):
        assert lib.hvla_train_attention_losses(h, ctypes.byref(bad)) == -1, (bad.struct_size, bad.entropy_weight, bad.alignment_weight)
        assert lib.hvla_last_error(h)
    keep = ft._select_attention
    ft._select_attention = lambda ref=None: 0.0                         # this one step does not set anything itself
    try:
        assert torch.equal(ft.forward_backward(*args, forward_only=True), loss_on)
    finally:
        ft._select_attention = keep
    assert torch.equal(plain.forward_backward(*args, forward_only=True), loss_plain)


def test_reference_map_helper(mid):
    """reference_attention_map(frames) is the last layer of `dino_cls_attention`, mean over heads, of a sample_actions(...,
    attention_maps=True) call on the same frames (whose parity with the oracle test_attention_maps_against_the_oracle holds)."""
    s = mid
    m, g, B = s["model"], s["g"], s["B"]
    w, tasks, _ = m.create_tasks(instruction_dict=s["ins"], initial_state=s["st"])
    _, inter = m.sample_actions(torch.as_tensor(s["im"]), s["ins"], tasks, np.ones((B, 1)), w, attention_maps=True)     # tensors in, tensors out
    got = m.reference_attention_map(s["im"])
    assert tuple(got.shape) == (B, g.patches) and got.dtype == torch.float32 and got.is_cuda
    want = inter["dino_cls_attention"][:, -1].mean(1)
    assert torch.equal(got, want)
    assert (got > 0).all() and (got.sum(-1) < 1).all()
    # and it is accepted as the target as it comes, on the device
    ft = _tuner(m, B, MID_W["alignment"])
    loss = ft.forward_backward(s["ins"], s["st"], s["tok"], s["batch"], forward_only=True, reference_attention=got)
    assert torch.isfinite(loss).all() and (ft.aux_metrics["attention_alignment_loss"] >= 0).all()
