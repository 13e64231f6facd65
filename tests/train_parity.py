"""The fine-tune step against the float64 autograd oracle (oracle.hvla_ref_torch.train_loss_and_grads) for one geometry and batch
size: per-sample loss and every gradient leaf.  Shared by tests/test_gpu_train.py (MID, the README widths, the large-batch kernels)
and tests/test_gpu_train_geometry.py (the edges of the accepted set).  Inputs are the seeded ones of hypervla.synthetic.

The metric of a leaf is max|got - ref| / max(max|ref|, 1e-4 gmax), gmax the largest gradient element of the whole step: leaves
whose true gradient is ~0 (key biases: the softmax is invariant to them) are held to the global scale."""
import numpy as np

LOSS_RTOL, LOSS_ATOL = 3e-4, 3e-5
FLOOR = 1e-4          # of gmax


def leaf_errors(got, grads):
    """[(metric, leaf)] worst first, and gmax.  `grads`: the oracle's {leaf: tensor}; `got`: unpack_params of the device's vector."""
    gmax = max(float(v.abs().max()) for v in grads.values())
    rel = sorted(((np.abs(got[k].reshape(v.shape) - v.numpy()).max() / max(float(v.abs().max()), FLOOR * gmax), k)
                  for k, v in grads.items()), reverse=True)
    return rel, gmax


def _report(what, g, B, got_loss, per, rel, report):
    err = np.abs(got_loss - per.numpy())
    print(f"{what} B = {B}: per-sample loss error max {err.max():.2e} (loss {per.numpy().min():.3f} .. {per.numpy().max():.3f}); "
          f"worst relative gradient errors: {[(f'{r:.2e}', k) for r, k in rel[:5]]}")
    if report is not None:
        report.update(loss_err=float(err.max()), worst=rel[0], rel=rel)


def assert_not_vacuous(grads, train_encoder):
    """On the oracle's gradients alone: at least 85 % of the leaves are above the floor of the metric (the rest are the key biases),
    and with the encoder trained at least one encoder leaf is non-zero."""
    gmax = max(float(v.abs().max()) for v in grads.values())
    above = sum(float(v.abs().max()) > FLOOR * gmax for v in grads.values())
    assert above >= 0.85 * len(grads), (above, len(grads))
    if train_encoder:
        assert any(float(v.abs().max()) > 0 for k, v in grads.items() if k.startswith("encoder_image_encoder_"))
    return above, len(grads)


def frozen_encoder_case(g, B, tol, report=None, **ft_kw):
    """Encoder frozen: random normal patch tokens [B, P, E] stand for hvla_encode's."""
    from hypervla import synthetic as syn
    from hypervla.config import generated_leaves
    from hypervla.model import HyperVLA
    from hypervla.train import FineTuner, unpack_params
    from oracle import hvla_ref_torch as ot
    model = HyperVLA.from_synthetic(g, max_batch=B)
    ins, st = syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g)
    batch = syn.synthetic_action_batch(B, g)
    tok = np.random.default_rng(9).standard_normal((B, g.patches, g.enc_dim)).astype(np.float32)   # frozen-encoder tokens
    params = {k: v for k, v in model.params.items() if not k.startswith("encoder_image_encoder_")}
    per, loss, grads = ot.train_loss_and_grads(params, g, generated_leaves(g), ins, st, tok, batch)
    ft = FineTuner(model, B, **ft_kw)
    got_loss = ft.forward_backward(ins, st, tok, batch).cpu().numpy()
    got = unpack_params(g, ft.grads.cpu().numpy())
    rel, _ = leaf_errors({k: got[k] for k in grads if k in got}, {k: v for k, v in grads.items() if k in got})
    _report("frozen encoder", g, B, got_loss, per, rel, report)
    if report is not None:
        report.update(grads=grads, leaves=set(got))
    np.testing.assert_allclose(got_loss, per.numpy(), rtol=LOSS_RTOL, atol=LOSS_ATOL)
    assert set(grads) <= set(got), set(grads) - set(got)
    assert rel[0][0] <= tol, rel[:5]
    return model, ft, (ins, st, tok, batch)


def encoder_case(g, B, tol, seed_rank=0, stats=None, report=None, **ft_kw):
    """Encoder trained: the DINOv2 leaves are in the vector, the oracle differentiates transformers' Dinov2Model."""
    from hypervla import synthetic as syn
    from hypervla.config import encoder_leaves, generated_leaves
    from hypervla.model import HyperVLA
    from hypervla.train import FineTuner, unpack_params
    from oracle import hvla_ref_torch as ot
    model = HyperVLA.from_synthetic(g, max_batch=B)
    ins, st, im = syn.synthetic_instructions(B, g, seed_rank), syn.synthetic_initial_state(B, g, seed_rank), syn.synthetic_images(B, g, seed_rank)
    batch = syn.synthetic_action_batch(B, g, seed_rank)
    per, loss, grads = ot.train_loss_and_grads(model.params, g, generated_leaves(g), ins, st, None, batch, images=im,
                                               enc_shapes=dict(encoder_leaves(g)))
    ft = FineTuner(model, B, train_encoder=True, **ft_kw)
    got_loss = ft.forward_backward(ins, st, im, batch).cpu().numpy()
    got = unpack_params(g, ft.grads.cpu().numpy(), train_encoder=True)
    both = set(got) & set(grads)
    rel, gmax = leaf_errors({k: got[k] for k in both}, {k: grads[k] for k in both})
    _report("trained encoder", g, B, got_loss, per, rel, report)
    if report is not None:
        report.update(grads=grads, leaves=set(got))
    np.testing.assert_allclose(got_loss, per.numpy(), rtol=LOSS_RTOL, atol=LOSS_ATOL)
    assert set(got) == set(grads), set(got) ^ set(grads)
    enc_rel = [r for r in rel if r[1].startswith("encoder_image_encoder_")]
    assert len(enc_rel) == len(encoder_leaves(g))
    assert any(float(grads[k].abs().max()) > 0 for _, k in enc_rel)
    if stats is not None:
        # the bias and LayerScale leaves of the encoder are the outputs of the column-sum / LayerScale kernels (colsum*_kernel,
        # ls_bwd*_kernel, the LayerNorm parameter gradients): per ELEMENT against the leaf's RMS, so that a lost column group or row
        # block is not hidden behind a large neighbour of the same leaf
        for k, v in grads.items():
            if k.startswith("encoder_image_encoder_encoder_layer_") and (k.endswith("bias") or k.endswith("lambda1") or k.endswith("scale")):
                ref = v.numpy()
                rms = float(np.sqrt((ref * ref).mean()))
                if rms > 1e-6 * gmax:                   # (key biases: the softmax is invariant to them, their gradient is rounding noise)
                    stats[k] = float(np.abs(got[k].reshape(ref.shape) - ref).max() / rms)
        stats["__max_metric__"] = rel[0]
    assert rel[0][0] <= tol, rel[:6]
    return model, ft, (ins, st, im, batch)
