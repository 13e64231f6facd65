"""GPU: fine-tuning a use_language_token model (FineTuner(language_tokens=True), hvla_train_language_tokens) -- the
step's per-sample loss and every gradient leaf against float64 autograd through tests/lang_policy_torch.py at the edges of the
policy's sequence, the trained encoder behind the patch rows, the optimizer, the metrics, the publish and the gate.

The geometries are tests/lang_policy_torch.py::GEOMETRIES (MID with the option: P = 64, D = 64, two policy layers, lang_dim 64);
tests/test_lang_train_host.py walks the same ones through the CPU extent trace.  Bounds: loss rtol 2e-4 / atol 2e-5
(tests/test_gpu_train.py::test_train_forward_loss), worst leaf max|d| / max(max|ref|, 1e-4 gmax) <= 2e-3
(test_train_gradients_match_autograd, test_encoder_gradients_match_autograd)."""
import gc

import numpy as np
import pytest

import lang_policy_torch as LT
from train_parity import LOSS_ATOL, LOSS_RTOL, assert_not_vacuous, leaf_errors

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LEAF_TOL = 2e-3
LANG_HEADS = {"output_head_encoder_language_token_projection_" + a + "/" + b for a in ("kernel", "bias") for b in ("kernel", "bias")}
FROZEN_LANG = ("output_head_encoder_language_token_projection_*",)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X; torch.cuda.is_available() is False")


def _rows(c, sl):
    """Samples `sl` of a case's inputs."""
    ins = {"language_instruction": {k: np.asarray(v)[sl] for k, v in c["ins"]["language_instruction"].items()}}
    st = {"patch_embeddings": np.asarray(c["st"]["patch_embeddings"])[sl]}
    return ins, st, c["tok"][sl], {k: np.asarray(v)[sl] for k, v in c["batch"].items()}


@pytest.fixture(scope="module")
def cases():
    """cases(name): one geometry with the encoder frozen, made on first use and shared by the module's tests; everything is released
    when the module is done."""
    _need_gpu()
    made = {}

    def get(name):
        if name not in made:
            made[name] = _make_case(name)
        return made[name]
    yield get
    made.clear()
    gc.collect()


def _make_case(name):
    """Model, seeded inputs, the oracle's loss and gradients (computed once), one FineTuner."""
    from hypervla import synthetic as syn
    from hypervla.config import generated_leaves
    from hypervla.model import HyperVLA
    from hypervla.train import FineTuner
    g, B = LT.geometry(name)
    model = HyperVLA.from_synthetic(g, max_batch=B)
    ins, st, batch = syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g), syn.synthetic_action_batch(B, g)
    tok = np.random.default_rng(9).standard_normal((B, g.patches, g.enc_dim)).astype(np.float32)      # frozen-encoder tokens
    params = {k: v for k, v in model.params.items() if not k.startswith("encoder_image_encoder_")}
    per, loss, grads = LT.train_loss_and_grads(params, g, generated_leaves(g), ins, st, tok, batch)
    return dict(g=g, B=B, model=model, ins=ins, st=st, tok=tok, batch=batch, per=per.numpy(), grads=grads,
                im=syn.synthetic_images(B, g), ft=FineTuner(model, B, language_tokens=True))


def _check_loss(c, name):
    ft = c["ft"]
    loss = ft.forward_backward(c["ins"], c["st"], c["tok"], c["batch"], forward_only=True).clone()
    err = np.abs(loss.cpu().numpy() - c["per"])
    print(f"LANG {name} B={c['B']} Sx={c['g'].policy_seq}: per-sample loss error max {err.max():.2e} (loss {c['per'].min():.3f} .. {c['per'].max():.3f})")
    np.testing.assert_allclose(loss.cpu().numpy(), c["per"], rtol=2e-4, atol=2e-5)
    again = ft.forward_backward(c["ins"], c["st"], c["tok"], c["batch"], forward_only=True)
    assert torch.equal(loss, again)                      # the forward pass has no atomics
    return loss


def _check_gradients(c, name):
    from hypervla.train import unpack_params
    ft, grads = c["ft"], c["grads"]
    loss = ft.forward_backward(c["ins"], c["st"], c["tok"], c["batch"])
    np.testing.assert_allclose(loss.cpu().numpy(), c["per"], rtol=2e-4, atol=2e-5)
    got = unpack_params(c["g"], ft.grads.cpu().numpy())
    assert set(got) == set(grads), set(got) ^ set(grads)
    rel, gmax = leaf_errors(got, grads)
    print(f"LANG {name} B={c['B']} Sx={c['g'].policy_seq}: worst relative gradient errors {[(f'{r:.2e}', k) for r, k in rel[:5]]}")
    assert LANG_HEADS <= set(grads)
    for k in LANG_HEADS:                                 # the new heads are compared, and against something
        assert float(grads[k].abs().max()) > 1e-4 * gmax, (k, float(grads[k].abs().max()), gmax)
    assert_not_vacuous(grads, False)
    for k in got:                                        # the policy's key biases: exactly the zero their gradient is
        if k.startswith("output_head_") and "_key_bias/" in k:
            assert not got[k].any() and float(grads[k].abs().max()) <= 1e-9 * gmax, k
    assert rel[0][0] <= LEAF_TOL, rel[:5]


def test_loss_matches_the_oracle_and_is_batch_invariant(cases):
    """T = 12, B = 4.  Also: each sample run alone (B = 1) has bitwise the loss it has in the batch."""
    from hypervla.train import FineTuner
    c = cases("T12")
    loss = _check_loss(c, "T12")
    one = FineTuner(c["model"], 1, language_tokens=True)
    for b in range(c["B"]):
        ins, st, tok, batch = _rows(c, slice(b, b + 1))
        alone = one.forward_backward(ins, st, tok, batch, forward_only=True)
        assert torch.equal(alone[0], loss[b]), (b, float(alone[0]), float(loss[b]))


def test_every_gradient_leaf_matches_autograd(cases):
    _check_gradients(cases("T12"), "T12")


EDGES = {"T2": 67, "T3": 68, "T32": 97, "T32-P256": 289}          # name: Sx


@pytest.mark.parametrize("name", list(EDGES))
def test_loss_at_the_edges_of_the_sequence(cases, name):
    """T = 2 (Sx = 67), T = 3 (Sx = 68: no padding behind an attention row), T = 32 (Sx = 97), and P = 256 with T = 32 (Sx = 289, B = 2)."""
    c = cases(name)
    assert c["g"].policy_seq == EDGES[name]
    _check_loss(c, name)


@pytest.mark.parametrize("name", list(EDGES))
def test_gradients_at_the_edges_of_the_sequence(cases, name):
    """The same four.  Measured on one MI355X (worst leaf: the context encoder's key bias, whose true gradient is zero and which the
    metric holds to 1e-4 gmax), with the option / without it at the same widths and batch:
        T12 2.1e-4 / 6.6e-4    T2 8.4e-4 / 8.4e-4    T3 4.5e-4 / 7.5e-4    T32 4.4e-4 / 1.2e-3    T32-P256 9.4e-4 / 7.7e-4
    The generated policy's own key biases are no longer among the worst: with the language rows the step does not form their
    gradient, which is zero under any mask, from the column sum of dk (block_bwd, csrc/train.hip) -- while it did, T2
    gave 2.23e-3 on output_head_..._encoderblock_0_..._key_bias/bias, the operand rounding of ds on a language query's two keys."""
    c = cases(name)
    assert c["g"].policy_seq == EDGES[name]
    _check_gradients(c, name)


def test_trained_encoder_gradients_match_autograd():
    """train_encoder=True at T = 12, B = 2: the shared DINOv2 leaves receive d tokens from the patch rows [T, T + P) of dx0 -- a row
    offset error shows here and nowhere else."""
    _need_gpu()
    from hypervla import synthetic as syn
    from hypervla.config import encoder_leaves, generated_leaves
    from hypervla.model import HyperVLA
    from hypervla.train import FineTuner, unpack_params
    g, B = LT.geometry("T12")[0], 2
    model = HyperVLA.from_synthetic(g, max_batch=B)
    ins, st, im, batch = (syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g), syn.synthetic_images(B, g),
                          syn.synthetic_action_batch(B, g))
    per, loss, grads = LT.train_loss_and_grads(model.params, g, generated_leaves(g), ins, st, None, batch, images=im,
                                               enc_shapes=dict(encoder_leaves(g)))
    ft = FineTuner(model, B, train_encoder=True, language_tokens=True)
    got_loss = ft.forward_backward(ins, st, im, batch).cpu().numpy()
    got = unpack_params(g, ft.grads.cpu().numpy(), train_encoder=True)
    assert set(got) == set(grads), set(got) ^ set(grads)
    rel, gmax = leaf_errors(got, grads)
    enc_rel = [r for r in rel if r[1].startswith("encoder_image_encoder_")]
    print(f"LANG trained encoder B={B}: loss error max {np.abs(got_loss - per.numpy()).max():.2e}; worst leaves "
          f"{[(f'{r:.2e}', k) for r, k in rel[:5]]}; worst encoder leaf {enc_rel[0][0]:.2e} {enc_rel[0][1]}")
    np.testing.assert_allclose(got_loss, per.numpy(), rtol=LOSS_RTOL, atol=LOSS_ATOL)
    assert len(enc_rel) == len(encoder_leaves(g))
    assert_not_vacuous(grads, True)
    assert rel[0][0] <= LEAF_TOL, rel[:6]


def test_optimizer_metrics_and_frozen_language_heads(cases):
    """Five steps on one batch lower the mean loss; info()["training_loss"] is the mean of ft.loss to one f32 rounding; with the two
    language heads frozen their columns of params, mu, nu and ema keep their bits over a step while the rest moves."""
    from hypervla.train import FineTuner
    c = cases("T12")
    ft = FineTuner(c["model"], c["B"], language_tokens=True, metrics=True, peak_lr=1e-3, ema_start_step=0)
    losses = []
    for _ in range(5):
        losses.append(float(ft.step(c["ins"], c["st"], c["im"], c["batch"], lr=1e-3)))
        want = ft.loss.double().mean().item()
        got = float(ft.info()["training_loss"])
        assert abs(got - want) <= 2.0 ** -23 * abs(want), (got, want)
    print("LANG five steps on one batch, mean loss:", [f"{x:.4f}" for x in losses])
    assert losses[-1] < losses[0], losses
    fz = FineTuner(c["model"], c["B"], language_tokens=True, frozen_keys=FROZEN_LANG, ema_start_step=0)
    mask = fz.frozen.bool()
    g = c["g"]
    assert int(mask.sum()) == (g.ctx_dim + 1) * (g.lang_dim + 1) * g.dim and fz.frozen_buckets == 0
    fz.step(c["ins"], c["st"], c["im"], c["batch"], lr=1e-3)              # moments and EMA away from their initial values
    before = {k: getattr(fz, k).clone() for k in ("params", "mu", "nu", "ema")}
    fz.step(c["ins"], c["st"], c["im"], c["batch"], lr=1e-3)
    assert float(fz.grads[mask].abs().max()) > 0                            # computed, and ignored by the optimizer
    for k, old in before.items():
        new = getattr(fz, k)
        assert torch.equal(new[mask], old[mask]), k
        assert not torch.equal(new[~mask], old[~mask]), k
    assert float(before["mu"][mask].float().abs().max()) == 0 and float(before["nu"][mask].abs().max()) == 0


def _outputs(m, c, w=None):
    """create_tasks (unless `w` is given) + one step from the case's tokens: theta, actions, gripper logits."""
    if w is None:
        w, _, _ = m.create_tasks(instruction_dict=c["ins"], initial_state=c["st"])
    act, logit = m.policy_from_tokens(c["tok"], w)
    torch.cuda.synchronize()
    return dict(theta=w.export()[0].clone(), actions=act.clone(), logits=logit.clone())


def test_publish(cases):
    """publish() straight after construction changes no output bit; after one step the published model has bitwise the outputs of a
    second model built from unpack_params of the vector; a GeneratedWeights handle made before the publish steps as before."""
    from hypervla.config import generated_leaves
    from hypervla.model import HyperVLA
    from hypervla.train import FineTuner, unpack_params
    c = cases("T12")
    m = HyperVLA.from_synthetic(c["g"], max_batch=c["B"])
    ft = FineTuner(m, c["B"], language_tokens=True)
    w_old, _, _ = m.create_tasks(instruction_dict=c["ins"], initial_state=c["st"])
    first = _outputs(m, c)
    old = _outputs(m, c, w_old)
    ft.publish()
    same = _outputs(m, c)
    for k in first:
        assert torch.equal(first[k], same[k]), k
    ft.step(c["ins"], c["st"], c["im"], c["batch"], lr=1e-3)
    ft.publish()
    after = _outputs(m, c)
    params = dict(m._params)
    params.update(unpack_params(c["g"], ft.params.cpu().numpy()))
    fresh = HyperVLA(m.config, params, None, m.dataset_statistics, max_batch=m.max_batch, enc_dtype=m.enc_dtype)
    want = _outputs(fresh, c)
    for k in after:
        assert torch.equal(after[k], want[k]), k
        assert not torch.equal(after[k], first[k]), k
    kept = _outputs(m, c, w_old)                          # generated earlier: its weights and its language prefix stay
    for k in old:
        assert torch.equal(kept[k], old[k]), k
    # the language heads moved, and what is served is their new value
    l = next(l for l in generated_leaves(c["g"]) if l.flat_name == "encoder_language_token_projection_kernel")
    assert not torch.equal(after["theta"][:, l.offset:l.offset + l.size], first["theta"][:, l.offset:l.offset + l.size])


def test_the_gate(cases):
    """hvla_train_language_tokens: off by default and after (ctx, 0), on after (ctx, 1); refused on a plain context, which trains as
    before; the attention terms stay refused on a language context."""
    from hypervla import _native, synthetic as syn
    from hypervla.config import MID
    from hypervla.model import HyperVLA
    from hypervla.train import FineTuner, train_param_layout
    c = cases("T12")
    lang = HyperVLA.from_synthetic(c["g"], max_batch=2)
    ctx = lang._ctx
    with pytest.raises(_native.NativeError, match="HVLA_E_SHAPE"):
        ctx.train_sizes(2)
    ctx.train_language_tokens(True)
    n, G, work, n_hyper = ctx.train_sizes(2)
    assert n == train_param_layout(c["g"])[1] == n_hyper and G == c["ft"].G and work > 0
    with pytest.raises(_native.NativeError, match="HVLA_E_SHAPE"):
        ctx.train_attention_losses(0.5, 0.0, 0, 0, 0)
    for bad in (2, -1):
        assert ctx.lib.hvla_train_language_tokens(ctx.h, bad) == -1          # HVLA_E_SHAPE, and the setting stays
    assert ctx.train_sizes(2)[0] == n
    ctx.train_language_tokens(False)
    with pytest.raises(_native.NativeError, match="HVLA_E_SHAPE"):
        ctx.train_sizes(2)
    with pytest.raises(_native.NativeError, match="HVLA_E_SHAPE"):
        ctx.train_attention_losses(0.5, 0.0, 0, 0, 0)
    # a plain context
    g, B = MID, 2
    plain = HyperVLA.from_synthetic(g, max_batch=B)
    ins, st, batch = syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g), syn.synthetic_action_batch(B, g)
    tok = np.random.default_rng(9).standard_normal((B, g.patches, g.enc_dim)).astype(np.float32)
    ft = FineTuner(plain, B)
    sizes = plain._ctx.train_sizes(B)
    before = ft.forward_backward(ins, st, tok, batch, forward_only=True).clone()
    with pytest.raises(_native.NativeError, match="HVLA_E_SHAPE"):
        plain._ctx.train_language_tokens(True)
    with pytest.raises(ValueError, match="language_tokens=True needs"):
        FineTuner(plain, B, language_tokens=True)
    assert plain._ctx.train_sizes(B) == sizes
    after = ft.forward_backward(ins, st, tok, batch, forward_only=True)
    assert torch.equal(before, after)
    ft.forward_backward(ins, st, tok, batch)
    assert float(ft.grads.abs().max()) > 0
