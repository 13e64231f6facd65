"""CPU: the attention entropy / alignment terms of the fine-tune step (scripts/train.py:348-373) -- the float64 restatement the GPU
tests compare against (tests/attention_loss_ref.py), the two formulas, the gradient the kernel adds, FineTuner's argument checks and
the binding of hvla_train_attention_losses."""
import ctypes
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_with_zero_weights_is_the_oracle():
    """Explicit masked softmax against the oracle's scaled_dot_product_attention at MID, B = 4, in float64: per-sample losses and
    every gradient leaf to 1e-12 relative (a leaf's largest error over its largest entry; leaves whose true gradient is zero --
    the key biases -- over 1e-4 of the largest entry of all leaves, the floor tests/test_gpu_train.py uses)."""
    import attention_loss_ref as ar
    from hypervla import synthetic as syn
    from hypervla.config import MID, encoder_leaves, generated_leaves
    from oracle import hvla_ref_np as onp, hvla_ref_torch as ot
    g, B = MID, 4
    P, leaves = syn.synthetic_params(g), generated_leaves(g)
    ins, st, im = syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g), syn.synthetic_images(B, g)
    batch = syn.synthetic_action_batch(B, g)
    tok = onp.dinov2(P, g, dict(encoder_leaves(g)), onp.normalize_images(im[:, 0]))[:, 1:]
    per, loss, grads = ot.train_loss_and_grads(P, g, leaves, ins, st, tok, batch)
    per2, ent, align, grads2 = ar.train_loss_and_grads_aux(P, g, leaves, ins, st, tok, batch, 0.0, 0.0, None)
    np.testing.assert_allclose(per2.numpy(), per.numpy(), rtol=1e-12, atol=0)
    assert set(grads) == set(grads2)
    gmax = max(float(v.abs().max()) for v in grads.values())
    worst = max((float((grads2[k] - v).abs().max()) / max(float(v.abs().max()), 1e-4 * gmax), k) for k, v in grads.items())
    print("restated policy against the oracle, worst leaf:", worst)
    assert worst[0] <= 1e-12, worst
    # the terms themselves are sane: 0 < ent <= log S, and no alignment without a map
    assert ((ent > 0) & (ent <= np.log(g.patches + 1))).all() and float(align.abs().max()) == 0.0


def _rows(B=3, H=4, S=65, seed=0, dtype=np.float64):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((B, H, S, S)) * 2.0
    e = np.exp(z - z.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(dtype)


def test_formulas_are_the_reference_s():
    """A literal numpy transcription of scripts/train.py:350-372 -- per sample, i.e. on a batch dimension of one, as the reference's
    vmap over `sample_loss_fn` evaluates it -- against attention_terms, on random softmax rows."""
    import attention_loss_ref as ar
    B, H, S = 3, 4, 65
    amap = _rows(B, H, S)
    dino = _rows(B, 2, S, seed=1)                                      # DINO_last_layer_attention_map [B, heads, 1 + P, 1 + P]
    ent, align = ar.attention_terms(torch.as_tensor(amap), dino[:, :, 0, 1:].mean(1))
    for b in range(B):
        policy_attention_map = amap[b:b + 1]                           # sample_data gets a batch dimension of 1 (:328)
        attention_prob = policy_attention_map[:, :, -1]
        epsilon = 1e-8
        log_prob = np.log(attention_prob + epsilon)
        per_head_entropy = -np.sum(attention_prob * log_prob, axis=-1)
        entropy_loss = np.mean(per_head_entropy)
        pam = policy_attention_map[:, :, -1, :-1]
        reference_attention_map = dino[b:b + 1][:, :, 0, 1:]
        alignment_loss = ((pam.mean(1) - reference_attention_map.mean(1)) ** 2).mean()
        np.testing.assert_allclose(float(ent[b]), entropy_loss, rtol=1e-14)
        np.testing.assert_allclose(float(align[b]), alignment_loss, rtol=1e-14)


@pytest.mark.parametrize("w_ent,w_align", [(0.7, 0.0), (0.0, 900.0), (0.7, 900.0)])
def test_analytic_gradient_wrt_the_probabilities_is_autograd_s(w_ent, w_align):
    """d(w_ent ent + w_align align) / dp[h][k], the expression attention_aux_kernel adds to dp, against autograd through attention_terms."""
    import attention_loss_ref as ar
    B, H, S = 2, 4, 65
    amap = torch.as_tensor(_rows(B, H, S, seed=2)).requires_grad_(True)
    r = ar.synthetic_reference_map(B, S - 1).astype(np.float64)
    ent, align = ar.attention_terms(amap, r)
    (w_ent * ent + w_align * align).sum().backward()
    for b in range(B):
        want = amap.grad[b, :, -1].numpy()
        got = ar.dterms_dp(amap.detach().numpy()[b, :, -1], w_ent, w_align, r[b])
        np.testing.assert_allclose(got, want, rtol=1e-11, atol=1e-13 * np.abs(want).max())
        assert np.abs(amap.grad[b, :, :-1].numpy()).max() == 0.0       # only the action token's row carries the terms
        if w_align and not w_ent:
            assert np.abs(want[:, -1]).max() == 0.0                    # the action key counts for the entropy, not for the alignment


def test_finetuner_argument_checks():
    """Before the model is touched: alignment needs num_steps; negative or non-finite coefficients are refused.  Before any launch:
    alignment needs reference_attention of shape [B, P]."""
    from hypervla import train as T
    with pytest.raises(ValueError, match="num_steps"):
        T.FineTuner(None, 4, attention_map_alignment=1.0)
    with pytest.raises(ValueError, match="num_steps"):
        T.FineTuner(None, 4, attention_map_alignment=1.0, num_steps=0)
    for bad in (dict(attention_entropy=-0.1), dict(attention_entropy=float("nan")), dict(attention_map_alignment=float("inf"), num_steps=10)):
        with pytest.raises(ValueError, match="finite"):
            T.FineTuner(None, 4, **bad)
    assert T.attention_loss_plan(0.0, 0.0, None) == (0.0, 0.0, None)
    assert T.attention_loss_plan(0.5, 2.0, 100) == (0.5, 2.0, 100)
    assert T.attention_loss_plan(0.5, 0.0, None) == (0.5, 0.0, None)   # the entropy alone needs no schedule
    T.check_reference_attention(0.0, None, 4, 64)                      # not needed, not looked at
    with pytest.raises(ValueError, match="reference_attention"):
        T.check_reference_attention(2.0, None, 4, 64)
    with pytest.raises(ValueError, match=r"\[4, 64\]"):
        T.check_reference_attention(2.0, np.zeros((4, 65), np.float32), 4, 64)
    T.check_reference_attention(2.0, np.zeros((4, 64), np.float32), 4, 64)
    T.check_reference_attention(2.0, torch.zeros(4, 64), 4, 64)
    # the methods themselves refuse before they read anything else of the tuner (an instance without a model proves the order)
    ft = object.__new__(T.FineTuner)
    ft.attention_map_alignment, ft.B = 2.0, 4
    ft.g = type("G", (), {"patches": 64})()
    with pytest.raises(ValueError, match="reference_attention"):
        ft.forward_backward(None, None, None, None)
    with pytest.raises(ValueError, match="reference_attention"):
        ft.step(None, None, None, None)


def test_annealing_factor():
    """scripts/train.py:370-371: (1 - step / num_steps) * coefficient with the count of applied updates."""
    from hypervla.train import alignment_weight
    assert alignment_weight(8.0, 0, 100) == 8.0
    assert alignment_weight(8.0, 1, 100) == pytest.approx(8.0 * 0.99, rel=1e-15)
    assert alignment_weight(8.0, 100, 100) == 0.0
    assert alignment_weight(8.0, 101, 100) == 0.0                      # never negative past the schedule's end
    assert alignment_weight(0.0, 5, None) == 0.0                       # off: num_steps is not read


def test_binding_is_the_header_s(tmp_path):
    """hvla_train_attention: size and field offsets of the ctypes mirror against the C compiler's view of include/hvla.h; the
    prototype; and the refusals that need no device."""
    import subprocess
    from hypervla import _native
    names = [n for n, _ in _native.hvla_train_attention._fields_]
    prog = "#include <stdio.h>\n#include <stddef.h>\n#include \"hvla.h\"\nint main(void) { printf(\"%zu\", sizeof(hvla_train_attention));\n"
    prog += "".join(f'printf(" %zu", offsetof(hvla_train_attention, {n}));\n' for n in names) + "return 0; }\n"
    (tmp_path / "l.c").write_text(prog)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "l.c"), "-o", str(tmp_path / "l")], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "l")], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == ctypes.sizeof(_native.hvla_train_attention)
    assert got[1:] == [getattr(_native.hvla_train_attention, n).offset for n in names]
    assert names[0] == "struct_size"
    src = open(os.path.join(ROOT, "include", "hvla.h")).read()
    assert re.search(r"\bint\s+hvla_train_attention_losses\s*\(\s*hvla_ctx\s*\*\s*ctx\s*,\s*const\s+hvla_train_attention\s*\*\s*opts\s*\)\s*;", src)
    assert "hvla_train_attention_losses" in _native.EXPORTS
    lib = _native.load_library()
    assert lib.hvla_train_attention_losses.restype is ctypes.c_int
    assert lib.hvla_train_attention_losses(None, None) == -7           # HVLA_E_STATE: no context (nothing else is touched)
