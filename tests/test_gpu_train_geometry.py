"""GPU: the fine-tune step at the edges of the accepted set (csrc/accept.h minus train_refusal) -- per-sample loss and
every gradient leaf against float64 autograd, one geometry per case.  tests/train_parity.py has the comparison; the bounds are the
suite's: loss rtol 3e-4 / atol 3e-5, worst leaf 2e-3 on the 64-patch base (the MID figure) and 3e-3 on the 256-patch base (the
full-width figure).  tests/test_train_workspace_extents.py walks the same geometries on the CPU (tools/train_extent_trace.hip uses
the names below)."""
import dataclasses

import numpy as np
import pytest

from adamw_ref import optax_step
from train_parity import assert_not_vacuous, encoder_case, frozen_encoder_case

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

MID_TOL, FULL_TOL = 2e-3, 3e-3
FULL1 = dict(enc_layers=1, layers=1, ctx_layers=1)          # the README widths with one layer of each kind

# name: (base, changes, B, encoder trained, extras)   extras: "update" one AdamW update after the gradient check,
#                                                             "repeat" the forward-only loss is bit-equal across two calls
CASES = {
    # ---- encoder frozen, B = 5 (325 rows: ragged tiles, odd batch)
    "P1": ("mid", dict(mlp=32), 5, False, ("repeat",)),                          # F < D: t.g receives rows x D; one hidden tile
    "P2": ("mid", dict(mlp=160, layers=3), 5, False, ()),                        # five hidden tiles, N not a power of two
    "P3": ("mid", dict(horizon=1), 5, False, ("update",)),                       # one head row in head_loss_kernel; vector length % 4 == 3
    "P4": ("mid", dict(horizon=4, action_dim=8), 5, False, ()),                  # all 32 head rows
    "P5": ("mid", dict(horizon=16, action_dim=2, ctx_layers=0), 5, False, ()),   # widest Hz; no context layers
    "P6": ("full", dict(mlp=32), 2, False, ()),                                  # S = 257, Sp = 260 padded attention rows with F < D
    "C1": ("mid", dict(lang_tokens=2), 5, False, ()),                            # context S = 4
    "C1n": ("mid", dict(lang_tokens=2, ctx_dim=32, ctx_heads=8, ctx_mlp=16), 5, False, ()),   # ... head width 4, F < C
    "C2": ("mid", dict(lang_tokens=38, lang_dim=20), 5, False, ("update",)),     # context S = 40, K = 20
    "C3": ("mid", dict(lang_tokens=15, ctx_mlp=48), 5, False, ()),               # S = 17 -> Sp = 20: zeros behind each row
    "C4": ("mid", dict(ctx_dim=128, ctx_heads=1), 5, False, ()),                 # one head of 128
    "C5": ("mid", dict(lang_dim=392), 5, False, ()),
    # ---- encoder trained
    "E1": ("mid", dict(enc_dim=256, enc_heads=4, enc_mlp=128), 5, True, ("repeat",)),          # F < E in the shared-weight GEMMs
    "E1-B128": ("mid", dict(enc_dim=256, enc_heads=4, enc_mlp=128), 128, True, ()),            # 8320 rows: colsum4, ls_bwd4
    "E2": ("mid", dict(enc_dim=640, enc_heads=10, enc_mlp=384), 3, True, ()),                  # MLP width no multiple of E
    "E3": ("mid", dict(patch=4, image_size=32), 5, True, ()),                                  # patch GEMM K = 48
    "E4": ("mid", dict(patch=16, image_size=128), 3, True, ()),                                # K = 768
    "E5": ("full", dict(patch=7, image_size=112), 2, True, ("update",)),                       # K = 147: the all-dword staging
    "E6": ("full", dict(enc_dim=1024, enc_heads=16, enc_mlp=128), 2, True, ()),                # ln_bwd_shared at D = 1024; F < E
    "E7": ("full", dict(enc_dim=128, enc_heads=2, enc_mlp=128, enc_layers=2), 3, True, ()),    # narrowest encoder
    "E8": ("full", dict(enc_layers=0), 2, True, ()),                                           # patch embedding + final LayerNorm only
    "E9": ("full", dict(enc_dim=256, enc_heads=4, enc_mlp=640), 9, True, ()),                  # 2313 rows: colsum4b for N = 640 only
}


def geometry(name):
    from hypervla.config import FULL, MID
    base, changes = CASES[name][:2]
    g = MID if base == "mid" else dataclasses.replace(FULL, **FULL1)
    return dataclasses.replace(g, **changes), (MID_TOL if base == "mid" else FULL_TOL)


def _one_update(ft, enc):
    """One FineTuner update from the gradient just computed against tests/adamw_ref.py::optax_step from the read-back state, at the
    tolerances of test_gpu_train.py::test_adamw_step_matches_reference_update (params and EMA atol 2e-6 at lr 1e-3, sum|mu| to 1 %);
    nu as test_adamw_six_updates_against_the_optax_chain holds it (rtol 1e-6 given the device's own clip scale)."""
    r64 = lambda x: x.float().cpu().numpy().astype(np.float64)
    lr = blr = 1e-3
    hy = dict(ft.hy, lr=lr, base_lr=blr)
    st = dict(p=r64(ft.params), mu=r64(ft.mu), nu=r64(ft.nu), ema=r64(ft.ema), g=r64(ft.grads), mask=ft.wd_mask.cpu().numpy(),
              p0=r64(ft.params0) if ft.params0 is not None else None)
    assert ft.step_count == 0 and (ft.n > ft.n_hyper) == enc and np.abs(st["g"]).max() > 0
    assert ft.apply(lr=lr, base_lr=blr) is True
    norm32 = np.sqrt(np.float32(ft.sqsum.cpu().numpy()[0]))
    clip32 = np.float32(hy["clip"])
    sc = 1.0 if norm32 < clip32 else float(clip32 / norm32)
    want = optax_step(st, hy, 1, sc, ft.n_hyper)
    got_p, got_mu, got_nu, got_ema = r64(ft.params), r64(ft.mu), r64(ft.nu), r64(ft.ema)
    print(f"one update over {ft.n} elements (n % 4 = {ft.n % 4}): clip scale {sc:.4g}; params max |d| {np.abs(got_p - want['p']).max():.2e}; "
          f"ema max |d| {np.abs(got_ema - want['ema']).max():.2e}; sum|mu| {np.abs(got_mu).sum():.6e} against {np.abs(want['m']).sum():.6e}")
    np.testing.assert_allclose(got_p, want["p"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(got_ema, want["ema"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(got_nu, want["nu"], rtol=1e-6, atol=1e-37)
    assert abs(np.abs(got_mu).sum() - np.abs(want["m"]).sum()) <= 1e-2 * np.abs(want["m"]).sum()


@pytest.mark.parametrize("name", list(CASES))
def test_loss_and_every_gradient_leaf_at_the_edge(name):
    _, _, B, enc, extras = CASES[name]
    g, tol = geometry(name)
    report = {}
    kw = dict(ema_start_step=0) if "update" in extras else {}
    try:
        model, ft, (ins, st, obs, batch) = (encoder_case if enc else frozen_encoder_case)(g, B, tol, report=report, **kw)
    finally:
        if "worst" in report:
            print(f"EDGE {name} B={B} loss_err={report['loss_err']:.2e} worst={report['worst'][0]:.2e} {report['worst'][1]}")
    assert report["leaves"] == set(report["grads"]), report["leaves"] ^ set(report["grads"])
    above, n = assert_not_vacuous(report["grads"], enc)
    print(f"EDGE {name} leaves above the floor: {above} of {n}")
    if "repeat" in extras:            # the forward pass has no atomics
        a = ft.forward_backward(ins, st, obs, batch, forward_only=True).clone()
        b = ft.forward_backward(ins, st, obs, batch, forward_only=True)
        assert torch.equal(a, b)
    elif "update" in extras:
        _one_update(ft, enc)
