"""CPU: the case table of tools/bgemm_check.py (the fine-tune GEMM's single-launch check, tests/test_gpu_train_gemm.py) through a CPU
emulation of the kernel's arithmetic -- operands split into bf16 halves, f32 accumulation chunk by chunk, K chunks and batch entries
added in random order, the store modes / alpha / bias of the epilogue -- held to the SAME two criteria the device is held to.  What this
proves without a GPU: the float64 reference honours every stride, transpose and batch field of every descriptor in the table (the
emulation gathers through the same descriptor but is otherwise independent: f32 chunks against one float64 product), the exact class's
inputs really make f32 accumulation order-free (bit-equality at every depth of the table, K = 16 288 and the thinned K = 201 500
included), and the arithmetic the kernel is meant to do stays inside the precision class's bound.  Only outer batch counts are cut
(to 3: outer batch entries, and the number of 257-row images folded into M or K of the shared-weight products) to keep this under a
minute; no edge size is.  Chunks are 16 deep where the product is small and 256 deep elsewhere (exact either way)."""
import importlib.util
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("bgemm_check", os.path.join(ROOT, "tools", "bgemm_check.py"))
    mod = importlib.util.module_from_spec(spec)
    import sys
    sys.modules["bgemm_check"] = mod          # dataclasses looks the module up while the class is made
    spec.loader.exec_module(mod)
    return mod


bc = _tool()
TABLE = bc.case_table()
GROUPS = sorted({c.group for c in TABLE})


def _run(c, drop=None):
    c = bc.shrunk(c)
    inp = bc.make_inputs(c)
    if c.cls == "exact":
        bc.assert_exactness(c, inp)
    want, tol = bc.reference(c, inp)
    got = bc.emulate(c, inp, np.random.default_rng(c.seed), drop=drop)
    return bc.compare(c, got, want, tol)


@pytest.mark.parametrize("group", GROUPS)
def test_emulated_kernel_meets_the_criteria_on_every_case_of_the_group(group):
    cases = [c for c in TABLE if c.group == group]
    assert cases
    worst, bad = 0.0, []
    for c in cases:
        ok, ratio, text = _run(c)
        worst = max(worst, ratio)
        if not ok:
            bad.append((c.name, text))
    print(group, len(cases), "cases; worst err/bound", worst)
    assert not bad, bad[:5]
    if group.startswith("precision"):
        # measured on the emulation: the correct product sits at 0.02 - 0.35 of the bound; half of it is not a vacuous bound
        assert 0.0 < worst <= 0.5, worst


def test_table_covers_what_it_promises():
    names = {c.group for c in TABLE}
    for g in ("calibration", "forms", "dword reasons", "a_padded", "edges", "k depth", "split-K 64", "split-K 128", "modes", "two batch levels", "f32 kernel",
              "replay B = 1", "replay B = 32", "precision forms", "precision k depth", "precision modes"):
        assert g in names, g
    assert TABLE[0].group == "calibration" and (TABLE[0].M, TABLE[0].N, TABLE[0].K, TABLE[0].order) == (64, 64, 32, "NN")
    assert all(c.K <= 257 for c in TABLE if c.cls == "precision")
    for Mn in (1, 31, 64, 95, 96, 127, 128, 129, 257, 384):
        assert any(c.M == Mn for c in TABLE) and any(c.N == Mn for c in TABLE), Mn
    for K in (1, 3, 4, 31, 32, 33, 63, 64, 65, 95, 96, 97, 257, 260, 1290):
        assert any(c.K == K for c in TABLE), K
    rep = [c for c in TABLE if c.group == "replay B = 32"]
    assert len(rep) >= 25 and all(c.cls == "exact" for c in rep)
    assert any(c.M == 1 for c in rep) and any(c.order == "TN" and c.K == 1 for c in rep) and any(c.order == "TN" and c.K == 32 for c in rep)
    assert any(c.N == 201500 for c in rep) and sum(c.nb1 == 3 for c in rep) >= 2 and sum(c.a_padded and c.lda == 260 and c.K in (64, 257) and c.M == 257 for c in rep) >= 4
    assert any(c.M == 8224 and c.N == 768 for c in rep)


def test_a_dropped_cross_term_fails_the_precision_class():
    """mutation: without the a.lo b.hi product (one of mma32_x3's three) the emulated kernel leaves the bound in every precision-class
    form case -- and a deep exact-class case is off by whole units."""
    hit = 0
    for c in TABLE:
        if c.group == "precision forms" and c.nb0 == 1:
            ok, ratio, _ = _run(c, drop="lohi")
            assert not ok and ratio > 3.0, (c.name, ratio)
            hit += 1
    assert hit >= 16
    c = next(c for c in TABLE if c.group == "k depth" and c.K == 257)
    assert not _run(c, drop="lohi")[0]


def test_bias_added_by_every_k_chunk_fails_the_split_k_cases():
    """mutation: `bias && kc == 0` -> `bias`."""
    cs = [c for c in TABLE if c.bias and (c.ksplit > 1 or c.allow_split) and c.K >= 256]
    assert len(cs) >= 8
    for c in cs:
        assert _run(c)[0] and not _run(c, drop="bias_every_chunk")[0], c.name


def test_every_lost_or_doubled_product_moves_an_exact_class_entry_by_about_one():
    """the exact class's sensitivity: zeroing or doubling one (m, k) element of A moves row m of the expected C by >= 1 - 2^-9 in every
    column, at the shallowest and the deepest K of the table (and the emulation, 16-deep f32 chunks,
    is bit-equal to float64 there)."""
    for K in (1, 97, 257, 8224, 16288):
        c = bc.Case("probe", "probe", "exact", "NN", 8, 8, K, seed=K)
        inp = bc.make_inputs(c)
        bc.assert_exactness(c, inp)
        want, tol = bc.reference(c, inp)
        assert bc.compare(c, bc.emulate(c, inp, np.random.default_rng(K)), want, tol)[0]        # 16-deep chunks at every one of these depths
        for f in (0.0, 2.0):
            alt = {k: (v.clone() if hasattr(v, "clone") else v) for k, v in inp.items()}
            alt["A"][alt["oA"] + 3 * c.lda + K // 2] *= f
            w2, _ = bc.reference(c, alt)
            d = (w2 - want)[bc.GUARD + 3 * 8:bc.GUARD + 4 * 8].abs()
            assert float(d.min()) >= 1 - 2.0 ** -9, (K, f, float(d.min()))
