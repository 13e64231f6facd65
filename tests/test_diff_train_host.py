"""CPU: fine-tuning a use_differential_transformer model (FineTuner(differential=True), hvla_train_differential) -- the
torch restatement against the numpy one and against finite differences, the backward formulas the kernels implement against autograd,
the training layout and the refusals in C++ under ASan / UBSan, the traced step's extents, the conditions on the GPU cases' inputs
and their float32 floor, and the Python plumbing.  No GPU.

Float32 floor of the GPU cases (tests/diff_train_ref.CASES; the whole restatement in torch float32 against float64; loss error as a
fraction of its tolerance 3e-5 + 3e-4 |loss|, worst leaf in train_parity's metric against 2e-3), measured:
    MID, B = 4, encoder frozen        0.0023, 1.8e-05
    README geometry, B = 2            0.0047, 7.2e-05
    MID, B = 2, encoder trained       0.0008, 3.4e-05
all under a quarter of the bounds, so the project's own bounds stand, on the synthetic checkpoint with the lambda heads x 5 and no
further sharpening."""
import ctypes
import dataclasses
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import diff_attention_ref as DR
import diff_train_ref as T
import test_train_workspace_extents as X
from hypervla.config import FULL, MID, generated_leaves
from train_parity import FLOOR, leaf_errors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hyper-vla_amd", "csrc")
MID_D = dataclasses.replace(MID, differential=True)
FULL_D = dataclasses.replace(FULL, differential=True)
ATTN = "DifferentialAttention_0"
MODULE = ("lambda_q1", "lambda_k1", "lambda_q2", "lambda_k2", "subln_weight", "q_proj_kernel", "k_proj_kernel", "v_proj_kernel",
          "out_proj_kernel")


# ---------------------------------------------------------------------------------------------- 1. the forward restatement
@pytest.mark.parametrize("g,B", [(MID_D, 4), (FULL_D, 2)])
def test_the_torch_forward_is_the_numpy_restatement(g, B):
    from hypervla import synthetic as syn
    from oracle import hvla_ref_torch as ot
    leaves = generated_leaves(g)
    P = T.case_params(g)
    ins, st = syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g)
    tok = np.random.default_rng(3).standard_normal((B, g.patches, g.enc_dim))
    hn = ot.HyperNetRef(P, g, leaves, torch.float64)
    li = ins["language_instruction"]
    theta = hn.generate(hn.context(li["token_embedding"], li["attention_mask"], np.asarray(st["patch_embeddings"])[:, 0]))
    act, logit, lam = T.PolicyDiffRef(g, leaves)(theta, torch.as_tensor(tok))
    bp = {l.flat_name: theta[:, l.offset:l.offset + l.size].reshape((B,) + tuple(l.shape)).numpy() for l in leaves}
    ract, rlog = DR.policy(bp, g, tok, "restated")
    assert np.abs(act.numpy() - ract).max() <= 1e-12 and np.abs(logit.numpy() - rlog).max() <= 1e-12
    assert np.abs(lam.numpy() - DR.lambdas(bp, g)).max() <= 1e-12
    pact, plog = DR.policy(bp, g, tok, "plain")                          # ... and so is the model without the flag
    act2, logit2, _ = T.PolicyDiffRef(g, leaves, "plain")(theta, torch.as_tensor(tok))
    assert np.abs(act2.numpy() - pact).max() <= 1e-12 and np.abs(logit2.numpy() - plog).max() <= 1e-12


# ---------------------------------------------------------------------------------------------- 2. autograd
def _block_inputs(B, S, D, H, seed=0, scale=0.3):
    r = np.random.default_rng(seed)
    t = lambda *s, k=scale: torch.as_tensor(r.standard_normal(s) * k).requires_grad_(True)
    hd = D // (2 * H)
    return [t(B, S, D, k=1.0), t(B, D, D), t(B, D, D), t(B, D, D), t(B, D, D), t(B, hd), t(B, hd), t(B, hd), t(B, hd),
            (torch.as_tensor(1.0 + 0.1 * r.standard_normal((B, 2 * hd)))).requires_grad_(True)]


def test_finite_differences_agree_with_autograd_on_one_block():
    """torch.autograd.gradcheck on diff_attention at S = 9 (two episodes, D = 16, H = 2, depth 1), every input and leaf."""
    inp = _block_inputs(2, 9, 16, 2)
    fn = lambda *a: T.diff_attention(*a, 1, 2)
    assert torch.autograd.gradcheck(fn, inp, eps=1e-6, atol=1e-7, rtol=1e-5)


def test_the_backward_the_kernels_implement_is_autograd_s():
    """DESIGN.md §23's formulas from dN on, as block_bwd sequences them (S = 9, D = 64, H = 4, depth 2), against autograd to 1e-10."""
    B, S, D, H, depth = 2, 9, 64, 4, 2
    hd = D // (2 * H)
    h, wq, wk, wv, wo, lq1, lk1, lq2, lk2, sw = inp = _block_inputs(B, S, D, H, 1)
    out = T.diff_attention(*inp, depth, H)
    dy = torch.as_tensor(np.random.default_rng(2).standard_normal(out.shape))
    want = torch.autograd.grad((out * dy).sum(), inp)
    with torch.no_grad():
        linit = DR.lambda_init_fn(depth)
        q = torch.bmm(h, wq).reshape(B, S, H, 2, hd)
        k = torch.bmm(h, wk).reshape(B, S, H, 2, hd)
        v = torch.bmm(h, wv).reshape(B, S, H, 2 * hd).transpose(1, 2)
        M = torch.as_tensor(DR.mask_matrix(S)).double()
        A1, A2 = (torch.softmax(torch.einsum("bqhd,bkhd->bhqk", q[:, :, :, c], k[:, :, :, c]) + M, -1) for c in range(2))
        l1, l2 = torch.exp((lq1 * lk1).sum(-1)), torch.exp((lq2 * lk2).sum(-1))
        lam = (l1 - l2 + linit)[:, None, None, None]
        A = A1 - lam * A2
        O = A @ v
        r = torch.rsqrt((O * O).mean(-1, keepdim=True) + 1e-5)
        n = O * r
        N = (n * sw[:, None, None] * (1 - linit)).transpose(1, 2).reshape(B, S, D)
        dwo = torch.bmm(N.transpose(1, 2), dy)
        dN = torch.bmm(dy, wo.transpose(1, 2)).reshape(B, S, H, 2 * hd).transpose(1, 2)
        g = (1 - linit) * dN
        dw = (g * n).sum((1, 2))
        gw = g * sw[:, None, None]
        dO = r * (gw - n * (gw * n).mean(-1, keepdim=True))
        dP = dO @ v.transpose(-1, -2)
        dV = A.transpose(-1, -2) @ dO
        t1, t2 = (dP * A1).sum(-1, keepdim=True), (dP * A2).sum(-1, keepdim=True)
        ds1, ds2 = A1 * (dP - t1), -lam * A2 * (dP - t2)
        dlam = -t2.sum((1, 2, 3))
        dq = torch.stack([torch.einsum("bhqk,bkhd->bqhd", ds, k[:, :, :, c]) for c, ds in enumerate((ds1, ds2))], 3).reshape(B, S, D)
        dk = torch.stack([torch.einsum("bhqk,bqhd->bkhd", ds, q[:, :, :, c]) for c, ds in enumerate((ds1, ds2))], 3).reshape(B, S, D)
        dv = dV.transpose(1, 2).reshape(B, S, D)
        got = [torch.bmm(dq, wq.transpose(1, 2)) + torch.bmm(dk, wk.transpose(1, 2)) + torch.bmm(dv, wv.transpose(1, 2)),
               torch.bmm(h.transpose(1, 2), dq), torch.bmm(h.transpose(1, 2), dk), torch.bmm(h.transpose(1, 2), dv), dwo,
               (dlam * l1)[:, None] * lk1, (dlam * l1)[:, None] * lq1, (-dlam * l2)[:, None] * lk2, (-dlam * l2)[:, None] * lq2, dw]
    for a, b in zip(got, want):
        assert float((a - b).abs().max()) <= 1e-10 * max(1.0, float(b.abs().max()))


# ---------------------------------------------------------------------------------------------- 3. layout and refusals in C++
@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_cxx_training_layout_finds_every_leaf_and_the_refusals_keep_their_forms(tmp_path):
    src = tmp_path / "train_diff_layout_check.cpp"
    src.write_text(r'''
#include <cstdio>
#include <cstring>
#include "train_layout.h"
using namespace hvla;
static int check(Geom g, const char* name) {
  Geom on = g; on.differential = 1;
  const TrainLayout L = make_train_layout(on), L0 = make_train_layout(g);
  if (!L.policy_ok || !L0.policy_ok) { printf("policy_ok\n"); return 1; }
  for (int l = 0; l < g.L; ++l) {
    const BlockLeaves& y = L.pol[l];
    const DiffLeaves& d = L.dif[l];
    if (y.bq != -1 || y.bk != -1 || y.bv != -1 || y.bo != -1) { printf("bias offsets\n"); return 1; }
    if (y.wq < 0 || y.wk < 0 || y.wv < 0 || y.wo < 0 || y.ln0_s < 0 || y.w1 < 0 || y.b2 < 0) { printf("block leaves\n"); return 1; }
    printf("dif %s %d %ld %ld %ld %ld %ld %ld %ld %ld %ld\n", name, l, d.lq1, d.lk1, d.lq2, d.lk2, d.sw, y.wq, y.wk, y.wv, y.wo);
    const DiffLeaves& d0 = L0.dif[l];
    if (d0.lq1 != -1 || d0.lk1 != -1 || d0.lq2 != -1 || d0.lk2 != -1 || d0.sw != -1 || L0.pol[l].bq < 0) { printf("flag off\n"); return 1; }
  }
  printf("## %s %ld %ld\n", name, L.total, L.G);
  if (train_refusal(on, false, true) || train_refusal(on, true, true)) { printf("three-argument form\n"); return 1; }
  const char* a = train_refusal(on);
  const char* b = train_refusal(on, false);
  const char* c = train_refusal(on, true);
  const char* d = train_refusal(on, false, false);
  if (!a || !b || !c || !d || a != b || a != c || a != d || !strstr(a, "use_differential_transformer")) { printf("old forms\n"); return 1; }
  if (train_refusal(g) || train_refusal(g, true) || train_refusal(g, false, true)) { printf("plain\n"); return 1; }
  Geom lang = g; lang.lang_in_policy = 1;
  if (!train_refusal(lang, false, true) || train_refusal(lang, true, true) || train_refusal(lang, true)) { printf("language\n"); return 1; }
  Geom deep = on; deep.L = TRAIN_MAX_POLICY_LAYERS + 1;
  if (!train_refusal(deep, false, true) || !strstr(train_refusal(deep, false, true), "too many layers")) { printf("layers\n"); return 1; }
  return 0;
}
int main() {
  Geom mid{112, 14, 128, 2, 2, 512, 64, 2, 4, 128, 4, 7, 5.f, 5.f, 128, 2, 4, 256, 12, 64, 1};
  Geom full{224, 14, 768, 12, 12, 3072, 64, 4, 4, 128, 4, 7, 5.f, 5.f, 128, 6, 4, 512, 32, 768, 1};
  if (check(mid, "MID") || check(full, "README")) return 1;
  printf("OK\n");
  return 0;
}
''')
    exe = tmp_path / "train_diff_layout_check"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                            "-I", CSRC, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.strip().endswith("OK"), run.stdout[-2000:] + run.stderr
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr
    from hypervla.train import train_param_layout
    for name, g in (("MID", MID_D), ("README", FULL_D)):
        at = {l.flat_name: l.offset for l in generated_leaves(g)}
        head = next(ln.split() for ln in run.stdout.splitlines() if ln.startswith(f"## {name} "))
        assert [int(head[2]), int(head[3])] == [train_param_layout(g)[1], generated_leaves(g)[-1].offset + generated_leaves(g)[-1].size]
        rows = [[int(x) for x in ln.split()[2:]] for ln in run.stdout.splitlines() if ln.startswith(f"dif {name} ")]
        assert len(rows) == g.layers
        for l, row in enumerate(rows):
            pa = f"encoder_Transformer_0_encoderblock_{l}_{ATTN}_"
            assert row == [l] + [at[pa + n] for n in ("lambda_q1", "lambda_k1", "lambda_q2", "lambda_k2", "subln_weight", "q_proj_kernel",
                                                      "k_proj_kernel", "v_proj_kernel", "out_proj_kernel")]


# ---------------------------------------------------------------------------------------------- 4. extents
def _points(exe_dir, tool):
    exe = os.path.join(str(exe_dir), tool)
    build = subprocess.run([X.HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O1", "-DHVLA_TRAIN_TRACE", "-I", CSRC,
                            os.path.join(ROOT, "tools", tool + ".hip"), X.TRAIN_HIP, "-o", exe],
                           cwd=str(exe_dir), capture_output=True, text=True, timeout=900)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr
    points = []
    for ln in run.stdout.splitlines():
        w = ln.split(" ")
        if w[0] == "#":
            points.append(dict(title=ln[2:], workspace=None, size={}, plan=[], lines=[]))
        elif w[0] == "workspace":
            points[-1]["workspace"] = int(w[1])
        elif w[0] == "size":
            points[-1]["size"][w[1]] = int(w[2])
        elif w[0] == "plan":
            points[-1]["plan"].append((w[1], int(w[2]), int(w[3])))
        elif w[0] != "step":
            points[-1]["lines"].append(ln)
    return points


@pytest.fixture(scope="module")
def points(tmp_path_factory):
    if not os.path.exists(X.HIPCC):
        pytest.skip("needs hipcc")
    return _points(tmp_path_factory.mktemp("diff_extent_trace"), "train_diff_extent_trace")


def test_differential_steps_obey_the_extent_rules(points):
    """MID at B = 4 and B = 1, the README widths at B = 2, encoder frozen and trained: the rules of
    tests/test_train_workspace_extents.py -- no GEMM's C extent meets its A or B extent, every operand inside ONE named plan buffer or
    its vector, nothing beyond the workspace the step reports; no buffer is named `?` (the checker refuses one)."""
    on = [pt for pt in points if "-diff " in pt["title"]]
    seen = {}
    for pt in on:
        w = dict(kv.split("=") for kv in pt["title"].split(" ")[1:])
        seen.setdefault(pt["title"].split(" ")[0], set()).add((int(w["B"]), int(w["enc"])))
    assert seen == {"MID-diff": {(4, 0), (4, 1), (1, 0), (1, 1)}, "README2-diff": {(2, 0), (2, 1)}}, seen
    for pt in on:
        names = [n for n, _, _ in pt["plan"]]
        assert "?" not in names and {"pb[0].pa", "pb[0].oraw", "t.dP", "t.t2"} <= set(names), pt["title"]
    bad = X.violations(on)
    assert not bad, "%d violations\n%s" % (len(bad), "\n".join(bad[:10]))


def test_the_step_launches_differential_attention_for_the_policy_only(points):
    """MID, B = 4, encoder frozen: per policy layer one additive softmax over B 2 H tables of S = 65 rows (stride 68), one combine, one
    subln forward and backward, one differential softmax backward and one lambda backward; the score product has K = 8, 2 H inner
    batches and alpha 1; no bias gradient of the four projections is launched; the context encoder keeps its kernels."""
    g, B = MID_D, 4
    pt = next(p for p in points if p["title"].startswith("MID-diff ") and " B=4 enc=0 " in p["title"])
    S, H, D = g.seq, g.heads, g.dim
    count = lambda k: sum(ln.startswith(k + " ") for ln in pt["lines"])
    soft = [ln.split(" ") for ln in pt["lines"] if ln.startswith("softmax_bias_fwd_kernel ")]
    assert len(soft) == g.layers and all(w[4:] == [str(B * 2 * H), str(S), "68"] for w in soft), soft
    for k in ("diff_combine_fwd_kernel", "diff_subln_fwd_kernel", "diff_subln_bwd_kernel", "diff_softmax_bwd_kernel", "diff_lambda_bwd_kernel"):
        assert count(k) == g.layers, k
    assert count("softmax_bwd_kernel") == g.ctx_layers and count("softmax_fwd_kernel") == g.ctx_layers
    gemms = [dict(zip(X.BG_FIELDS, ln.split(" ", 4)[4][3:-1].split(" ")), tb=ln.split(" ")[2]) for ln in pt["lines"] if ln.startswith("bgemm ")]
    scores = [f for f in gemms if f["K"] == "8" and f["tb"] == "1"]
    assert len(scores) == g.layers and all((f["M"], f["N"], f["nb1"], f["alpha"], f["sA1"], f["sB1"]) == (str(S), str(S), str(2 * H), "1", "8", "8")
                                           for f in scores), scores
    at = {l.flat_name: l.offset for l in generated_leaves(g)}
    sizes = {l.flat_name: l.size for l in generated_leaves(g)}
    for ln in pt["lines"]:                                   # column sums into dtheta: none lands inside a differential leaf
        w = ln.split(" ")
        if w[0].startswith("colsum") and w[4].startswith("dtheta+"):
            o = int(w[4][7:])
            hit = [k for k in at if ATTN in k and at[k] <= o < at[k] + sizes[k]]
            assert not hit, (ln, hit)


def test_a_flag_off_point_is_what_the_plain_driver_prints(points, tmp_path_factory):
    """MID at B = 4, encoder frozen and trained, without the flag: the plan, the workspace and every launch are those of
    tools/train_extent_trace.hip's point of the same title -- with the flag off nothing moved."""
    base = _points(tmp_path_factory.mktemp("extent_trace_base"), "train_extent_trace")
    off = [pt for pt in points if pt["title"].startswith("MID ")]
    assert len(off) == 2
    for pt in off:
        same = [b for b in base if b["title"] == pt["title"]]
        assert same and same[0] == pt, pt["title"]
        assert not any(ln.startswith("diff_") for ln in pt["lines"]) and not any(n.endswith(".pa") or n.endswith(".oraw") or n in ("t.dP", "t.t2") for n, _, _ in pt["plan"])


def test_the_rules_see_a_table_sized_for_h_heads(points):
    """Not vacuous: with pb[*].p and t.dp of the MID point cut back to H tables, rule (b) reports the score product, the softmax
    backward's output and the dq / dk products."""
    pt = next(p for p in points if p["title"].startswith("MID-diff ") and " B=4 enc=0 " in p["title"])
    cut = dict(pt, plan=[(n, off, sz // 2 if n.endswith("].p") and n.startswith("pb[") or n == "t.dp" else sz) for n, off, sz in pt["plan"]])
    bad = X._Checker(cut).run()
    assert bad and all("(b)" in v for v in bad), bad[:3]


# ---------------------------------------------------------------------------------------------- 5. the inputs and the float32 floor
@pytest.fixture(scope="module", params=sorted(T.CASES))
def ref(request):
    return (request.param,) + T.case_reference(request.param)


def test_conditions_on_the_gpu_cases_inputs(ref):
    """On the reference alone: every lambda_*, subln_weight and *_proj_kernel head is above the floor of the leaf metric, and so is
    every other output head (the only leaves under it are the context encoder's and DINOv2's key biases and DINOv2's unused mask
    token, whose true gradient is zero); lambda spreads over the episodes by >= 1.0 in some layer; the restatements with lambda
    frozen at lambda_init and with plain attention are >= 10 tolerances away in the loss or in some leaf."""
    name, per, grads, lam = ref
    g = T.case_geometry(name)
    gmax = max(float(v.abs().max()) for v in grads.values())
    heads = [k for k in grads if k.startswith("output_head_")]
    module = [k for k in heads if ATTN in k]
    assert len(module) == 2 * 9 * g.layers and all(any(k.split("/")[0].endswith(m) for m in MODULE) for k in module)
    low = [k for k in grads if float(grads[k].abs().max()) <= FLOOR * gmax]
    assert not [k for k in low if k in heads], low
    assert all("key/bias" in k or k.endswith("key_bias") or k.endswith("mask_token") for k in low), low
    spread = (lam.max(0).values - lam.min(0).values).numpy()
    print(f"{name}: lambda {lam.numpy().round(3).tolist()}, spread per layer {spread.round(3)}; smallest module head "
          f"{min(float(grads[k].abs().max()) for k in module) / gmax:.2e} of gmax; under the floor: {low}")
    assert spread.max() >= 1.0
    for mode in ("lambda_init", "plain"):
        per2, grads2, _ = T.case_reference(name, mode)
        tol = T.LOSS_ATOL + T.LOSS_RTOL * per.abs().numpy()
        moved = float(((per - per2).abs().numpy() / tol).max())
        rel, _ = leaf_errors({k: v.numpy() for k, v in grads2.items()}, grads)
        print(f"{name}: {mode} is {moved:.0f} loss tolerances and {rel[0][0] / T.LEAF_TOL:.0f} leaf tolerances away")
        assert max(moved, rel[0][0] / T.LEAF_TOL) >= 10.0


def test_float32_floor_is_under_a_quarter_of_the_bounds(ref):
    """The whole restatement in torch float32 against float64 on the GPU case's inputs (module docstring): the bounds stand."""
    name, per, grads, _ = ref
    per32, grads32, _ = T.case_reference(name, "diff", torch.float32)
    err = (per32.double() - per).abs().numpy()
    tol = T.LOSS_ATOL + T.LOSS_RTOL * per.abs().numpy()
    rel, _ = leaf_errors({k: v.double().numpy() for k, v in grads32.items()}, grads)
    print(f"{name}: float32 loss error {err.max():.2e} = {(err / tol).max():.4f} of its tolerance; worst leaves "
          f"{[(f'{r:.2e}', k) for r, k in rel[:3]]}")
    assert (err / tol).max() <= 0.25 and rel[0][0] <= T.LEAF_TOL / 4


# ---------------------------------------------------------------------------------------------- 6. Python plumbing
def _head_cols(g, mask_w, mask_b):
    out = {}
    for l in generated_leaves(g):
        out[l.flat_name] = (mask_w[:, l.offset:l.offset + l.size], mask_b[l.offset:l.offset + l.size])
    return out


@pytest.mark.parametrize("strategy", ["v1", "v2", "v3", "v5"])
def test_weight_decay_mask_marks_the_projection_heads(strategy):
    from hypervla.train import train_param_layout, weight_decay_mask
    g = MID_D
    at = {n: (o, s) for n, o, s in train_param_layout(g)[0]}
    m = weight_decay_mask(g, strategy)
    (wo, ws), (bo, bs) = at["W_cat"], at["b_cat"]
    cols = _head_cols(g, m[wo:wo + int(np.prod(ws))].reshape(ws), m[bo:bo + bs[0]])
    for l in range(g.layers):
        pa = f"encoder_Transformer_0_encoderblock_{l}_{ATTN}_"
        for n in ("q_proj_kernel", "k_proj_kernel", "v_proj_kernel", "out_proj_kernel"):
            assert cols[pa + n][0].all() and cols[pa + n][1].all(), (strategy, n)     # kernel and bias: the head's name holds "kernel"
        for n in ("lambda_q1", "lambda_k1", "lambda_q2", "lambda_k2", "subln_weight"):
            if strategy in ("v3", "v5"):
                assert not cols[pa + n][0].any() and not cols[pa + n][1].any(), (strategy, n)


def test_frozen_keys_freeze_exactly_the_lambda_heads():
    from hypervla.train import frozen_plan, train_param_layout
    g = MID_D
    mask, buckets = frozen_plan(g, frozen_keys=("output_head_*lambda*",))
    at = {n: (o, s) for n, o, s in train_param_layout(g)[0]}
    (wo, ws), (bo, bs) = at["W_cat"], at["b_cat"]
    cols = _head_cols(g, mask[wo:wo + int(np.prod(ws))].reshape(ws), mask[bo:bo + bs[0]])
    assert buckets == 0 and not mask[:wo].any()
    n_lambda = 0
    for name, (w, b) in cols.items():
        if "_lambda_" in name:
            assert w.all() and b.all(), name
            n_lambda += 1
        else:
            assert not w.any() and not b.any(), name
    assert n_lambda == 4 * g.layers


class _Model:
    """What FineTuner's constructor may look at before it refuses: the geometry.  Anything else is an AttributeError."""
    def __init__(self, g):
        self.geometry = g


def test_finetuner_refusals_need_no_device():
    from hypervla.train import FineTuner
    with pytest.raises(ValueError, match=r"use_differential_transformer is not built; serving is"):      # the keyword missing: its present words
        FineTuner(_Model(MID_D), 2)
    with pytest.raises(ValueError, match="differential=True needs a model with vit_kwargs.use_differential_transformer"):
        FineTuner(_Model(MID), 2, differential=True)
    for kw in (dict(attention_entropy=0.1), dict(attention_map_alignment=1.0, num_steps=10)):
        with pytest.raises(ValueError, match="attention_entropy / attention_map_alignment are not defined with differential=True"):
            FineTuner(_Model(MID_D), 2, differential=True, **kw)
    for kw in (dict(dropout_rate=0.1), dict(image_embedding_noise=0.1), dict(embedding_dropout_rate=0.1), dict(image_dropout=0.1)):
        with pytest.raises(ValueError, match="with differential=True are not built"):
            FineTuner(_Model(MID_D), 2, differential=True, **kw)
    with pytest.raises(ValueError, match="language_tokens"):
        FineTuner(_Model(MID_D), 2, differential=True, language_tokens=True)
    with pytest.raises(AttributeError):                                      # accepted: the constructor goes on to the model
        FineTuner(_Model(MID_D), 2, differential=True)


def test_binding_and_header_have_the_setting():
    from hypervla import _native
    src = open(os.path.join(ROOT, "include", "hvla.h")).read()
    assert re.search(r"\bint\s+hvla_train_differential\s*\(\s*hvla_ctx\s*\*\s*ctx\s*,\s*int32_t\s+on\s*\)\s*;", src)
    assert "hvla_train_differential" in _native.EXPORTS
    lib = _native.load_library()
    assert lib.hvla_train_differential.restype is ctypes.c_int
    for on in (0, 1, 2):                                   # HVLA_E_STATE: a NULL context, whatever the value
        assert lib.hvla_train_differential(None, on) == -7
