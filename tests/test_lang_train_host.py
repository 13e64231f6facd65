"""CPU: fine-tuning a use_language_token model (FineTuner(language_tokens=True), hvla_train_language_tokens) -- the
float64 torch restatement the GPU tests differentiate against the numpy one, the C++ layout against Python's, every launch of the
step inside the workspace plan for the language geometries, and the constructor's refusals.  No GPU."""
import dataclasses
import os
import shutil
import subprocess

import numpy as np
import pytest

import lang_policy_ref as LR
import lang_policy_torch as LT
import test_train_workspace_extents as X
from hypervla import synthetic as syn
from hypervla.config import MID, generated_leaves

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hyper-vla_amd", "csrc")


@pytest.mark.parametrize("name", ["T12", "T2"])
def test_torch_restatement_is_the_numpy_one(name):
    """Actions and gripper logits of LangPolicyRef (torch float64, what autograd differentiates) against tests/lang_policy_ref.policy
    (numpy float64) on synthetic weights: both float64, different summation orders -> 1e-9 absolute."""
    g, B = LT.geometry(name)
    P = syn.synthetic_params(g)
    ins, st = syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g)
    lang = np.asarray(ins["language_instruction"]["token_embedding"], np.float64)
    tok = np.random.default_rng(9).standard_normal((B, g.patches, g.enc_dim))
    bp = LR.create_tasks(P, g, ins, st)
    leaves = generated_leaves(g)
    theta = np.concatenate([np.asarray(bp[l.flat_name], np.float64).reshape(B, -1) for l in leaves], 1)
    act, logit, _ = LT.LangPolicyRef(g, leaves)(torch.as_tensor(theta), torch.as_tensor(tok), torch.as_tensor(lang))
    ract, rlog, _ = LR.policy(bp, g, tok, lang)
    da, dl = np.abs(act.numpy()[..., :-1] - ract[..., :-1]).max(), np.abs(logit.numpy() - rlog).max()
    print(f"{name}: torch against numpy restatement, actions max |d| {da:.2e}, logits {dl:.2e}")
    assert da <= 1e-9 and dl <= 1e-9
    assert np.abs(ract[..., :-1]).max() > 1e-3                 # not a comparison of zeros
    # the language rows matter to it: other token embeddings, other actions
    act2, _, _ = LT.LangPolicyRef(g, leaves)(torch.as_tensor(theta), torch.as_tensor(tok), torch.as_tensor(lang[::-1].copy()))
    assert np.abs(act2.numpy()[..., :-1] - ract[..., :-1]).max() > 1e-6
    keep = LT.policy_keep(g.lang_tokens, g.patches).numpy()
    assert np.array_equal(keep, LR.policy_mask(g.lang_tokens, g.patches, True)[0, 0])


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_layout_of_the_language_geometries(tmp_path):
    """tests/native/train_lang_layout_check.cpp: the two new offsets, the pos_rows() extent, the policy members tile a row of theta, the
    refusal is lifted only when asked, -1 and nothing else moved without the option; and what it prints per geometry is Python's:
    train_param_layout's total (encoder trained), G and the three leaves' offsets of hypervla.config.generated_leaves."""
    from hypervla.config import Geometry
    from hypervla.train import train_param_layout
    exe = tmp_path / "train_lang_layout_check"
    build = subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
         "-I", CSRC, os.path.join(ROOT, "tests", "native", "train_lang_layout_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.strip().endswith("OK"), run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr
    printed = {ln.split()[1]: [int(x) for x in ln.split()[2:]] for ln in run.stdout.split("\n") if ln.startswith("## ")}
    want = {name: LT.geometry(name)[0] for name in LT.GEOMETRIES}
    want["README"] = dataclasses.replace(Geometry(), lang_in_policy=True)
    assert sorted(printed) == sorted(want)
    for name, g in want.items():
        lv = {l.flat_name: l for l in generated_leaves(g)}
        G = generated_leaves(g)[-1].offset + generated_leaves(g)[-1].size
        assert printed[name] == [train_param_layout(g, True)[1], G, lv["encoder_language_token_projection_kernel"].offset,
                                 lv["encoder_language_token_projection_bias"].offset, lv["encoder_pos_embedding"].offset], name
        assert lv["encoder_pos_embedding"].size == g.policy_seq * g.dim


def _trace(tmp_path):
    """tools/train_lang_extent_trace.hip built against csrc/train.hip with -DHVLA_TRAIN_TRACE, parsed into the points of
    tests/test_train_workspace_extents.py."""
    exe = os.path.join(str(tmp_path), "train_lang_extent_trace")
    build = subprocess.run(
        [X.HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O1", "-DHVLA_TRAIN_TRACE", "-I", CSRC,
         os.path.join(ROOT, "tools", "train_lang_extent_trace.hip"), X.TRAIN_HIP, "-o", exe],
        cwd=str(tmp_path), capture_output=True, text=True, timeout=900)
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
    return _trace(tmp_path_factory.mktemp("lang_extent_trace"))


def test_language_geometries_obey_the_extent_rules(points):
    """Every GPU case of tests/test_gpu_train_with_language_tokens.py, encoder frozen and trained, at its batch and at B = 1: (a) no
    GEMM's C extent meets its A or B extent, (b) every operand in `work` inside one plan buffer, in params / theta / dtheta / tok / tokens inside the
    vector, (c) copies and memsets likewise, (d) nothing beyond the workspace the step reports."""
    seen = {}
    for pt in points:
        w = dict(kv.split("=") for kv in pt["title"].split(" ")[1:])
        seen.setdefault(pt["title"].split(" ")[0], set()).add((int(w["B"]), int(w["enc"])))
    for name, (_, B) in LT.GEOMETRIES.items():
        assert seen.get(name) == {(B, 0), (B, 1), (1, 0), (1, 1)}, (name, seen.get(name))
    assert "README2-lang" in seen
    bad = X.violations(points)
    assert not bad, "%d violations\n%s" % (len(bad), "\n".join(bad[:10]))


def test_the_step_launches_the_language_rows(points):
    """The traced step of T12 (B = 4, encoder frozen) has what the option adds and sizes it by Sx = 12 + 64 + 1 = 77: the masked softmax
    of the language mode over Sx x Sx matrices with row stride 80, the language projection as a per-episode GEMM from `tok` with
    K = lang_dim into rows [0, 12) of x0, the patch projection at row offset 12, and dWl = tok^T dx0[:12] into dtheta."""
    pt = next(p for p in points if p["title"].startswith("T12 ") and " B=4 enc=0 " in p["title"])
    g, B = LT.geometry("T12")
    T, D, Sx, H = g.lang_tokens, g.dim, g.policy_seq, g.heads
    assert Sx == 77
    soft = [ln.split(" ") for ln in pt["lines"] if ln.startswith("softmax_lang_fwd_kernel ")]
    assert len(soft) == g.layers and all(w[4:] == [str(B * H), str(Sx), str(T), "80"] for w in soft), soft
    assert all(ln.split(" ")[7] == "1" for ln in pt["lines"] if ln.startswith("softmax_fwd_kernel "))        # only the context encoder's mode
    gemms = [dict(zip(X.BG_FIELDS, ln.split(" ", 4)[4][3:-1].split(" ")), ta=ln.split(" ")[1]) for ln in pt["lines"] if ln.startswith("bgemm ")]
    x0 = next(p for p in pt["plan"] if p[0] == "pb[0].x_in")
    assert x0[2] == B * Sx * D
    proj = [f for f in gemms if f["A"] == "tok+0" and f["C"] == f"work+{x0[1]}"]
    assert len(proj) == 1 and (proj[0]["M"], proj[0]["N"], proj[0]["K"], proj[0]["sC0"]) == (str(T), str(D), str(g.lang_dim), str(Sx * D))
    patch = [f for f in gemms if f["A"] == "tokens+0" and f["ta"] == "0"]
    assert len(patch) == 1 and patch[0]["C"] == f"work+{x0[1] + T * D}" and patch[0]["sC0"] == str(Sx * D)
    dwl = [f for f in gemms if f["A"] == "tok+0" and f["ta"] == "1" and f["C"].startswith("dtheta+")]
    assert len(dwl) == 1 and (dwl[0]["M"], dwl[0]["N"], dwl[0]["K"]) == (str(g.lang_dim), str(D), str(T))


def test_the_rules_see_a_policy_buffer_sized_without_the_language_rows(points):
    """Not vacuous: with the plan of T12 cut back to P + 1 rows in the policy's buffers (what make_plan took before it knew the option),
    rule (b) reports operands that leave their buffer."""
    pt = next(p for p in points if p["title"].startswith("T12 ") and " B=4 enc=0 " in p["title"])
    g, B = LT.geometry("T12")
    Sx, S = g.policy_seq, g.seq
    cut = dict(pt, plan=[(n, off, sz * S // Sx if n.startswith("pb[") or n in ("px_fin", "pdx") else sz) for n, off, sz in pt["plan"]])
    bad = X._Checker(cut).run()
    assert bad and all("(b)" in v or "(c)" in v for v in bad), bad[:3]


class _Model:
    """What FineTuner's constructor may look at before it refuses: the geometry.  Anything else is an AttributeError."""
    def __init__(self, g):
        self.geometry = g


def test_finetuner_refusals_need_no_device():
    from hypervla.train import FineTuner
    lang, plain = _Model(dataclasses.replace(MID, lang_in_policy=True)), _Model(MID)
    with pytest.raises(ValueError, match="use_language_token"):             # the keyword missing: as before
        FineTuner(lang, 4)
    with pytest.raises(ValueError, match="use_language_token"):
        FineTuner(lang, 4, language_tokens=False)
    with pytest.raises(ValueError, match="language_tokens=True needs a model with vit_kwargs.use_language_token"):
        FineTuner(plain, 4, language_tokens=True)
    for kw in (dict(attention_entropy=0.1), dict(attention_map_alignment=1.0, num_steps=10), dict(attention_entropy=0.1, attention_map_alignment=1.0, num_steps=10)):
        with pytest.raises(ValueError, match=r"not defined with language_tokens=True.*does not broadcast"):
            FineTuner(lang, 4, language_tokens=True, **kw)
    with pytest.raises(AttributeError):                                      # accepted: the constructor goes on to the model
        FineTuner(lang, 4, language_tokens=True)


def test_binding_and_header_have_the_setting():
    import ctypes
    import re
    from hypervla import _native
    src = open(os.path.join(ROOT, "include", "hvla.h")).read()
    assert re.search(r"\bint\s+hvla_train_language_tokens\s*\(\s*hvla_ctx\s*\*\s*ctx\s*,\s*int32_t\s+on\s*\)\s*;", src)
    assert "hvla_train_language_tokens" in _native.EXPORTS
    lib = _native.load_library()
    assert lib.hvla_train_language_tokens.restype is ctypes.c_int
    STATE = -7                                             # HVLA_E_STATE: a NULL context, whatever the value
    assert lib.hvla_train_language_tokens(None, 0) == STATE and lib.hvla_train_language_tokens(None, 1) == STATE
