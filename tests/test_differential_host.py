"""Host side of vit_kwargs.use_differential_transformer (Geometry.differential): leaves, config, checkpoint layer,
refusals, the C++ layout against Python's, the v3 options struct, and the float64 restatement (tests/diff_attention_ref.py) in its
two forms, against the model without the flag, and in float32.  No GPU."""
import ctypes
import dataclasses
import os
import shutil
import subprocess

import numpy as np
import pytest

import diff_attention_ref as DR
from hypervla import convert as cv
from hypervla import synthetic as syn
from hypervla.config import (FULL, MID, TINY, Geometry, default_config, encoder_leaves, generated_leaves, geometry_from_config,
                             hypernet_param_shapes, pytree_from_theta, theta_from_pytree, total_generated)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hyper-vla_amd", "csrc")
FULL_D = dataclasses.replace(FULL, differential=True)
MID_D = dataclasses.replace(MID, differential=True)
TINY_D = dataclasses.replace(TINY, differential=True)
NEW, OLD = "DifferentialAttention_0", "MultiHeadDotProductAttention_0"
ATTN = ("k_proj_kernel", "lambda_k1", "lambda_k2", "lambda_q1", "lambda_q2", "out_proj_kernel", "q_proj_kernel", "subln_weight",
        "v_proj_kernel")


# ---------------------------------------------------------------------------------------------- leaves
@pytest.mark.parametrize("g,n,G", [(FULL_D, 77, 200_668), (MID_D, 43, 81_308 - 2 * 208), (TINY_D, 43, None)])
def test_leaf_names_order_offsets_and_totals(g, n, G):
    lv, lv0 = generated_leaves(g), generated_leaves(dataclasses.replace(g, differential=False))
    D, H = g.dim, g.heads
    per_block = -4 * D + 4 * (D // (2 * H)) + D // H                  # four biases out, four lambda vectors and subln's weight in
    assert len(lv) == len(lv0) + g.layers == n
    assert total_generated(g) == total_generated(dataclasses.replace(g, differential=False)) + g.layers * per_block
    if G is not None:
        assert total_generated(g) == G
    assert [l.path for l in lv] == sorted(l.path for l in lv)         # jax pytree order: dict keys sorted at every level
    off = 0
    for l in lv:
        assert l.offset == off
        off += l.size
    names = [l.flat_name for l in lv]
    for b in range(g.layers):
        blk = f"encoder_Transformer_0_encoderblock_{b}_"
        i = names.index(blk + "LayerNorm_0_bias")
        assert names[i - 9:i] == [blk + NEW + "_" + s for s in ATTN]      # the nine leaves lead the block, sorted
        shapes = {l.flat_name[len(blk + NEW) + 1:]: l.shape for l in lv[i - 9:i]}
        assert shapes == {"k_proj_kernel": (D, D), "q_proj_kernel": (D, D), "v_proj_kernel": (D, D), "out_proj_kernel": (D, D),
                          "lambda_k1": (D // (2 * H),), "lambda_k2": (D // (2 * H),), "lambda_q1": (D // (2 * H),),
                          "lambda_q2": (D // (2 * H),), "subln_weight": (D // H,)}
    assert names[names.index("encoder_Transformer_0_encoderblock_0_LayerNorm_0_bias") - 10] == "encoder_Transformer_0_encoder_norm_scale"
    assert not any(OLD in l.path or "bias" == l.path[-1] and NEW in l.path for l in lv)
    assert lv[6].head_name == "output_head_encoder_Transformer_0_encoderblock_0_DifferentialAttention_0_k_proj_kernel"
    at, at0 = {l.flat_name: l.offset for l in lv}, {l.flat_name: l.offset for l in lv0}
    for k in ("action_head_continuous_head_bias", "encoder_Transformer_0_encoder_norm_scale"):
        assert at[k] == at0[k]
    assert at["encoder_pos_embedding"] == at0["encoder_pos_embedding"] + g.layers * per_block


# ---------------------------------------------------------------------------------------------- config and checkpoint layer
def test_config_round_trip_and_the_both_flags_mapping():
    for g in (FULL, MID, FULL_D, MID_D):
        cfg = default_config(g)
        assert cfg["base_net_kwargs"]["vit_kwargs"]["use_differential_transformer"] is g.differential
        assert geometry_from_config(cfg) == g
    cfg = default_config(MID)
    cfg["base_net_kwargs"]["vit_kwargs"]["use_differential_transformer"] = True
    assert geometry_from_config(cfg) == MID_D                        # what was refused before the flag was read
    cfg["base_net_kwargs"]["vit_kwargs"]["return_attention_map"] = True
    g = geometry_from_config(cfg)                                    # transformer.py:166-172: the first `if` wins
    assert g == MID_D and g.differential and not g.mask_as_bias
    assert g.attention_name == NEW


def test_refused_geometries():
    with pytest.raises(ValueError, match="use_differential_transformer"):
        dataclasses.replace(MID_D, lang_in_policy=True)
    with pytest.raises(ValueError, match="mask_as_bias"):
        Geometry(differential=True, mask_as_bias=True)
    cfg = default_config(dataclasses.replace(MID, lang_in_policy=True))
    cfg["base_net_kwargs"]["vit_kwargs"]["use_differential_transformer"] = True
    with pytest.raises(ValueError, match="use_differential_transformer together with use_language_token"):
        geometry_from_config(cfg)


class _Model:                                                         # what the constructors' checks read
    def __init__(self, g):
        self.geometry, self.config = g, default_config(g)


def test_attention_maps_and_fine_tuning_are_refused_by_name():
    from hypervla.interface import InferenceWrapper
    from hypervla.model import HyperVLA
    from hypervla.train import FineTuner
    with pytest.raises(ValueError, match="use_differential_transformer"):
        InferenceWrapper(_Model(MID_D), save_attention_map=True)
    with pytest.raises(ValueError, match=r"use_differential_transformer is not built; serving is"):
        FineTuner(_Model(MID_D), 2)
    m = HyperVLA.__new__(HyperVLA)                                   # sample_actions refuses before it looks at anything else
    m.geometry, m.config = MID_D, default_config(MID_D)
    with pytest.raises(ValueError, match="use_differential_transformer"):
        m.sample_actions(np.zeros((1, 112, 112, 3), np.uint8), attention_maps=True)


def test_theta_and_pytree_round_trip_in_the_variant_s_order():
    g = MID_D
    G = total_generated(g)
    theta = np.random.default_rng(1).standard_normal((2, G)).astype(np.float32)
    tree = pytree_from_theta(g, theta)
    blk = tree["encoder"]["Transformer_0"]["encoderblock_1"]
    assert sorted(blk) == [NEW, "LayerNorm_0", "LayerNorm_1", "MlpBlock_0"]
    assert sorted(blk[NEW]) == ["k_proj", "lambda_k1", "lambda_k2", "lambda_q1", "lambda_q2", "out_proj", "q_proj", "subln", "v_proj"]
    assert blk[NEW]["lambda_q1"].shape == (2, 8) and blk[NEW]["subln"]["weight"].shape == (2, 16) and list(blk[NEW]["q_proj"]) == ["kernel"]
    np.testing.assert_array_equal(theta_from_pytree(g, tree), theta)
    lf = next(l for l in generated_leaves(g) if l.path[-2:] == (NEW, "lambda_q2") and "encoderblock_1" in l.path)
    np.testing.assert_array_equal(blk[NEW]["lambda_q2"], theta[:, lf.offset:lf.offset + lf.size])
    with pytest.raises(ValueError, match="unknown leaf"):            # the plain model's tree is another model's
        theta_from_pytree(g, pytree_from_theta(MID, np.zeros((2, total_generated(MID)), np.float32)))
    with pytest.raises((KeyError, ValueError)):
        theta_from_pytree(MID, tree)


def test_synthetic_checkpoint_and_converter_round_trip():
    P = syn.synthetic_params(MID_D)
    assert set(P) == set(hypernet_param_shapes(MID_D))
    pre = "output_head_encoder_Transformer_0_encoderblock_1_DifferentialAttention_0_"
    assert abs(float(P[pre + "subln_weight/bias"].mean()) - 1.0) < 0.1 and float(P[pre + "lambda_q1/bias"].std()) < 0.3
    assert not any(k.startswith("output_head_") and OLD in k for k in P)
    assert all(OLD in k for k in P if k.startswith("Transformer_0/encoderblock_") and "Attention" in k)   # the context encoder keeps flax's
    back = cv.params_from_tree(cv.tree_from_params(P), MID_D)
    assert set(back) == set(P)
    for k in P:
        np.testing.assert_array_equal(back[k], P[k])
    with pytest.raises((KeyError, ValueError)):                      # the same checkpoint read as a flag-off model
        cv.params_from_tree(cv.tree_from_params(P), MID)
    # a flag-off checkpoint is what it was: drawn leaf by leaf in the same order from the same stream
    P0 = syn.synthetic_params(MID)
    assert set(P0) == set(hypernet_param_shapes(MID)) and not any(NEW in k for k in P0)


# ---------------------------------------------------------------------------------------------- C++ layout, C ABI
@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_cxx_layout_is_python_s(tmp_path):
    """generated_leaves / build_layout of csrc with Geom::differential: names, offsets and G are Python's; every non-padding perm
    entry is hit exactly once; the lambda vectors and subln's weight sit behind fc2's bias in every layer's vector block; the q / k /
    v / out bias slots are padding; the matrix region and a flag-off geometry's layout are unchanged; the LDS description grows by the
    second partial table; the two-argument forms of accept.h keep their meaning; the training path refuses by name."""
    src = tmp_path / "layout_diff_check.cpp"
    src.write_text(r'''
#include <cstdio>
#include <cstring>
#include "serving_layout.h"
#include "accept.h"
#include "train_layout.h"
using namespace hvla;
static int check(Geom g, const char* name) {
  Geom on = g; on.differential = 1;
  const auto lv = generated_leaves(on);
  printf("## %s %zu %lld\n", name, lv.size(), (long long)(lv.back().offset + lv.back().size));
  for (const auto& l : lv) printf("leaf %s %s %lld %lld\n", name, l.flat.c_str(), (long long)l.offset, (long long)l.size);
  const PackedLayout a = build_layout(g), b = build_layout(on);
  const int D = g.D, hd = g.hd(), extra = 4 * (hd / 2) + hd;
  if (b.pl.Gm != a.pl.Gm || b.pl.m_layer_stride != a.pl.m_layer_stride || b.pl.m_head != a.pl.m_head) { printf("matrix region moved\n"); return 1; }
  if (b.pl.v_layer_stride != a.pl.v_layer_stride + extra || b.pl.v_layer0 != a.pl.v_layer0 || b.pl.v_fc2_b != a.pl.v_fc2_b) { printf("vector block\n"); return 1; }
  if (b.pl.Gv % 32 || b.pl.Gv < a.pl.Gv + g.L * extra - 31 || b.pl.Gv > a.pl.Gv + g.L * extra) { printf("Gv\n"); return 1; }
  if ((size_t)b.pl.Gm + b.pl.Gv != b.perm.size()) return 1;
  std::vector<int> seen(b.pl.G, 0);
  for (size_t i = 0; i < b.perm.size(); ++i) {
    if (b.perm[i] < 0) continue;
    if (b.perm[i] >= b.pl.G) { printf("perm out of range\n"); return 1; }
    ++seen[b.perm[i]];
  }
  for (int s : seen) if (s != 1) { printf("perm is no bijection\n"); return 1; }
  for (int i = 0; i < a.pl.Gm; ++i) if ((a.perm[i] < 0) != (b.perm[i] < 0)) { printf("matrix padding moved\n"); return 1; }
  auto at = [&](const std::string& n) { for (const auto& l : lv) if (l.flat == n) return l.offset; return (int64_t)-1; };
  for (int l = 0; l < g.L; ++l) {
    const int vb = b.pl.Gm + b.pl.v_layer0 + l * b.pl.v_layer_stride;
    const std::string A = "encoder_Transformer_0_encoderblock_" + std::to_string(l) + "_DifferentialAttention_0_";
    for (int i = 0; i < 3 * D; ++i) if (b.perm[vb + b.pl.v_qkv_b + i] != -1) { printf("qkv bias slot\n"); return 1; }
    for (int i = 0; i < D; ++i) if (b.perm[vb + b.pl.v_out_b + i] != -1) { printf("out bias slot\n"); return 1; }
    const char* lam[4] = {"lambda_q1", "lambda_k1", "lambda_q2", "lambda_k2"};
    for (int k = 0; k < 4; ++k)
      for (int d = 0; d < hd / 2; ++d)
        if (b.perm[vb + diff_v_lambda(b.pl, D) + k * (hd / 2) + d] != at(A + lam[k]) + d) { printf("lambda slot\n"); return 1; }
    for (int d = 0; d < hd; ++d) if (b.perm[vb + diff_v_subln(b.pl, D, hd) + d] != at(A + "subln_weight") + d) { printf("subln slot\n"); return 1; }
    if (diff_v_subln(b.pl, D, hd) + hd != b.pl.v_layer_stride) { printf("stride\n"); return 1; }
  }
  // q_proj [D, D]: fragment 0 of the layer's qkv tiles, lane 0, j = 0 is W[k = kphi(0, 0, 0) = 0][n = 0]; lane 1 is n = 1
  if (b.perm[b.pl.m_layer0 + b.pl.m_qkv] != at("encoder_Transformer_0_encoderblock_0_DifferentialAttention_0_q_proj_kernel") ||
      b.perm[b.pl.m_layer0 + b.pl.m_qkv + 8] != at("encoder_Transformer_0_encoderblock_0_DifferentialAttention_0_q_proj_kernel") + 1) { printf("q_proj\n"); return 1; }
  const char* why = train_refusal(on);
  if (!why || !strstr(why, "use_differential_transformer") || train_refusal(g)) { printf("train refusal\n"); return 1; }
  return 0;
}
int main() {
  Geom mid{112, 14, 128, 2, 2, 512, 64, 2, 4, 128, 4, 7, 5.f, 5.f, 128, 2, 4, 256, 12, 64, 1};
  Geom full{224, 14, 768, 12, 12, 3072, 64, 4, 4, 128, 4, 7, 5.f, 5.f, 128, 6, 4, 512, 32, 768, 1};
  if (check(mid, "MID") || check(full, "README")) return 1;
  // accept.h: the LDS description and the predicate
  static_assert(policy_lds(8, false).vlds == policy_lds(8, false, false).vlds, "two-argument form");
  static_assert(policy_lds(8, false, true).vlds >= policy_lds(8, false).vlds, "the second partial table");
  static_assert(policy_lds(8, false, true).act_floats == policy_lds(8, false).act_floats + 2 * 9 * 20, "the second partial table");
  if (policy_lds_bytes(8, false, 3000) != policy_lds_bytes(8, false, 3000, false)) return 1;
  hvla_config c{};
  c.struct_size = sizeof c; c.image_size = 224; c.patch = 14; c.enc_dim = 768; c.enc_layers = 12; c.enc_heads = 12; c.enc_mlp = 3072;
  c.dim = 64; c.layers = 4; c.heads = 4; c.mlp = 128; c.horizon = 4; c.action_dim = 7; c.tanh_scale = 5.f; c.max_action = 5.f;
  c.ctx_dim = 128; c.ctx_layers = 6; c.ctx_heads = 4; c.ctx_mlp = 512; c.lang_tokens = 32; c.lang_dim = 768; c.scale_context = 1;
  c.max_batch = 4; c.enc_dtype = HVLA_ENC_F16; c.streams = 1; c.clip_target = 1;
  if (accept_geometry(c, 0) != HVLA_OK || accept_geometry(c, 0, 0) != HVLA_OK || accept_geometry(c, 0, 1) != HVLA_OK) { printf("accept\n"); return 1; }
  if (accept_geometry(c, 1, 1) != HVLA_E_SHAPE || accept_geometry(c, 0, 2) != HVLA_E_SHAPE) { printf("accept combos\n"); return 1; }
  // the largest layer count the plain geometry fits; the differential one refuses at or before it
  int lp = 0, ld = 0;
  for (int l = 1; l < 64; ++l) { c.layers = l; if (accept_geometry(c, 0) == HVLA_OK) lp = l; if (accept_geometry(c, 0, 1) == HVLA_OK) ld = l; }
  printf("layers %d %d\n", lp, ld);
  if (ld < 4 || ld > lp) return 1;
  c.layers = ld + 1;
  if (policy_lds_bytes_of(c, 0, 1) <= LDS_LIMIT || accept_geometry(c, 0, 1) != HVLA_E_SHAPE) { printf("refusal by LDS\n"); return 1; }
  printf("OK\n");
  return 0;
}
''')
    exe = tmp_path / "layout_diff_check"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                            "-I", CSRC, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.strip().endswith("OK"), run.stdout[-2000:] + run.stderr
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr
    for name, g in (("MID", MID_D), ("README", FULL_D)):
        lv = generated_leaves(g)
        head = next(ln.split() for ln in run.stdout.splitlines() if ln.startswith(f"## {name} "))
        assert [int(head[2]), int(head[3])] == [len(lv), total_generated(g)]
        got = [(w[2], int(w[3]), int(w[4])) for w in (ln.split() for ln in run.stdout.splitlines()) if w[:2] == ["leaf", name]]
        assert got == [(l.flat_name, l.offset, l.size) for l in lv]


def test_options_v3_struct_is_the_header_s_and_the_older_structs_are_unchanged(tmp_path):
    from hypervla import _native
    names = [n for n, _ in _native.hvla_policy_options_v3._fields_]
    assert names == ["struct_size", "use_language_token", "attention_mask_as_bias", "differential_attention"]
    prog = ("#include <stdio.h>\n#include <stddef.h>\n#include \"hvla.h\"\nint main(void) { printf(\"%zu %zu %zu\", sizeof(hvla_policy_options), "
            "sizeof(hvla_policy_options_v2), sizeof(hvla_policy_options_v3));\n"
            + "".join(f'printf(" %zu", offsetof(hvla_policy_options_v3, {n}));\n' for n in names) + "return 0; }\n")
    (tmp_path / "l.c").write_text(prog)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "l.c"), "-o", str(tmp_path / "l")], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "l")], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == ctypes.sizeof(_native.hvla_policy_options) == 8
    assert got[1] == ctypes.sizeof(_native.hvla_policy_options_v2) == 12
    assert got[2] == ctypes.sizeof(_native.hvla_policy_options_v3) == 16
    assert got[3:] == [getattr(_native.hvla_policy_options_v3, n).offset for n in names] == [0, 4, 8, 12]
    src = open(os.path.join(ROOT, "include", "hvla.h")).read()
    assert "differential_transformer.py:99-252" in src and "transformer.py:166-171" in src
    assert "hvla_create_with_v3" in _native.EXPORTS


def test_create_with_v3_refusals_need_no_device():
    """The exact-size rule at the v3 size, values that are not 0 or 1, and the two combinations, which say why: all HVLA_E_SHAPE
    before a device is looked for, *out left NULL; the older entries keep their own sizes."""
    from hypervla import _native
    lib = _native.load_library()
    cfg = _native.hvla_config()
    cfg.struct_size = ctypes.sizeof(_native.hvla_config)
    size = ctypes.sizeof(_native.hvla_policy_options_v3)
    opt = _native.hvla_policy_options_v3()
    create = lambda h: lib.hvla_create_with_v3(ctypes.byref(cfg), ctypes.byref(opt), 0, ctypes.byref(h))

    def put(sz, lang, mab, diff):
        opt.struct_size, opt.use_language_token, opt.attention_mask_as_bias, opt.differential_attention = sz, lang, mab, diff

    for bad in (0, 8, 12, size + 4):
        put(bad, 0, 0, 1)
        h = ctypes.c_void_p()
        assert create(h) == -1 and not h.value
    for vals in ((0, 0, 2), (0, 0, -1), (2, 0, 1), (0, 2, 1)):
        put(size, *vals)
        h = ctypes.c_void_p()
        assert create(h) == -1 and not h.value
        assert lib.hvla_last_error(None) == b"null ctx"
    for vals, words in (((1, 0, 1), ("differential_attention", "use_language_token")),
                        ((0, 1, 1), ("differential_attention", "attention_mask_as_bias")),
                        ((1, 1, 0), ("attention_mask_as_bias", "use_language_token"))):
        put(size, *vals)
        h = ctypes.c_void_p()
        assert create(h) == -1 and not h.value
        why = lib.hvla_last_error(None).decode()
        assert all(w in why for w in words), why
    put(size, 0, 0, 2)                                                # the next refusal has no text of its own: the old one is gone
    h = ctypes.c_void_p()
    assert create(h) == -1 and lib.hvla_last_error(None) == b"null ctx"
    old2 = _native.hvla_policy_options_v2(size, 0, 0)                 # the v3 size is another struct's
    assert lib.hvla_create_with_v2(ctypes.byref(cfg), ctypes.byref(old2), 0, ctypes.byref(h)) == -1 and not h.value
    old1 = _native.hvla_policy_options(size, 0)
    assert lib.hvla_create_with(ctypes.byref(cfg), ctypes.byref(old1), 0, ctypes.byref(h)) == -1 and not h.value


# ---------------------------------------------------------------------------------------------- the restatement
def _full_case(params_of=lambda p: p):
    """The inputs of tests/test_gpu_differential.py's README-geometry cases."""
    g, B = FULL_D, 4
    P = params_of(syn.synthetic_params(g))
    ins, st = syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g)
    tok = np.random.default_rng(3).standard_normal((B, g.patches, g.enc_dim)).astype(np.float32).astype(np.float64)
    return g, DR.create_tasks(P, g, ins, st), tok


def _mid_case():
    """... and of its MID end-to-end case: the tokens are the float64 DINOv2's."""
    from oracle import hvla_ref_np as onp
    g, B = MID_D, 4
    P = syn.synthetic_params(g)
    ins, st, im = syn.synthetic_instructions(8, g), syn.synthetic_initial_state(8, g), syn.synthetic_images(8, g)[:B]
    ins = {"language_instruction": {k: np.asarray(v)[:B] for k, v in ins["language_instruction"].items()}}
    st = {"patch_embeddings": st["patch_embeddings"][:B]}
    tok = onp.dinov2(P, g, dict(encoder_leaves(g)), onp.normalize_images(im[:, 0] if im.ndim == 5 else im))[:, 1:]
    return g, DR.create_tasks(P, g, ins, st), tok


def _scaled(p):
    return DR.lambda_scaled(p)


@pytest.fixture(scope="module", params=["full", "full_lambda_x5", "mid"])
def case(request):
    g, bp, tok = {"full": _full_case, "full_lambda_x5": lambda: _full_case(_scaled), "mid": _mid_case}[request.param]()
    return request.param, g, bp, tok, DR.policy(bp, g, tok, "restated")


def test_the_literal_transcription_is_the_restatement(case):
    _, g, bp, tok, (act, logit) = case
    a, l = DR.policy(bp, g, tok, "literal")
    assert np.abs(a - act).max() <= 1e-12 and np.abs(l - logit).max() <= 1e-12


def test_the_restatements_tell_the_models_apart(case):
    """Differential against the model without the flag on the same tensors: more than 5 serving tolerances in the actions."""
    name, g, bp, tok, (act, logit) = case
    a, l = DR.policy(bp, g, tok, "plain")
    tol = 2e-3 if name == "mid" else 1e-3
    print(name, "actions differ by %.3e, logits by %.3e" % (np.abs(a[..., :6] - act[..., :6]).max(), np.abs(l - logit).max()))
    assert np.abs(a[..., :6] - act[..., :6]).max() > 5 * tol


def test_float32_stays_within_a_quarter_of_the_serving_bounds(case):
    """Conditioning: the RMSNorm divides by the norm of (A1 - lambda A2) V.  The same restatement in numpy float32, on the GPU tests'
    inputs, against float64.  Measured (action max / mean, logit max / mean):
        README geometry, given tokens      7.3e-06 / 2.0e-06, 6.8e-06 / 2.5e-06     (bounds 1e-3 max, 1.5e-3 max)
        ... lambda heads x 5               of the same order (printed)
        MID, DINOv2 tokens                 3.1e-06 / 8.2e-07, 3.0e-06 / 9.2e-07     (bounds 5e-4 mean, 2e-3 max, 2e-3 mean)"""
    name, g, bp, tok, (act, logit) = case
    a, l = DR.policy(bp, g, tok, "restated", np.float32)
    d, dl = np.abs(a[..., :6] - act[..., :6]), np.abs(l - logit)
    print(name, "float32: action max %.3e mean %.3e, logit max %.3e mean %.3e" % (d.max(), d.mean(), dl.max(), dl.mean()))
    if name == "mid":
        assert d.mean() <= 5e-4 / 4 and d.max() <= 2e-3 / 4 and dl.mean() <= 2e-3 / 4
    else:
        assert d.max() <= 1e-3 / 4 and dl.max() <= 1.5e-3 / 4


def test_lambda_spreads_over_the_episodes_of_the_scaled_checkpoint():
    g, bp, _ = _full_case(_scaled)
    lam = DR.lambdas(bp, g)
    assert lam.shape == (4, 4) and (lam.max(0) - lam.min(0)).max() > 0.05
    g0, bp0, _ = _full_case()
    np.testing.assert_allclose(DR.lambdas(bp0, g0).mean(0), [DR.lambda_init_fn(l) for l in range(4)], atol=0.2)
