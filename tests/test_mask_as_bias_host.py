"""CPU: vit_kwargs.return_attention_map (Geometry.mask_as_bias) -- the float64 restatement
(tests/mask_bias_ref.py) against the oracle, a literal transcription of flax's call and the masked model; the config and checkpoint
layer; leaf names, order and offsets in Python and in C++; the v2 options struct of the C ABI; every launch of a flag-on fine-tune step
inside the workspace plan; and that the restatements tell the two models apart by a multiple of the serving tolerances.  No GPU."""
import ctypes
import dataclasses
import os
import shutil
import subprocess

import numpy as np
import pytest

import mask_bias_ref as MB
import test_train_workspace_extents as X
from hypervla import convert as cv
from hypervla import synthetic as syn
from hypervla.config import (FULL, MID, Geometry, default_config, generated_leaves, geometry_from_config, hypernet_param_shapes,
                             pytree_from_theta, theta_from_pytree, total_generated)

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hyper-vla_amd", "csrc")
FULL_B = dataclasses.replace(FULL, mask_as_bias=True)
MID_B = dataclasses.replace(MID, mask_as_bias=True)
NEW, OLD = "CustomMultiHeadDotProductAttention_0", "MultiHeadDotProductAttention_0"


def _case(g, B=3, seed=3):
    P = syn.synthetic_params(g)
    ins, st = syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g)
    bp = MB.create_tasks(P, g, ins, st)
    tok = np.random.default_rng(seed).standard_normal((B, g.patches, g.enc_dim))
    return P, ins, st, bp, tok


@pytest.fixture(scope="module")
def mid_case():
    return _case(MID_B)


# ---------------------------------------------------------------------------------------------- config and checkpoint layer
def test_config_round_trip():
    for g in (FULL, MID, FULL_B, MID_B):
        cfg = default_config(g)
        assert cfg["base_net_kwargs"]["vit_kwargs"]["return_attention_map"] is g.mask_as_bias
        assert geometry_from_config(cfg) == g


def test_a_return_attention_map_config_is_the_variant_and_its_checkpoint_loads():
    """What failed before the flag was read: the config gave the masked geometry, whose leaf names the checkpoint does not have."""
    cfg = default_config(MID)
    cfg["base_net_kwargs"]["vit_kwargs"]["return_attention_map"] = True
    g = geometry_from_config(cfg)
    assert g.mask_as_bias and g == MID_B
    P = syn.synthetic_params(g)
    assert set(P) == set(hypernet_param_shapes(g))
    assert any(NEW in k for k in P) and not any(k.startswith("output_head_") and "_" + OLD in k and NEW not in k for k in P)
    back = cv.params_from_tree(cv.tree_from_params(P), g)
    assert set(back) == set(P)
    for k in P:
        np.testing.assert_array_equal(back[k], P[k])
    with pytest.raises(KeyError, match=OLD):          # the same checkpoint read as the masked model: its head names are missing
        cv.params_from_tree(cv.tree_from_params(P), MID)
    # the context encoder's blocks keep flax's module (hypernetwork.py builds them without the flag)
    assert all(OLD in k for k in P if k.startswith("Transformer_0/encoderblock_") and "Attention" in k)


def test_the_flag_with_use_language_token_is_refused():
    with pytest.raises(ValueError, match="use_language_token"):
        dataclasses.replace(MID_B, lang_in_policy=True)
    cfg = default_config(dataclasses.replace(MID, lang_in_policy=True))
    cfg["base_net_kwargs"]["vit_kwargs"]["return_attention_map"] = True
    with pytest.raises(ValueError, match="return_attention_map together with use_language_token"):
        geometry_from_config(cfg)


@pytest.mark.parametrize("g,n,G", [(FULL_B, 73, 201_500), (MID_B, 41, 81_308)])
def test_leaf_names_order_offsets_and_totals(g, n, G):
    lv, lv0 = generated_leaves(g), generated_leaves(dataclasses.replace(g, mask_as_bias=False))
    assert len(lv) == len(lv0) == n and total_generated(g) == total_generated(dataclasses.replace(g, mask_as_bias=False)) == G
    for leaves in (lv, lv0):                          # jax pytree order: dict keys sorted at every level == the paths sorted as tuples
        assert [l.path for l in leaves] == sorted(l.path for l in leaves)
        off = 0
        for l in leaves:
            assert l.offset == off
            off += l.size
    # the same leaves under the other module name ...
    rename = lambda p: tuple(OLD if k == NEW else k for k in p)
    assert {(rename(l.path), l.shape) for l in lv} == {(l.path, l.shape) for l in lv0}
    assert sum(NEW in l.path for l in lv) == 8 * g.layers and not any(OLD in l.path for l in lv)
    # ... first in their block, in front of LayerNorm_0
    names = [l.flat_name for l in lv]
    i = names.index("encoder_Transformer_0_encoderblock_0_LayerNorm_0_bias")
    blk = f"encoder_Transformer_0_encoderblock_0_{NEW}_"
    assert names[i - 8:i] == [blk + s for s in ("key_bias", "key_kernel", "out_bias", "out_kernel", "query_bias", "query_kernel",
                                                "value_bias", "value_kernel")]
    assert names[i - 9] == "encoder_Transformer_0_encoder_norm_scale"
    assert lv[i - 8].head_name == "output_head_" + blk + "key_bias"
    # block l starts where it started; inside it the eight leaves moved from the back to the front
    per = sum(l.size for l in lv if "encoderblock_0" in l.path)
    at = {l.flat_name: l.offset for l in lv}
    at0 = {l.flat_name: l.offset for l in lv0}
    for l in range(g.layers):
        assert at[f"encoder_Transformer_0_encoderblock_{l}_{NEW}_key_bias"] == at0[f"encoder_Transformer_0_encoderblock_{l}_LayerNorm_0_bias"] \
            == at["encoder_Transformer_0_encoderblock_0_" + NEW + "_key_bias"] + l * per
    for k in ("action_head_continuous_head_bias", "encoder_image_embedding_projection_bias", "encoder_pos_embedding"):
        assert at[k] == at0[k]


def test_theta_and_pytree_round_trip_in_the_variant_s_order():
    g = MID_B
    G = total_generated(g)
    theta = np.random.default_rng(1).standard_normal((2, G)).astype(np.float32)
    tree = pytree_from_theta(g, theta)
    blk = tree["encoder"]["Transformer_0"]["encoderblock_1"]
    assert NEW in blk and OLD not in blk and list(sorted(blk)) == [NEW, "LayerNorm_0", "LayerNorm_1", "MlpBlock_0"]
    np.testing.assert_array_equal(theta_from_pytree(g, tree), theta)
    lf = next(l for l in generated_leaves(g) if l.path[-3:] == (NEW, "query", "kernel") and "encoderblock_1" in l.path)
    np.testing.assert_array_equal(blk[NEW]["query"]["kernel"], theta[:, lf.offset:lf.offset + lf.size].reshape((2,) + lf.shape))
    with pytest.raises(ValueError, match="unknown leaf"):            # the masked model's tree is another model's
        theta_from_pytree(g, pytree_from_theta(MID, theta))
    # the same values read in the masked model's order land elsewhere: the order matters
    assert not np.array_equal(theta_from_pytree(MID, {**pytree_from_theta(MID, theta)}), theta_from_pytree(
        MID, _renamed(tree)))


def _renamed(tree):
    return {(OLD if k == NEW else k): (_renamed(v) if isinstance(v, dict) else v) for k, v in tree.items()}


def test_train_vector_follows_the_leaf_names():
    """pack_params / unpack_params / weight_decay_mask / frozen_plan go through generated_leaves: a round trip keeps every tensor, the
    decay mask marks the same number of elements as in the masked model, and a frozen key under the variant's name is found.  A
    synthetic checkpoint of the variant holds the masked model's tensors, the attention heads under the variant's names."""
    from hypervla.train import frozen_plan, pack_params, train_param_layout, unpack_params, weight_decay_mask
    g = MID_B
    P, P0 = syn.synthetic_params(g), syn.synthetic_params(MID)
    assert set(P) != set(P0) and all(np.array_equal(v, P0[k.replace(NEW, OLD)]) for k, v in P.items())
    flat = pack_params(g, P)
    assert not np.array_equal(flat, pack_params(MID, P0))                   # the same tensors in another order
    assert flat.size == train_param_layout(g)[1] == train_param_layout(MID)[1]
    back = unpack_params(g, flat)
    hyper = {k for k in P if not k.startswith("encoder_image_encoder_")}
    assert set(back) == hyper
    for k in hyper:
        np.testing.assert_array_equal(back[k].reshape(P[k].shape), P[k])
    for strategy in ("v1", "v5"):
        assert int(np.asarray(weight_decay_mask(g, strategy)).sum()) == int(np.asarray(weight_decay_mask(MID, strategy)).sum()) > 0
    mask, _ = frozen_plan(g, (f"output_head_encoder_Transformer_0_encoderblock_0_{NEW}_query_kernel*",))
    C, D = g.ctx_dim, g.dim
    assert int(np.asarray(mask).sum()) == (C + 1) * D * D
    assert int(np.asarray(frozen_plan(g, (f"output_head_encoder_Transformer_0_encoderblock_0_{OLD}_query_kernel*",))[0]).sum()) == 0


# ---------------------------------------------------------------------------------------------- the float64 restatement
def _theta(bp, leaves, B, rename=None):
    name = (lambda n: n) if rename is None else rename
    return np.concatenate([np.asarray(bp[name(l.flat_name)], np.float64).reshape(B, -1) for l in leaves], 1)


def test_masked_in_place_of_the_bias_is_the_oracle(mid_case):
    """-inf where the mask is False instead of the added bias: oracle.hvla_ref_torch.PolicyRef (and the numpy oracle) on the same
    leaves under the masked model's names, to 1e-12."""
    from oracle import hvla_ref_np as onp
    from oracle import hvla_ref_torch as ot
    P, ins, st, bp, tok = mid_case
    g, B = MID_B, tok.shape[0]
    a, l, _ = MB.policy(bp, g, tok, "masked")
    lv0 = generated_leaves(MID)
    theta0 = _theta(bp, lv0, B, lambda n: n.replace(OLD, NEW))
    a_t, l_t, _ = ot.PolicyRef(MID, lv0)(torch.as_tensor(theta0), torch.as_tensor(tok))
    assert np.abs(a - a_t.numpy()).max() <= 1e-12 and np.abs(l - l_t.numpy()).max() <= 1e-12
    a_n, l_n, _ = onp.policy(MB.to_masked_names(bp, g), MID, tok)
    assert np.abs(a - a_n).max() <= 1e-12 and np.abs(l - l_n).max() <= 1e-12
    lv = generated_leaves(g)
    a_m, l_m, _ = MB.PolicyBiasRef(g, lv, "masked")(torch.as_tensor(_theta(bp, lv, B)), torch.as_tensor(tok))
    assert np.abs(a - a_m.numpy()).max() <= 1e-12 and np.abs(l - l_m.numpy()).max() <= 1e-12
    assert np.abs(a[..., :6]).max() > 1e-3


def test_the_literal_transcription_and_the_torch_form_are_the_restatement(mid_case):
    P, ins, st, bp, tok = mid_case
    g, B = MID_B, tok.shape[0]
    a, l, h = MB.policy(bp, g, tok, "bias")
    a2, l2, h2 = MB.policy(bp, g, tok, "literal")
    assert np.abs(a - a2).max() <= 1e-12 and np.abs(l - l2).max() <= 1e-12 and np.abs(h - h2).max() <= 1e-12
    lv = generated_leaves(g)
    a3, l3, attn = MB.PolicyBiasRef(g, lv)(torch.as_tensor(_theta(bp, lv, B)), torch.as_tensor(tok))
    assert np.abs(a - a3.numpy()).max() <= 1e-12 and np.abs(l - l3.numpy()).max() <= 1e-12
    assert np.abs(attn.numpy()[:, :, -1, :-1] - h[:, -1]).max() <= 1e-12
    assert h.shape == (B, g.layers, g.heads, g.patches)


def test_patch_rows_see_the_action_key_and_the_action_row_is_the_masked_model_s(mid_case):
    """With the layers below held equal (the masked run restarted from the additive run's block inputs): the action token's row of
    every layer is the masked model's row; a patch row puts mass on the action key, exp(-1) of what an equal score among the others
    would get, and its other weights keep their ratios."""
    P, ins, st, bp, tok = mid_case
    g = MID_B
    one = {k: np.asarray(v[0], np.float64) for k, v in bp.items()}
    _, _, maps, inputs = MB._policy_one(one, g, tok[0], "bias")
    _, _, maps_m, _ = MB._policy_one(one, g, tok[0], "masked", below=inputs)
    for w, wm in zip(maps, maps_m):
        assert np.abs(w[:, -1] - wm[:, -1]).max() <= 1e-12                  # [H, S]: the action row, every key
        assert (wm[:, :-1, -1] == 0).all() and (w[:, :-1, -1] > 0).all()
        rest = w[:, :-1, :-1] / w[:, :-1, :-1].sum(-1, keepdims=True)
        assert np.abs(rest - wm[:, :-1, :-1]).max() <= 1e-12
    top = max(float(w[:, :-1, -1].max()) for w in maps)
    print("largest weight of a patch query on the action key: %.3f" % top)
    assert top > 0.01
    # without the restart the layers above layer 0 differ: the models are different networks
    _, _, maps_free, _ = MB._policy_one(one, g, tok[0], "masked")
    assert np.abs(maps[-1][:, -1] - maps_free[-1][:, -1]).max() > 1e-6


@pytest.mark.parametrize("name", ["README", "MID"])
def test_the_restatements_tell_the_two_models_apart(name):
    """Masked against additive on the restatements alone, Gaussian tokens of default_rng(3), B = 4: actions and gripper logits differ
    by at least 5 serving tolerances (actions max 1e-3 and logits 1.5e-3 at the README geometry, tests/test_gpu_mask_as_bias.py; the
    MID end-to-end bound on the action maximum is 2e-3).  Measured: README actions 1.16e-2, logits 1.16e-2; MID 2.2e-2, 1.35e-2.
    No scaling of the action row of pos_embedding was needed (factor 1)."""
    g, tol_a = (FULL_B, 1e-3) if name == "README" else (MID_B, 2e-3)
    P, ins, st, bp, tok = _case(g, B=4, seed=3)
    a, l, _ = MB.policy(bp, g, tok, "bias")
    am, lm, _ = MB.policy(bp, g, tok, "masked")
    da, dl = np.abs(a[..., :6] - am[..., :6]).max(), np.abs(l - lm).max()
    print(f"{name}: masked against additive, actions max |d| {da:.3e}, gripper logits {dl:.3e}")
    assert da >= 5 * tol_a and dl >= 5 * 1.5e-3, (da, dl)


# ---------------------------------------------------------------------------------------------- C++ layout, C ABI
@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_cxx_layout_is_python_s(tmp_path):
    """generated_leaves / build_layout / make_train_layout of csrc with Geom::mask_as_bias: names, offsets and G are Python's, every
    policy leaf of the training layout is found, perm is a bijection onto [0, G), and PolicyLayout and the arena of a flag-off geometry
    do not depend on the field's existence (the offsets are equal with the flag on: only perm's values differ)."""
    src = tmp_path / "layout_bias_check.cpp"
    src.write_text(r'''
#include <cstdio>
#include <cstring>
#include "serving_layout.h"
using namespace hvla;
static int check(Geom g, const char* name) {
  Geom on = g; on.mask_as_bias = 1;
  const auto lv = generated_leaves(on);
  printf("## %s %zu %lld\n", name, lv.size(), (long long)(lv.back().offset + lv.back().size));
  for (const auto& l : lv) printf("leaf %s %s %lld %lld\n", name, l.flat.c_str(), (long long)l.offset, (long long)l.size);
  const PackedLayout a = build_layout(g), b = build_layout(on);
  if (memcmp(&a.pl, &b.pl, sizeof(PolicyLayout)) != 0) { printf("PolicyLayout moved\n"); return 1; }
  if (a.perm.size() != b.perm.size()) return 1;
  std::vector<char> seen(b.pl.G, 0);
  long moved = 0;
  for (size_t i = 0; i < b.perm.size(); ++i) {
    if ((a.perm[i] < 0) != (b.perm[i] < 0)) { printf("padding moved\n"); return 1; }
    if (b.perm[i] < 0) continue;
    if (b.perm[i] >= b.pl.G || seen[b.perm[i]]) { printf("perm is no bijection\n"); return 1; }
    seen[b.perm[i]] = 1;
    moved += a.perm[i] != b.perm[i];
  }
  for (char s : seen) if (!s) { printf("perm misses an element\n"); return 1; }
  if (!moved) { printf("perm did not follow the leaf order\n"); return 1; }
  const TrainLayout L = make_train_layout(on), L0 = make_train_layout(g);
  if (!L.policy_ok || train_refusal(on)) { printf("training layout\n"); return 1; }
  if (L.total != L0.total || L.G != L0.G || L.wp != L0.wp || L.pos != L0.pos) { printf("training totals\n"); return 1; }
  if (L.pol[0].wq == L0.pol[0].wq || L.pol[0].ln0_s == L0.pol[0].ln0_s) { printf("block leaves did not move\n"); return 1; }
  printf("pol %s %ld %ld %ld %ld\n", name, L.pol[0].bk, L.pol[0].wq, L.pol[0].ln0_b, L.pol[g.L - 1].w2);
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
    exe = tmp_path / "layout_bias_check"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                            "-I", CSRC, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.strip().endswith("OK"), run.stdout[-2000:] + run.stderr
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr
    for name, g in (("MID", MID_B), ("README", FULL_B)):
        lv = generated_leaves(g)
        head = next(ln.split() for ln in run.stdout.splitlines() if ln.startswith(f"## {name} "))
        assert [int(head[2]), int(head[3])] == [len(lv), total_generated(g)]
        got = [(w[2], int(w[3]), int(w[4])) for w in (ln.split() for ln in run.stdout.splitlines()) if w[:2] == ["leaf", name]]
        assert got == [(l.flat_name, l.offset, l.size) for l in lv]
        at = {l.flat_name: l.offset for l in lv}
        b0, bl = f"encoder_Transformer_0_encoderblock_0_", f"encoder_Transformer_0_encoderblock_{g.layers - 1}_"
        pol = next(ln.split() for ln in run.stdout.splitlines() if ln.startswith(f"pol {name} "))
        assert [int(x) for x in pol[2:]] == [at[b0 + NEW + "_key_bias"], at[b0 + NEW + "_query_kernel"], at[b0 + "LayerNorm_0_bias"],
                                             at[bl + "MlpBlock_0_Dense_1_kernel"]]


def test_options_v2_struct_is_the_header_s_and_the_first_struct_is_unchanged(tmp_path):
    """hvla_policy_options_v2 has the field behind use_language_token, header against binding; hvla_policy_options keeps its two
    fields and eight bytes (its size is ABI: the exact-size rule of hvla_create_with)."""
    from hypervla import _native
    names = [n for n, _ in _native.hvla_policy_options_v2._fields_]
    assert names == ["struct_size", "use_language_token", "attention_mask_as_bias"]
    prog = ("#include <stdio.h>\n#include <stddef.h>\n#include \"hvla.h\"\nint main(void) { printf(\"%zu %zu\", sizeof(hvla_policy_options), "
            "sizeof(hvla_policy_options_v2));\n"
            + "".join(f'printf(" %zu", offsetof(hvla_policy_options_v2, {n}));\n' for n in names) + "return 0; }\n")
    (tmp_path / "l.c").write_text(prog)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "l.c"), "-o", str(tmp_path / "l")], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "l")], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == ctypes.sizeof(_native.hvla_policy_options) == 8
    assert got[1] == ctypes.sizeof(_native.hvla_policy_options_v2) == 12
    assert got[2:] == [getattr(_native.hvla_policy_options_v2, n).offset for n in names] == [0, 4, 8]
    src = open(os.path.join(ROOT, "include", "hvla.h")).read()
    assert "multi_head_attetion.py:88-98" in src and "transformer.py:172-181" in src
    assert "hvla_create_with_v2" in _native.EXPORTS


def test_create_with_v2_refusals_need_no_device():
    """The exact-size rule at the v2 size (the 8 bytes of hvla_policy_options included), a value that is not 0 or 1, and the
    combination with use_language_token, which says why: all HVLA_E_SHAPE before a device is looked for, *out left NULL."""
    from hypervla import _native
    lib = _native.load_library()
    cfg = _native.hvla_config()
    cfg.struct_size = ctypes.sizeof(_native.hvla_config)
    size = ctypes.sizeof(_native.hvla_policy_options_v2)
    opt = _native.hvla_policy_options_v2()
    create = lambda h: lib.hvla_create_with_v2(ctypes.byref(cfg), ctypes.byref(opt), 0, ctypes.byref(h))
    for bad in (0, 8, size - 4, size + 4):
        opt.struct_size, opt.use_language_token, opt.attention_mask_as_bias = bad, 0, 1
        h = ctypes.c_void_p()
        assert create(h) == -1 and not h.value
    for lang, value in ((0, 2), (0, -1), (2, 0)):
        opt.struct_size, opt.use_language_token, opt.attention_mask_as_bias = size, lang, value
        h = ctypes.c_void_p()
        assert create(h) == -1 and not h.value
        assert lib.hvla_last_error(None) == b"null ctx"
    opt.struct_size, opt.use_language_token, opt.attention_mask_as_bias = size, 1, 1
    h = ctypes.c_void_p()
    assert create(h) == -1 and not h.value
    why = lib.hvla_last_error(None).decode()
    assert "attention_mask_as_bias" in why and "use_language_token" in why
    opt.attention_mask_as_bias = 2                                          # the next refusal has no text of its own: the old one is gone
    assert create(h) == -1
    assert lib.hvla_last_error(None) == b"null ctx"
    # hvla_create_with keeps its own rule: the v2 size is another struct's
    old = _native.hvla_policy_options(size, 1)
    assert lib.hvla_create_with(ctypes.byref(cfg), ctypes.byref(old), 0, ctypes.byref(h)) == -1 and not h.value


# ---------------------------------------------------------------------------------------------- the train step's launches
def _trace(tmp_path):
    exe = os.path.join(str(tmp_path), "train_bias_extent_trace")
    build = subprocess.run(
        [X.HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O1", "-DHVLA_TRAIN_TRACE", "-I", CSRC,
         os.path.join(ROOT, "tools", "train_bias_extent_trace.hip"), X.TRAIN_HIP, "-o", exe],
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
    return _trace(tmp_path_factory.mktemp("bias_extent_trace"))


def test_flag_on_steps_obey_the_extent_rules(points):
    """Every fine-tune case of tests/test_gpu_mask_as_bias.py, encoder frozen and trained, at its batch and at B = 1: the rules of
    tests/test_train_workspace_extents.py -- no GEMM's C extent meets its A or B extent, every operand inside one plan buffer or its
    vector, nothing beyond the workspace the step reports."""
    seen = {}
    for pt in points:
        w = dict(kv.split("=") for kv in pt["title"].split(" ")[1:])
        seen.setdefault(pt["title"].split(" ")[0], set()).add((int(w["B"]), int(w["enc"])))
    want = {"MID-bias": 4, "MID-bias-aux": 4, "MID-bias-B2": 2, "README2-bias": 2}
    for name, B in want.items():
        assert seen.get(name) == {(B, 0), (B, 1), (1, 0), (1, 1)}, (name, seen.get(name))
    bad = X.violations(points)
    assert not bad, "%d violations\n%s" % (len(bad), "\n".join(bad[:10]))


def test_the_step_launches_the_additive_softmax_for_the_policy_only(points):
    """MID, B = 4, encoder frozen: one softmax_bias_fwd_kernel per policy layer over B H matrices of S = 65 rows, row stride 68; the
    context encoder keeps softmax_fwd_kernel in its mode 1 and no launch uses the policy's masked mode 0; the backward is the one
    softmax_bwd_kernel per block of any model.  With the encoder trained DINOv2 keeps mode 2."""
    g = MID_B
    pt = next(p for p in points if p["title"].startswith("MID-bias ") and " B=4 enc=0 " in p["title"])
    S, H, B = g.seq, g.heads, 4
    soft = [ln.split(" ") for ln in pt["lines"] if ln.startswith("softmax_bias_fwd_kernel ")]
    assert len(soft) == g.layers and all(w[4:] == [str(B * H), str(S), "68"] for w in soft), soft
    modes = [ln.split(" ")[7] for ln in pt["lines"] if ln.startswith("softmax_fwd_kernel ")]
    assert modes == ["1"] * g.ctx_layers, modes
    assert sum(ln.startswith("softmax_bwd_kernel ") for ln in pt["lines"]) == g.layers + g.ctx_layers
    assert not any(ln.startswith("softmax_lang_fwd_kernel ") for ln in pt["lines"])
    enc = next(p for p in points if p["title"].startswith("MID-bias ") and " B=4 enc=1 " in p["title"])
    modes = sorted(ln.split(" ")[7] for ln in enc["lines"] if ln.startswith("softmax_fwd_kernel "))
    assert modes == ["1"] * g.ctx_layers + ["2"] * g.enc_layers, modes
    aux = next(p for p in points if p["title"].startswith("MID-bias-aux ") and " B=4 enc=0 " in p["title"])
    assert sum(ln.startswith("attention_aux_kernel ") for ln in aux["lines"]) >= 1
