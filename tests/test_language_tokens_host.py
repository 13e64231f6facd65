"""CPU: vit_kwargs.use_language_token -- config and checkpoint layer, the float64 restatement
(tests/lang_policy_ref.py) and the C ABI's options struct.  No GPU."""
import ctypes
import dataclasses
import os
import subprocess

import numpy as np
import pytest

from hypervla import convert as cv
from hypervla import synthetic as syn
from hypervla.config import (FULL, MID, default_config, generated_leaves, geometry_from_config, hypernet_param_shapes,
                             total_generated)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_L = dataclasses.replace(FULL, lang_in_policy=True)
MID_L = dataclasses.replace(MID, lang_in_policy=True)


def test_config_round_trip():
    for g in (FULL, MID, FULL_L, MID_L):
        cfg = default_config(g)
        assert cfg["base_net_kwargs"]["vit_kwargs"]["use_language_token"] is g.lang_in_policy
        assert geometry_from_config(cfg) == g


def test_flag_off_keeps_every_leaf():
    assert not FULL.lang_in_policy and FULL.policy_seq == FULL.seq
    assert len(generated_leaves(FULL)) == 73 and total_generated(FULL) == 201_500


@pytest.mark.parametrize("g,n,G", [(FULL_L, 75, 252_764), (MID_L, 43, 86_236)])
def test_leaf_order_names_offsets_and_totals(g, n, G):
    lv = generated_leaves(g)
    assert len(lv) == n and total_generated(g) == G
    names = [l.flat_name for l in lv]
    i = names.index("encoder_language_token_projection_bias")
    assert names[i - 1] == "encoder_image_embedding_projection_kernel"           # jax pytree order: keys sorted
    assert names[i + 1] == "encoder_language_token_projection_kernel" and names[i + 2] == "encoder_pos_embedding"
    assert lv[i].shape == (g.dim,) and lv[i + 1].shape == (g.lang_dim, g.dim)
    assert lv[i + 2].shape == (1, g.lang_tokens + g.patches + 1, g.dim)
    off = 0
    for l in lv:
        assert l.offset == off
        off += l.size
    # everything before the new leaves is where the flag-off model has it
    base = {l.flat_name: l for l in generated_leaves(dataclasses.replace(g, lang_in_policy=False))}
    for l in lv[:i]:
        assert (l.offset, l.shape) == (base[l.flat_name].offset, base[l.flat_name].shape)
    assert lv[i].head_name == "output_head_encoder_language_token_projection_bias"


def test_hypernet_param_shapes_have_the_new_heads():
    s, s0 = hypernet_param_shapes(FULL_L), hypernet_param_shapes(FULL)
    C = FULL.ctx_dim
    assert s["output_head_encoder_language_token_projection_kernel/kernel"] == (C, 768 * 64)
    assert s["output_head_encoder_language_token_projection_kernel/bias"] == (768 * 64,)
    assert s["output_head_encoder_language_token_projection_bias/kernel"] == (C, 64)
    assert s["output_head_encoder_pos_embedding/bias"] == ((32 + 256 + 1) * 64,)
    assert set(s) - set(s0) == {"output_head_encoder_language_token_projection_" + a + "/" + b
                                for a in ("bias", "kernel") for b in ("bias", "kernel")}


def test_convert_round_trip_with_the_new_heads():
    P = syn.synthetic_params(MID_L)
    assert set(P) == set(hypernet_param_shapes(MID_L))
    back = cv.params_from_tree(cv.tree_from_params(P), MID_L)
    assert set(back) == set(P)
    for k in P:
        np.testing.assert_array_equal(back[k], P[k])
    with pytest.raises(ValueError):                   # the same checkpoint read as a flag-off model: extra tensors, refused
        cv.params_from_tree(cv.tree_from_params(P), MID)


@pytest.mark.parametrize("key,value", [("include_class_token", True), ("add_positional_embedding", False),
                                       ("use_differential_transformer", True)])
def test_unbuilt_vit_options_are_refused(key, value):
    cfg = default_config(FULL_L)
    cfg["base_net_kwargs"]["vit_kwargs"][key] = value
    with pytest.raises(ValueError, match=key):
        geometry_from_config(cfg)


def test_more_than_32_language_tokens_are_refused():
    cfg = default_config(FULL_L)
    cfg["geometry"]["lang_tokens"] = 33
    with pytest.raises(ValueError, match="32-key tile"):
        geometry_from_config(cfg)
    cfg["base_net_kwargs"]["vit_kwargs"]["use_language_token"] = False
    assert geometry_from_config(cfg).lang_tokens == 33                             # (without the flag: the context encoder's business)
    cfg = default_config(FULL_L)
    cfg["base_net_kwargs"]["action_token_num"] = 2
    with pytest.raises(ValueError, match="action_token_num"):
        geometry_from_config(cfg)


# ---------------------------------------------------------------------------------------------- the float64 restatement
def _mid_case(g, B=3, seed=0):
    import lang_policy_ref as LR
    P = syn.synthetic_params(g)
    ins, st = syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g)
    bp = LR.create_tasks(P, g, ins, st)
    rng = np.random.default_rng(seed)
    tok = rng.standard_normal((B, g.patches, g.enc_dim))
    return P, ins, st, bp, tok


def test_restatement_with_the_flag_off_is_the_oracle_bit_for_bit():
    import lang_policy_ref as LR
    from oracle import hvla_ref_np as R
    P, ins, st, bp, tok = _mid_case(MID)
    a, l, e = LR.policy(bp, MID, tok)
    a0, l0, e0 = R.policy(bp, MID, tok)
    assert np.array_equal(a, a0) and np.array_equal(l, l0) and np.array_equal(e, e0)


def test_language_kv_does_not_depend_on_the_image():
    import lang_policy_ref as LR
    P, ins, st, bp, tok = _mid_case(MID_L, B=1)
    lang = ins["language_instruction"]["token_embedding"]
    one = {k: v[0] for k, v in bp.items()}
    k0, v0 = LR.language_kv(one, MID_L, tok[0], lang[0])
    other = np.random.default_rng(5).standard_normal(tok[0].shape)
    k1, v1 = LR.language_kv(one, MID_L, other, lang[0])
    assert np.array_equal(k0, k1) and np.array_equal(v0, v1)
    a0, _, _ = LR.policy(bp, MID_L, tok, lang)
    a1, _, _ = LR.policy(bp, MID_L, other[None], lang)
    assert np.abs(a0 - a1).max() > 1e-3                                            # ... while the actions do


def test_padded_t5_positions_change_the_actions():
    """The base net does not mask padding (base_vit.py:159-166,207-212), unlike the hypernetwork (attend_to_padding=False):
    changing a padded position leaves the generated weights alone and changes the actions."""
    import lang_policy_ref as LR
    P, ins, st, _, tok = _mid_case(MID_L)
    li = dict(ins["language_instruction"])
    last = li["attention_mask"].shape[1] - 1
    li["attention_mask"] = li["attention_mask"].copy()
    li["attention_mask"][:, last] = 0                                             # the last position is padding in every episode
    bp = LR.create_tasks(P, MID_L, {"language_instruction": li}, st)
    emb2 = li["token_embedding"].copy()
    emb2[:, last] += 1.0
    bp2 = LR.create_tasks(P, MID_L, {"language_instruction": dict(li, token_embedding=emb2)}, st)
    for k in bp:
        np.testing.assert_array_equal(bp[k], bp2[k])
    a0, l0, _ = LR.policy(bp, MID_L, tok, li["token_embedding"])
    a1, l1, _ = LR.policy(bp, MID_L, tok, emb2)
    assert np.abs(a0[..., :6] - a1[..., :6]).max() > 1e-4 and np.abs(l0 - l1).max() > 1e-4


def test_head_attention_covers_the_language_and_patch_keys():
    import lang_policy_ref as LR
    P, ins, st, bp, tok = _mid_case(MID_L, B=2)
    h = LR.head_attention(bp, MID_L, tok, ins["language_instruction"]["token_embedding"])
    assert h.shape == (2, MID_L.layers, MID_L.heads, MID_L.lang_tokens + MID_L.patches)
    s = h.sum(-1)
    assert (s < 1.0).all() and (s > 0.5).all()                                    # the rest is the action token's own key


# ---------------------------------------------------------------------------------------------- C ABI
def test_policy_options_struct_layout_is_the_header_s(tmp_path):
    from hypervla import _native
    names = [n for n, _ in _native.hvla_policy_options._fields_]
    prog = ("#include <stdio.h>\n#include <stddef.h>\n#include \"hvla.h\"\nint main(void) { printf(\"%zu\", sizeof(hvla_policy_options));\n"
            + "".join(f'printf(" %zu", offsetof(hvla_policy_options, {n}));\n' for n in names) + "return 0; }\n")
    (tmp_path / "l.c").write_text(prog)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "l.c"), "-o", str(tmp_path / "l")], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "l")], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == ctypes.sizeof(_native.hvla_policy_options)
    assert got[1:] == [getattr(_native.hvla_policy_options, n).offset for n in names]
    assert names == ["struct_size", "use_language_token"]


def test_create_with_refuses_an_options_struct_of_another_size():
    """hvla_policy_options follows hvla_config's exact-size rule: HVLA_E_SHAPE before anything else is read, GPU or not."""
    from hypervla import _native
    lib = _native.load_library()
    cfg = _native.hvla_config()
    cfg.struct_size = ctypes.sizeof(_native.hvla_config)
    opt = _native.hvla_policy_options()
    for bad in (0, ctypes.sizeof(_native.hvla_policy_options) - 4, ctypes.sizeof(_native.hvla_policy_options) + 4):
        opt.struct_size, opt.use_language_token = bad, 1
        h = ctypes.c_void_p()
        assert lib.hvla_create_with(ctypes.byref(cfg), ctypes.byref(opt), 0, ctypes.byref(h)) == -1 and not h.value
    opt.struct_size, opt.use_language_token = ctypes.sizeof(_native.hvla_policy_options), 2
    h = ctypes.c_void_p()
    assert lib.hvla_create_with(ctypes.byref(cfg), ctypes.byref(opt), 0, ctypes.byref(h)) == -1 and not h.value
