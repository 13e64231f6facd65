"""CPU: hypernet_kwargs.share_layer_index=False (`Geometry.layer_tokens`) and share_TF_output_head (`Geometry.shared_block_heads`),
DESIGN.md §24 -- the token table, the config mapping, the checkpoint schema, the mask of the float64 restatement
(tests/layer_tokens_ref.py) and, under AddressSanitizer / UBSan, the C++ side: the token table of csrc/layout.h against
hypervla.config's, the segment list of csrc/pack.h and the acceptance rule of csrc/accept.h (tests/native/layer_tokens_check.cpp)."""
import dataclasses
import os
import shutil
import subprocess

import numpy as np
import pytest

import layer_tokens_ref as LR
from hypervla import config as cfgm
from hypervla.config import FULL, MID, Geometry, default_config, generated_leaves, geometry_from_config, hypernet_param_shapes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T0 = ("encoder", "Transformer_0")


def _lt(g, **kw):
    return dataclasses.replace(g, layer_tokens=True, **kw)


def _tokens_by_module(g):
    return {m: i for i, m in enumerate(cfgm.layer_token_modules(g))}


def test_token_table_of_mid():
    g = _lt(MID)
    assert g.num_layer_tokens == 7 and g.ctx_seq == 12 + 1 + 7 and MID.num_layer_tokens == 1 and MID.ctx_seq == 14
    t = _tokens_by_module(g)
    assert t[("encoder", "image_encoder")] == 0
    assert t[T0 + ("encoder_norm",)] == 1 and t[T0 + ("encoderblock_0",)] == 2 and t[T0 + ("encoderblock_1",)] == 3
    assert t[("encoder", "image_embedding_projection")] == 4 and t[("encoder", "pos_embedding")] == 5 and t[("action_head",)] == 6
    for lf in generated_leaves(g):
        want = 6 if lf.path[0] == "action_head" else t[lf.path[:3]] if lf.path[1] == "Transformer_0" else t[lf.path[:2]]
        assert cfgm.token_of(g, lf) == want and want != 0, lf.path


def test_token_table_with_language_tokens_and_many_layers():
    g = _lt(MID, lang_in_policy=True)
    t = _tokens_by_module(g)
    assert g.num_layer_tokens == 8
    assert (t[("encoder", "image_embedding_projection")], t[("encoder", "language_token_projection")], t[("encoder", "pos_embedding")],
            t[("action_head",)]) == (4, 5, 6, 7)
    assert _lt(FULL).num_layer_tokens == 9 and _lt(FULL, lang_in_policy=True).num_layer_tokens == 10
    # eleven layers: the blocks sort as strings, so encoderblock_10 is module 3 of Transformer_0 (encoder_norm, _0, _1, _10, _2, ...),
    # the token behind the image encoder's and those three: index 4
    g11 = _lt(FULL, layers=11)
    mods = cfgm.layer_token_modules(g11)
    inside = [m[2] for m in mods if m[:2] == T0]
    assert inside.index("encoderblock_10") == 3 and inside.index("encoderblock_2") == 4 and inside[0] == "encoder_norm"
    assert cfgm.token_of(g11, T0 + ("encoderblock_10", "LayerNorm_0", "bias")) == 1 + 3
    assert cfgm.token_of(g11, T0 + ("encoderblock_2", "LayerNorm_0", "bias")) == 1 + 4
    assert g11.num_layer_tokens == 16


@pytest.mark.parametrize("flag", ["differential", "mask_as_bias"])
def test_attention_variants_keep_a_block_s_leaves_on_its_token(flag):
    g = _lt(MID, **{flag: True})
    assert g.num_layer_tokens == 7
    per_block = {}
    for lf in generated_leaves(g):
        tok = cfgm.token_of(g, lf)
        assert tok != 0
        if len(lf.path) > 2 and lf.path[2].startswith("encoderblock_"):
            per_block.setdefault(lf.path[2], set()).add(tok)
    assert per_block == {"encoderblock_0": {2}, "encoderblock_1": {3}}
    assert any(g.attention_name in lf.path for lf in generated_leaves(g))


def test_config_round_trip_and_refusals():
    for g in (_lt(MID), _lt(FULL, shared_block_heads=True), _lt(MID, lang_in_policy=True), _lt(MID, differential=True), MID):
        cfg = default_config(g)
        assert cfg["hypernet_kwargs"]["share_layer_index"] == (not g.layer_tokens)
        assert cfg["hypernet_kwargs"]["share_TF_output_head"] == g.shared_block_heads
        assert cfg["geometry"]["layer_tokens"] == g.layer_tokens
        assert geometry_from_config(cfg) == g
    # a raw reference-shaped config has no geometry block: share_layer_index decides (its own default is False,
    # scripts/configs/hypervla_pretrain_config.py:353)
    raw = default_config(_lt(FULL))
    del raw["geometry"]
    assert geometry_from_config(raw).layer_tokens and geometry_from_config(raw).num_layer_tokens == 9
    raw["hypernet_kwargs"]["share_layer_index"] = True
    assert not geometry_from_config(raw).layer_tokens
    for flip in (MID, _lt(MID)):
        cfg = default_config(flip)
        cfg["hypernet_kwargs"]["share_layer_index"] = not cfg["hypernet_kwargs"]["share_layer_index"]
        with pytest.raises(ValueError, match="share_layer_index") as e:
            geometry_from_config(cfg)
        assert "geometry.layer_tokens" in str(e.value)
    with pytest.raises(ValueError, match="shared_block_heads"):
        Geometry(shared_block_heads=True)
    cfg = default_config(MID)
    cfg["hypernet_kwargs"]["share_TF_output_head"] = True
    with pytest.raises(ValueError, match="share_TF_output_head"):
        geometry_from_config(cfg)
    for key, bad in (("generation_strategy", "full"), ("use_initial_image", False), ("use_all_image_tokens", True),
                     ("attend_to_padding", True), ("task_attend_to_layer", True)):
        cfg = default_config(_lt(MID))
        cfg["hypernet_kwargs"][key] = bad
        with pytest.raises(ValueError, match=key):
            geometry_from_config(cfg)


def test_checkpoint_schema_follows_the_flags():
    from hypervla import convert as cv
    from hypervla.synthetic import synthetic_params
    heads = lambda s: sorted(k[:-7] for k in s if k.startswith("output_head_") and k.endswith("/kernel"))
    assert len(heads(hypernet_param_shapes(_lt(FULL)))) == 73
    sh = hypernet_param_shapes(_lt(FULL, shared_block_heads=True))
    assert len(heads(sh)) == 73 - (FULL.layers - 1) * 16
    assert hypernet_param_shapes(_lt(FULL))["layer_pos_embedding"] == (1, 9, 128) and hypernet_param_shapes(FULL)["layer_pos_embedding"] == (1, 1, 128)
    assert "output_head_encoder_Transformer_0_encoderblock_MlpBlock_0_Dense_0_kernel/kernel" in sh
    assert not any("encoderblock_0" in k for k in heads(sh))
    assert set(hypernet_param_shapes(_lt(FULL))) == set(hypernet_param_shapes(FULL))
    for g in (_lt(MID), _lt(MID, shared_block_heads=True), _lt(MID, shared_block_heads=True, mask_as_bias=True)):
        shapes = hypernet_param_shapes(g)
        P = synthetic_params(g)
        assert {k: v.shape for k, v in P.items()} == {k: tuple(v) for k, v in shapes.items()}
        back = cv.params_from_tree(cv.tree_from_params(P), g)
        assert set(back) == set(P) and all(np.array_equal(back[k], P[k]) for k in P)
        assert P["layer_pos_embedding"].shape == (1, 7, g.ctx_dim)


@pytest.mark.parametrize("seed", range(4))
def test_mask_of_the_restatement(seed):
    rng = np.random.default_rng(seed)
    g = _lt(MID, layers=int(rng.integers(1, 6)), lang_in_policy=bool(seed % 2))
    B, T, NL = 5, g.lang_tokens, g.num_layer_tokens
    am = rng.integers(0, 2, (B, T))
    am[0] = 0                                            # an instruction of padding alone still attends to the image token
    pad = rng.integers(0, 2, B).astype(bool)
    tm = LR.layer_token_mask(g)
    assert tm.shape == (NL,) and not tm[0] and tm[1:].all()
    m = LR.context_mask(am, pad, tm)[:, 0]
    S = T + 1 + NL
    assert m.shape == (B, S, S) and S == g.ctx_seq
    assert not m[:, :, T + 1].any()                      # token 0 is attended by nobody, itself included
    assert not m[:, :T + 1, T + 1:].any()                # layer columns are false on non-layer rows
    assert m[:, T + 1:, T + 2:].all()                    # ... and, but for token 0's, true on every layer row
    assert m.any(-1).all()                               # no row is fully masked
    assert m[:, :, T].all() and (m[:, :, :T] == (am.astype(bool) & pad[:, None])[:, None, :]).all()
    # random token masks: the rule is layer_token_mask's, whatever it holds
    tm2 = rng.integers(0, 2, NL).astype(bool)
    m2 = LR.context_mask(am, pad, tm2)[:, 0]
    assert (m2[:, T + 1:, T + 1:] == tm2[None, None, :]).all() and not m2[:, :T + 1, T + 1:].any() and m2.any(-1).all()


def test_restatement_routes_every_leaf_to_its_token():
    """With the kernels zero but row 0 = 1 and the biases zero, leaf p of the restatement is ctx[:, token_of(p), 0]."""
    from hypervla import synthetic as syn
    g = _lt(MID, shared_block_heads=True)
    P = dict(syn.synthetic_params(g))
    for k in P:
        if k.startswith("output_head_"):
            P[k] = np.zeros_like(P[k])
            if k.endswith("/kernel"):
                P[k][0] = 1.0
    bp, ctx, theta = LR.create_tasks(P, g, syn.synthetic_instructions(2, g), syn.synthetic_initial_state(2, g))
    assert ctx.shape == (2, 7, g.ctx_dim) and theta.shape == (2, cfgm.total_generated(g))
    for lf in generated_leaves(g):
        want = ctx[:, cfgm.token_of(g, lf), 0]
        assert np.array_equal(bp[lf.flat_name].reshape(2, -1), np.broadcast_to(want[:, None], (2, lf.size))), lf.path


def test_fine_tuner_names_the_flag():
    from hypervla.train import FineTuner

    class Model:
        geometry = _lt(MID)
    with pytest.raises(ValueError, match="share_layer_index=False is not built; serving is"):
        FineTuner(Model(), 2)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_segments_token_table_and_acceptance_under_asan_ubsan(tmp_path):
    exe = tmp_path / "layer_tokens_check"
    build = subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
         "-Werror", "-I", os.path.join(ROOT, "hyper-vla_amd", "csrc"), os.path.join(ROOT, "tests", "native", "layer_tokens_check.cpp"),
         "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.strip().endswith("OK"), run.stdout[-2000:] + run.stderr
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr
    table, segs = {}, {}
    for line in run.stdout.split("\n"):
        w = line.split()
        if w[:1] == ["TOKEN"]:
            table.setdefault(w[1], {})[w[2]] = int(w[3])
        elif w[:1] == ["SEGMENTS"]:
            segs[w[1]] = dict(zip(w[2::2], map(int, w[3::2])))
    # the C++ table is hypervla.config's, leaf for leaf
    for name, g in (("MID", _lt(MID)), ("MID_lang", _lt(MID, lang_in_policy=True)), ("MID_diff", _lt(MID, differential=True)),
                    ("L11", _lt(MID, layers=11))):
        assert table[name] == {lf.flat_name: cfgm.token_of(g, lf) for lf in generated_leaves(g)}, name
    assert sorted(segs) == sorted(["MID", "MID_shared", "README", "README_shared", "L7", "M768_S48", "MID_lang", "MID_diff", "README_diff_shared"])
    assert segs["README"]["NL"] == 9 and segs["M768_S48"]["NL"] == 9 and segs["L7"]["NL"] == 12 and segs["MID_lang"]["NL"] == 8
    # a differential block's vectors end on an odd multiple of 16 floats: those geometries have tiles of two tokens
    assert segs["MID_diff"]["multi"] >= 1 and segs["MID_diff"]["most"] == 2 and segs["README_diff_shared"]["multi"] >= 1
    assert all(v["segments"] <= v["tiles"] + v["multi"] * (v["most"] - 1) for v in segs.values())
