"""CPU: the host side of importing policies -- theta <-> pytree both ways, their refusals, the host restatement of
the device's split (hi = bf16(x), lo = bf16(x - hi)) with the fixed point that `export(import(.))` rests on, and the three new
symbols as include/hvla.h declares them."""
import ctypes
import dataclasses
import os
import re
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hvla_weights_import", "hvla_weights_import_slots", "hvla_weights_copy_slots")


def _geo(name, lang):
    from hypervla import config
    return dataclasses.replace(getattr(config, name), lang_in_policy=lang)


GEOS = [("TINY", False), ("MID", False), ("FULL", False), ("MID", True), ("FULL", True)]


def _walk(tree, path=()):
    for k, v in tree.items():
        if isinstance(v, dict):
            yield from _walk(v, path + (k,))
        else:
            yield path + (k,), v


@pytest.mark.parametrize("name,lang", GEOS)
def test_theta_and_pytree_are_inverses(name, lang):
    from hypervla.config import generated_leaves, pytree_from_theta, theta_from_pytree, total_generated
    g = _geo(name, lang)
    G, B = total_generated(g), 3
    theta = np.random.default_rng(1).standard_normal((B, G)).astype(np.float32)
    tree = pytree_from_theta(g, theta)
    leaves = dict(_walk(tree))
    assert sorted(leaves) == sorted(lf.path for lf in generated_leaves(g))
    for lf in generated_leaves(g):
        assert leaves[lf.path].shape == (B,) + lf.shape
        assert np.array_equal(leaves[lf.path].reshape(B, -1), theta[:, lf.offset:lf.offset + lf.size])
    back = theta_from_pytree(g, tree)
    assert back.dtype == np.float32 and back.shape == (B, G) and np.array_equal(back.view(np.uint32), theta.view(np.uint32))
    again = pytree_from_theta(g, back)                               # and the other way round: tree -> theta -> the same tree
    for p, v in _walk(again):
        assert np.array_equal(v, leaves[p])


def test_single_episode_form():
    from hypervla.config import MID, pytree_from_theta, theta_from_pytree, total_generated
    theta = np.random.default_rng(2).standard_normal((1, total_generated(MID))).astype(np.float32)
    one = pytree_from_theta(MID, theta, squeeze=True)
    assert one["encoder"]["pos_embedding"].shape == (1, MID.policy_seq, MID.dim)
    assert one["action_head"]["continuous_head"]["bias"].shape == (MID.horizon * (MID.action_dim - 1),)
    assert np.array_equal(theta_from_pytree(MID, one), theta)


def test_image_encoder_subtree_is_ignored():
    from hypervla.config import MID, pytree_from_theta, theta_from_pytree, total_generated
    theta = np.random.default_rng(3).standard_normal((2, total_generated(MID))).astype(np.float32)
    tree = pytree_from_theta(MID, theta)
    tree["encoder"]["image_encoder"] = {"embeddings": {"cls_token": np.zeros((2, 1, 1, MID.enc_dim), np.float32)}}
    assert np.array_equal(theta_from_pytree(MID, tree), theta)


def test_refusals_name_the_leaf():
    from hypervla.config import MID, pytree_from_theta, theta_from_pytree, total_generated
    theta = np.zeros((2, total_generated(MID)), np.float32)
    path = "encoder/Transformer_0/encoderblock_1/MlpBlock_0/Dense_1/kernel"
    tree = pytree_from_theta(MID, theta)
    del tree["encoder"]["Transformer_0"]["encoderblock_1"]["MlpBlock_0"]["Dense_1"]["kernel"]
    with pytest.raises(KeyError, match=path):
        theta_from_pytree(MID, tree)
    tree = pytree_from_theta(MID, theta)
    tree["encoder"]["Transformer_0"]["encoderblock_1"]["MlpBlock_0"]["Dense_2"] = {"kernel": np.zeros((2, 4))}
    with pytest.raises(ValueError, match="unknown leaf encoder/Transformer_0/encoderblock_1/MlpBlock_0/Dense_2/kernel"):
        theta_from_pytree(MID, tree)
    tree = pytree_from_theta(MID, theta)
    tree["encoder"]["Transformer_0"]["encoderblock_1"]["MlpBlock_0"]["Dense_1"]["kernel"] = np.zeros((2, MID.dim, MID.mlp), np.float32)
    with pytest.raises(ValueError) as e:
        theta_from_pytree(MID, tree)
    msg = str(e.value)
    assert path in msg and str((2, MID.dim, MID.mlp)) in msg and str((2, MID.mlp, MID.dim)) in msg
    tree = pytree_from_theta(MID, theta)                             # one leaf of another batch
    tree["action_head"]["discrete_head"]["bias"] = np.zeros((3, MID.horizon), np.float32)
    with pytest.raises(ValueError, match="action_head/discrete_head/bias"):
        theta_from_pytree(MID, tree)
    with pytest.raises(ValueError, match="theta must be"):
        pytree_from_theta(MID, theta[:, :-1])


def _split(x):
    """The host restatement of split1 (csrc/common.h): torch's CPU conversion to bfloat16 rounds to nearest even, as the device's."""
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    return hi, lo


@pytest.mark.parametrize("scale", [1e-3, 0.02, 1.0, 37.0])
def test_split_sum_is_a_fixed_point_but_the_halves_are_not(scale):
    """x -> hi + lo is idempotent (what `export . import` being the identity on exports rests on), while the re-split of hi + lo takes
    another hi where lo is exactly half an ulp of hi: a share above 0 (the draws reach the tie) and below 0.5 %."""
    gen = torch.Generator().manual_seed(int(scale * 1000) + 5)
    x = torch.randn(1 << 24, generator=gen, dtype=torch.float32) * scale
    hi, lo = _split(x)
    s = hi.float() + lo.float()
    hi2, lo2 = _split(s)
    s2 = hi2.float() + lo2.float()
    assert torch.equal(s.view(torch.int32), s2.view(torch.int32))
    share = (hi2.view(torch.int16) != hi.view(torch.int16)).float().mean().item()
    print("scale %g: hi differs after the re-split on %.4f %% of %d values" % (scale, 100 * share, x.numel()))
    assert 0.0 < share < 0.005


def _prototypes():
    src = open(os.path.join(ROOT, "include", "hvla.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return {m.group(1): [a.strip() for a in m.group(2).split(",")]
            for m in re.finditer(r"\bint\s+(hvla_weights_(?:import|import_slots|copy_slots))\s*\(([^)]*)\)\s*;", src)}


def test_new_symbols_are_bound_with_the_header_s_argument_lists(tmp_path):
    from hypervla import _native
    protos = _prototypes()
    assert sorted(protos) == sorted(NEW)
    # the header's view, checked by the C compiler: each symbol assigned to a pointer of the issue's prototype
    prog = """#include "hvla.h"
int (*a)(hvla_ctx*, const float*, const float*, const float*, int32_t, hvla_weights**, void*) = hvla_weights_import;
int (*b)(hvla_ctx*, hvla_weights*, const int32_t*, int32_t, const float*, const float*, const float*, void*) = hvla_weights_import_slots;
int (*c)(hvla_ctx*, hvla_weights*, const int32_t*, const hvla_weights*, const int32_t*, int32_t, void*) = hvla_weights_copy_slots;
"""
    (tmp_path / "p.c").write_text(prog)
    subprocess.run(["gcc", "-Werror", "-Wall", "-I", os.path.join(ROOT, "include"), "-c", str(tmp_path / "p.c"), "-o",
                    str(tmp_path / "p.o")], check=True)
    lib = _native.load_library()
    for name, args in protos.items():
        want = []
        for a in args:
            if "*" in a:
                want.append("ptr")
            else:
                assert a.split()[0] == "int32_t", (name, a)
                want.append("i32")
        fn = getattr(lib, name)
        got = ["i32" if t is ctypes.c_int32 else "ptr" for t in fn.argtypes]
        assert all(t is ctypes.c_int32 or t is ctypes.c_void_p or issubclass(t, ctypes._Pointer) for t in fn.argtypes), name
        assert got == want, (name, got, want)
        assert fn.restype is ctypes.c_int and name in _native.EXPORTS
    # a null context is HVLA_E_STATE, with or without a GPU
    out = ctypes.c_void_p()
    assert lib.hvla_weights_import(None, None, None, None, 1, ctypes.byref(out), None) == -7 and not out.value
    assert lib.hvla_weights_import_slots(None, None, None, 1, None, None, None, None) == -7
    assert lib.hvla_weights_copy_slots(None, None, None, None, None, 1, None) == -7
