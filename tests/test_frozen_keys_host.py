"""CPU: `frozen_keys` on the host -- hypervla.train.frozen_plan against masks built here from the layout and fnmatch alone, its
bucket flags, counts and refusals, and the ctypes binding of hvla_train_frozen against the header's declaration."""
import ctypes
import os
import re
from fnmatch import fnmatch

import numpy as np
import pytest

from hypervla.config import FULL, MID, generated_leaves
from hypervla.train import POSITION_LEAF, POSITION_SOURCE, frozen_plan, gradient_buckets, train_param_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTEXT = ("Transformer_0.*", "task_*", "initial_image_*", "layer_pos_embedding")
HEADS = ("output_head_*",)
SOURCE_N = 5


def _expected(g, keys, train_encoder=False, position_source=0):
    """The mask element by element from the dotted names: the reference's `".".join(path)` of every leaf, the heads' leaves found
    through their columns of W_cat / b_cat."""
    layout, total = train_param_layout(g, train_encoder, position_source)
    hit = lambda dotted: any(fnmatch(dotted, k) for k in keys)
    want = np.zeros(total, np.uint8)
    for name, off, shape in layout:
        n = int(np.prod(shape))
        if name == "W_cat":
            rows = want[off:off + n].reshape(shape)
            for l in generated_leaves(g):
                if hit("output_head_" + l.flat_name + ".kernel"):
                    rows[:, l.offset:l.offset + l.size] = 1
        elif name == "b_cat":
            for l in generated_leaves(g):
                if hit("output_head_" + l.flat_name + ".bias"):
                    want[off + l.offset:off + l.offset + l.size] = 1
        elif name in (POSITION_SOURCE, POSITION_LEAF) and position_source:
            want[off:off + n] = hit(POSITION_LEAF)              # the tail is that leaf; the slot is derived from it
        else:
            assert "/" in name or "." not in name
            want[off:off + n] = hit(name.replace("/", "."))
    return want


def _ranges(g, train_encoder=False, position_source=0):
    b = {name: (off, n) for name, off, n in gradient_buckets(g, train_encoder, position_source)}
    wcat, n_heads = b["output_heads"]
    return wcat, wcat + n_heads


@pytest.mark.parametrize("g", [MID, FULL], ids=["MID", "FULL"])
def test_masks_and_flags_of_the_usual_pattern_sets(g):
    total = train_param_layout(g)[1]
    wcat, n_hyper = _ranges(g)
    assert n_hyper == total

    mask, flags = frozen_plan(g, ("*hf_model*",))                   # the reference's default: matches nothing, accepted silently
    assert mask.dtype == np.uint8 and mask.shape == (total,) and not mask.any() and flags == 0
    mask, flags = frozen_plan(g, ())
    assert not mask.any() and flags == 0

    mask, flags = frozen_plan(g, CONTEXT)
    np.testing.assert_array_equal(mask, _expected(g, CONTEXT))
    assert mask[:wcat].all() and not mask[wcat:].any() and flags == 4

    mask, flags = frozen_plan(g, HEADS)
    np.testing.assert_array_equal(mask, _expected(g, HEADS))
    assert not mask[:wcat].any() and mask[wcat:n_hyper].all() and flags == 2

    one = ("output_head_encoder_pos_embedding.kernel",)
    mask, flags = frozen_plan(g, one)
    np.testing.assert_array_equal(mask, _expected(g, one))
    leaf = next(l for l in generated_leaves(g) if l.flat_name == "encoder_pos_embedding")
    G = generated_leaves(g)[-1].offset + generated_leaves(g)[-1].size
    rows = mask[wcat:wcat + g.ctx_dim * G].reshape(g.ctx_dim, G)
    cols = np.zeros(G, np.uint8)
    cols[leaf.offset:leaf.offset + leaf.size] = 1
    assert (rows == cols[None]).all()                               # its columns in every row of W_cat
    assert not mask[wcat + g.ctx_dim * G:].any() and not mask[:wcat].any() and flags == 0     # nothing in b_cat
    assert int(mask.sum()) == g.ctx_dim * leaf.size

    # a single context-encoder leaf by its full dotted name, and a pattern across blocks
    for keys in (("Transformer_0.encoderblock_1.MlpBlock_0.Dense_0.kernel",), ("Transformer_0.encoderblock_*",), ("task_token_projection.bias",)):
        mask, flags = frozen_plan(g, keys)
        np.testing.assert_array_equal(mask, _expected(g, keys))
        assert mask.any() and flags == 0


@pytest.mark.parametrize("g", [MID, FULL], ids=["MID", "FULL"])
def test_encoder_leaves_and_the_position_source(g):
    layer = ("encoder_image_encoder_encoder_layer_0_*",)
    mask, flags = frozen_plan(g, layer, train_encoder=True)
    want = _expected(g, layer, True)
    np.testing.assert_array_equal(mask, want)
    layout, total = train_param_layout(g, True)
    wcat, n_hyper = _ranges(g, True)
    named = [(name, off, int(np.prod(shape))) for name, off, shape in layout if name.startswith("encoder_image_encoder_encoder_layer_0_")]
    assert len(named) == 18 and int(mask.sum()) == sum(n for _, _, n in named) and not mask[:n_hyper].any() and flags == 0
    assert not frozen_plan(g, layer)[0].any()                      # frozen encoder: the pattern has nothing to match

    # with a position source the tail IS the position leaf; the baked slot follows it
    pos = (POSITION_LEAF,)
    layout, total = train_param_layout(g, True, SOURCE_N)
    at = {name: (off, int(np.prod(shape))) for name, off, shape in layout}
    for keys in (pos, layer + pos):
        mask, flags = frozen_plan(g, keys, train_encoder=True, position_source=SOURCE_N)
        np.testing.assert_array_equal(mask, _expected(g, keys, True, SOURCE_N))
        (so, sn), (to, tn) = at[POSITION_LEAF], at[POSITION_SOURCE]
        assert mask[so:so + sn].all() and mask[to:to + tn].all() and to + tn == total and flags == 0
    mask, _ = frozen_plan(g, pos, train_encoder=True, position_source=SOURCE_N)
    assert int(mask.sum()) == at[POSITION_LEAF][1] + at[POSITION_SOURCE][1]
    mask, _ = frozen_plan(g, layer, train_encoder=True, position_source=SOURCE_N)
    assert not mask[at[POSITION_LEAF][0]:at[POSITION_LEAF][0] + at[POSITION_LEAF][1]].any() and not mask[at[POSITION_SOURCE][0]:].any()

    # heads and context frozen, the encoder trained: both hypernetwork buckets are flagged
    mask, flags = frozen_plan(g, CONTEXT + HEADS, train_encoder=True)
    assert mask[:n_hyper].all() and not mask[n_hyper:].any() and flags == 6


@pytest.mark.parametrize("g", [MID, FULL], ids=["MID", "FULL"])
def test_refusals(g):
    with pytest.raises(ValueError, match="nothing is left to train"):
        frozen_plan(g, CONTEXT + HEADS)
    with pytest.raises(ValueError, match="nothing is left to train"):
        frozen_plan(g, ("*",), train_encoder=True)
    with pytest.raises(ValueError, match="train_encoder=False"):
        frozen_plan(g, ("encoder_image_encoder_*",), train_encoder=True)
    with pytest.raises(ValueError, match="train_encoder=False"):
        frozen_plan(g, ("encoder_image_encoder_*",), train_encoder=True, position_source=SOURCE_N)
    with pytest.raises(ValueError, match="delta_change_decay"):
        frozen_plan(g, ("encoder_image_encoder_encoder_layer_0_*",), train_encoder=True, base_weight_decay=0.01)
    # base_weight_decay with only hypernetwork leaves frozen, or with the encoder not trained at all, is fine
    assert frozen_plan(g, HEADS, train_encoder=True, base_weight_decay=0.01)[1] == 2
    assert frozen_plan(g, CONTEXT, base_weight_decay=0.01)[1] == 4


def test_counts():
    for g in (MID, FULL):
        for keys, enc in ((CONTEXT, False), (HEADS, False), (("Transformer_0.encoderblock_*",), False),
                          (("encoder_image_encoder_encoder_layer_0_*",), True), (("*hf_model*",), True)):
            mask, _ = frozen_plan(g, keys, train_encoder=enc)
            n = train_param_layout(g, enc)[1]
            frozen_count = int(mask.sum())
            trainable_count = int((mask == 0).sum())
            assert frozen_count + trainable_count == n == mask.size
            assert frozen_count == int(_expected(g, keys, enc).sum())


def test_the_binding_is_the_header_s_declaration():
    from hypervla import _native
    src = open(os.path.join(ROOT, "include", "hvla.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+hvla_train_frozen\s*\(([^)]*)\)\s*;", src)
    assert m, "hvla_train_frozen is not declared in include/hvla.h"
    args = [a.strip() for a in m.group(1).split(",")]
    assert args == ["hvla_ctx* ctx", "const uint8_t* frozen", "int64_t n_params", "int32_t frozen_buckets"]
    as_ctypes = lambda a: ctypes.c_void_p if "*" in a else {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32}[a.split()[0]]
    assert "hvla_train_frozen" in _native.EXPORTS
    if not os.path.exists(_native.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    lib = _native.load_library()
    assert list(lib.hvla_train_frozen.argtypes) == [as_ctypes(a) for a in args]
    assert lib.hvla_train_frozen.restype is ctypes.c_int
    assert lib.hvla_train_frozen(None, None, 0, 0) == -7           # HVLA_E_STATE: no context (nothing else is touched)
