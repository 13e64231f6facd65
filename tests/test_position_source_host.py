"""CPU: the host side of training DINOv2's position table through its interpolation -- the float64 adjoint of the converter's resize,
the source table through convert / save / reload / export, and the flat layout, buckets and weight-decay mask with the source as
the vector's tail."""
import json

import numpy as np
import pytest

from hypervla import convert as cv
from hypervla import synthetic as syn
from hypervla.config import MID, TINY, default_config
from hypervla.train import (POSITION_LEAF, POSITION_SOURCE, gradient_buckets, pack_params, train_param_layout, unpack_params,
                            weight_decay_mask)

SHAPES = [(37, 16), (9, 8), (5, 8), (8, 8)]     # README shape; both borders renormalised; up-sampling with missing taps; identity
E = 8


def _nest(flat):
    tree = {}
    for k, v in flat.items():
        node = tree
        keys = k.split("/")
        for kk in keys[:-1]:
            node = node.setdefault(kk, {})
        node[keys[-1]] = v
    return tree


def _bake64(u, n, grid):
    """`bake_position_embeddings` as the linear map A in float64 (its float32 weights, exact products)."""
    if n == grid:
        return u.copy()
    w = cv.position_interp_weights(n, grid).astype(np.float64)
    out = np.einsum("hwe,hi,wj->ije", u[0, 1:].reshape(n, n, -1), w, w)
    return np.concatenate([u[:, :1], out.reshape(1, grid * grid, -1)], axis=1)


@pytest.mark.parametrize("n,grid", SHAPES)
def test_adjoint_is_the_transpose_of_the_resize(n, grid):
    rng = np.random.default_rng(n * 100 + grid)
    u = rng.standard_normal((1, 1 + n * n, E))
    v = rng.standard_normal((1, 1 + grid * grid, E))
    Au, Atv = _bake64(u, n, grid), cv.position_table_adjoint(v, n)
    assert Atv.shape == u.shape and Atv.dtype == np.float64
    lhs, rhs = float((Au * v).sum()), float((u * Atv).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs)), (lhs, rhs)
    # A itself is the converter's resize (float32 there)
    np.testing.assert_allclose(cv.bake_position_embeddings(u.astype(np.float32), grid), _bake64(u.astype(np.float32).astype(np.float64), n, grid),
                               rtol=0, atol=1e-5)
    np.testing.assert_array_equal(Atv[:, 0], v[:, 0])           # the class row passes through
    if n == grid:
        np.testing.assert_array_equal(Atv, v)


@pytest.mark.parametrize("n,grid", SHAPES)
def test_adjoint_equals_autograd_through_the_two_einsums(n, grid):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(7 + n)
    u = torch.tensor(rng.standard_normal((1, 1 + n * n, E)), dtype=torch.float64, requires_grad=True)
    v = torch.tensor(rng.standard_normal((1, 1 + grid * grid, E)), dtype=torch.float64)
    if n == grid:
        out = u * 1.0
    else:
        w = torch.tensor(cv.position_interp_weights(n, grid).astype(np.float64))
        tmp = torch.einsum("hwe,hi->iwe", u[0, 1:].reshape(n, n, E), w)          # height first, then width: bake_position_embeddings
        out = torch.cat([u[:, :1], torch.einsum("iwe,wj->ije", tmp, w).reshape(1, grid * grid, E)], dim=1)
    (out * v).sum().backward()
    np.testing.assert_allclose(cv.position_table_adjoint(v.numpy(), n), u.grad.numpy(), rtol=0, atol=1e-13)


def test_all_ones_gradient_gives_the_column_sums_of_w_x_w():
    n, grid = 9, 8
    w = cv.position_interp_weights(n, grid).astype(np.float64)
    got = cv.position_table_adjoint(np.ones((1, 1 + grid * grid, 2)), n)[0, 1:, 0].reshape(n, n)
    np.testing.assert_allclose(got, np.outer(w.sum(1), w.sum(1)), rtol=0, atol=1e-14)
    assert (w.sum(1) != 0).all()                                 # every source row feeds some output: a lost border tap would show


def test_converter_keeps_the_source_table(tmp_path):
    from hypervla.model import read_params_file
    g = TINY                                                     # 4 x 4 patches
    P = syn.synthetic_params(g)
    big = np.random.default_rng(0).standard_normal((1, 1 + 9 * 9, g.enc_dim)).astype(np.float32)
    tree = _nest({k: (big.reshape(-1) if k == POSITION_LEAF else v) for k, v in P.items()})
    src, dst = tmp_path / "run", tmp_path / "out"
    src.mkdir()
    (src / "config.json").write_text(json.dumps(default_config(g)))
    out = cv.convert_checkpoint(str(src), str(dst), 3, tree=tree)
    params, source = read_params_file(out)
    assert source.dtype == np.float32 and source.shape == big.shape
    np.testing.assert_array_equal(source, big)                   # bit for bit
    assert set(params) == set(P)                                 # beside the parameters, not one of them
    np.testing.assert_array_equal(params[POSITION_LEAF].reshape(1, 17, g.enc_dim), cv.bake_position_embeddings(big, 4))
    assert json.loads((dst / "config.json").read_text())["position_embeddings_baked_from"] == [9, 9]
    # a checkpoint already at the run-time grid has no source and no marker
    out2 = cv.convert_checkpoint(str(src), str(tmp_path / "out2"), 3, tree=_nest(P))
    params2, source2 = read_params_file(out2)
    assert source2 is None and set(params2) == set(P)
    assert "position_embeddings_baked_from" not in json.loads((tmp_path / "out2" / "config.json").read_text())
    # params_from_tree: the dict as before, the source on request
    assert isinstance(cv.params_from_tree(tree, g), dict)
    p3, s3 = cv.params_from_tree(tree, g, return_source=True)
    np.testing.assert_array_equal(s3, big)
    assert cv.params_from_tree(_nest(P), g, return_source=True)[1] is None
    # the reference-shaped export: the source in the baked table's place, ravelled; converting it again bakes back
    exported = cv.tree_from_params(params, position_table_source=source)
    np.testing.assert_array_equal(exported[POSITION_LEAF], big.reshape(-1))
    back, again = cv.params_from_tree(exported, g, return_source=True)
    np.testing.assert_array_equal(back[POSITION_LEAF], params[POSITION_LEAF])
    np.testing.assert_array_equal(again, big)
    np.testing.assert_array_equal(cv.tree_from_params(params)[POSITION_LEAF], params[POSITION_LEAF].reshape(-1))   # without: as before


def test_layout_buckets_and_packing_with_the_source_as_the_tail():
    g, n = MID, 9
    for enc in (False, True):                                     # without the new argument: what they returned before
        assert train_param_layout(g, enc) == train_param_layout(g, enc, 0)
        assert gradient_buckets(g, enc) == gradient_buckets(g, enc, 0)
    assert train_param_layout(g, False, n) == train_param_layout(g, False)      # a frozen encoder has no tail
    base, total = train_param_layout(g, True)
    lay, total_s = train_param_layout(g, True, n)
    tail = (1 + n * n) * g.enc_dim
    assert lay[:-1] == base and lay[-1] == (POSITION_SOURCE, total, (1, 1 + n * n, g.enc_dim)) and total_s == total + tail
    b0, b1 = gradient_buckets(g, True), gradient_buckets(g, True, n)
    assert [b[0] for b in b1] == ["image_encoder", "output_heads", "context_encoder"]
    assert b1[1:] == b0[1:] and b1[0] == (b0[0][0], b0[0][1], b0[0][2] + tail)
    covered = np.zeros(total_s, np.int32)                         # the buckets tile the vector
    for _, off, ln in b1:
        covered[off:off + ln] += 1
    assert (covered == 1).all()
    P = syn.synthetic_params(g)
    src = syn.synthetic_position_table_hub(g, n)
    flat = pack_params(g, P, True, src)
    assert flat.shape == (total_s,)
    np.testing.assert_array_equal(flat[:total], pack_params(g, P, True))
    np.testing.assert_array_equal(flat[total:], src.reshape(-1))
    got, got_src = unpack_params(g, flat, True, n)
    assert POSITION_SOURCE not in got and set(got) == set(unpack_params(g, flat[:total], True))
    np.testing.assert_array_equal(got_src, src)
    np.testing.assert_array_equal(got[POSITION_LEAF], P[POSITION_LEAF])


@pytest.mark.parametrize("strategy", ["v1", "v2", "v3", "v5"])
def test_weight_decay_mask_gives_the_tail_the_leaf_s_value_and_the_slot_zero(strategy):
    g, n = MID, 9
    np.testing.assert_array_equal(weight_decay_mask(g, strategy, True, 0), weight_decay_mask(g, strategy, True))
    old = weight_decay_mask(g, strategy, True)
    new = weight_decay_mask(g, strategy, True, n)
    lay, total = train_param_layout(g, True, n)
    at = {name: (off, int(np.prod(shape))) for name, off, shape in lay}
    (so, sn), (to, tn) = at[POSITION_LEAF], at[POSITION_SOURCE]
    leaf_value = {"v1": 0, "v2": 1, "v3": 1, "v5": 1}[strategy]    # no "kernel" in the leaf's path; no "norm"; an image-encoder leaf
    assert (old[so:so + sn] == leaf_value).all()
    assert (new[to:to + tn] == leaf_value).all() and (new[so:so + sn] == 0).all()
    rest = np.ones(len(old), bool)
    rest[so:so + sn] = False
    np.testing.assert_array_equal(new[:len(old)][rest], old[rest])
