"""GPU: DINOv2's position table trained through its interpolation -- the two kernels of csrc/position.hip against the converter's
own resize and its float64 transpose, and the fine-tune step / optimizer / publish with the un-resized table as the parameter."""
import dataclasses

import numpy as np
import pytest

from adamw_ref import optax_step as _optax_step

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

U = 2.0 ** -24
SHAPES = [(37, 16, 128), (9, 8, 128), (5, 8, 128), (8, 8, 128), (37, 16, 768)]       # (n, grid, E)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")


def _geometry(grid, E):
    from hypervla.config import MID
    return dataclasses.replace(MID, image_size=14 * grid, enc_dim=E, enc_heads=E // 64, enc_mlp=4 * E)


_ctx_cache = {}


def _context(grid, E):
    """A context of the kernels' geometry; nothing is loaded into it (the two entry points read its grid and width only)."""
    from hypervla import _native
    _need_gpu()
    if (grid, E) not in _ctx_cache:
        _ctx_cache[(grid, E)] = _native.Context(_geometry(grid, E), 0, max_batch=1)
    return _ctx_cache[(grid, E)]


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _interp(ctx, src, n, w, grid):
    dst = torch.full((1, 1 + grid * grid, src.shape[-1]), float("nan"), dtype=torch.float32, device="cuda")
    ctx.position_interp(src.data_ptr(), n, w.data_ptr(), dst.data_ptr())
    torch.cuda.synchronize()
    return dst


def _adjoint(ctx, ddst, n, w):
    dsrc = torch.full((1, 1 + n * n, ddst.shape[-1]), float("nan"), dtype=torch.float32, device="cuda")
    ctx.position_interp_adjoint(ddst.data_ptr(), n, w.data_ptr(), dsrc.data_ptr())
    torch.cuda.synchronize()
    return dsrc


# ------------------------------------------------------------------ 1, 2: the kernels
@pytest.mark.parametrize("n,grid,E", SHAPES)
def test_interp_is_the_converter_s_resize(n, grid, E):
    """Against convert.bake_position_embeddings.  Bound: an output is two four-tap float32 contractions, 4
    products + 3 additions each = 14 roundings, every one at most 2^-24 of a partial result that sum|w_y| sum|w_x| max|src| bounds;
    numpy sums the same taps in an order of its own (and may fuse), so the two float32 results are each within that of the exact
    value: 2 x 14 x 2^-24 x max_i sum_h |w[h, i]| x max_j sum_w |w[w, j]| x max|src|."""
    from hypervla import convert as cv
    ctx = _context(grid, E)
    rng = np.random.default_rng(1000 * n + grid + E)
    src = (0.02 * rng.standard_normal((1, 1 + n * n, E))).astype(np.float32)
    w = cv.position_interp_weights(n, grid)
    want = cv.bake_position_embeddings(src, grid)
    d_src, d_w = _dev(src), _dev(w)
    got = _interp(ctx, d_src, n, d_w, grid)
    again = _interp(ctx, d_src, n, d_w, grid)
    assert torch.equal(got, again)                                        # two runs, the same bits
    got = got.cpu().numpy()
    assert got.shape == want.shape and np.isfinite(got).all()
    np.testing.assert_array_equal(got[:, 0].view(np.uint32), src[:, 0].view(np.uint32))     # the class row is copied
    w1 = float(np.abs(w).sum(axis=0).max())
    bound = 2 * 14 * U * w1 * w1 * float(np.abs(src).max())
    err = float(np.abs(got - want).max())
    print(f"interp n={n} grid={grid} E={E}: max |d| {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    if n == grid:                                                         # interpolate_pos_encoding returns the table untouched
        np.testing.assert_array_equal(got.view(np.uint32), src.view(np.uint32))


@pytest.mark.parametrize("n,grid,E", SHAPES)
def test_adjoint_is_the_transpose_in_float64(n, grid, E):
    """Against convert.position_table_adjoint (float64).  A source element sums T = (outputs rows it feeds) x (output columns it feeds)
    terms  w_y w_x ddst, each with 3 roundings (the weight product, the product with ddst, the addition): at most
    3 T x 2^-24 x sum_i |w[y, i]| x sum_j |w[x, j]| x max|ddst|, with T and the sums taken at their largest over the source rows."""
    from hypervla import convert as cv
    ctx = _context(grid, E)
    rng = np.random.default_rng(2000 * n + grid + E)
    dd = rng.standard_normal((1, 1 + grid * grid, E)).astype(np.float32)
    w = cv.position_interp_weights(n, grid)
    want = cv.position_table_adjoint(dd.astype(np.float64), n)
    d_dd, d_w = _dev(dd), _dev(w)
    got = _adjoint(ctx, d_dd, n, d_w)
    assert torch.equal(got, _adjoint(ctx, d_dd, n, d_w))                 # a gather: no atomics, the same bits
    got = got.cpu().numpy()
    np.testing.assert_array_equal(got[:, 0].view(np.uint32), dd[:, 0].view(np.uint32))
    if n == grid:
        np.testing.assert_array_equal(got.view(np.uint32), dd.view(np.uint32))
        return
    feeds = int((w != 0).sum(axis=1).max())
    w1 = float(np.abs(w).sum(axis=1).max())
    bound = 3 * feeds * feeds * U * w1 * w1 * float(np.abs(dd).max())
    err = float(np.abs(got - want).max())
    print(f"adjoint n={n} grid={grid} E={E}: max |d| {err:.3e}, bound {bound:.3e}")
    assert err <= bound


def test_adjoint_of_all_ones_gives_the_column_sums():
    """(9, 8): every source row feeds some output and both borders are renormalised -- a lost border tap shows here."""
    from hypervla import convert as cv
    n, grid, E = 9, 8, 128
    w = cv.position_interp_weights(n, grid)
    got = _adjoint(_context(grid, E), torch.ones(1, 1 + grid * grid, E, device="cuda"), n, _dev(w)).cpu().numpy()
    s = w.astype(np.float64).sum(axis=1)
    want = np.outer(s, s).reshape(n * n)
    assert (s != 0).all()
    feeds = int((w != 0).sum(axis=1).max())
    w1 = float(np.abs(w).sum(axis=1).max())
    assert np.abs(got[0, 1:] - want[:, None]).max() <= 3 * feeds * feeds * U * w1 * w1
    assert (got[0, 0] == 1).all()


def test_abi_refusals():
    from hypervla import _native, convert as cv
    n, grid, E = 9, 8, 128
    ctx = _context(grid, E)
    src, w = torch.zeros(1, 1 + n * n, E, device="cuda"), _dev(cv.position_interp_weights(n, grid))
    dst = torch.zeros(1, 1 + grid * grid, E, device="cuda")
    for f, a, b in ((ctx.position_interp, src, dst), (ctx.position_interp_adjoint, dst, src)):
        for args in ((0, n, w.data_ptr(), b.data_ptr()), (a.data_ptr(), n, 0, b.data_ptr()), (a.data_ptr(), n, w.data_ptr(), 0),
                     (a.data_ptr(), 1, w.data_ptr(), b.data_ptr()), (a.data_ptr(), 0, w.data_ptr(), b.data_ptr()),
                     (a.data_ptr(), -3, w.data_ptr(), b.data_ptr())):
            with pytest.raises(_native.NativeError, match="HVLA_E_SHAPE"):
                f(*args)
    with pytest.raises(_native.NativeError, match="HVLA_E_SHAPE"):
        ctx.train_position_source(n, 0)
    with pytest.raises(_native.NativeError, match="HVLA_E_SHAPE"):
        ctx.train_position_source(1, w.data_ptr())
    # with train_encoder off the source changes no size
    off = ctx.train_sizes(2, False), ctx.train_sizes(2, True), ctx.train_bucket_ranges(False), ctx.train_bucket_ranges(True)
    ctx.train_position_source(n, w.data_ptr())
    try:
        assert ctx.train_sizes(2, False) == off[0] and ctx.train_bucket_ranges(False) == off[2]
        tail = (1 + n * n) * E
        on = ctx.train_sizes(2, True)
        assert on[0] == off[1][0] + tail and on[1:] == off[1][1:]
        r = ctx.train_bucket_ranges(True)
        assert r[0] == (off[3][0][0], off[3][0][1] + tail) and r[1:] == off[3][1:]
    finally:
        ctx.train_position_source(0)
    assert ctx.train_sizes(2, True) == off[1]


# ------------------------------------------------------------------ 3 .. 7: the training path at MID, n = 9
N_SRC = 9


@pytest.fixture(scope="module")
def case():
    """MID, B = 3, a hub-shaped 9 x 9 source; the float64 oracle's loss and gradients on the served (baked) parameters, once."""
    _need_gpu()
    from hypervla import synthetic as syn
    from hypervla.config import MID, encoder_leaves, generated_leaves
    from hypervla.model import HyperVLA
    from oracle import hvla_ref_torch as ot
    g, B = MID, 3
    src = syn.synthetic_position_table_hub(g, N_SRC)
    model = HyperVLA.from_synthetic(g, position_table_source=src, max_batch=B)
    ins, st, im = syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g), syn.synthetic_images(B, g)
    batch = syn.synthetic_action_batch(B, g)
    per, loss, grads = ot.train_loss_and_grads(model.params, g, generated_leaves(g), ins, st, None, batch, images=im,
                                               enc_shapes=dict(encoder_leaves(g)))
    return dict(g=g, B=B, src=src, model=model, ins=ins, st=st, im=im, batch=batch, per=per.numpy(),
                grads={k: v.numpy() for k, v in grads.items()}, params=dict(model.params), config=dict(model.config))


def _model(c, **kw):
    """A model of its own (publish changes the one it is given), the fixture's parameters and source."""
    from hypervla.model import HyperVLA
    kw.setdefault("position_table_source", c["src"])
    return HyperVLA(dict(c["config"]), dict(c["params"]), None, None, max_batch=c["B"], **kw)


def _check_gradients(g, ft, n, per, grads, got_loss, tol):
    """test_gpu_train._encoder_case's comparison, with the source's gradient held to A^T (float64) of the oracle's gradient of the
    baked table and the slot's to exactly zero."""
    from hypervla import convert as cv
    from hypervla.train import POSITION_LEAF, unpack_params
    np.testing.assert_allclose(got_loss, per, rtol=3e-4, atol=3e-5)
    got, got_src = unpack_params(g, ft.grads.cpu().numpy(), True, n)
    assert set(got) == set(grads)
    gmax = max(float(np.abs(v).max()) for v in grads.values())
    assert not got[POSITION_LEAF].any()                                      # the slot is no parameter
    rel = sorted(((np.abs(got[k].reshape(v.shape) - v).max() / max(float(np.abs(v).max()), 1e-4 * gmax), k)
                  for k, v in grads.items() if k != POSITION_LEAF), reverse=True)
    want_src = cv.position_table_adjoint(grads[POSITION_LEAF].reshape(1, -1, g.enc_dim).astype(np.float64), n)
    assert float(np.abs(want_src).max()) > 0
    rel_src = float(np.abs(got_src - want_src).max() / max(float(np.abs(want_src).max()), 1e-4 * gmax))
    print("worst relative gradient errors:", [(f"{r:.2e}", k) for r, k in rel[:4]], f"source table {rel_src:.2e}")
    assert rel[0][0] <= tol, rel[:6]
    assert rel_src <= tol, rel_src


def test_gradients_through_the_interpolation(case):
    from hypervla.train import FineTuner
    c = case
    ft = FineTuner(_model(c), c["B"], train_encoder=True)                    # no flag, no refusal (the parent raises here)
    assert ft.source_n == N_SRC and ft.n == ft.model._ctx.train_sizes(c["B"], True)[0]
    loss = ft.forward_backward(c["ins"], c["st"], c["im"], c["batch"]).cpu().numpy()
    _check_gradients(c["g"], ft, N_SRC, c["per"], c["grads"], loss, 2e-3)


def test_two_updates_against_the_optax_chain(case):
    """Two apply() against tests/adamw_ref.optax_step on the vector WITHOUT the slot (tolerances of
    test_adamw_step_matches_reference_update: 2e-6 at lr = 1e-3).  clip = 1e-2 bites; the scale is that of the norm without the slot
    (whose gradient is zero).  The tail moves at base_lr; after each apply the slot of params and of ema is the kernel's resize of its
    tail, bit for bit."""
    from hypervla.train import FineTuner
    c = case
    ft = FineTuner(_model(c), c["B"], train_encoder=True, base_weight_decay=0.01, clip=1e-2, ema_start_step=0)
    m = ft.model
    lr, blr, tol = 1e-3, 2e-4, 2e-6
    hy = dict(ft.hy, lr=lr, base_lr=blr)
    nh = ft.n_hyper
    keep = np.ones(ft.n, bool)
    keep[ft.slot] = False
    assert keep[:nh].all() and ft.tail.stop == ft.n
    r64 = lambda x: x.float().cpu().numpy().astype(np.float64)
    w = ft.interp_w
    for it in range(2):
        ft.forward_backward(c["ins"], c["st"], c["im"], c["batch"])
        full = dict(p=r64(ft.params), mu=r64(ft.mu), nu=r64(ft.nu), ema=r64(ft.ema), g=r64(ft.grads), mask=ft.wd_mask.cpu().numpy())
        st = {k: v[keep] for k, v in full.items()}
        st["p0"] = r64(ft.params0)[keep[nh:]]
        assert not full["g"][ft.slot].any() and not full["mask"][ft.slot].any()
        assert ft.apply(lr=lr, base_lr=blr) is True
        # the device's norm is the one without the slot, to the bound of test_adamw_six_updates_against_the_optax_chain (the
        # longest chain of additions in sqsum_kernel + the square's rounding, all terms positive)
        sq64 = float((st["g"] * st["g"]).sum())
        sq_dev = np.float32(ft.sqsum.cpu().numpy()[0])
        chain = -(-ft.n // (1024 * 256)) + 6 + 1024 * 256 // 64 + 1
        assert abs(float(sq_dev) - sq64) <= chain * U * sq64
        norm32, clip32 = np.sqrt(sq_dev), np.float32(hy["clip"])
        assert norm32 > clip32                                               # the clip bites
        sc = float(clip32 / norm32)
        want = _optax_step(st, hy, it + 1, sc, nh)
        got_p, got_ema = r64(ft.params), r64(ft.ema)
        np.testing.assert_allclose(got_p[keep], want["p"], rtol=0, atol=tol)
        np.testing.assert_allclose(got_ema[keep], want["ema"], rtol=0, atol=tol)
        moved = np.abs(got_p[ft.tail] - full["p"][ft.tail]).max()
        assert 0.5 * blr <= moved <= 1.5 * blr, moved                        # Adam's first steps are ~ lr: base_lr here, not lr
        for vec in (ft.params, ft.ema):
            dst = _interp(m._ctx, vec[ft.tail].view(1, -1, c["g"].enc_dim), N_SRC, w, c["g"].grid)
            assert torch.equal(dst.reshape(-1), vec[ft.slot])


def test_publish_serves_and_saves_the_trained_source(case, tmp_path):
    from hypervla.model import HyperVLA
    from hypervla.train import FineTuner
    c = case
    m = _model(c)
    ft = FineTuner(m, c["B"], train_encoder=True, ema_start_step=0)
    tasks = lambda mm: mm.create_tasks(instruction_dict=c["ins"], initial_state=c["st"])[0]
    act = lambda mm: mm.sample_actions(c["im"], c["ins"], None, None, tasks(mm))[0]
    before = act(m)
    for _ in range(2):
        ft.step(c["ins"], c["st"], c["im"], c["batch"], lr=1e-3, base_lr=1e-3)
    for ema in (True, False):
        vec = ft.ema if ema else ft.params
        ft.publish(ema=ema)
        got = act(m)
        assert np.abs(got - before).max() > 0
        np.testing.assert_array_equal(m.position_table_source.reshape(-1), vec[ft.tail].cpu().numpy())
        assert np.abs(m.position_table_source - c["src"]).max() > 0
        fresh = HyperVLA(m.config, m.params, None, m.dataset_statistics, max_batch=c["B"], position_table_source=m.position_table_source)
        np.testing.assert_array_equal(got.view(np.uint32), act(fresh).view(np.uint32))
        del fresh
    # the parameters were published last: a reloaded checkpoint trains on from where this one stands
    now = ft.forward_backward(c["ins"], c["st"], c["im"], c["batch"], forward_only=True).clone()
    m.save_pretrained(7, str(tmp_path))
    m2 = HyperVLA.load_pretrained(str(tmp_path), max_batch=c["B"], audit="off")
    np.testing.assert_array_equal(m2.position_table_source, m.position_table_source)
    assert m2.config["position_embeddings_baked_from"] == [N_SRC, N_SRC]
    ft2 = FineTuner(m2, c["B"], train_encoder=True)
    again = ft2.forward_backward(c["ins"], c["st"], c["im"], c["batch"], forward_only=True)
    assert torch.equal(now, again)                                           # the forward pass has no atomics
    # replace(): the source follows the table it is the source of, and is left behind by parameters that bring another
    assert m2.replace(dataset_statistics=None).position_table_source is not None
    assert m2.replace(params=dict(m2.params)).position_table_source is not None
    assert m2.replace(params=dict(c["params"])).position_table_source is None


def test_the_tail_goes_through_the_encoder_bucket_on_one_rank(case, tmp_path):
    """The pattern of test_bucketed_all_reduce_path_on_one_rank: a one-rank RCCL group, so the reduction is the identity."""
    import torch.distributed as dist
    from hypervla.train import FineTuner
    c = case
    dist.init_process_group("nccl", init_method=f"file://{tmp_path}/rdzv", world_size=1, rank=0)
    try:
        ft = FineTuner(_model(c), c["B"], train_encoder=True)
        assert [b[0] for b in ft.buckets] == ["image_encoder", "output_heads", "context_encoder"] and ft._bucket_id == [0, 1, 2]
        _, off, ln = ft.buckets[0]
        assert off + ln == ft.n == ft.tail.stop                              # the tail closes the encoder's bucket
        ft.forward_backward(c["ins"], c["st"], c["im"], c["batch"])
        torch.cuda.synchronize()
        g0 = ft.grads.clone()
        assert float(g0[ft.tail].abs().max()) > 0
        ft.all_reduce_gradient(single_rank_too=True)
        torch.cuda.synchronize()
        assert torch.equal(ft.grads, g0)
        ft.forward_backward(c["ins"], c["st"], c["im"], c["batch"])        # enqueued behind the step, nothing synchronised in between
        ft.all_reduce_gradient(single_rank_too=True)
        torch.cuda.synchronize()
        # (two runs of the step differ in the last bits -- the split-K sums in front of the adjoint -- as in the pattern)
        assert float((ft.grads - g0).abs().max()) <= 1e-4 * float(g0.abs().max()) and not ft.grads[ft.slot].any()
    finally:
        dist.destroy_process_group()


def test_refusals_and_precedence(case):
    from hypervla.train import FineTuner, POSITION_LEAF, train_param_layout
    c = case
    # the marker without a source: today's refusal
    with pytest.raises(ValueError, match="baked"):
        FineTuner(_model(c, position_table_source=None), c["B"], train_encoder=True)
    # a source that is not the source of the served table
    wrong = c["src"].copy()
    wrong[0, 5] += 1e-3
    with pytest.raises(ValueError, match=f"position_table_source.*{POSITION_LEAF}"):
        FineTuner(_model(c, position_table_source=wrong), c["B"], train_encoder=True)
    # a frozen encoder is not concerned
    fz = FineTuner(_model(c), c["B"])
    assert fz.source_n == 0 and fz.n == train_param_layout(c["g"], False)[1]
    # accept_baked_position_table wins over a source: the slot is trained as before, no tail, and the source is dropped on publish
    m = _model(c)
    ft = FineTuner(m, c["B"], train_encoder=True, accept_baked_position_table=True)
    layout, total = train_param_layout(c["g"], True)
    assert ft.source_n == 0 and ft.n == total
    off, shape = next((o, s) for name, o, s in layout if name == POSITION_LEAF)
    ft.forward_backward(c["ins"], c["st"], c["im"], c["batch"])
    assert float(ft.grads[off:off + shape[0]].abs().max()) > 0
    ft.apply(lr=1e-3, base_lr=1e-3)
    assert m.position_table_source is not None
    ft.publish()
    assert m.position_table_source is None
    np.testing.assert_array_equal(m.params[POSITION_LEAF], ft.params[off:off + shape[0]].cpu().numpy())


# ------------------------------------------------------------------ 8: README widths once
@pytest.mark.timeout(600)
def test_readme_widths_once():
    """DINOv2-base widths and the hub's 37 x 37 table, one layer of each transformer, B = 1."""
    _need_gpu()
    from hypervla import synthetic as syn
    from hypervla.config import FULL, encoder_leaves, generated_leaves
    from hypervla.model import HyperVLA
    from hypervla.train import FineTuner
    from oracle import hvla_ref_torch as ot
    g, B, n = dataclasses.replace(FULL, enc_layers=1, layers=1, ctx_layers=1), 1, 37
    model = HyperVLA.from_synthetic(g, position_table_source=syn.synthetic_position_table_hub(g, n), max_batch=B)
    assert model.config["position_embeddings_baked_from"] == [n, n]
    ins, st, im = syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g), syn.synthetic_images(B, g)
    batch = syn.synthetic_action_batch(B, g)
    per, loss, grads = ot.train_loss_and_grads(model.params, g, generated_leaves(g), ins, st, None, batch, images=im,
                                               enc_shapes=dict(encoder_leaves(g)))
    ft = FineTuner(model, B, train_encoder=True)
    got_loss = ft.forward_backward(ins, st, im, batch).cpu().numpy()
    _check_gradients(g, ft, n, per.numpy(), {k: v.numpy() for k, v in grads.items()}, got_loss, 2e-3)
