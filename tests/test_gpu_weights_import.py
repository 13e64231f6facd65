"""GPU: policies as values -- hvla_weights_import / hvla_weights_import_slots / hvla_weights_copy_slots through
import_tasks / assign_base_params / copy_tasks / save / load_tasks.  What is bitwise: export(import(theta)) on the vector leaves and
against the host restatement of the split on the matrix leaves; export . import on an export; a slot against the same row imported
alone; a copy against its source.  What is held to the policy kernel's oracle bounds: a theta the hypernetwork never produced, and
a re-imported export against the handle it came from (whose bf16 halves the re-split does not always reproduce).

MID, B = 4 and a pool of 6 unless a test says otherwise: more than one fragment per leaf, several rows, scattered slots."""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

B, CAP = 4, 6


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X; torch.cuda.is_available() is False")


def _rows(d, idx):
    return {"language_instruction": {k: np.asarray(v)[idx] for k, v in d["language_instruction"].items()}}


def _st(st, idx):
    return {"patch_embeddings": st["patch_embeddings"][idx]}


def _flat(g, theta):
    """oracle-style base_params ({flat leaf name: float64 [B, *shape]}) of pytree_from_theta(g, theta)"""
    from hypervla.config import generated_leaves, pytree_from_theta
    tree, out = pytree_from_theta(g, np.asarray(theta, np.float64)), {}
    for lf in generated_leaves(g):
        node = tree
        for key in lf.path:
            node = node[key]
        out[lf.flat_name] = node
    return out


def _leaf_std(g, theta):
    """per generated leaf, the std of its elements over a generated batch, as a [G] vector"""
    from hypervla.config import generated_leaves
    s = np.empty(theta.shape[1], np.float32)
    for lf in generated_leaves(g):
        s[lf.offset:lf.offset + lf.size] = theta[:, lf.offset:lf.offset + lf.size].std()
    return s


def _restated(theta):
    """float(hi) + float(lo) of the host restatement of split1 (torch CPU bfloat16: round to nearest even)"""
    x = torch.as_tensor(np.ascontiguousarray(theta))
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    return (hi.float() + lo.float()).numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _fixture(g, oracle_tokens):
    from hypervla import synthetic as syn
    from hypervla.config import encoder_leaves, generated_leaves
    from hypervla.model import HyperVLA
    m = HyperVLA.from_synthetic(g, max_batch=8)
    ins, st, im = syn.synthetic_instructions(CAP, g), syn.synthetic_initial_state(CAP, g), syn.synthetic_images(CAP, g)
    w, _, _ = m.create_tasks(instruction_dict=_rows(ins, slice(0, B)), initial_state=_st(st, slice(0, B)))
    theta, ctx = (t.cpu().numpy() for t in w.export())
    d = dict(g=g, m=m, ins=ins, st=st, im=im, w=w, theta=theta, ctx=ctx, std=_leaf_std(g, theta))
    if oracle_tokens:
        from oracle import hvla_ref_np as onp
        P = syn.synthetic_params(g)
        bp, _ = onp.create_tasks(P, g, generated_leaves(g), _rows(ins, slice(0, B)), _st(st, slice(0, B)))
        d["tok"] = onp.sample_actions(P, g, dict(encoder_leaves(g)), bp, im[:B])[3]
    else:
        d["tok"] = np.random.default_rng(11).standard_normal((B, g.patches, g.enc_dim))
    return d


@pytest.fixture(scope="module")
def mid():
    _need_gpu()
    from hypervla.config import MID
    return _fixture(MID, True)


@pytest.fixture(scope="module")
def lang():
    _need_gpu()
    from hypervla.config import MID
    return _fixture(dataclasses.replace(MID, lang_in_policy=True), False)


def _midpoints(theta):
    return (0.5 * (theta + np.roll(theta, -1, axis=0))).astype(np.float32)        # rows (0, 1), (1, 2), (2, 3), (3, 0)


def _random_theta(fx, seed=21):
    n = np.random.default_rng(seed).standard_normal(fx["theta"].shape).astype(np.float32)
    return n * fx["std"][None]


def _filled_pool(fx):
    m = fx["m"]
    pool = m.create_pool(CAP)
    m.assign_tasks(pool, list(range(CAP)), fx["ins"], fx["st"])
    return pool


def _dstats(m):
    from hypervla.interface import device_unnormalization
    return device_unnormalization(m.dataset_statistics["bridge_dataset"]["action"], "normal")


def _age_counters(fx, pool):
    """two ensemble calls on every slot: counters and rings no longer those of a fresh slot"""
    m, g = fx["m"], fx["g"]
    rng = np.random.default_rng(8)
    for _ in range(2):
        m.ensemble_actions(pool, rng.uniform(-2, 2, (CAP, g.horizon, g.action_dim)).astype(np.float32), _dstats(m), list(range(CAP)))


def _assert_first_call_ensemble(fx, pool, slots):
    m, g = fx["m"], fx["g"]
    a = np.random.default_rng(9).uniform(-2, 2, (len(slots), g.horizon, g.action_dim)).astype(np.float32)
    got = m.ensemble_actions(pool, a, _dstats(m), slots)
    fresh = m.ensemble_actions(m.create_pool(CAP), a, _dstats(m), slots)
    np.testing.assert_array_equal(got, fresh)


# ------------------------------------------------------------------ fixed point
def test_export_of_an_imported_export_is_the_export(mid):
    m = mid["m"]
    theta, ctx = mid["w"].export()
    w2 = m.import_tasks(theta, context=ctx)
    t2, c2 = w2.export()
    assert torch.equal(t2, theta) and torch.equal(c2, ctx)
    w3 = m.import_tasks(mid["w"].to_pytree(), context=mid["ctx"])          # and through the host forms
    t3, c3 = w3.export()
    assert torch.equal(t3, theta) and torch.equal(c3, ctx)
    assert not m.import_tasks(theta).export()[1].any()                     # no context given: zeros


def test_fixed_point_at_the_full_geometry():
    """FULL, B = 2: the full-size leaves have a permutation of their own."""
    _need_gpu()
    from hypervla import synthetic as syn
    from hypervla.config import FULL
    from hypervla.model import HyperVLA
    m = HyperVLA.from_synthetic(FULL, max_batch=2)
    w, _, _ = m.create_tasks(instruction_dict=syn.synthetic_instructions(2, FULL), initial_state=syn.synthetic_initial_state(2, FULL))
    theta, ctx = w.export()
    assert theta.shape == (2, 201_500) and theta.abs().max() > 0
    t2, c2 = m.import_tasks(theta, context=ctx).export()
    assert torch.equal(t2, theta) and torch.equal(c2, ctx)


# ------------------------------------------------------------------ host restatement
def test_random_theta_against_the_host_restatement(mid):
    from hypervla.config import generated_leaves
    m, g = mid["m"], mid["g"]
    theta = _random_theta(mid)
    w = m.import_tasks(theta)
    out = w.export()[0].cpu().numpy()
    rest = _restated(theta)
    kinds = {}
    for lf in generated_leaves(g):
        sl = slice(lf.offset, lf.offset + lf.size)
        same = np.array_equal(_bits(out[:, sl]), _bits(theta[:, sl]))
        split = np.array_equal(_bits(out[:, sl]), _bits(rest[:, sl]))
        assert same or split, lf.flat_name
        if lf.path[-1] == "kernel":
            assert split, lf.flat_name
            assert not same or not theta[:, sl].any(), lf.flat_name          # (a random f32 matrix is not made of bf16 pairs)
        else:
            assert same, lf.flat_name
        kinds[lf.flat_name] = "split" if lf.path[-1] == "kernel" else "f32"
    assert set(kinds.values()) == {"split", "f32"}
    # padding and everything else the permutation does not name: the same rows imported over a pool that held other weights
    pool = _filled_pool(mid)
    m.assign_base_params(pool, [4, 1, 0, 5], theta)
    tp = pool.export()[0].cpu().numpy()
    assert np.array_equal(_bits(tp[[4, 1, 0, 5]]), _bits(out))
    a, it = m.sample_actions(mid["im"][:B], None, None, None, pool, slots=[4, 1, 0, 5])
    a0, it0 = m.sample_actions(mid["im"][:B], None, None, None, w)
    np.testing.assert_array_equal(a, a0)
    np.testing.assert_array_equal(it["gripper_logits"], it0["gripper_logits"])


# ------------------------------------------------------------------ a theta the hypernetwork did not produce, against the oracle
@pytest.mark.parametrize("case", ["midpoint", "perturbed"])
def test_imported_theta_against_the_oracle(mid, case):
    """The bounds test_gpu_parity.test_policy_from_oracle_tokens holds the same kernel to."""
    from oracle import hvla_ref_np as onp
    m, g = mid["m"], mid["g"]
    if case == "midpoint":
        theta = _midpoints(mid["theta"])
    else:
        theta = (mid["theta"] + 0.1 * _random_theta(mid, seed=22)).astype(np.float32)
    assert np.abs(theta - mid["theta"]).max() > 1e-3                         # not what the hypernetwork gave these tasks
    w = m.import_tasks(theta)
    act, logit = (t.cpu().numpy() for t in m.policy_from_tokens(mid["tok"].astype(np.float32), w))
    ract, rlogit, _ = onp.policy(_flat(g, theta), g, mid["tok"])
    d, dl = np.abs(act[..., :6] - ract[..., :6]), np.abs(logit - rlogit)
    print("imported %s theta against the oracle: action MAE %.3e max %.3e, logit max %.3e" % (case, d.mean(), d.max(), dl.max()))
    assert d.mean() <= 1e-4 and d.max() <= 1e-3, (d.mean(), d.max())
    assert dl.max() <= 1e-3
    safe = np.abs(rlogit) > 2e-3
    assert (act[..., 6][safe] == ract[..., 6][safe]).all()


def test_reimported_export_steps_close_to_the_generated_handle(mid):
    """Not bitwise (the re-split does not reproduce every hi / lo pair): each side is within the oracle bound, so within twice it
    of the other."""
    m = mid["m"]
    tok = mid["tok"].astype(np.float32)
    a0, l0 = (t.cpu().numpy() for t in m.policy_from_tokens(tok, mid["w"]))
    w2 = m.import_tasks(mid["w"].export()[0])
    a1, l1 = (t.cpu().numpy() for t in m.policy_from_tokens(tok, w2))
    d, dl = np.abs(a1[..., :6] - a0[..., :6]), np.abs(l1 - l0)
    print("re-imported export against the generated handle: action max %.3e MAE %.3e, logit max %.3e" % (d.max(), d.mean(), dl.max()))
    assert d.mean() <= 2e-4 and d.max() <= 2e-3 and dl.max() <= 2e-3, (d.mean(), d.max(), dl.max())


# ------------------------------------------------------------------ pool
def test_import_into_slots_writes_exactly_its_rows(mid):
    m = mid["m"]
    theta, ctx = _midpoints(mid["theta"]), mid["ctx"][::-1].copy()
    pool = _filled_pool(mid)
    _age_counters(mid, pool)
    th0, cx0 = (t.clone() for t in pool.export())
    m.assign_base_params(pool, [4, 1], theta[:2], context=ctx[:2])
    th1, cx1 = pool.export()
    rest = [0, 2, 3, 5]
    assert torch.equal(th1[rest], th0[rest]) and torch.equal(cx1[rest], cx0[rest])
    single = m.import_tasks(theta[:2], context=ctx[:2])
    ts, cs = single.export()
    assert torch.equal(th1[[4, 1]], ts) and torch.equal(cx1[[4, 1]], cs)
    _assert_first_call_ensemble(mid, pool, [4, 1])
    # a slot steps bitwise as the same row imported alone
    a, it = m.sample_actions(mid["im"][:2], None, None, None, pool, slots=[1, 4])
    for k, row in enumerate((1, 0)):                                          # slot 1 holds theta row 1, slot 4 row 0
        w1 = m.import_tasks(theta[row:row + 1], context=ctx[row:row + 1])
        a1, it1 = m.sample_actions(mid["im"][k:k + 1], None, None, None, w1)
        np.testing.assert_array_equal(a1[0], a[k])
        np.testing.assert_array_equal(it1["gripper_logits"][0], it["gripper_logits"][k])
    # K = 1, from a device tensor used in place
    td = torch.as_tensor(theta[2:3]).to(m.device)
    m.assign_base_params(pool, [3], td)
    th2 = pool.export()[0]
    assert torch.equal(th2[3:4], m.import_tasks(td).export()[0]) and torch.equal(th2[[0, 2, 5]], th0[[0, 2, 5]])
    assert torch.equal(th2[[4, 1]], ts)


# ------------------------------------------------------------------ copy
def test_copy_from_a_handle_into_pool_slots(mid):
    m, w = mid["m"], mid["w"]
    pool = _filled_pool(mid)
    _age_counters(mid, pool)
    th0 = pool.export()[0].clone()
    S = [5, 0, 2, 3]
    m.copy_tasks(pool, S, w)
    a0, it0 = m.sample_actions(mid["im"][:B], None, None, None, w)
    a, it = m.sample_actions(mid["im"][:B], None, None, None, pool, slots=S)
    np.testing.assert_array_equal(a, a0)
    np.testing.assert_array_equal(it["gripper_logits"], it0["gripper_logits"])
    th, cx = pool.export()
    tw, cw = w.export()
    assert torch.equal(th[S], tw) and torch.equal(cx[S], cw)
    assert torch.equal(th[[1, 4]], th0[[1, 4]])
    _assert_first_call_ensemble(mid, pool, S)


def test_copy_within_one_pool_and_overlap_refusal(mid):
    m = mid["m"]
    pool = _filled_pool(mid)
    th0, cx0 = (t.clone() for t in pool.export())
    m.copy_tasks(pool, [1, 4], pool, [5, 0])
    th, cx = pool.export()
    assert torch.equal(th[[1, 4]], th0[[5, 0]]) and torch.equal(cx[[1, 4]], cx0[[5, 0]])
    assert torch.equal(th[[0, 2, 3, 5]], th0[[0, 2, 3, 5]])
    with pytest.raises(ValueError, match="overlapping"):
        m.copy_tasks(pool, [1, 4], pool, [4, 2])
    with pytest.raises(ValueError, match="overlapping"):
        m.copy_tasks(pool, [0, 1], pool)                                      # src_slots None = 0 .. K-1
    assert torch.equal(pool.export()[0], th)


# ------------------------------------------------------------------ use_language_token
def _check_lang_against_reference(g, m, theta, ins, tok):
    import lang_policy_ref as LR
    emb = ins["language_instruction"]["token_embedding"]
    w = m.import_tasks(theta, ins)
    act, logit = (t.cpu().numpy() for t in m.policy_from_tokens(tok.astype(np.float32), w))
    ract, rlog, _ = LR.policy(_flat(g, theta), g, tok.astype(np.float32).astype(np.float64), emb)
    d, dl = np.abs(act[..., :6] - ract[..., :6]), np.abs(logit - rlog)
    print("use_language_token T=%d imported midpoint theta: action MAE %.3e max %.3e, logit mean %.3e max %.3e"
          % (g.lang_tokens, d.mean(), d.max(), dl.mean(), dl.max()))
    # the bounds test_gpu_language_tokens asserts for MID
    assert d.mean() <= 5e-4 and d.max() <= 2e-3 and dl.mean() <= 2e-3, (d.mean(), d.max(), dl.mean())
    return w


def test_language_tokens_import_against_the_reference(lang):
    g, m = lang["g"], lang["m"]
    ins = _rows(lang["ins"], slice(0, B))
    _check_lang_against_reference(g, m, _midpoints(lang["theta"]), ins, lang["tok"])
    # other tokens, other actions: the prefix is built from what the import was given
    w0 = m.import_tasks(_midpoints(lang["theta"]), ins)
    w1 = m.import_tasks(_midpoints(lang["theta"]), _rows(lang["ins"], slice(2, 2 + B)))
    a0, a1 = (m.policy_from_tokens(lang["tok"].astype(np.float32), w)[0] for w in (w0, w1))
    assert (a0[..., :6] - a1[..., :6]).abs().max() > 1e-4


def test_language_tokens_lower_edge_two_tokens():
    _need_gpu()
    from hypervla import synthetic as syn
    from hypervla.config import MID
    from hypervla.model import HyperVLA
    g = dataclasses.replace(MID, lang_in_policy=True, lang_tokens=2)
    m = HyperVLA.from_synthetic(g, max_batch=B)
    ins, st = syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g)
    theta = m.create_tasks(instruction_dict=ins, initial_state=st)[0].export()[0].cpu().numpy()
    tok = np.random.default_rng(12).standard_normal((B, g.patches, g.enc_dim))
    _check_lang_against_reference(g, m, _midpoints(theta), ins, tok)


def test_language_copy_carries_the_prefix_and_refusals(lang, mid):
    from hypervla import _native
    m, w = lang["m"], lang["w"]
    pool = m.create_pool(CAP)
    S = [5, 0, 2, 3]
    m.copy_tasks(pool, S, w)
    a0, it0 = m.sample_actions(lang["im"][:B], None, None, None, w)
    a, it = m.sample_actions(lang["im"][:B], None, None, None, pool, slots=S)
    np.testing.assert_array_equal(a, a0)
    np.testing.assert_array_equal(it["gripper_logits"], it0["gripper_logits"])
    th0 = pool.export()[0].clone()
    theta = torch.as_tensor(lang["theta"]).to(m.device)
    with pytest.raises(ValueError, match="instruction_dict"):
        m.import_tasks(theta)
    with pytest.raises(_native.NativeError, match="HVLA_E_SHAPE.*token"):
        m._ctx.weights_import(theta.data_ptr(), 0, 0, B, m._stream())
    sd = torch.as_tensor(np.array(S, np.int32)).to(m.device)
    with pytest.raises(_native.NativeError, match="HVLA_E_SHAPE.*token"):
        m._ctx.weights_import_slots(pool._h, sd.data_ptr(), B, theta.data_ptr(), 0, 0, m._stream())
    assert torch.equal(pool.export()[0], th0)
    # tokens given to a model without the option
    m0 = mid["m"]
    t0 = torch.as_tensor(mid["theta"]).to(m0.device)
    emb = torch.zeros(B, mid["g"].lang_tokens, mid["g"].lang_dim, device=m0.device)
    with pytest.raises(_native.NativeError, match="HVLA_E_SHAPE.*use_language_token"):
        m0._ctx.weights_import(t0.data_ptr(), 0, emb.data_ptr(), B, m0._stream())
    w0 = m0.import_tasks(t0, _rows(mid["ins"], slice(0, B)))                 # the Python surface reads no tokens for such a model
    assert torch.equal(w0.export()[0], mid["w"].export()[0])


# ------------------------------------------------------------------ capture
def test_hipgraph_replay_of_import_copy_and_step_equals_eager(mid):
    m, g = mid["m"], mid["g"]
    dev = m.device
    pool = _filled_pool(mid)
    th_before = pool.export()[0].clone()
    theta = torch.as_tensor(_midpoints(mid["theta"])[:2]).to(dev)
    cx = torch.as_tensor(mid["ctx"][:2].copy()).to(dev)
    i32 = lambda v: torch.as_tensor(np.array(v, np.int32)).to(dev)
    s_imp, s_src, s_dst, s_step = i32([4, 1]), i32([0, 3]), i32([2, 5]), i32([4, 1, 2, 5])
    K = 4
    img = torch.as_tensor(mid["im"][:K]).to(dev).contiguous()
    if img.dim() == 5:
        img = img[:, 0].contiguous()
    act = torch.empty(K, g.horizon, g.action_dim, device=dev)
    lg = torch.empty(K, g.horizon, device=dev)

    def run():
        st = m._stream()
        m._ctx.weights_import_slots(pool._h, s_imp.data_ptr(), 2, theta.data_ptr(), cx.data_ptr(), 0, st)
        m._ctx.weights_copy_slots(pool._h, s_dst.data_ptr(), pool._h, s_src.data_ptr(), 2, st)
        m._ctx.step_slots(pool._h, s_step.data_ptr(), K, img.data_ptr(), act.data_ptr(), lg.data_ptr(), st)

    run()
    torch.cuda.synchronize()
    eager, eager_lg, th_eager = act.clone(), lg.clone(), pool.export()[0].clone()
    assert not torch.equal(th_eager, th_before)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        run()                                                      # warm-up
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            run()
    for _ in range(2):
        m.assign_tasks(pool, list(range(CAP)), mid["ins"], mid["st"])          # the replay has the rows to write again
        assert torch.equal(pool.export()[0], th_before)
        act.zero_()
        lg.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(act, eager) and torch.equal(lg, eager_lg)
        assert torch.equal(pool.export()[0], th_eager)


# ------------------------------------------------------------------ save / load
@pytest.mark.parametrize("which", ["mid", "lang"])
def test_save_and_load_tasks(which, mid, lang, tmp_path):
    fx = mid if which == "mid" else lang
    m, w = fx["m"], fx["w"]
    p = str(tmp_path / "tasks.npz")
    w.save(p)
    w2 = m.load_tasks(p)
    (t, c), (t2, c2) = w.export(), w2.export()
    assert w2.batch == B and torch.equal(t2, t) and torch.equal(c2, c)
    if which == "lang":                                            # the saved tokens rebuild the language prefix
        saved = np.load(p)["token_embedding"]
        np.testing.assert_array_equal(saved, fx["ins"]["language_instruction"]["token_embedding"][:B].astype(np.float32))
        a, _ = m.sample_actions(fx["im"][:B], None, None, None, w)
        a2, _ = m.sample_actions(fx["im"][:B], None, None, None, w2)
        d = np.abs(a2[..., :6] - a[..., :6])                       # a re-import: each side within the MID bound of the reference
        assert d.mean() <= 2 * 5e-4 and d.max() <= 2 * 2e-3, (d.mean(), d.max())
        zeros = {"language_instruction": {"token_embedding": np.zeros_like(saved)}}
        a3, _ = m.sample_actions(fx["im"][:B], None, None, None, m.import_tasks(t, zeros))
        assert np.abs(a3[..., :6] - a[..., :6]).max() > 1e-4       # (and the tokens do matter)
    other = lang if which == "mid" else mid
    with pytest.raises(ValueError, match="G="):
        other["m"].load_tasks(p)


# ------------------------------------------------------------------ refusals through the ABI
def test_abi_refusals_leave_the_pool_as_it_was(mid, lang):
    from hypervla import _native
    m, c = mid["m"], mid["m"]._ctx
    pool = _filled_pool(mid)
    th0, cx0 = (t.clone() for t in pool.export())
    theta = torch.as_tensor(np.repeat(_midpoints(mid["theta"]), 2, axis=0)).to(m.device)          # 8 rows
    sd = torch.as_tensor(np.arange(CAP + 1, dtype=np.int32)).to(m.device)
    st = m._stream()
    with pytest.raises(_native.NativeError, match="HVLA_E_SHAPE.*null theta"):
        c.weights_import_slots(pool._h, sd.data_ptr(), 2, 0, 0, 0, st)
    with pytest.raises(_native.NativeError, match="HVLA_E_SHAPE.*null theta"):
        c.weights_import(0, 0, 0, 2, st)
    for K in (0, CAP + 1):
        with pytest.raises(_native.NativeError, match=r"HVLA_E_SHAPE.*slots outside \[1, 6\]"):
            c.weights_import_slots(pool._h, sd.data_ptr(), K, theta.data_ptr(), 0, 0, st)
        with pytest.raises(_native.NativeError, match=r"HVLA_E_SHAPE.*slots outside \[1, 6\]"):
            c.weights_copy_slots(pool._h, sd.data_ptr(), pool._h, sd.data_ptr(), K, st)
    with pytest.raises(_native.NativeError, match=r"HVLA_E_SHAPE.*slots outside \[1, 4\]"):
        c.weights_copy_slots(pool._h, sd.data_ptr(), mid["w"]._h, sd.data_ptr(), 5, st)     # more than the source has
    with pytest.raises(_native.NativeError, match="HVLA_E_SHAPE.*null slot map"):
        c.weights_import_slots(pool._h, 0, 2, theta.data_ptr(), 0, 0, st)
    # a handle of another context's geometry, as destination and as source
    alien = lang["m"].create_pool(CAP)
    ta, _ = alien.export()
    with pytest.raises(_native.NativeError, match="HVLA_E_SHAPE.*another geometry"):
        c.weights_import_slots(alien._h, sd.data_ptr(), 2, theta.data_ptr(), 0, 0, st)
    with pytest.raises(_native.NativeError, match="HVLA_E_SHAPE.*another geometry"):
        c.weights_copy_slots(pool._h, sd.data_ptr(), alien._h, sd.data_ptr(), 2, st)
    with pytest.raises(_native.NativeError, match="HVLA_E_SHAPE.*another geometry"):
        c.weights_copy_slots(alien._h, sd.data_ptr(), pool._h, sd.data_ptr(), 2, st)
    with pytest.raises(TypeError):
        m.copy_tasks(pool, [0], alien)
    torch.cuda.synchronize()
    th1, cx1 = pool.export()
    assert torch.equal(th1, th0) and torch.equal(cx1, cx0) and torch.equal(alien.export()[0], ta)


def test_sample_actions_still_wants_a_handle(mid):
    with pytest.raises(TypeError, match="import_tasks"):
        mid["m"].sample_actions(mid["im"][:B], None, None, None, mid["w"].to_pytree())
