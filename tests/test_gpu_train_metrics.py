"""GPU: the training metrics (hvla_train_metrics, hvla_loss_terms, FineTuner.info / validate) at the MID geometry.
Every test compares the device with float64 (tests/train_metrics_ref.py) of the device's OWN buffers read back; the loss terms also
with the float64 oracle.  The norm kernels accumulate in f64 and round once (2^-24), then one f64 square root is cast (2^-24):
BOUND = 2^-23, relative."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import train_metrics_ref as ref
from train_metrics_ref import masked_batch
from train_parity import LOSS_ATOL, LOSS_RTOL

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

BOUND = ref.BOUND
SENTINEL = -12345.5


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")


def _np(t):
    return t.detach().cpu().numpy()


def _vec(ft):
    torch.cuda.synchronize()
    return _np(ft.metric_vec).astype(np.float64)


def _close(got, want, what):
    err = ref.rel_err(got, want)
    print(f"{what}: device {got:.9g}  float64 {want:.9g}  relative error {err:.2e} (bound {BOUND:.2e})")
    assert err <= BOUND, (what, got, want, err)


@pytest.fixture(scope="module")
def frozen_case():
    """MID, encoder frozen, B = 5 with both mask floors hit, three tasks (one empty, two samples unclaimed): one forward_backward +
    apply with metrics on, every buffer the metrics read copied to the host once."""
    _need_gpu()
    from hypervla import synthetic as syn
    from hypervla.config import MID
    from hypervla.model import HyperVLA
    from hypervla.train import FineTuner
    g, B = MID, 5
    model = HyperVLA.from_synthetic(g, max_batch=B)
    ins, st = syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g)
    batch = masked_batch(g, B)
    tok = np.random.default_rng(9).standard_normal((B, g.patches, g.enc_dim)).astype(np.float32)
    names = ("bridge", "fractal", "kuka")
    index = {"fractal": np.array([1, 0, 0, 1, 0], bool), "bridge": np.array([0, 1, 0, 0, 0], bool)}
    ft = FineTuner(model, B, metrics=True, task_names=names)
    ft.forward_backward(ins, st, tok, batch, task_index=index)
    assert ft.apply(lr=1e-3) is True                            # (the schedule's own rate at update 0 is 0: nothing would move)
    torch.cuda.synchronize()
    host = {k: _np(getattr(ft, k)) for k in ("grads", "params", "prev_params", "theta", "loss", "actions", "logits")}
    return dict(g=g, B=B, model=model, ft=ft, ins=ins, st=st, batch=batch, tok=tok, names=names, index=index, host=host, vec=_vec(ft),
                vec_dev=ft.metric_vec.clone())        # tests that overwrite the step's vector put it back


# ------------------------------------------------------------------ 1
def test_norm_metrics_frozen_encoder():
    """B = 3, one forward_backward + apply."""
    _need_gpu()
    from hypervla import synthetic as syn
    from hypervla.config import MID, encoder_leaves, shared_name
    from hypervla.model import HyperVLA
    from hypervla.train import FineTuner, INFO_KEYS
    g, B = MID, 3
    model = HyperVLA.from_synthetic(g, max_batch=B)
    ins, st, batch = syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g), syn.synthetic_action_batch(B, g)
    tok = np.random.default_rng(9).standard_normal((B, g.patches, g.enc_dim)).astype(np.float32)
    ft = FineTuner(model, B, metrics=True)
    assert bool(torch.isnan(ft.metric_vec).all())
    ft.forward_backward(ins, st, tok, batch)
    ft.apply(lr=1e-3)
    v = _vec(ft)
    grads, params, prev, theta = _np(ft.grads), _np(ft.params), _np(ft.prev_params), _np(ft.theta)
    enc_sq = sum((np.asarray(model.params[shared_name(p)], np.float64) ** 2).sum() for p, _ in encoder_leaves(g))
    assert enc_sq > 0 and abs(ft.encoder_sqsum - enc_sq) <= 1e-12 * enc_sq
    _close(v[ref.GRAD_NORM], ref.grad_norm(grads), "grad_norm")
    _close(v[ref.PARAM_NORM], ref.param_norm(prev), "param_norm (before the update)")
    _close(v[ref.UPDATE_NORM], ref.update_norm(params, prev), "update_norm")
    _close(v[ref.BASE_PARAMS_NORM], ref.base_params_norm(theta, enc_sq), "base_params_norm")
    assert v[ref.UPDATE_NORM] > 0 and v[ref.PARAM_NORM] > 0 and v[ref.GRAD_NORM] > 0
    assert ref.rel_err(ref.param_norm(params), ref.param_norm(prev)) > BOUND          # before / after the update can be told apart
    info = ft.info()
    assert list(info) == [k for k in INFO_KEYS if not k.startswith("attention_")]
    assert all(t.is_cuda and t.dim() == 0 for t in info.values())
    assert float(info["grad_norm"]) == np.float32(v[ref.GRAD_NORM]) and float(info["learning_rate"]) == np.float32(1e-3)
    assert np.isnan(v[ref.ATTENTION_ENTROPY]) and np.isnan(v[ref.ATTENTION_ALIGNMENT])       # inputs NULL: not written


# ------------------------------------------------------------------ 2
def test_norm_metrics_trained_encoder_with_position_source_and_frozen_heads():
    _need_gpu()
    from hypervla import synthetic as syn
    from hypervla.config import MID
    from hypervla.model import HyperVLA
    from hypervla.train import FineTuner
    g, B = MID, 2
    model = HyperVLA.from_synthetic(g, position_table_source=syn.synthetic_position_table_hub(g, 9), max_batch=B)
    ins, st, im = syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g), syn.synthetic_images(B, g)
    batch = syn.synthetic_action_batch(B, g)
    ft = FineTuner(model, B, train_encoder=True, frozen_keys=("output_head_*",), metrics=True)
    assert ft.source_n == 9 and ft.frozen_count > 0
    ft.forward_backward(ins, st, im, batch)
    ft.apply(lr=1e-3, base_lr=2e-4)
    v = _vec(ft)
    grads, params, prev, theta, frozen = _np(ft.grads), _np(ft.params), _np(ft.prev_params), _np(ft.theta), _np(ft.frozen)
    slot = ft.slot
    assert not grads[slot].any() and frozen[slot].sum() == 0
    _close(v[ref.GRAD_NORM], ref.grad_norm(grads), "grad_norm")
    _close(v[ref.PARAM_NORM], ref.param_norm(prev, frozen, slot), "param_norm without frozen elements and the baked slot")
    _close(v[ref.UPDATE_NORM], ref.update_norm(params, prev, slot), "update_norm without the baked slot")
    enc_sq = ref.encoder_sqsum(prev, ft.n_hyper, slot)
    _close(v[ref.BASE_PARAMS_NORM], ref.base_params_norm(theta, enc_sq), "base_params_norm, the table as its source")
    assert v[ref.UPDATE_NORM] > 0 and v[ref.PARAM_NORM] > 0
    # the restatements that get it wrong are further from the device than the bound: the test can tell them apart
    wrong = {"param_norm with the slot": (v[ref.PARAM_NORM], ref.param_norm(prev, frozen, None)),
             "param_norm with the frozen elements": (v[ref.PARAM_NORM], ref.param_norm(prev, None, slot)),
             "update_norm with the slot": (v[ref.UPDATE_NORM], ref.update_norm(params, prev, None)),
             "base_params_norm with the slot and without the tail":
                 (v[ref.BASE_PARAMS_NORM], ref.base_params_norm(theta, float((prev[ft.n_hyper:ft.tail.start].astype(np.float64) ** 2).sum())))}
    for what, (got, bad) in wrong.items():
        print(f"{what}: relative distance {ref.rel_err(got, bad):.2e}")
        assert ref.rel_err(got, bad) > BOUND, what


# ------------------------------------------------------------------ 3
# The two training vectors whose length is no multiple of 4 (hypervla.train.train_param_layout): MID with horizon 1, frozen encoder,
# 10604487 elements (% 4 == 3; G % 4 == 3 too: the row pass goes scalar), and MID with horizon 3, trained encoder, 11203157 (% 4 == 1).
EDGE_TOTALS = {"horizon 1, frozen encoder": (dict(horizon=1), False, 10604487), "horizon 3, trained encoder": (dict(horizon=3), True, 11203157)}


def _wide(rng, n):
    """float32 values with exponents over +-20 (|x| from 2^-25 to 2^25) and random signs."""
    return (np.ldexp(rng.uniform(0.5, 1.0, n), rng.integers(-24, 26, n)) * rng.choice([-1.0, 1.0], n)).astype(np.float32)


@pytest.mark.parametrize("case", list(EDGE_TOTALS))
@pytest.mark.parametrize("misaligned", [False, True])
def test_chunk_edges_on_synthetic_vectors(case, misaligned):
    """hvla_train_metrics driven through the binding on vectors of its own (a context without weights).  One chunk of the fixed grid is
    all zeros; `misaligned` shifts every vector by one element, which sends the pass down its scalar path."""
    _need_gpu()
    from hypervla import _native
    from hypervla.config import MID
    kw, enc, total = EDGE_TOTALS[case]
    g, B = dataclasses.replace(MID, **kw), 2
    ctx = _native.Context(g, 0, B)
    try:
        n, G, _, n_hyper = ctx.train_sizes(B, enc)
        assert n == total and n % 4 != 0
        rng = np.random.default_rng(n % 1000)
        chunk = ((n + _native.HVLA_TRAIN_METRICS_WORKGROUPS - 1) // _native.HVLA_TRAIN_METRICS_WORKGROUPS + 3) & ~3
        host = {k: _wide(rng, n) for k in ("grads", "params", "prev")}
        for a in host.values():
            a[5 * chunk:6 * chunk] = 0.0
        frozen = (rng.random(n) < 0.3).astype(np.uint8) if enc else None
        theta = _wide(rng, B * G).reshape(B, G)
        o = 1 if misaligned else 0
        dev = {k: torch.as_tensor(np.concatenate([np.zeros(o, a.dtype), a])).cuda()[o:] for k, a in host.items()}
        dmask = None if frozen is None else torch.as_tensor(frozen).cuda()
        dtheta = torch.as_tensor(np.concatenate([np.zeros(o, np.float32), theta.reshape(-1)])).cuda()[o:]
        assert all((t.data_ptr() % 16 != 0) == misaligned for t in dev.values())
        scratch = torch.empty(_native.HVLA_TRAIN_METRICS_SCRATCH_DOUBLES, dtype=torch.float64, device="cuda")
        out = torch.full((_native.HVLA_METRIC_N,), SENTINEL, device="cuda")
        buf = _native.hvla_train_buffers(params=dev["params"].data_ptr(), grads=dev["grads"].data_ptr(), theta=dtheta.data_ptr())
        ctx.train_frozen(dmask.data_ptr() if enc else 0, n, 0)
        enc_sq_host = 1234.5
        both = _native.HVLA_METRICS_PRE | _native.HVLA_METRICS_UPDATE
        ctx.train_metrics(buf, both, out.data_ptr(), B, enc, scratch.data_ptr(), prev_params_ptr=dev["prev"].data_ptr(),
                          encoder_sqsum=enc_sq_host)
        torch.cuda.synchronize()
        v = _np(out).astype(np.float64)
        _close(v[ref.GRAD_NORM], ref.grad_norm(host["grads"]), "grad_norm")
        _close(v[ref.PARAM_NORM], ref.param_norm(host["params"], frozen), "param_norm")
        _close(v[ref.UPDATE_NORM], ref.update_norm(host["params"], host["prev"]), "update_norm")
        enc_sq = ref.encoder_sqsum(host["params"], n_hyper) if enc else enc_sq_host
        _close(v[ref.BASE_PARAMS_NORM], ref.base_params_norm(theta, enc_sq), "base_params_norm")
        for slot in (ref.TRAINING_LOSS, ref.CONTINUOUS_LOSS, ref.GRIPPER_LOSS, ref.MSE, ref.ATTENTION_ENTROPY, ref.ATTENTION_ALIGNMENT):
            assert v[slot] == SENTINEL, slot                     # inputs NULL: not written
    finally:
        ctx.train_frozen(0, 0, 0)
        ctx.close()


# ------------------------------------------------------------------ 4
def test_reproducible_and_pure(frozen_case):
    from hypervla import _native
    c, ft = frozen_case, frozen_case["ft"]
    names = ("params", "grads", "mu", "nu", "ema", "theta", "dtheta", "work", "loss", "actions", "logits", "sqsum", "wd_mask", "prev_params")
    before = {k: getattr(ft, k).clone() for k in names}
    runs = []
    for select, untouched in ((_native.HVLA_METRICS_PRE, [ref.UPDATE_NORM + 6]),
                              (_native.HVLA_METRICS_UPDATE, [i for i in range(ref.N + 6) if i != ref.UPDATE_NORM + 6])):
        for _ in range(2):
            ft.metric_vec.fill_(SENTINEL)
            ft._select()
            ft._metrics_call(select)
            torch.cuda.synchronize()
            runs.append(ft.metric_vec.clone())
        a, b = runs[-2], runs[-1]
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))                 # identical bits
        assert all(float(a[i]) == SENTINEL for i in untouched), a
        written = [i for i in range(ref.N + 6) if i not in untouched and i not in (ref.ATTENTION_ENTROPY, ref.ATTENTION_ALIGNMENT)]
        assert all(float(a[i]) != SENTINEL for i in written), a
    for k in names:
        assert torch.equal(getattr(ft, k), before[k]), k
    # and the bits are those of the step's own two calls (param_norm aside: the step took it before the update)
    got = torch.where(runs[0] == SENTINEL, runs[2], runs[0]).cpu().numpy().astype(np.float64)
    keep = ~np.isnan(c["vec"])
    keep[ref.PARAM_NORM + 6] = False
    _close(got[ref.PARAM_NORM + 6], ref.param_norm(c["host"]["params"]), "param_norm of the updated parameters")
    ft.metric_vec.copy_(c["vec_dev"])
    assert np.array_equal(got[keep], c["vec"][keep])


# ------------------------------------------------------------------ 5
def test_loss_terms(frozen_case):
    from hypervla.config import generated_leaves
    from oracle import hvla_ref_torch as ot
    c, ft, g, B, h = frozen_case, frozen_case["ft"], frozen_case["g"], frozen_case["B"], frozen_case["host"]
    tgt, am, tm = ft._keep[4], ft._keep[5], ft._keep[6]
    terms = torch.full((3, B), SENTINEL, device="cuda")
    ft.model._ctx.loss_terms(ft.actions.data_ptr(), ft.logits.data_ptr(), tgt.data_ptr(), tm.data_ptr(), am.data_ptr(),
                             terms[0].data_ptr(), terms[1].data_ptr(), terms[2].data_ptr(), B)
    torch.cuda.synchronize()
    cont, grip, sq = (_np(terms[i]) for i in range(3))
    loss = h["loss"]
    print("continuous", cont, "gripper", grip, "loss", loss)
    assert (cont >= 0).all() and (grip >= 0).all()
    assert cont[1] == 0 and grip[1] == 0 and cont[3] == 0 and grip[3] == 0 and loss[1] == 0 and loss[3] == 0     # the 1e-5 floors
    assert (np.abs((cont + grip) - loss) <= 2 * np.spacing(loss)).all(), (cont + grip, loss)      # 2 ulp of the loss
    # against the oracle: float64 context encoder -> theta -> policy on the same tokens, the restatement on its outputs
    leaves = generated_leaves(g)
    params = {k: v for k, v in c["model"].params.items() if not k.startswith("encoder_image_encoder_")}
    hn = ot.HyperNetRef(params, g, leaves, torch.float64)
    li = c["ins"]["language_instruction"]
    theta = hn.generate(hn.context(li["token_embedding"], li["attention_mask"], np.asarray(c["st"]["patch_embeddings"])[:, 0]))
    act, logit, _ = ot.PolicyRef(g, leaves)(theta, torch.as_tensor(c["tok"]).double())
    target = np.asarray(c["batch"]["action"])[:, 0]
    want_c, want_g = ref.loss_terms(act[..., :-1].numpy(), logit.numpy(), target, np.asarray(c["batch"]["timestep_pad_mask"])[:, 0],
                                    np.asarray(c["batch"]["action_pad_mask"])[:, 0], g.max_action, g.clip_target)
    np.testing.assert_allclose(cont, want_c, rtol=LOSS_RTOL, atol=LOSS_ATOL)
    np.testing.assert_allclose(grip, want_g, rtol=LOSS_RTOL, atol=LOSS_ATOL)
    # the squared error and the means: float64 of the device's own outputs
    want_sq = ref.sqerr(h["actions"], target)
    assert (np.abs(target) > 5).any() and want_sq.min() > 0
    assert (np.abs(sq - want_sq) <= BOUND * want_sq).all(), (sq, want_sq)
    v = c["vec"]
    _close(v[ref.MSE], ref.mse(h["actions"], target), "mse")
    _close(v[ref.TRAINING_LOSS], loss.astype(np.float64).mean(), "training_loss")
    _close(v[ref.CONTINUOUS_LOSS], cont.astype(np.float64).mean(), "continuous_loss")
    _close(v[ref.GRIPPER_LOSS], grip.astype(np.float64).mean(), "gripper_loss")
    np.testing.assert_allclose(v[ref.CONTINUOUS_LOSS], want_c.mean(), rtol=LOSS_RTOL, atol=LOSS_ATOL)
    np.testing.assert_allclose(v[ref.GRIPPER_LOSS], want_g.mean(), rtol=LOSS_RTOL, atol=LOSS_ATOL)


# ------------------------------------------------------------------ 6
def test_per_task_losses(frozen_case):
    from hypervla import _native
    from hypervla.train import resolve_task_index
    c, ft, h = frozen_case, frozen_case["ft"], frozen_case["host"]
    L, nt = ref.LOCAL_N, 3
    ids = resolve_task_index(c["index"], c["names"], c["B"])
    assert ids.tolist() == [1, 0, -1, 1, -1] and _np(ft.task_ids).tolist() == ids.tolist()
    sums, counts = ref.task_sums(h["loss"], ids, nt)
    v = c["vec"]
    assert np.array_equal(v[L + nt:L + 2 * nt], counts) and counts.tolist() == [1.0, 2.0, 0.0]
    assert (np.abs(v[L:L + nt] - sums) <= 2.0 ** -24 * np.abs(sums)).all(), (v[L:L + nt], sums)
    assert v[L + 1] > 0 and v[L + 2] == 0
    info = ft.info()
    assert [k for k in info if k.startswith("task_loss_")] == ["task_loss_bridge", "task_loss_fractal", "task_loss_kuka"]
    assert np.isnan(float(info["task_loss_kuka"])) and float(info["task_loss_fractal"]) == np.float32(v[L + 1]) / np.float32(2.0)
    # ids outside [0, n_tasks) are counted nowhere
    keep = ft.task_ids.clone()
    try:
        ft.task_ids.copy_(torch.tensor([0, 7, -3, 0, 1], dtype=torch.int32))
        ft._select()
        ft._metrics_call(_native.HVLA_METRICS_PRE)
        v2 = _vec(ft)
        sums2, counts2 = ref.task_sums(h["loss"], [0, 7, -3, 0, 1], nt)
        assert np.array_equal(v2[L + nt:L + 2 * nt], counts2) and counts2.sum() == 3
        assert (np.abs(v2[L:L + nt] - sums2) <= 2.0 ** -24 * np.abs(sums2)).all()
    finally:
        ft.task_ids.copy_(keep)
        ft.metric_vec.copy_(c["vec_dev"])
        torch.cuda.synchronize()


# ------------------------------------------------------------------ 7
def test_validate_is_pure_and_follows_the_ema():
    _need_gpu()
    from hypervla import synthetic as syn
    from hypervla.config import MID
    from hypervla.model import HyperVLA
    from hypervla.train import FineTuner
    g, B = MID, 3
    model = HyperVLA.from_synthetic(g, max_batch=B)
    ins, st, im = syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g), syn.synthetic_images(B, g)
    batch = syn.synthetic_action_batch(B, g)
    ft = FineTuner(model, B, ema_start_step=0, metrics=True)
    ft.step(ins, st, im, batch, lr=1e-2)                       # moves params; the EMA is 0.999 of where it started
    torch.cuda.synchronize()
    names = ("grads", "mu", "nu", "params", "ema", "loss", "actions", "logits", "metric_vec")
    before = {k: getattr(ft, k).clone() for k in names}
    count, aux = ft.step_count, dict(ft.aux_metrics)
    assert not torch.equal(ft.params, ft.ema) and float(ft.grads.abs().max()) > 0
    plain = ft.validate(ins, st, im, batch)
    on_ema = ft.validate(ins, st, im, batch, ema=True)
    twice = ft.validate_batches([(ins, st, im, batch), (ins, st, im, batch)])
    torch.cuda.synchronize()
    for k in names:
        a, b = getattr(ft, k), before[k]
        assert torch.equal(a.view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32), b.view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32)), k
    assert ft.step_count == count and ft.aux_metrics == aux
    assert set(plain) == {"mse"} and plain["mse"].is_cuda and plain["mse"].dim() == 0
    tokens = model.encode_images(im)
    ft.forward_backward(ins, st, tokens, batch, forward_only=True)
    want = ref.mse(_np(ft.actions), np.asarray(batch["action"])[:, 0])
    assert ref.rel_err(float(plain["mse"]), want) <= BOUND
    assert float(twice["mse"]) == float(plain["mse"])
    assert float(on_ema["mse"]) != float(plain["mse"])
    ft2 = FineTuner(model, B)                                   # no metrics: validate brings its own gradient sink
    ft2.params.copy_(ft.ema)
    g2 = ft2.grads.clone()
    again = ft2.validate(ins, st, im, batch)
    torch.cuda.synchronize()
    assert float(again["mse"]) == float(on_ema["mse"]) and torch.equal(ft2.grads, g2)


# ------------------------------------------------------------------ 8
def test_refusals_leave_out_untouched(frozen_case):
    from hypervla import _native
    ft = frozen_case["ft"]
    ctx, lib = ft.model._ctx, ft.model._ctx.lib
    out = torch.full((ref.N + 6,), SENTINEL, device="cuda")
    ids = torch.zeros(ft.B, dtype=torch.int32, device="cuda")
    size = C.sizeof(_native.hvla_train_metrics_in)

    def call(train_encoder=0, out_ptr=None, **kw):
        f = dict(struct_size=size, select=_native.HVLA_METRICS_PRE, prev_params=ft.prev_params.data_ptr(), n_tasks=0,
                 scratch=ft.metric_scratch.data_ptr())
        f.update(kw)
        opts = _native.hvla_train_metrics_in(**f)
        rc = lib.hvla_train_metrics(ctx.h, C.byref(ft.buf), C.byref(opts), C.c_void_p(out.data_ptr() if out_ptr is None else out_ptr or None),
                                    ft.B, train_encoder, None)
        return rc, lib.hvla_last_error(ctx.h).decode()

    ft._select()
    SHAPE, STATE = -1, -7
    cases = [(dict(struct_size=size - 8), "struct_size"), (dict(struct_size=size + 8), "struct_size"), (dict(struct_size=0), "struct_size"),
             (dict(scratch=None), "null scratch or out"), (dict(out_ptr=0), "null scratch or out"),
             (dict(select=_native.HVLA_METRICS_UPDATE, prev_params=None), "needs prev_params"),
             (dict(select=_native.HVLA_METRICS_PRE | _native.HVLA_METRICS_UPDATE, prev_params=None), "needs prev_params"),
             (dict(select=0), "select"), (dict(select=4), "select"),
             (dict(n_tasks=-1), "n_tasks -1"), (dict(task_ids=ids.data_ptr(), n_tasks=0), "task_ids given with n_tasks == 0")]
    for kw, text in cases:
        rc, msg = call(**kw)
        assert rc == SHAPE and text in msg, (kw, rc, msg)
    rc = lib.hvla_train_metrics(ctx.h, C.byref(ft.buf), None, C.c_void_p(out.data_ptr()), ft.B, 0, None)
    assert rc == STATE
    # a frozen mask set for the other train_encoder value: HVLA_E_STATE, as from hvla_train_apply
    mask = torch.zeros(ft.n, dtype=torch.uint8, device="cuda")
    try:
        ctx.train_frozen(mask.data_ptr(), ft.n, 0)
        rc, msg = call(train_encoder=1)
        assert rc == STATE and "frozen mask was set for train_encoder = 0" in msg, (rc, msg)
        rc, msg = call(train_encoder=0)
        assert rc == 0, msg
    finally:
        ctx.train_frozen(0, 0, 0)
    torch.cuda.synchronize()
    assert float(out[ref.TRAINING_LOSS]) != SENTINEL                         # the one call that was let through wrote
    out.fill_(SENTINEL)
    for kw, text in cases:
        call(**kw)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    # hvla_loss_terms
    with pytest.raises(_native.NativeError, match="null pointer"):
        ctx.loss_terms(ft.actions.data_ptr(), ft.logits.data_ptr(), 0, 0, 0, out.data_ptr(), out.data_ptr(), out.data_ptr(), ft.B)
    with pytest.raises(_native.NativeError, match="batch 0"):
        ctx.loss_terms(ft.actions.data_ptr(), ft.logits.data_ptr(), 1, 1, 1, out.data_ptr(), out.data_ptr(), out.data_ptr(), 0)
    with pytest.raises(ValueError, match="overlap"):
        ft.forward_backward(frozen_case["ins"], frozen_case["st"], frozen_case["tok"], frozen_case["batch"],
                            task_index={"kuka": np.ones(5, bool), "bridge": np.ones(5, bool)})


# ------------------------------------------------------------------ 9
def test_one_pre_call_captured_alone_replays_the_eager_bits(frozen_case):
    from hypervla import _native
    ft = frozen_case["ft"]
    ft._select()
    ft.metric_vec.fill_(SENTINEL)
    ft._metrics_call(_native.HVLA_METRICS_PRE)
    torch.cuda.synchronize()
    eager = ft.metric_vec.clone()
    side = torch.cuda.Stream(ft.model.device)
    with torch.cuda.stream(side):
        ft._metrics_call(_native.HVLA_METRICS_PRE)               # warm the side stream
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):               # one stream, no parallel branch
            ft._metrics_call(_native.HVLA_METRICS_PRE)
    torch.cuda.synchronize()
    for _ in range(2):
        ft.metric_vec.fill_(SENTINEL)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(ft.metric_vec.view(torch.int32), eager.view(torch.int32))
    assert float(eager[ref.UPDATE_NORM + 6]) == SENTINEL and float(eager[ref.GRAD_NORM + 6]) > 0
    ft.metric_vec.copy_(frozen_case["vec_dev"])
