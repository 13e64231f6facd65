"""GPU: FineTuner.publish / hvla_train_publish -- the training vector packed on the device into the serving buffers.

Every comparison is bitwise.  The reference is the host packer: a fresh HyperVLA built from unpack_params(vector.cpu()), merged
over the served model's tensors when the encoder is frozen.  Each case also asserts that the outputs DIFFER from those before the
publish, so that a publish that does nothing cannot pass."""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KEYS = ("theta", "context", "tokens", "hidden", "actions", "gripper_logits")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")


def _inputs(g, B):
    from hypervla import synthetic as syn
    return dict(g=g, B=B, ins=syn.synthetic_instructions(B, g), st=syn.synthetic_initial_state(B, g), im=syn.synthetic_images(B, g),
                batch=syn.synthetic_action_batch(B, g))


def _outputs(m, s, hidden=True):
    """What a caller of the serving path sees: theta / context of create_tasks, the encoder's tokens and hidden state, a step."""
    w, _, _ = m.create_tasks(instruction_dict=s["ins"], initial_state=s["st"])
    theta, ctx = w.export()
    img = torch.as_tensor(s["im"]).to(m.device)
    out = dict(theta=theta, context=ctx, tokens=m.encode_images(img))
    if hidden:
        out["hidden"] = m.encode_initial_image(img)
    act, inter = m.sample_actions(img, s["ins"], None, None, w)
    out["actions"], out["gripper_logits"] = act, inter["gripper_logits"]
    torch.cuda.synchronize()
    for k, v in out.items():
        assert torch.isfinite(v).all(), k
    return out


def _fresh(m, vector, train_encoder, **kw):
    """The reference: a new model (its own context, loaded by the host packer) from the tensors unpack_params cuts out of `vector`."""
    from hypervla.model import HyperVLA
    from hypervla.train import unpack_params
    params = dict(m._params)
    params.update(unpack_params(m.geometry, vector.cpu().numpy(), train_encoder))
    return HyperVLA(m.config, params, None, m.dataset_statistics, max_batch=m.max_batch, enc_dtype=m.enc_dtype, **kw)


def _same(a, b, keys):
    for k in keys:
        assert torch.equal(a[k], b[k]), k


def _all_differ(a, b, keys):
    for k in keys:
        assert not torch.equal(a[k], b[k]), k


@pytest.fixture(scope="module")
def mid():
    _need_gpu()
    from hypervla.config import MID
    return _inputs(MID, 4)


def _trained(s, train_encoder=True, steps=3, **kw):
    from hypervla.model import HyperVLA
    from hypervla.train import FineTuner
    m = HyperVLA.from_synthetic(s["g"], max_batch=s["B"], **kw)
    ft = FineTuner(m, s["B"], train_encoder=train_encoder, ema_start_step=0)
    for _ in range(steps):
        ft.step(s["ins"], s["st"], s["im"], s["batch"])
    return m, ft


def test_trained_encoder(mid):
    """Three updates with the encoder trained, then publish(): theta, context, tokens, hidden state, actions and gripper logits are
    the fresh model's, and none is what the model served before.  Weights generated before the publish keep their theta."""
    m, ft = _trained(mid)
    w_old, _, _ = m.create_tasks(instruction_dict=mid["ins"], initial_state=mid["st"])
    theta_old = w_old.export()[0].clone()
    before = _outputs(m, mid)
    assert ft.publish() is None
    after = _outputs(m, mid)
    want = _outputs(_fresh(m, ft.params, True), mid)
    _same(after, want, KEYS)
    _all_differ(after, before, KEYS)
    assert torch.equal(w_old.export()[0], theta_old)
    # host_copy=True: model.params is what is served
    from hypervla.train import pack_params
    assert np.array_equal(pack_params(mid["g"], m.params, True), ft.params.cpu().numpy())
    # audit=True runs the operand-range audit (on the checkpoint's example batch) over the published encoder
    m.example_batch = {"observation": {"image_primary": mid["im"]}}
    sites = ft.publish(audit=True)
    assert set(sites) == {"layernorm_out", "qkv", "attention_out", "gelu_out"} and sites == m.operand_range


def test_frozen_encoder(mid):
    """train_encoder=False: theta and actions are the fresh model's; the image encoder's buffers are not touched."""
    m, ft = _trained(mid, train_encoder=False)
    before = _outputs(m, mid)
    ft.publish()
    after = _outputs(m, mid)
    want = _outputs(_fresh(m, ft.params, False), mid)
    _same(after, want, KEYS)
    _all_differ(after, before, ("theta", "context", "actions", "gripper_logits"))
    assert torch.equal(after["tokens"], before["tokens"]) and torch.equal(after["hidden"], before["hidden"])


def test_ema(mid):
    """publish(ema=True) serves the moving average, which is not the parameters."""
    m, ft = _trained(mid)
    assert not torch.equal(ft.ema, ft.params)
    ft.publish(ema=True)
    ema = _outputs(m, mid)
    _same(ema, _outputs(_fresh(m, ft.ema, True), mid), KEYS)
    ft.publish(ema=False)
    _all_differ(_outputs(m, mid), ema, KEYS)


def test_bf16_encoder(mid):
    """enc_dtype="bf16": the encoder's matrices, residues and patch embedding are rounded to bfloat16."""
    m, ft = _trained(mid, enc_dtype="bf16")
    before = _outputs(m, mid)
    ft.publish()
    after = _outputs(m, mid)
    keys = ("tokens", "hidden", "actions", "gripper_logits")
    _same(after, _outputs(_fresh(m, ft.params, True), mid), keys)
    _all_differ(after, before, keys)


@pytest.mark.parametrize("enc_dtype", ["f16", "bf16"])
def test_rounding_edge_values(mid, enc_dtype):
    """Blocks of +-(2m+1) 2^-e (tests/publish_edge_values.py: exact binary16 ties, exact bfloat16 ties, ties that appear only after
    the hi part is subtracted, magnitudes 2^-27 .. 2^2 -- binary16 subnormals and values that round to zero -- and +-0; nothing
    overflows) in layer 0's query and fc1 kernels, one output head, and the patch kernel.  The packed vector is published as it is,
    without a training step, into a model that served the plain synthetic weights.  tests/test_publish_host.py asserts that the value
    set holds these cases."""
    from hypervla import synthetic as syn
    from hypervla.model import HyperVLA
    from hypervla.train import FineTuner, pack_params
    from publish_edge_values import overwrite_edge_blocks
    g = mid["g"]
    edge = overwrite_edge_blocks(syn.synthetic_params(g), g)
    m = HyperVLA.from_synthetic(g, max_batch=mid["B"], enc_dtype=enc_dtype)
    ft = FineTuner(m, mid["B"], train_encoder=True)
    before = _outputs(m, mid)
    ft.params.copy_(torch.as_tensor(pack_params(g, edge, True)))
    ft.publish()
    after = _outputs(m, mid)
    want = _outputs(HyperVLA(m.config, edge, None, m.dataset_statistics, max_batch=mid["B"], enc_dtype=enc_dtype), mid)
    _same(after, want, KEYS)
    _all_differ(after, before, ("theta", "tokens", "hidden", "actions", "gripper_logits"))


def test_readme_geometry():
    """README geometry, B = 2: theta reaches the 201 500-column tail and every fragment tile, the encoder every layer and both
    rectangular matrix shapes.  The parameters are perturbed on the device by 1e-3 of each element's magnitude."""
    _need_gpu()
    from hypervla.config import FULL
    from hypervla.model import HyperVLA
    from hypervla.train import FineTuner
    s = _inputs(FULL, 2)
    m = HyperVLA.from_synthetic(FULL, max_batch=2)
    ft = FineTuner(m, 2, train_encoder=True)
    before = _outputs(m, s, hidden=False)
    gen = torch.Generator(device=m.device).manual_seed(20)
    ft.params.mul_(1.0 + 1e-3 * torch.randn(ft.params.shape, generator=gen, device=m.device))
    ft.publish(host_copy=False)
    after = _outputs(m, s, hidden=False)
    want = _outputs(_fresh(m, ft.params, True), s, hidden=False)
    keys = ("theta", "context", "tokens", "actions", "gripper_logits")
    _same(after, want, keys)
    _all_differ(after, before, keys)


def test_captured_graph_sees_the_published_weights(mid):
    """A step captured on one stream before the publish replays with the new weights: no buffer moved.  create_tasks is redone
    after the publish on both sides (into the captured arena with assign_tasks: weights generated earlier keep their values)."""
    m, ft = _trained(mid)
    g, B, dev = mid["g"], mid["B"], m.device
    w, _, _ = m.create_tasks(instruction_dict=mid["ins"], initial_state=mid["st"])
    img = torch.as_tensor(mid["im"][:, 0]).to(dev).contiguous()
    act = torch.empty(B, g.horizon, g.action_dim, device=dev)
    lg = torch.empty(B, g.horizon, device=dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        m._ctx.step(w._h, img.data_ptr(), act.data_ptr(), lg.data_ptr(), B, m._stream())
        side.synchronize()
        old = act.clone()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            m._ctx.step(w._h, img.data_ptr(), act.data_ptr(), lg.data_ptr(), B, m._stream())
    torch.cuda.synchronize()
    ft.publish()
    m.assign_tasks(w, list(range(B)), instruction_dict=mid["ins"], initial_state=mid["st"])
    torch.cuda.synchronize()
    act.zero_()
    lg.zero_()
    graph.replay()
    torch.cuda.synchronize()
    want = _outputs(_fresh(m, ft.params, True), mid)
    assert torch.equal(act, want["actions"]) and torch.equal(lg, want["gripper_logits"])
    assert not torch.equal(act, old)


def test_refusals(mid, tmp_path):
    from hypervla import _native
    from hypervla.model import HyperVLA
    from hypervla.train import FineTuner
    g, B = mid["g"], mid["B"]
    m = HyperVLA.from_synthetic(g, max_batch=B)
    ft = FineTuner(m, B, train_encoder=True)
    before = _outputs(m, mid)
    with pytest.raises(_native.NativeError, match="HVLA_E_SHAPE"):
        m._ctx.train_publish(ft.params.data_ptr(), ft.n + 1, True, m._stream())
    with pytest.raises(_native.NativeError, match="HVLA_E_SHAPE"):
        m._ctx.train_publish(ft.params.data_ptr(), ft.n, False, m._stream())        # the vector with the encoder, the flag without
    with pytest.raises(_native.NativeError, match="HVLA_E_SHAPE"):
        m._ctx.train_publish(0, ft.n, True, m._stream())
    lang = HyperVLA.from_synthetic(dataclasses.replace(g, lang_in_policy=True), max_batch=B)
    with pytest.raises(_native.NativeError, match="HVLA_E_SHAPE"):
        lang._ctx.train_publish(ft.params.data_ptr(), ft.n, True, lang._stream())
    _same(_outputs(m, mid), before, KEYS)                                            # a refusal launches nothing
    # a context without weights: HVLA_E_STATE
    bare = _native.Context(g, 0, B)
    with pytest.raises(_native.NativeError, match="HVLA_E_STATE"):
        bare.train_publish(ft.params.data_ptr(), ft.n, True, m._stream())
    # host_copy=False: the host tensors are stale, and the model says so
    ft.publish(host_copy=False)
    with pytest.raises(RuntimeError, match=r"publish\(host_copy=True\)"):
        m.save_pretrained(0, str(tmp_path / "ckpt"))
    with pytest.raises(RuntimeError, match=r"publish\(host_copy=True\)"):
        m.params
    ft.publish(host_copy=True)
    m.save_pretrained(0, str(tmp_path / "ckpt"))
    with np.load(tmp_path / "ckpt" / "params_0.npz") as z:
        assert set(z.files) == set(m.params)


def test_load_refuses_an_incomplete_checkpoint_and_serves_after_a_complete_one():
    """hvla_load_weights with one encoder tensor missing names it (HVLA_E_WEIGHTS) and leaves the context without weights
    (hvla_generate: HVLA_E_STATE); the complete set loaded into the same context afterwards serves, bit for bit, what a model that
    never saw the failure serves."""
    _need_gpu()
    from hypervla import _native
    from hypervla import synthetic as syn
    from hypervla.config import MID, hypernet_param_shapes
    from hypervla.model import HyperVLA
    s = _inputs(MID, 2)
    P = syn.synthetic_params(MID)
    want = _outputs(HyperVLA.from_synthetic(MID, params=P, max_batch=2), s)
    params = {k: P[k] for k in hypernet_param_shapes(MID)}
    gone = "encoder_image_encoder_encoder_layer_1_mlp_fc1_bias"
    assert gone in params
    ctx = _native.Context(MID, 0, 2)
    with pytest.raises(_native.NativeError, match="HVLA_E_WEIGHTS") as e:
        ctx.load_weights({k: v for k, v in params.items() if k != gone})
    assert f"checkpoint tensor {gone} (absent)" in str(e.value)
    dev = torch.device("cuda", 0)
    tok = torch.zeros(1, MID.lang_tokens, MID.lang_dim, device=dev)
    mask = torch.ones(1, MID.lang_tokens, dtype=torch.int64, device=dev)
    cls = torch.zeros(1, MID.enc_dim, device=dev)
    with pytest.raises(_native.NativeError, match="HVLA_E_STATE"):
        ctx.generate(tok.data_ptr(), mask.data_ptr(), cls.data_ptr(), 1)
    ctx.load_weights(params)
    m = HyperVLA.from_synthetic(MID, params=P, max_batch=2)
    m._ctx.close()
    m._ctx = ctx                                       # the model now serves from the context whose first load failed
    _same(_outputs(m, s), want, KEYS)
