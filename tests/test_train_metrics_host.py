"""CPU: the host side of the training metrics -- the float64 restatements of tests/train_metrics_ref.py against the
oracle and against the reference's literal expressions, the key names of FineTuner.info, task_index -> task_ids, the cross-rank
reduction of the metric vector over gloo, and that metrics=False allocates nothing."""
import ast
import inspect
import os
import socket
import textwrap

import numpy as np
import pytest

import train_metrics_ref as ref
from train_metrics_ref import masked_batch

torch = pytest.importorskip("torch")
import torch.distributed as dist            # noqa: E402
import torch.multiprocessing as mp          # noqa: E402

from hypervla import _native                 # noqa: E402
from hypervla import train as tr             # noqa: E402
from hypervla.config import MID              # noqa: E402


def test_split_terms_sum_to_the_oracle_s_mix_loss():
    from oracle import hvla_ref_torch as ot
    g, B = MID, 5
    rng = np.random.default_rng(3)
    for clip_target in (True, False):
        batch = masked_batch(g, B)
        pred = rng.standard_normal((B, g.horizon, g.action_dim - 1)) * 2.0
        logits = rng.standard_normal((B, g.horizon)) * 4.0
        per, _ = ot.mix_loss(g, torch.as_tensor(pred), torch.as_tensor(logits), batch["action"], batch["timestep_pad_mask"],
                             batch["action_pad_mask"], clip_target=clip_target)
        cont, grip = ref.loss_terms(pred, logits, batch["action"][:, 0], batch["timestep_pad_mask"][:, 0], batch["action_pad_mask"][:, 0],
                                    g.max_action, clip_target)
        assert (cont >= 0).all() and (grip >= 0).all()
        assert cont[1] == 0 and grip[1] == 0 and cont[3] == 0 and grip[3] == 0          # the floor, not 0 / 0
        assert cont[[0, 2, 4]].min() > 0 and grip[[0, 2, 4]].min() > 0
        np.testing.assert_allclose(cont + grip, per.numpy(), rtol=1e-12, atol=1e-12)


def test_mse_restatement_is_the_reference_s_expression():
    rng = np.random.default_rng(4)
    B, H, ad = 5, 4, 7
    predicted = rng.standard_normal((B, 1, H, ad)) * 3.0
    action = rng.standard_normal((B, 1, H, ad)) * 4.0                  # some beyond +-5
    assert (np.abs(action) > 5).any()
    literal = ((predicted - np.clip(action, -5., 5.)) ** 2).mean() * ad            # scripts/train.py:580-581
    assert abs(ref.mse(predicted[:, 0], action[:, 0]) - literal) <= 1e-12 * literal


def test_info_keys_are_the_reference_s():
    """scripts/train.py:506-512 (`info`), action_heads.py:517-521 and scripts/train.py:358, 373, 384 (`metrics`), :525 (tasks)."""
    want = ["training_loss", "grad_norm", "update_norm", "param_norm", "learning_rate", "continuous_loss", "gripper_loss",
            "base_params_norm", "attention_entropy_loss", "attention_alignment_loss"]
    assert list(tr.INFO_KEYS) == want
    names = ("bridge", "fractal")
    vec = torch.arange(_native.HVLA_METRIC_N + 4, dtype=torch.float32)
    info = tr.info_from_vector(vec, names, torch.tensor(3e-4))
    assert list(info) == want + ["task_loss_bridge", "task_loss_fractal"]
    assert float(info["training_loss"]) == ref.TRAINING_LOSS and float(info["grad_norm"]) == ref.GRAD_NORM + 4
    assert float(info["update_norm"]) == ref.UPDATE_NORM + 4 and float(info["base_params_norm"]) == ref.BASE_PARAMS_NORM
    assert info["param_norm"].data_ptr() == vec[ref.PARAM_NORM + 4].data_ptr()      # a view, not a copy
    assert float(info["task_loss_fractal"]) == float(np.float32(8.0) / np.float32(10.0))       # sum slot 8 / count slot 10
    plain = tr.info_from_vector(vec[:_native.HVLA_METRIC_N], (), None, attention_entropy=False, attention_alignment=False)
    assert list(plain) == [k for k in want if k != "learning_rate" and not k.startswith("attention_")]
    assert (_native.HVLA_METRIC_LOCAL_N, _native.HVLA_METRIC_N) == (ref.LOCAL_N, ref.N)


def test_task_index_resolves_to_ids_and_refuses_overlap():
    names = ("bridge", "fractal", "kuka")
    idx = {"fractal": np.array([1, 0, 0, 1, 0], bool), "bridge": np.array([0, 1, 0, 0, 0], bool)}
    ids = tr.resolve_task_index(idx, names, 5)
    assert ids.dtype == np.int32 and ids.tolist() == [1, 0, -1, 1, -1]
    assert tr.resolve_task_index(None, names, 3).tolist() == [-1, -1, -1]
    with pytest.raises(ValueError, match="overlap"):
        tr.resolve_task_index({"fractal": np.array([1, 1, 0], bool), "kuka": np.array([0, 1, 0], bool)}, names, 3)
    with pytest.raises(ValueError, match="task_names"):
        tr.resolve_task_index({"other": np.zeros(3, bool)}, names, 3)
    with pytest.raises(ValueError, match="entries"):
        tr.resolve_task_index({"kuka": np.zeros(4, bool)}, names, 3)
    # a task without a sample: 0 / 0 = NaN, as the reference's psum(sum) / psum(count)
    loss = np.array([1.0, 2.0, 4.0, 8.0, 16.0])
    sums, counts = ref.task_sums(loss, ids, 3)
    assert sums.tolist() == [2.0, 9.0, 0.0] and counts.tolist() == [1.0, 2.0, 0.0]
    vec = torch.zeros(_native.HVLA_METRIC_N + 6)
    vec[ref.LOCAL_N:ref.LOCAL_N + 3] = torch.as_tensor(sums, dtype=torch.float32)
    vec[ref.LOCAL_N + 3:ref.LOCAL_N + 6] = torch.as_tensor(counts, dtype=torch.float32)
    info = tr.info_from_vector(vec, names)
    assert float(info["task_loss_bridge"]) == 2.0 and float(info["task_loss_fractal"]) == 4.5
    assert np.isnan(float(info["task_loss_kuka"]))


def _rank_vector(rank, n_tasks):
    v = torch.arange(_native.HVLA_METRIC_N + 2 * n_tasks, dtype=torch.float32) + 1.0
    return v * (1.0 + rank) if rank else v.clone()


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        n_tasks = 2
        vec = _rank_vector(rank, n_tasks)
        vec[ref.LOCAL_N + 2 * n_tasks:] = torch.tensor([0.1, 0.2, 0.3])           # replicated: equal on both ranks, odd bit patterns
        before = vec.clone()
        out = tr.reduce_info_vector(vec, n_tasks, world)
        q.put((rank, out.data_ptr() == vec.data_ptr(), before.numpy(), out.numpy()))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(120)
def test_reduce_info_vector_over_two_gloo_ranks():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    [p.start() for p in ps]
    got = sorted(q.get(timeout=90) for _ in ps)
    [p.join(30) for p in ps]
    assert all(p.exitcode == 0 for p in ps)
    n_tasks, L = 2, ref.LOCAL_N
    b0, b1 = got[0][2], got[1][2]
    for rank, in_place, before, out in got:
        assert in_place
        np.testing.assert_array_equal(out[:L], ((b0[:L] + b1[:L]) / 2).astype(np.float32))                  # means: averaged
        np.testing.assert_array_equal(out[L:L + 2 * n_tasks], b0[L:L + 2 * n_tasks] + b1[L:L + 2 * n_tasks])  # sums, counts: added
        assert out[L + 2 * n_tasks:].tobytes() == before[L + 2 * n_tasks:].tobytes()                          # replicated: its bytes
    assert (b0[:L] != b1[:L]).all()


def test_metrics_off_builds_no_metric_buffer():
    """By inspection of FineTuner's source (no GPU): __init__ reaches _metrics_setup only under `if self.metrics:`, the metric buffers
    are assigned nowhere else, the snapshot vector is None in __init__, and apply() leaves for the optimizer before any metrics
    call when they are off."""
    tree = ast.parse(textwrap.dedent(inspect.getsource(tr.FineTuner)))
    fns = {f.name: f for f in tree.body[0].body if isinstance(f, ast.FunctionDef)}
    sig = inspect.signature(tr.FineTuner.__init__)
    assert sig.parameters["metrics"].default is False and sig.parameters["task_names"].default == ()
    guarded = [n for n in ast.walk(fns["__init__"]) if isinstance(n, ast.If) and ast.unparse(n.test) == "self.metrics"]
    assert len(guarded) == 1 and "self._metrics_setup()" in ast.unparse(guarded[0].body[0])
    assert ast.unparse(fns["__init__"]).count("_metrics_setup") == 1

    def assigned(fn):
        return {ast.unparse(t) for n in ast.walk(fn) if isinstance(n, ast.Assign) for t in n.targets}
    buffers = {"self.metric_vec", "self.metric_scratch"}
    assert buffers <= assigned(fns["_metrics_setup"]) and "self.prev_params" in assigned(fns["_metrics_setup"])
    for name, fn in fns.items():
        if name != "_metrics_setup":
            assert not buffers & assigned(fn), name
    init_prev = [n for n in ast.walk(fns["__init__"]) if isinstance(n, ast.Assign) and ast.unparse(n.targets[0]) == "self.prev_params"]
    assert [ast.unparse(n.value) for n in init_prev] == ["None"]
    body = fns["apply"].body
    first_if = next(i for i, n in enumerate(body) if isinstance(n, ast.If))
    assert ast.unparse(body[first_if].test) == "not self.metrics" and isinstance(body[first_if].body[0], ast.Return)
    assert "_metrics_call" not in "".join(ast.unparse(n) for n in body[:first_if + 1])
