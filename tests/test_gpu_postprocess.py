"""GPU: post-processing of pool slots on the device (hvla_post_*, hypervla.postprocess.DevicePostprocessor) against one
InferenceWrapper per slot fed the same rows: raw_action and the translation bitwise, the rotation within 1 f32 ulp, the gripper
exactly -- for every policy setup, with and without the temporal ensemble, normal and bounds statistics, a masked and an un-masked
gripper column; mixed setups and scattered slot subsets in one call; the evaluator with postprocess="device" against "host"; and a
hipGraph of hvla_step_slots -> hvla_post_step.  Slot maps given to the device are always valid ones."""
import copy
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SETUPS = ("libero", "widowx_bridge", "google_robot")
DATASETS = ("bridge_dataset", "fractal20220817_data", "libero")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X; torch.cuda.is_available() is False")


@pytest.fixture(scope="module")
def mid():
    _need_gpu()
    from hypervla.config import MID
    from hypervla.model import HyperVLA
    return HyperVLA.from_synthetic(MID, max_batch=64)


def _with_stats(m, kinds, gripper_masked, seed=0):
    """A view of `m` with its own statistics per dataset: the gripper column spans [0, 1] after un-normalisation when masked."""
    rng = np.random.default_rng(seed)
    st = {}
    for d in DATASETS:
        mean = (0.1 * rng.standard_normal(7)).astype(np.float32)
        std = rng.uniform(0.05, 0.5, 7).astype(np.float32)
        p01, p99 = (mean - 2.3 * std).astype(np.float32), (mean + 2.3 * std).astype(np.float32)
        mean[6], std[6], p01[6], p99[6] = 0.5, 0.5, 0.0, 1.0
        st[d] = {"action": {"mean": mean, "std": std, "p01": p01, "p99": p99, "mask": np.array([True] * 6 + [gripper_masked])}}
    v = copy.copy(m)
    v.dataset_statistics = st
    v.config = dict(m.config, dataset_kwargs={"dataset_kwargs_list": [
        {"name": d, "action_proprio_normalization_type": kinds[d]} for d in DATASETS]})
    return v


def _predictions(rng, K, H, gripper_masked):
    """f32 [K, H, 7]: continuous columns ~ N(0, 1); the gripper a random bit per entry (0 / 1 raw, -1 / +1 when it is
    un-normalised to [0, 1]) plus noise, so the ensembled gripper jumps by more than 0.5 often enough for the sticky rule."""
    a = rng.normal(0.0, 1.0, (K, H, 7))
    lo = -1.0 if gripper_masked else 0.0
    a[..., 6] = lo + (1.0 - lo) * rng.integers(0, 2, (K, H)) + rng.normal(0.0, 0.05, (K, H))
    return a.astype(np.float32)


def _compare(raw_d, env_d, raw_h, env_h, what):
    np.testing.assert_array_equal(raw_d, raw_h, err_msg=f"{what}: raw_action")
    np.testing.assert_array_equal(env_d[:, :3], env_h[:, :3], err_msg=f"{what}: translation")
    np.testing.assert_array_max_ulp(env_d[:, 3:6].astype(np.float32), env_h[:, 3:6].astype(np.float32), maxulp=1)
    np.testing.assert_array_equal(env_d[:, 6], env_h[:, 6], err_msg=f"{what}: gripper")


@pytest.mark.parametrize("masked", [False, True], ids=["raw_gripper", "masked_gripper"])
@pytest.mark.parametrize("kind", ["normal", "bounds"])
@pytest.mark.parametrize("ensemble", [True, False], ids=["ensemble", "no_ensemble"])
@pytest.mark.parametrize("setup", SETUPS)
def test_slots_match_one_wrapper_each(mid, setup, ensemble, kind, masked):
    from hypervla.interface import InferenceWrapper
    from hypervla.postprocess import DevicePostprocessor
    S, T, H = 40, 60, mid.geometry.horizon
    m = _with_stats(mid, {d: kind for d in DATASETS}, masked)
    post = DevicePostprocessor(m, S)
    post.assign(range(S), setup, ensemble)
    wr = [InferenceWrapper(m, policy_setup=setup, pred_action_horizon=H, action_ensemble=ensemble) for _ in range(S)]
    rng = np.random.default_rng([SETUPS.index(setup), int(ensemble), int(kind == "bounds"), int(masked)])
    fired = np.zeros(S, int)
    for t in range(T):
        a = _predictions(rng, S, H, masked)
        raw_d, env_d = post.step(a, np.arange(S))
        out = []
        for k in range(S):
            was = wr[k].sticky_action_is_on
            out.append(wr[k].postprocess(a[k]))
            fired[k] += int(wr[k].sticky_action_is_on and not was) if setup == "google_robot" else 0
        _compare(raw_d, env_d, np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), f"t={t}")
    if setup == "google_robot":                # the sticky rule fired, ran its 15 repeats and fired again
        assert fired.max() >= 2, fired


def test_mixed_setups_scattered_subsets_and_reassignment(mid):
    """One post-processor, three setups with their own statistics (bridge: bounds), ensemble on for some slots; every step a random
    permuted subset; slots left out keep their state; a re-assigned slot (possibly to another setup) restarts as a fresh wrapper."""
    from hypervla.interface import InferenceWrapper
    from hypervla.postprocess import DevicePostprocessor
    S, H = 24, mid.geometry.horizon
    m = _with_stats(mid, {"bridge_dataset": "bounds", "fractal20220817_data": "normal", "libero": "normal"}, True, seed=3)
    rng = np.random.default_rng(17)
    post = DevicePostprocessor(m, S)
    setups = [SETUPS[i % 3] for i in range(S)]
    ens = [bool(i % 4) for i in range(S)]
    perm = rng.permutation(S)
    post.assign(perm, [setups[i] for i in perm], [ens[i] for i in perm])

    def fresh(i):
        return InferenceWrapper(m, policy_setup=setups[i], pred_action_horizon=H, action_ensemble=ens[i])

    wr = [fresh(i) for i in range(S)]
    for t in range(50):
        if t in (12, 30, 41):
            re_ = rng.permutation(S)[:5]
            for i in re_:
                setups[i] = SETUPS[rng.integers(3)]
                ens[i] = bool(rng.integers(2))
                wr[i] = fresh(i)
            post.assign(re_, [setups[i] for i in re_], [ens[i] for i in re_])
        ids = rng.permutation(S)[: rng.integers(1, S + 1)]
        a = _predictions(rng, len(ids), H, True)
        raw_d, env_d = post.step(torch.as_tensor(a).to(m.device), torch.as_tensor(ids))
        assert raw_d.dtype == env_d.dtype == torch.float64 and raw_d.is_cuda
        out = [wr[i].postprocess(a[k]) for k, i in enumerate(ids)]
        _compare(raw_d.cpu().numpy(), env_d.cpu().numpy(), np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), f"t={t}")


# ------------------------------------------------------------------ evaluator
class ToyEnv:
    """Frames depend on (seed, t) only, so every driver sees the same observations; it records what it was told to do."""

    def __init__(self, seed=0, size=96, limit=9):
        self.seed, self.size, self.limit, self.t, self.log, self.logs = seed, size, limit, 0, [], {}

    def _frame(self):
        return np.random.default_rng(1000 * self.seed + self.t).integers(0, 256, (self.size, self.size, 3), dtype=np.uint8)

    def reset(self, seed=None, **kw):
        if seed is not None:
            self.seed = seed
        self.t, self.log = 0, []
        self.logs[self.seed] = self.log
        return self._frame(), {"seed": self.seed}

    def get_language_instruction(self):
        return f"move block {self.seed}"

    def step(self, action):
        self.t += 1
        self.log.append(np.array(action, dtype=np.float64))
        return self._frame(), float(self.t), self.t >= 3 + self.seed % 5, self.t >= self.limit, {"t": self.t}

    def get_logs(self):
        return {k: np.array(v) for k, v in self.logs.items()}


def _tokenizer(m, n):
    from hypervla.synthetic import synthetic_instructions
    base = synthetic_instructions(n, m.geometry)["language_instruction"]

    def tokenize(instrs):
        idx = [int(s.split()[-1]) for s in instrs]
        return {k: np.asarray(v)[idx] for k, v in base.items()}
    return tokenize


def _logs_close(dev, host, what):
    assert dev.shape == host.shape, (what, dev.shape, host.shape)
    np.testing.assert_array_equal(dev[:, 6], host[:, 6], err_msg=f"{what}: gripper")
    np.testing.assert_allclose(dev[:, :6], host[:, :6], rtol=0, atol=1e-6, err_msg=what)


def test_run_device_postprocess_equals_host(mid):
    """run(): one setup per simulator with postprocess="device" against a host run of each setup: simulator i tells the same
    story as simulator i of the host run with its setup."""
    from hypervla.evaluate import BatchEvaluator, DummyVectorEnv
    E, H = 3, mid.geometry.horizon
    tok = _tokenizer(mid, E)

    def go(setup, mode):
        venv = DummyVectorEnv([functools.partial(ToyEnv, s) for s in range(E)], (96, 96, 3))
        ev = BatchEvaluator(mid, policy_setup=setup, pred_action_horizon=H, action_ensemble=True, crop=True, postprocess=mode)
        res = ev.run(venv, tok, max_steps=12)
        return res, [e.get_logs()[e.seed] for e in venv.envs]

    mixed = ["google_robot", "libero", "widowx_bridge"]
    dev, dlogs = go(mixed, "device")
    assert set(dev) == {"success", "steps", "instructions", "model_seconds", "sim_seconds", "raw_actions"}
    same, _ = go("libero", "device")
    host_same, _ = go("libero", "host")
    for k in ("success", "steps"):
        np.testing.assert_array_equal(same[k], host_same[k])
    for r_d, r_h in zip(same["raw_actions"], host_same["raw_actions"]):
        np.testing.assert_array_equal(r_d, r_h)
    for i, setup in enumerate(mixed):
        host, hlogs = go(setup, "host")
        assert dev["success"][i] == host["success"][i] and dev["steps"][i] == host["steps"][i]
        _logs_close(dlogs[i], hlogs[i], f"simulator {i} ({setup})")


@pytest.mark.parametrize("setup", ["google_robot", "widowx_bridge"])
def test_run_episodes_device_postprocess_equals_host(mid, setup):
    """run_episodes(): 8 episodes on 3 simulators, slots re-assigned as episodes end."""
    from hypervla.evaluate import BatchEvaluator, DummyVectorEnv
    E, N, H = 3, 8, mid.geometry.horizon
    tok = _tokenizer(mid, N)

    def go(mode):
        venv = DummyVectorEnv([functools.partial(ToyEnv, 0) for _ in range(E)], (96, 96, 3))
        ev = BatchEvaluator(mid, policy_setup=setup, pred_action_horizon=H, action_ensemble=True, postprocess=mode)
        res = ev.run_episodes(venv, tok, N, max_steps=8, reset_kwargs_for=lambda n: {"seed": n})
        logs = {}
        for e in venv.envs:
            logs.update(e.get_logs())
        return res, logs

    dev, dlogs = go("device")
    host, hlogs = go("host")
    for k in ("success", "steps", "env_index", "rows_stepped"):
        np.testing.assert_array_equal(dev[k], host[k])
    assert dev["instructions"] == host["instructions"]
    assert sorted(dlogs) == sorted(hlogs) == list(range(N))
    for n in range(N):
        _logs_close(dlogs[n], hlogs[n], f"episode {n}")


# ------------------------------------------------------------------ hipGraph
def test_hipgraph_step_and_postprocess_replay_matches_eager(mid):
    """hvla_step_slots -> hvla_post_step allocate nothing and do not synchronise: captured once, replayed with new frames in the same
    buffers, the graph gives every step what the eager calls give (the post-processing state advances inside the graph)."""
    from hypervla import synthetic as syn
    from hypervla.postprocess import DevicePostprocessor
    m, g = mid, mid.geometry
    S, T = 6, 8
    slots = [4, 0, 5, 2]
    K = len(slots)
    pool = m.create_pool(S)
    ins, st = syn.synthetic_instructions(K, g, rank=4), syn.synthetic_initial_state(K, g, rank=4)
    m.assign_tasks(pool, slots, ins, st)
    setups = ["google_robot", "libero", "widowx_bridge", "google_robot"]
    posts = [DevicePostprocessor(m, S) for _ in range(2)]
    for p in posts:
        p.assign(slots, setups, [True, True, False, True])
    dev = m.device
    rng = np.random.default_rng(9)
    frames = [torch.as_tensor(rng.integers(0, 256, (K, g.image_size, g.image_size, 3), dtype=np.uint8)).to(dev) for _ in range(T)]
    img = torch.empty_like(frames[0])
    sd = torch.as_tensor(np.array(slots, np.int32)).to(dev)
    act = torch.empty(K, g.horizon, g.action_dim, device=dev)
    lg = torch.empty(K, g.horizon, device=dev)
    raw = torch.empty(K, 7, dtype=torch.float64, device=dev)
    env = torch.empty(K, 7, dtype=torch.float64, device=dev)

    def step(p):
        m._ctx.step_slots(pool._h, sd.data_ptr(), K, img.data_ptr(), act.data_ptr(), lg.data_ptr(), m._stream())
        m._ctx.post_step(p._h, sd.data_ptr(), K, act.data_ptr(), p._table.data_ptr(), len(p._host_rows), raw.data_ptr(),
                         env.data_ptr(), m._stream())

    eager = []
    for t in range(T):
        img.copy_(frames[t])
        step(posts[0])
        torch.cuda.synchronize()
        eager.append((raw.clone(), env.clone()))
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        m._ctx.step_slots(pool._h, sd.data_ptr(), K, img.data_ptr(), act.data_ptr(), lg.data_ptr(), m._stream())   # warm-up
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            step(posts[1])
    for t in range(T):
        img.copy_(frames[t])
        raw.zero_()
        env.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(raw, eager[t][0]) and torch.equal(env, eager[t][1]), f"step {t}"
