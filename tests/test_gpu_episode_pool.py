"""GPU: the episode pool (hvla_weights_alloc / hvla_generate_slots / hvla_step_slots / hvla_ensemble_slots).  Every slot is
bitwise the same episode run alone: assigned rows equal a fresh create_tasks, a subset step equals those rows of a full step,
a slot's ensemble restarts when it is reassigned, and the continuous evaluator tells every simulator what the per-episode loop
would have.  Slot maps given to the device are always valid ones (hypervla.pool.check_slots guards the rest, tested on the CPU)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CAP = 72                   # pool capacity: room for a >= 64-slot step (the two-stream form)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X; torch.cuda.is_available() is False")


def _rows(d, idx):
    return {"language_instruction": {k: np.asarray(v)[idx] for k, v in d["language_instruction"].items()}}


@pytest.fixture(scope="module", params=["MID", "FULL"])
def geo(request):
    _need_gpu()
    from hypervla import config, synthetic as syn
    from hypervla.model import HyperVLA
    g = getattr(config, request.param)
    m = HyperVLA.from_synthetic(g, max_batch=CAP)
    ins, st, im = syn.synthetic_instructions(CAP, g), syn.synthetic_initial_state(CAP, g), syn.synthetic_images(CAP, g)
    w, tasks, _ = m.create_tasks(instruction_dict=ins, initial_state=st)
    act, inter = m.sample_actions(im, ins, tasks, None, w, attention_maps=True)
    return dict(name=request.param, g=g, m=m, ins=ins, st=st, im=im, w=w, act=act, inter=inter)


@pytest.mark.parametrize("kind", ["create_pool", "create_tasks"])
def test_assign_tasks_writes_exactly_its_rows(geo, kind):
    from hypervla import synthetic as syn
    m, g = geo["m"], geo["g"]
    cap = 12
    if kind == "create_pool":
        pool = m.create_pool(cap)
    else:
        pool, _, _ = m.create_tasks(instruction_dict=_rows(geo["ins"], slice(0, cap)),
                                    initial_state={"patch_embeddings": geo["st"]["patch_embeddings"][:cap]})
    th0, cx0 = (t.clone() for t in pool.export())
    if kind == "create_pool":
        assert not th0.any() and not cx0.any()                     # empty slots are zero-filled
    S = [9, 2, 5]
    ins, st = syn.synthetic_instructions(3, g, rank=1), syn.synthetic_initial_state(3, g, rank=1)
    m.assign_tasks(pool, S, ins, st)
    th1, cx1 = pool.export()
    fresh, _, _ = m.create_tasks(instruction_dict=ins, initial_state=st)
    thf, cxf = fresh.export()
    assert torch.equal(th1[S], thf) and torch.equal(cx1[S], cxf)
    rest = [i for i in range(cap) if i not in S]
    assert torch.equal(th1[rest], th0[rest]) and torch.equal(cx1[rest], cx0[rest])


def _subset_cases(rng):
    return {"one": [37], "scattered": [70, 3, 41, 12, 58], "permutation": rng.permutation(CAP).tolist(),
            "sixty_six": rng.permutation(CAP)[:66].tolist()}


@pytest.mark.parametrize("case", ["one", "scattered", "permutation", "sixty_six"])
def test_subset_step_equals_those_rows_of_a_full_step(geo, case):
    m, im, w = geo["m"], geo["im"], geo["w"]
    S = _subset_cases(np.random.default_rng(3))[case]
    a, inter = m.sample_actions(im[S], None, None, None, w, attention_maps=True, slots=S)
    np.testing.assert_array_equal(a, geo["act"][S])
    for k in ("gripper_logits", "dino_cls_attention", "head_attention"):
        np.testing.assert_array_equal(inter[k], geo["inter"][k][S])


def test_two_stream_subset_step(geo):
    """hvla_config.streams = 2: a >= 64-slot step runs its halves on two streams, with the slot map split along with them."""
    from hypervla.model import HyperVLA
    m2 = HyperVLA.from_synthetic(geo["g"], max_batch=CAP, streams=2)
    w2, _, _ = m2.create_tasks(instruction_dict=geo["ins"], initial_state=geo["st"])
    S = _subset_cases(np.random.default_rng(3))["sixty_six"]
    a, inter = m2.sample_actions(geo["im"][S], None, None, None, w2, slots=S)
    np.testing.assert_array_equal(a, geo["act"][S])
    np.testing.assert_array_equal(inter["gripper_logits"], geo["inter"]["gripper_logits"][S])


def test_pooled_episode_against_the_oracle():
    """One episode assigned into slot 4 of an empty pool, stepped alone, against the float64 oracle (MID bounds of
    test_gpu_parity.test_sample_actions_end_to_end)."""
    _need_gpu()
    from hypervla import synthetic as syn
    from hypervla.config import MID, encoder_leaves, generated_leaves
    from hypervla.model import HyperVLA
    from oracle import hvla_ref_np as onp
    g = MID
    m = HyperVLA.from_synthetic(g, max_batch=8)
    ins, st, im = syn.synthetic_instructions(1, g, rank=2), syn.synthetic_initial_state(1, g, rank=2), syn.synthetic_images(1, g)
    pool = m.create_pool(8)
    m.assign_tasks(pool, [4], ins, st)
    act, inter = m.sample_actions(im, None, None, None, pool, slots=[4])
    bp, _ = onp.create_tasks(m.params, g, generated_leaves(g), ins, st)
    ref, ref_logit, _, _ = onp.sample_actions(m.params, g, dict(encoder_leaves(g)), bp, im)
    d = np.abs(act[..., :6] - ref[..., :6])
    assert d.mean() <= 5e-4 and d.max() <= 2e-3, (d.mean(), d.max())
    assert np.abs(inter["gripper_logits"] - ref_logit).mean() <= 2e-3


def test_per_slot_ensemble_restarts_with_each_episode():
    """Slots join at different steps -- slots 0 and 3 at t = 0, slot 1 at t = 1, slot 3 reassigned at t = 2 -- and each slot's
    device ensemble equals interface.ActionEnsembler plus the affine un-normalisation of that episode alone."""
    _need_gpu()
    from hypervla import synthetic as syn
    from hypervla.config import MID
    from hypervla.interface import ActionEnsembler, device_unnormalization
    from hypervla.model import HyperVLA
    g = MID
    m = HyperVLA.from_synthetic(g, max_batch=8)
    stats = m.dataset_statistics["bridge_dataset"]["action"]
    dstats = device_unnormalization(stats, "normal")
    pool = m.create_pool(6)
    ins, st = syn.synthetic_instructions(4, g, rank=3), syn.synthetic_initial_state(4, g, rank=3)
    joins = {0: [0, 3], 1: [1], 2: [3]}                    # t -> slots (re)assigned before that step
    ens, active = {}, []
    rng = np.random.default_rng(11)
    nxt = 0
    for t in range(7):
        if t in joins:
            S = joins[t]
            m.assign_tasks(pool, S, _rows(ins, slice(nxt, nxt + len(S))),
                           {"patch_embeddings": st["patch_embeddings"][nxt:nxt + len(S)]})
            nxt += len(S)
            for s in S:
                ens[s] = ActionEnsembler(g.horizon, 0.0)
                if s not in active:
                    active.append(s)
        a = rng.uniform(-2, 2, size=(len(active), g.horizon, g.action_dim)).astype(np.float32)
        out = m.ensemble_actions(pool, a, dstats, active)
        for k, s in enumerate(active):
            un = np.where(stats["mask"], a[k].astype(np.float64) * stats["std"] + stats["mean"], a[k])
            np.testing.assert_allclose(out[k], ens[s].ensemble_action(un), atol=1e-5, err_msg=f"t={t} slot={s}")


# ------------------------------------------------------------------ continuous evaluator
class ToyEnv:
    """test_evaluate_glue's toy simulator with the seed given at every reset; keeps the action log of every episode it ran."""

    def __init__(self, size=96):
        self.size, self.seed, self.t, self.log, self.logs = size, 0, 0, [], {}

    def _frame(self):
        return np.random.default_rng(1000 * self.seed + self.t).integers(0, 256, (self.size, self.size, 3), dtype=np.uint8)

    def reset(self, seed=0, **kw):
        self.seed, self.t, self.log = seed, 0, []
        self.logs[seed] = self.log
        return self._frame(), {"seed": seed}

    def get_language_instruction(self):
        return f"move block {self.seed}"

    def step(self, action):
        self.t += 1
        self.log.append(np.array(action, dtype=np.float64))
        goal, limit = 2 + self.seed % 3, 4
        return self._frame(), float(self.t), self.t >= goal, self.t >= limit, {"t": self.t}

    def get_logs(self):
        return {k: np.array(v) for k, v in self.logs.items()}


def test_continuous_evaluator_equals_one_episode_at_a_time():
    _need_gpu()
    from hypervla.config import MID
    from hypervla.evaluate import BatchEvaluator, ShmemVectorEnv
    from hypervla.interface import InferenceWrapper
    from hypervla.model import HyperVLA
    from hypervla.synthetic import synthetic_instructions
    g, E, N = MID, 3, 7
    m = HyperVLA.from_synthetic(g, max_batch=4)
    base = synthetic_instructions(N, g)["language_instruction"]

    def tokenize(instrs):
        idx = [int(s.split()[-1]) for s in instrs]
        return {k: np.asarray(v)[idx] for k, v in base.items()}

    venv = ShmemVectorEnv([functools.partial(ToyEnv, 96) for _ in range(E)], (96, 96, 3))
    try:
        ev = BatchEvaluator(m, policy_setup="widowx_bridge", pred_action_horizon=g.horizon, action_ensemble=True, crop=True)
        res = ev.run_episodes(venv, tokenize, N, max_steps=10, reset_kwargs_for=lambda n: {"seed": n})
        logs = {}
        for d in venv.call("get_logs"):
            logs.update(d)
    finally:
        venv.close()
    assert sorted(logs) == list(range(N))
    assert res["steps"].tolist() == [2 + n % 3 for n in range(N)] and res["success"].all()
    assert res["rows_stepped"] == res["steps"].sum()
    assert res["instructions"] == [f"move block {n}" for n in range(N)]
    for n in range(N):
        env = ToyEnv(96)
        wr = InferenceWrapper(m, policy_setup="widowx_bridge", horizon=1, pred_action_horizon=g.horizon,
                              image_size=g.image_size, action_ensemble=True, crop=True)
        frame, _ = env.reset(seed=n)
        ins = {"language_instruction": tokenize([env.get_language_instruction()])}
        wr.reset(env.get_language_instruction(), ins, wr.initial_state_from_image(frame))
        done = trunc = False
        while not (done or trunc):
            _, act, _, _, _ = wr.step(frame)
            frame, _, done, trunc, _ = env.step(act)
        np.testing.assert_array_equal(np.array(env.log), logs[n], err_msg=f"episode {n}")
