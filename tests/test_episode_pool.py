"""CPU: the episode pool's host side -- the slot-map check every pooled call goes through, and the continuous evaluator
(`BatchEvaluator.run_episodes`) driven by a stand-in model that records what it is asked to do."""
import numpy as np
import pytest


# ------------------------------------------------------------------ check_slots
def test_check_slots_returns_int32():
    from hypervla.pool import check_slots
    s = check_slots([3, 0, 2], 4)
    assert s.dtype == np.int32 and s.tolist() == [3, 0, 2] and s.flags["C_CONTIGUOUS"]
    assert check_slots(np.arange(5, dtype=np.int64)[::-1], 5).tolist() == [4, 3, 2, 1, 0]


@pytest.mark.parametrize("slots,capacity", [([1, 2, 1], 4), ([0, 0], 2)])
def test_check_slots_refuses_duplicates(slots, capacity):
    from hypervla.pool import check_slots
    with pytest.raises(ValueError, match="more than once"):
        check_slots(slots, capacity)


@pytest.mark.parametrize("slots", [[-1], [0, 4], [2**31 - 1], [0, -7, 1]])
def test_check_slots_refuses_values_outside_the_pool(slots):
    from hypervla.pool import check_slots
    with pytest.raises(ValueError, match="outside"):
        check_slots(slots, 4)


def test_check_slots_refuses_empty_oversize_and_malformed_maps():
    from hypervla.pool import check_slots
    with pytest.raises(ValueError, match="empty"):
        check_slots([], 4)
    with pytest.raises(ValueError, match="for a pool of 3"):
        check_slots([0, 1, 2, 3], 3)
    with pytest.raises(ValueError, match="one-dimensional"):
        check_slots([[0, 1]], 4)
    with pytest.raises(TypeError):
        check_slots([0.0, 1.0], 4)
    with pytest.raises(TypeError):
        check_slots([True, False], 4)


# ------------------------------------------------------------------ run_episodes with a stand-in model
class ToyEnv:
    """Seeded frames; an episode ends with success after `goal` steps (the seed comes with each reset)."""

    def __init__(self, index, size=16):
        self.index, self.size, self.seed, self.t, self.goal = index, size, -1, 0, 1

    def reset(self, seed=None, goal=None, **kw):
        self.seed, self.goal, self.t = seed, goal, 0
        return self._frame(), {}

    def _frame(self):
        return np.random.default_rng(1000 * self.seed + self.t).integers(0, 256, (self.size, self.size, 3), dtype=np.uint8)

    def get_language_instruction(self):
        return f"task {self.seed}"

    def step(self, action):
        self.t += 1
        return self._frame(), 0.0, self.t >= self.goal, False, {}


class RecordingModel:
    """What `run_episodes` needs of a HyperVLA, recording every call; actions are a function of (slot, step of its episode)."""

    def __init__(self, size=16):
        from hypervla import synthetic as syn
        from hypervla.config import MID, default_config
        import dataclasses
        self.geometry = dataclasses.replace(MID, image_size=size)
        self.config = default_config(MID)
        self.dataset_statistics = syn.synthetic_dataset_statistics(MID)
        self.calls = []
        self.capacity = None
        self.assigned = {}                 # slot -> instruction now in it

    def _dev(self, a, dtype):
        return np.asarray(a)

    def create_pool(self, capacity):
        self.calls.append(("create_pool", capacity))
        self.capacity = capacity
        return "pool"

    def encode_initial_image(self, frames):
        self.calls.append(("encode_initial_image", len(frames)))
        return np.zeros((len(frames), 2, 4), np.float32)

    def assign_tasks(self, pool, slots, instruction_dict, initial_state):
        from hypervla.pool import check_slots
        s = check_slots(slots, self.capacity)
        ids = instruction_dict["language_instruction"]["ids"]
        assert pool == "pool" and len(ids) == len(s) == len(initial_state["patch_embeddings"])
        self.calls.append(("assign_tasks", s.tolist(), list(ids)))
        for k, i in enumerate(s):
            self.assigned[int(i)] = int(ids[k])
        return {}

    def sample_actions(self, images, instruction_dict, task, pad, base_params, slots=None):
        from hypervla.pool import check_slots
        s = check_slots(slots, self.capacity)
        assert base_params == "pool" and len(images) == len(s)
        self.calls.append(("sample_actions", s.tolist()))
        out = np.zeros((len(s), 4, 7), np.float32)
        out[:, :, 0] = s[:, None]
        return out, {}


GOALS = [3, 1, 4, 2, 5, 2, 3]        # episode n's length (reset_kwargs_for gives it to whichever simulator runs n)


@pytest.fixture(scope="module")
def pooled_run():
    from hypervla.evaluate import BatchEvaluator, DummyVectorEnv
    import functools
    E, N = 3, len(GOALS)
    m = RecordingModel()
    venv = DummyVectorEnv([functools.partial(ToyEnv, i) for i in range(E)], (16, 16, 3))
    ev = BatchEvaluator(m, policy_setup="libero", pred_action_horizon=4, action_ensemble=True)

    def tokenize(instrs):
        return {"ids": np.array([int(s.split()[-1]) for s in instrs])}

    res = ev.run_episodes(venv, tokenize, N, max_steps=10, reset_kwargs_for=lambda n: {"seed": n, "goal": GOALS[n]})
    return m, res, E, N


def test_every_episode_runs_once_in_its_simulator_s_slot(pooled_run):
    m, res, E, N = pooled_run
    assert m.calls[0] == ("create_pool", E)
    assigned = [(slot, ep) for c in m.calls if c[0] == "assign_tasks" for slot, ep in zip(c[1], c[2])]
    assert sorted(ep for _, ep in assigned) == list(range(N))                    # each episode assigned exactly once
    assert res["instructions"] == [f"task {n}" for n in range(N)]
    for slot, ep in assigned:
        assert res["env_index"][ep] == slot                                      # simulator i <-> slot i
    assert res["steps"].tolist() == GOALS and res["success"].all()
    # one encode_initial_image per assign_tasks, of the same episodes
    encs = [c[1] for c in m.calls if c[0] == "encode_initial_image"]
    assert encs == [len(c[1]) for c in m.calls if c[0] == "assign_tasks"]


def test_only_active_slots_are_stepped_and_never_more_than_E(pooled_run):
    m, res, E, N = pooled_run
    active = {}                                                                  # slot -> [episode, steps left]
    for c in m.calls[1:]:
        if c[0] == "assign_tasks":
            for slot, ep in zip(c[1], c[2]):
                assert slot not in active                                        # only a free slot gets a new episode
                active[slot] = [ep, GOALS[ep]]
        elif c[0] == "sample_actions":
            assert sorted(c[1]) == sorted(active) and len(c[1]) <= E             # exactly the running episodes' slots
            for slot in c[1]:
                active[slot][1] -= 1
                if active[slot][1] == 0:
                    del active[slot]
    assert not active


def test_rows_stepped_is_the_sum_of_episode_lengths(pooled_run):
    m, res, E, N = pooled_run
    stepped = sum(len(c[1]) for c in m.calls if c[0] == "sample_actions")
    assert res["rows_stepped"] == stepped == res["steps"].sum() == sum(GOALS)
    waves = -(-N // E)
    assert res["rows_stepped"] < waves * E * max(GOALS)                          # what lockstep waves would have stepped


def test_max_steps_ends_an_episode():
    from hypervla.evaluate import BatchEvaluator, DummyVectorEnv
    import functools
    m = RecordingModel()
    venv = DummyVectorEnv([functools.partial(ToyEnv, i) for i in range(2)], (16, 16, 3))
    ev = BatchEvaluator(m, policy_setup="libero", pred_action_horizon=4, action_ensemble=False)
    res = ev.run_episodes(venv, lambda s: {"ids": np.array([int(x.split()[-1]) for x in s])}, 3, max_steps=2,
                          reset_kwargs_for=lambda n: {"seed": n, "goal": [1, 5, 5][n]})
    assert res["steps"].tolist() == [1, 2, 2] and res["success"].tolist() == [True, False, False]
    assert res["rows_stepped"] == 5
