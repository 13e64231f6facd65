"""GPU: vit_kwargs.use_language_token -- lang_prefix_kernel + policy_kernel_lang against the float64
restatement (tests/lang_policy_ref.py), batch and pool invariance, determinism, hipGraph replay, and the ABI's default path."""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CAP = 72                   # pool capacity: room for a >= 64-slot step (the two-stream form)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X; torch.cuda.is_available() is False")


def _geo(name):
    from hypervla import config
    return dataclasses.replace(getattr(config, name), lang_in_policy=True)


def _rows(d, idx):
    return {"language_instruction": {k: np.asarray(v)[idx] for k, v in d["language_instruction"].items()}}


@pytest.fixture(scope="module")
def mid():
    _need_gpu()
    from hypervla import synthetic as syn
    from hypervla.model import HyperVLA
    g = _geo("MID")
    m = HyperVLA.from_synthetic(g, max_batch=CAP, streams=2)
    return dict(g=g, m=m, P=syn.synthetic_params(g), ins=syn.synthetic_instructions(CAP, g),
                st=syn.synthetic_initial_state(CAP, g), im=syn.synthetic_images(CAP, g))


@pytest.fixture(scope="module")
def full():
    _need_gpu()
    from hypervla import synthetic as syn
    from hypervla.model import HyperVLA
    import lang_policy_ref as LR
    g, B = _geo("FULL"), 64
    m = HyperVLA.from_synthetic(g, max_batch=B)
    ins, st = syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g)
    tok = (np.random.default_rng(11).standard_normal((B, g.patches, g.enc_dim))).astype(np.float32)
    bp = LR.create_tasks(m.params, g, ins, st)
    return dict(g=g, m=m, B=B, ins=ins, st=st, tok=tok, bp=bp)


def test_mid_end_to_end_from_images_and_head_maps(mid):
    from hypervla.config import encoder_leaves, generated_leaves
    from oracle import hvla_ref_np as onp
    import lang_policy_ref as LR
    m, g, B = mid["m"], mid["g"], 5
    ins, st, im = _rows(mid["ins"], slice(0, B)), {"patch_embeddings": mid["st"]["patch_embeddings"][:B]}, mid["im"][:B]
    lang = ins["language_instruction"]["token_embedding"]
    w, tasks, _ = m.create_tasks(instruction_dict=ins, initial_state=st)
    act, inter = m.sample_actions(im, ins, tasks, np.ones((B, 1)), w, attention_maps=True)
    bp = LR.create_tasks(mid["P"], g, ins, st)
    theta = w.export()[0].cpu().numpy().astype(np.float64)
    ref = np.concatenate([bp[l.flat_name].reshape(B, -1) for l in generated_leaves(g)], 1)
    assert theta.shape == ref.shape and np.abs(theta - ref).max() <= 1e-4
    ract, rlog, tok = LR.sample_actions(mid["P"], g, dict(encoder_leaves(g)), bp, im, lang)
    d = np.abs(act[..., :6] - ract[..., :6])
    dl = np.abs(inter["gripper_logits"] - rlog)
    print("MID use_language_token end to end: action MAE %.3e max %.3e, logit max %.3e" % (d.mean(), d.max(), dl.max()))
    assert d.mean() <= 5e-4 and d.max() <= 2e-3 and dl.mean() <= 2e-3, (d.mean(), d.max(), dl.mean())
    head = LR.head_attention(bp, g, tok, lang)
    assert inter["head_attention"].shape == head.shape == (B, g.layers, g.heads, g.lang_tokens + g.patches)
    dh = np.abs(inter["head_attention"] - head)
    print("MID head attention [B, L, H, T + P]: max |d| %.2e (max weight %.2e)" % (dh.max(), head.max()))
    assert dh.max() <= 1e-3
    # the flag-off oracle on the same weights is a different model: the language tokens matter
    a0, _, _ = onp.policy({k: v for k, v in bp.items() if "language" not in k and "pos_embedding" not in k} |
                          {"encoder_pos_embedding": bp["encoder_pos_embedding"][:, :, g.lang_tokens:]},
                          dataclasses.replace(g, lang_in_policy=False), tok)
    assert np.abs(a0[..., :6] - ract[..., :6]).max() > 1e-3


@pytest.mark.parametrize("B", [4, 64])
def test_full_from_tokens(full, B):
    import lang_policy_ref as LR
    m, g = full["m"], full["g"]
    ins, st = _rows(full["ins"], slice(0, B)), {"patch_embeddings": full["st"]["patch_embeddings"][:B]}
    w, _, _ = m.create_tasks(instruction_dict=ins, initial_state=st)
    act, logit = m.policy_from_tokens(full["tok"][:B], w)
    act, logit = act.cpu().numpy(), logit.cpu().numpy()
    bp = {k: v[:B] for k, v in full["bp"].items()}
    ract, rlog, _ = LR.policy(bp, g, full["tok"][:B].astype(np.float64), ins["language_instruction"]["token_embedding"])
    d, dl = np.abs(act[..., :6] - ract[..., :6]), np.abs(logit - rlog)
    print("FULL use_language_token B=%d from tokens: action max %.3e MAE %.3e, logit max %.3e" % (B, d.max(), d.mean(), dl.max()))
    assert d.max() <= 1e-3 and dl.max() <= 1.5e-3, (d.max(), dl.max())
    safe = np.abs(rlog) > 2e-3
    assert (act[..., 6][safe] == ract[..., 6][safe]).all()


def test_batch_of_one_rows_equal_the_batch_of_64(full):
    m, B = full["m"], full["B"]
    w, _, _ = m.create_tasks(instruction_dict=full["ins"], initial_state=full["st"])
    act, logit = (t.cpu().numpy() for t in m.policy_from_tokens(full["tok"], w))
    for b in (0, 37, 63):
        w1, _, _ = m.create_tasks(instruction_dict=_rows(full["ins"], slice(b, b + 1)),
                                  initial_state={"patch_embeddings": full["st"]["patch_embeddings"][b:b + 1]})
        a1, l1 = (t.cpu().numpy() for t in m.policy_from_tokens(full["tok"][b:b + 1], w1))
        assert np.array_equal(a1[0], act[b]) and np.array_equal(l1[0], logit[b]), b


def test_run_to_run_determinism(full):
    m = full["m"]
    w, _, _ = m.create_tasks(instruction_dict=full["ins"], initial_state=full["st"])
    first = [t.cpu().numpy() for t in m.policy_from_tokens(full["tok"], w)]
    for _ in range(3):
        w2, _, _ = m.create_tasks(instruction_dict=full["ins"], initial_state=full["st"])
        again = [t.cpu().numpy() for t in m.policy_from_tokens(full["tok"], w2)]
        assert all(np.array_equal(a, b) for a, b in zip(first, again))


def test_padded_t5_positions_change_the_actions(mid):
    """Mirror image of test_padding_tokens_do_not_matter: the hypernetwork ignores padded positions (same weights), the policy
    attends to them (base_vit.py:159-166,207-212)."""
    m, g, B = mid["m"], mid["g"], 4
    ins = _rows(mid["ins"], slice(0, B))
    li = ins["language_instruction"]
    last = g.lang_tokens - 1
    li["attention_mask"] = li["attention_mask"].copy()
    li["attention_mask"][:, last] = 0
    st, im = {"patch_embeddings": mid["st"]["patch_embeddings"][:B]}, mid["im"][:B]
    emb2 = li["token_embedding"].copy()
    emb2[:, last] += 1.0
    ins2 = {"language_instruction": dict(li, token_embedding=emb2)}
    w, t, _ = m.create_tasks(instruction_dict=ins, initial_state=st)
    w2, t2, _ = m.create_tasks(instruction_dict=ins2, initial_state=st)
    assert torch.equal(w.export()[0], w2.export()[0])
    a, _ = m.sample_actions(im, ins, t, None, w)
    a2, _ = m.sample_actions(im, ins2, t2, None, w2)
    assert np.abs(a[..., :6] - a2[..., :6]).max() > 1e-4


def test_pool_scattered_slots_equal_a_full_batch_step(mid):
    """assign_tasks into scattered slots, then a >= 64-slot pooled step (two streams): bitwise the rows of a full-batch step."""
    m, g = mid["m"], mid["g"]
    w, tasks, _ = m.create_tasks(instruction_dict=mid["ins"], initial_state=mid["st"])
    act, inter = m.sample_actions(mid["im"], mid["ins"], tasks, None, w, attention_maps=True)
    perm = np.random.default_rng(4).permutation(CAP).tolist()
    pool = m.create_pool(CAP)
    m.assign_tasks(pool, perm, mid["ins"], mid["st"])             # episode k -> slot perm[k]
    K = 66
    a, it = m.sample_actions(mid["im"][:K], None, None, None, pool, attention_maps=True, slots=perm[:K])
    np.testing.assert_array_equal(a, act[:K])
    for k in ("gripper_logits", "head_attention"):
        np.testing.assert_array_equal(it[k], inter[k][:K])
    s1 = [perm[9]]                                                 # and one slot alone
    a1, _ = m.sample_actions(mid["im"][9:10], None, None, None, pool, slots=s1)
    np.testing.assert_array_equal(a1[0], act[9])


def test_hipgraph_replay_of_a_pooled_step_equals_eager(mid):
    from hypervla import synthetic as syn
    m, g = mid["m"], mid["g"]
    slots = [4, 0, 5, 2]
    K, T = len(slots), 4
    pool = m.create_pool(6)
    m.assign_tasks(pool, slots, _rows(mid["ins"], slice(0, K)), {"patch_embeddings": mid["st"]["patch_embeddings"][:K]})
    dev = m.device
    rng = np.random.default_rng(9)
    frames = [torch.as_tensor(rng.integers(0, 256, (K, g.image_size, g.image_size, 3), dtype=np.uint8)).to(dev) for _ in range(T)]
    img = torch.empty_like(frames[0])
    sd = torch.as_tensor(np.array(slots, np.int32)).to(dev)
    act = torch.empty(K, g.horizon, g.action_dim, device=dev)
    lg = torch.empty(K, g.horizon, device=dev)
    step = lambda: m._ctx.step_slots(pool._h, sd.data_ptr(), K, img.data_ptr(), act.data_ptr(), lg.data_ptr(), m._stream())
    eager = []
    for t in range(T):
        img.copy_(frames[t])
        step()
        torch.cuda.synchronize()
        eager.append(act.clone())
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        step()                                                     # warm-up
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            step()
    for t in range(T):
        img.copy_(frames[t])
        act.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(act, eager[t]), t


def test_create_with_null_options_is_create():
    """hvla_create(cfg) == hvla_create_with(cfg, NULL): the same bytes on the default geometry."""
    _need_gpu()
    from hypervla import _native, synthetic as syn
    from hypervla.config import MID
    from hypervla.model import HyperVLA
    g, B = MID, 3
    ins, st, im = syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g), syn.synthetic_images(B, g)
    outs = []
    lib = _native.load_library()
    orig = lib.hvla_create
    for route in ("create", "create_with"):
        if route == "create_with":
            lib.hvla_create = lambda cfg, dev, h: lib.hvla_create_with(cfg, None, dev, h)
        try:
            m = HyperVLA.from_synthetic(g, max_batch=4)
        finally:
            lib.hvla_create = orig
        w, t, _ = m.create_tasks(instruction_dict=ins, initial_state=st)
        a, inter = m.sample_actions(im, ins, t, None, w, attention_maps=True)
        outs.append((w.export()[0].cpu().numpy(), a, inter["head_attention"]))
        del w, m
    for x, y in zip(*outs):
        assert np.array_equal(x, y)


def test_finetuner_refuses_the_model(mid):
    from hypervla.train import FineTuner
    with pytest.raises(ValueError, match="use_language_token"):
        FineTuner(mid["m"], 4)
    with pytest.raises(Exception, match="HVLA_E_SHAPE"):
        mid["m"]._ctx.train_sizes(4)
