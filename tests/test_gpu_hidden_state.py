"""GPU: hvla_encode_hidden (`model.encode_initial_image`) -- last_hidden_state WITH the CLS row -- in every encoder regime and at
every geometry edge.  The CLS row is `initial_state["patch_embeddings"][:, 0]`, the one image input of the hypernetwork, and
BatchEvaluator encodes all starting episodes at once: the big-batch regime (image-aligned 256-row tiles, LayerNorm fused into the
residual GEMMs, the B CLS rows in the strided gemm64_kernel launch in front of each big GEMM).  The patch tokens witness the CLS
rows of layers 0 .. L-2 (the CLS token is a key of the next layer's attention); the LAST layer's CLS row -- out-projection, norm2,
fc1, fc2 (an instantiation no earlier layer uses: no LayerNorm follows it), layernorm_kernel<Op, 2> -- is read by nothing but
this output, so it is compared here:

  1. bit for bit with the same image encoded alone, README geometry, on both sides of every kernel choice
  2. with the float64 oracle at every 256-patch edge of tests/geometry_cases.py in the aligned regime (B = 9)
  3. the same at 64 patches, small-batch forms (B = 5) and the 128 x 128 kernels (B = 40)
  4. through create_tasks, as the evaluators use it, at B = 16
  5. (the other opt-in output) the attention maps under streams = 2, batch and pool

Bounds are the `hidden state` line of the table at the top of tests/test_gpu_parity.py (tests/geometry_cases.py HIDDEN_*), not
widened; tests/test_oracle_properties.py checks on the CPU that they see a missing last-layer term.  Every parity case prints its
figures before it asserts (DESIGN.md section 16 records one run)."""
import dataclasses
import gc

import numpy as np
import pytest

from geometry_cases import ENCODER_P64, ENCODER_P256, HIDDEN_BF16_RMS, HIDDEN_F16_MAX, HIDDEN_F16_RMS, _full, _mid

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X; torch.cuda.is_available() is False")


def _rows_that_differ(a, b):
    """For an assertion's message: which of the 1 + P rows of two hidden states differ (row 0 is the CLS row)."""
    rows = torch.nonzero((a != b).any(-1)).flatten().tolist()
    return "rows %s%s differ, max |d| %.2e" % (rows[:8], " ..." if len(rows) > 8 else "", float((a - b).abs().max()))


# ------------------------------------------------------------------------------------------------ 1. batch invariance, bit for bit
# batch sizes: 2, 3, 7 the small-batch forms on both sides of the 64 x 32 switch; 8, 9 the first aligned batch and a ragged last
# block of the small launch; 40 a ragged batch; 86 the small launch's two-workgroups-per-CU instantiation; 256 the persistent grid
# on 256 CUs.  Whichever kernel the plan picks on this device, equality must hold.
INVARIANCE = {
    ("FULL", "f16"): (2, 3, 7, 8, 9, 40, 86, 256),
    ("FULL", "bf16"): (8, 40, 256),
    ("SMALL_E", "f16"): (8, 40, 256),           # two column tiles per image, the last one half wide
}
PROBES = (0, 1, 7, 39, 85, 255)


@pytest.mark.parametrize("geometry,enc_dtype", sorted(INVARIANCE))
def test_hidden_state_of_an_image_is_the_same_bytes_in_every_batch(geometry, enc_dtype):
    """Every probe image's [1 + P, E] hidden state in a batch equals that of the image encoded alone (B = 1: the gemm64c forms),
    the rows behind the CLS row equal hvla_encode's tokens of the same batch, and a permuted batch covers the position."""
    _need_gpu()
    from hypervla import config
    from hypervla import synthetic as syn
    from hypervla.model import HyperVLA
    g = getattr(config, geometry)
    m = HyperVLA.from_synthetic(g, max_batch=256, enc_dtype=enc_dtype)
    im = syn.synthetic_images(256, g)[:, 0]
    alone = {i: m.encode_initial_image(im[i:i + 1]).cpu()[0] for i in PROBES}
    for idx in [list(range(B)) for B in INVARIANCE[geometry, enc_dtype]] + [[39, 0, 255, 0]]:
        x = np.ascontiguousarray(im[idx])
        hid = m.encode_initial_image(x).cpu()
        assert tuple(hid.shape) == (len(idx), g.patches + 1, g.enc_dim) and bool(torch.isfinite(hid).all()), len(idx)
        assert torch.equal(hid[:, 1:], m.encode_images(x).cpu()), len(idx)
        for pos, i in enumerate(idx):
            if i in alone:
                assert torch.equal(hid[pos], alone[i]), ("batch of %d, image %d at %d" % (len(idx), i, pos), _rows_that_differ(hid[pos], alone[i]))


# ------------------------------------------------------------------------------------------------ 2, 3. float64 parity at the edges
# The one case with a CLS-row bound of its own: the project has no max bound under bf16 operands.  The float64 emulation of the
# encoder with every operand site rounded to bf16 and the weight rounding compensated per image
# (`python tests/studies/precision_budget.py --geometry e1024 --episodes 9 --study bias --kind bf16`: this case's geometry, batch
# and inputs) puts the CLS row of the first and last image at max |d| 1.28e-2 against exact float64 (rms 3.65e-3 over the nine rows,
# about three times the patch rows'); the bound is 3 x that, the factor covering what the emulation leaves out, the f32
# accumulation order, as for E1024_BF16_END_TO_END of tests/test_gpu_geometry_contract.py.  Measured on the GPU: max 1.57e-2
# (rms 4.07e-3), 1.23 of the emulation, and the same bytes at B = 1.  (The same emulation in f16: 1.50e-3; measured 1.98e-3.)
E1024_BF16_CLS_ROW_MAX = 3 * 1.28e-2


def _parity(name, g, B, enc_dtype, max_batch, cls_row_max=HIDDEN_F16_MAX, whole=None):
    """encode_initial_image at batch B: images 0 and B - 1 against the float64 oracle and, bit for bit, against the same image
    alone; rows 1 .. P against encode_images of the batch.  Prints the figures, then asserts.  whole: (rms, max) of the whole
    hidden state where the case has tighter bounds than the table's."""
    _need_gpu()
    from hypervla import synthetic as syn
    from hypervla.config import encoder_leaves
    from hypervla.model import HyperVLA
    from oracle import hvla_ref_np as onp
    P = syn.synthetic_params(g)
    m = HyperVLA.from_synthetic(g, params=P, max_batch=max_batch, enc_dtype=enc_dtype)
    im = syn.synthetic_images(B, g)[:, 0]
    ends = [0, B - 1]
    ref = onp.dinov2(P, g, dict(encoder_leaves(g)), onp.normalize_images(im[ends]))
    hid = m.encode_initial_image(im).cpu()
    tok = m.encode_images(im).cpu()
    alone = [m.encode_initial_image(im[i:i + 1]).cpu()[0] for i in ends]
    del m
    gc.collect()
    assert tuple(hid.shape) == (B, g.patches + 1, g.enc_dim) and ref.shape == (2,) + tuple(hid.shape[1:])
    d = hid[ends].numpy().astype(np.float64) - ref
    rms, mx = np.sqrt((d * d).mean()), np.abs(d).max()
    cls_rms, cls_max = np.sqrt((d[:, 0] * d[:, 0]).mean()), np.abs(d[:, 0]).max()
    same = [torch.equal(hid[i], a) for i, a in zip(ends, alone)]
    same_tokens = [torch.equal(hid[i, 1:], a[1:]) for i, a in zip(ends, alone)]
    print("hidden state | %s | B %d %s | hidden rms %.2e max %.2e | CLS row rms %.2e max %.2e | alone: %s"
          % (name, B, enc_dtype, rms, mx, cls_rms, cls_max,
             "same bytes" if all(same) else "DIFFERENT (rows 1 .. P the same: %s)" % all(same_tokens)))
    assert bool(torch.isfinite(hid).all())
    if enc_dtype == "f16":
        assert rms <= HIDDEN_F16_RMS and mx <= HIDDEN_F16_MAX, (rms, mx)
    else:
        assert rms <= HIDDEN_BF16_RMS, rms
    if whole is not None:
        assert rms <= whole[0] and mx <= whole[1], (rms, mx)
    assert cls_max <= cls_row_max, cls_max
    assert torch.equal(hid[:, 1:], tok)
    for i, a in zip(ends, alone):
        assert torch.equal(hid[i], a), (i, _rows_that_differ(hid[i], a))


README_WIDTHS = "README widths"
P256_CASES = {README_WIDTHS: (dict(), "f16"), **ENCODER_P256}


@pytest.mark.parametrize("edge", sorted(P256_CASES))
def test_hidden_state_at_256_patches_in_the_aligned_regime(edge):
    """B = 9: 2313 rows, image-aligned 256-row tiles, the nine CLS rows in the small launch in front of each GEMM (its last
    64-row block ragged); two encoder layers except where the edge says otherwise.  "no encoder layers" is the CLS rows that
    im2col writes plus the final norm.  The README widths also meet the bounds test_hf_torch_dinov2_state_dict_through_the_encoder
    asserts for them at B = 3 (rms 1e-3, max 1e-2)."""
    change, dtype = P256_CASES[edge]
    g = _full(**{**dict(enc_layers=2), **change})
    _parity("full, %s" % edge, g, 9, dtype, 16,
            cls_row_max=E1024_BF16_CLS_ROW_MAX if dtype == "bf16" else HIDDEN_F16_MAX,
            whole=(1e-3, 1e-2) if edge == README_WIDTHS else None)


@pytest.mark.parametrize("B", [5, 40])
@pytest.mark.parametrize("edge", sorted(ENCODER_P64))
def test_hidden_state_at_64_patches(edge, B):
    """B = 5: 325 rows, the small-batch forms; B = 40: 2600 rows, the 128 x 128 kernels, the CLS rows inline with the plain bias
    (P = 64 has no image-aligned tiles)."""
    _parity("mid, %s" % edge, _mid(**ENCODER_P64[edge]), B, "f16", 40)


# ------------------------------------------------------------------------------------------------ 4. the evaluators' conditioning path
def _episodes(ins, idx):
    return {"language_instruction": {k: np.asarray(v)[idx] for k, v in ins["language_instruction"].items()}}


def test_evaluator_conditioning_path_at_sixteen_episodes():
    """BatchEvaluator's start of an episode batch (hypervla/evaluate.py): hidden = encode_initial_image(frames) for all episodes
    at once, create_tasks(initial_state={"patch_embeddings": hidden}), here at the README widths with two encoder layers and
    B = 16 -- the one place where a wrong CLS row at B >= 8 becomes wrong policy weights for every episode.  theta and context
    of the first and last episode equal, bit for bit, those of the episode taken through both calls alone; and theta from the
    device's hidden state is within 5e-3 of theta from the oracle's (test_initial_image_hidden_state's bound, MID at B = 5)."""
    _need_gpu()
    from hypervla import synthetic as syn
    from hypervla.config import FULL, encoder_leaves
    from hypervla.model import HyperVLA
    from oracle import hvla_ref_np as onp
    g, B = dataclasses.replace(FULL, enc_layers=2), 16
    ends = [0, B - 1]
    P = syn.synthetic_params(g)
    m = HyperVLA.from_synthetic(g, params=P, max_batch=B)
    ins, im = syn.synthetic_instructions(B, g), syn.synthetic_images(B, g)
    hidden = m.encode_initial_image(im)
    w, _, _ = m.create_tasks(instruction_dict=ins, initial_state={"patch_embeddings": hidden})
    theta, ctx = (t.clone() for t in w.export())
    assert bool(torch.isfinite(theta).all()) and bool(torch.isfinite(ctx).all())
    for e in ends:
        h1 = m.encode_initial_image(im[e:e + 1])
        w1, _, _ = m.create_tasks(instruction_dict=_episodes(ins, [e]), initial_state={"patch_embeddings": h1})
        th1, cx1 = w1.export()
        assert torch.equal(h1[0], hidden[e]), (e, _rows_that_differ(h1[0].cpu(), hidden[e].cpu()))
        assert torch.equal(cx1[0], ctx[e]) and torch.equal(th1[0], theta[e]), e
    ref = onp.dinov2(P, g, dict(encoder_leaves(g)), onp.normalize_images(im[ends, 0]))
    w_ref, _, _ = m.create_tasks(instruction_dict=_episodes(ins, ends), initial_state={"patch_embeddings": ref.astype(np.float32)})
    d_theta = float((theta[ends] - w_ref.export()[0]).abs().max())
    d_cls = np.abs(hidden[ends, 0].cpu().numpy().astype(np.float64) - ref[:, 0]).max()
    print("hidden state | conditioning path, README widths, 2 layers | B %d f16 | CLS row max %.2e | theta from it against theta "
          "from the oracle's max %.2e" % (B, d_cls, d_theta))
    assert d_cls <= HIDDEN_F16_MAX, d_cls
    assert d_theta <= 5e-3, d_theta


# ------------------------------------------------------------------------------------------------ 5. attention maps under two streams
def test_attention_maps_under_two_streams():
    """hvla_set_attention_outputs with streams = 2 and >= 64 rows: encode_range / policy_range offset the two map outputs by the
    half's first episode.  B = 66 (33 + 33) at the README widths with two encoder layers: both maps, the actions and the gripper
    logits of the two-stream model equal the one-stream model's bit for bit, as a batch step and as 66 slots of a 72-slot pool
    in a permuted slot map; and asking for the maps changes no action bit."""
    _need_gpu()
    from hypervla import synthetic as syn
    from hypervla.config import FULL
    from hypervla.model import HyperVLA
    g, B, CAP = dataclasses.replace(FULL, enc_layers=2), 66, 72
    P = syn.synthetic_params(g)
    ins, st, im = syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g), syn.synthetic_images(B, g)
    keys = ("gripper_logits", "dino_cls_attention", "head_attention")
    m1 = HyperVLA.from_synthetic(g, params=P, max_batch=CAP, streams=1)
    w1, tasks, _ = m1.create_tasks(instruction_dict=ins, initial_state=st)
    a1, i1 = m1.sample_actions(im, ins, tasks, np.ones((B, 1)), w1, attention_maps=True)
    assert i1["dino_cls_attention"].shape == (B, g.enc_layers, g.enc_heads, g.patches)
    assert i1["head_attention"].shape == (B, g.layers, g.heads, g.patches)
    for k in keys[1:]:                                    # softmax weights of the patch keys
        assert np.isfinite(i1[k]).all() and i1[k].min() >= 0.0 and i1[k].sum(-1).max() <= 1.0 + 1e-5, k
    m2 = HyperVLA.from_synthetic(g, params=P, max_batch=CAP, streams=2)
    w2, tasks2, _ = m2.create_tasks(instruction_dict=ins, initial_state=st)
    plain, _ = m2.sample_actions(im, ins, tasks2, np.ones((B, 1)), w2)
    a2, i2 = m2.sample_actions(im, ins, tasks2, np.ones((B, 1)), w2, attention_maps=True)
    np.testing.assert_array_equal(a2, plain)
    np.testing.assert_array_equal(a2, a1)
    for k in keys:
        np.testing.assert_array_equal(i2[k], i1[k], err_msg=k)
    pool = m2.create_pool(CAP)
    S = np.random.default_rng(3).permutation(CAP)[:B].tolist()
    m2.assign_tasks(pool, S, ins, st)                     # task k into slot S[k]: row k of the slot step is episode k
    ap, ip = m2.sample_actions(im, None, None, None, pool, slots=S, attention_maps=True)
    np.testing.assert_array_equal(ap, a1)
    for k in keys:
        np.testing.assert_array_equal(ip[k], i1[k], err_msg="pool, " + k)
