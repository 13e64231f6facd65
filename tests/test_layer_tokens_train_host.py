"""CPU: the host side of fine-tuning share_layer_index=False models -- the training vector's run table and head
columns (hypervla.train against csrc/train_layout.h, the latter under ASan / UBSan), the names pack_params / unpack_params use, the
weight-decay and frozen_keys masks, train_refusal's four-argument form, the torch oracle against the numpy restatement, the traced
step (three grouped launches, NL B rows through the final LayerNorm, every operand inside the plan) and the conditions on the GPU
cases' inputs, which tests/test_gpu_layer_tokens_train.py runs on the device."""
import dataclasses
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import layer_tokens_ref as LR
import layer_tokens_torch as LTT
import test_train_workspace_extents as X
from hypervla import synthetic as syn
from hypervla.config import FULL, MID, generated_leaves, hypernet_param_shapes, token_of
from hypervla.train import (frozen_plan, gradient_buckets, head_columns, pack_params, token_runs, train_param_layout, unpack_params,
                            weight_decay_mask)
from train_parity import assert_not_vacuous

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hyper-vla_amd", "csrc")


def _geo(shared=False, base=MID, **kw):
    return dataclasses.replace(base, layer_tokens=True, shared_block_heads=shared, **kw)


# name -> geometry of the native check's cases (tests/native/layer_tokens_train_check.cpp), with and without shared heads
NATIVE = {"MID": dict(), "README": dict(base=FULL), "LANG": dict(lang_in_policy=True), "DIFF": dict(differential=True),
          "L11": dict(layers=11), "S48": dict(layers=4, lang_tokens=38)}


# ---------------------------------------------------------------------------------------------- 1. run table, Gh
@pytest.mark.parametrize("shared", [False, True], ids=["own_heads", "shared_heads"])
@pytest.mark.parametrize("case", sorted(NATIVE))
def test_run_table(case, shared):
    """NL - 1 runs, each contiguous in theta, tiling [0, G); their head columns tile [0, Gh) once without shared heads and the block
    range L times with them; every leaf lies inside the run of its token; Gh is the number of floats of the checkpoint's heads."""
    g = _geo(shared, **NATIVE[case])
    leaves = generated_leaves(g)
    G = leaves[-1].offset + leaves[-1].size
    runs = token_runs(g)
    cols, Gh = head_columns(g)
    assert len(runs) == g.num_layer_tokens - 1
    assert [r[0] for r in runs] == [0] + list(np.cumsum([r[1] for r in runs]))[:-1] and sum(r[1] for r in runs) == G
    assert sorted(r[3] for r in runs) == list(range(1, g.num_layer_tokens))            # every token but 0, once
    cover = np.zeros(Gh, int)
    for t, w, h, _ in runs:
        cover[h:h + w] += 1
    block = [r for r in runs if r[3] == token_of(g, ("encoder", "Transformer_0", "encoderblock_0", "x"))][0]
    want = np.ones(Gh, int)
    if shared:
        want[block[2]:block[2] + block[1]] = g.layers
        assert Gh == G - (g.layers - 1) * block[1]
    else:
        assert Gh == G
    assert (cover == want).all()
    for lf, _, h in cols:
        r = [r for r in runs if r[0] <= lf.offset < r[0] + r[1]][0]
        assert r[3] == token_of(g, lf) and h - r[2] == lf.offset - r[0] and lf.offset + lf.size <= r[0] + r[1]
    shapes = hypernet_param_shapes(g)
    assert Gh == sum(int(np.prod(s)) for k, s in shapes.items() if k.startswith("output_head_") and k.endswith("/bias"))
    order = ["action_head", "encoder_norm"] + ["encoderblock"] * g.layers
    names = [[lf.flat_name for lf, _, _ in cols if r[0] <= lf.offset < r[0] + r[1]][0] for r in runs]
    assert all(o in n for o, n in zip(order, names)) and "pos_embedding" in names[-1], names


def test_string_order_of_an_eleven_layer_policy():
    """encoderblock_10 sorts before encoderblock_2: its run reads token 4, encoderblock_2's token 5."""
    g = _geo(layers=11)
    runs = token_runs(g)
    by_block = {}
    for lf in generated_leaves(g):
        if "encoderblock_" in lf.flat_name:
            l = int(lf.flat_name.split("encoderblock_")[1].split("_")[0])
            by_block[l] = [r for r in runs if r[0] <= lf.offset < r[0] + r[1]][0][3]
    assert by_block[10] == 4 and by_block[2] == 5 and by_block[0] == 2 and by_block[1] == 3 and by_block[9] == 12


# ---------------------------------------------------------------------------------------------- 2. names and masks
@pytest.mark.parametrize("shared", [False, True], ids=["own_heads", "shared_heads"])
@pytest.mark.parametrize("kw", [dict(), dict(differential=True), dict(lang_in_policy=True)], ids=["mid", "differential", "language"])
def test_pack_and_unpack_round_trip_a_checkpoint(kw, shared):
    """A convert_checkpoint-shaped dict goes in and comes out: every hypernetwork tensor of hypernet_param_shapes, a shared head once
    under its `encoderblock` name; the layout is csrc/train_layout.h's (held to it below)."""
    g = _geo(shared, **kw)
    P = {k: v for k, v in syn.synthetic_params(g).items() if not k.startswith("encoder_image_encoder_")}
    assert set(P) == {k for k in hypernet_param_shapes(g) if not k.startswith("encoder_image_encoder_")}
    flat = pack_params(g, P)
    layout, total = train_param_layout(g)
    assert flat.shape == (total,)
    back = unpack_params(g, flat)
    assert set(back) == set(P)
    for k in P:
        assert back[k].shape == P[k].shape and (back[k] == P[k]).all(), k
    if shared:
        assert any("encoderblock_MlpBlock" in k for k in back) and not any("encoderblock_0_" in k for k in back if k.startswith("output_head_"))
    # every element of the vector belongs to exactly one tensor: a vector of its own indices unpacks to disjoint ranges
    idx = unpack_params(g, np.arange(total, dtype=np.float64))
    allv = np.concatenate([v.reshape(-1) for v in idx.values()])
    assert allv.size == total and np.unique(allv).size == total
    at = dict((n, (o, s)) for n, o, s in layout)
    assert at["layer_pos_embedding"][1] == (1, g.num_layer_tokens, g.ctx_dim)
    assert at["W_cat"][1] == (g.ctx_dim, head_columns(g)[1])


def test_masks_land_on_the_heads_and_a_shared_head_is_frozen_once():
    g = _geo(True)
    layout, total = train_param_layout(g)
    at = dict((n, o) for n, o, _ in layout)
    cols, Gh = head_columns(g)
    C = g.ctx_dim
    wd = weight_decay_mask(g, "v5")
    w = wd[at["W_cat"]:at["W_cat"] + C * Gh].reshape(C, Gh)
    b = wd[at["b_cat"]:at["b_cat"] + Gh]
    for lf, _, h in cols:
        want = int("kernel" in lf.flat_name)
        assert (w[:, h:h + lf.size] == want).all() and (b[h:h + lf.size] == want).all(), lf.flat_name
    assert wd[at["layer_pos_embedding"]:at["layer_pos_embedding"] + g.num_layer_tokens * C].sum() == 0
    # frozen_keys: the shared MLP heads, kernel and bias -- one range of columns each, whichever block's leaf names it
    mask, flags = frozen_plan(g, ("output_head_*encoderblock_MlpBlock_0_Dense_0_kernel.*",))
    w = mask[at["W_cat"]:at["W_cat"] + C * Gh].reshape(C, Gh)
    b = mask[at["b_cat"]:at["b_cat"] + Gh]
    hit = [(lf, h) for lf, name, h in cols if name.endswith("encoderblock_MlpBlock_0_Dense_0_kernel")]
    assert len(hit) == g.layers and len({h for _, h in hit}) == 1
    lf, h = hit[0]
    assert w[:, h:h + lf.size].all() and b[h:h + lf.size].all() and flags == 0
    assert int(mask.sum()) == (C + 1) * lf.size                                      # frozen once, and nothing else
    # every head frozen: bucket 1 as a whole; the buckets are [context encoder | heads | DINOv2] and end where the layout ends
    mask, flags = frozen_plan(g, ("output_head_*",))
    assert flags == 2 and int(mask.sum()) == (C + 1) * Gh
    bk = {n: (o, c) for n, o, c in gradient_buckets(g)}
    assert bk["context_encoder"] == (0, at["W_cat"]) and bk["output_heads"] == (at["W_cat"], (C + 1) * Gh) and sum(c for _, c in bk.values()) == total
    # an own-heads model freezes L ranges under the same pattern of block names
    g2 = _geo(False)
    m2, _ = frozen_plan(g2, ("output_head_*_MlpBlock_0_Dense_0_kernel.*",))
    assert int(m2.sum()) == g2.layers * (C + 1) * lf.size


# ---------------------------------------------------------------------------------------------- 3. the C++ layout and refusals
@pytest.fixture(scope="module")
def native(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    d = tmp_path_factory.mktemp("layer_tokens_train_check")
    exe = d / "layer_tokens_train_check"
    build = subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
         "-I", CSRC, os.path.join(ROOT, "tests", "native", "layer_tokens_train_check.cpp"), "-o", str(exe)],
        capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.rstrip().endswith("OK"), run.stdout[-2000:] + run.stderr[-2000:]
    return run.stdout.splitlines()


def test_refusal_matrix_and_tiles_under_asan_ubsan(native):
    """train_refusal(g, language_tokens, differential, layer_tokens) for the 12 geometries x 8 switch settings, the layouts' extents
    and the bounds of every tile of the three grouped products (the program checks them; here: that it covered the matrix)."""
    assert sum(ln.startswith("REFUSAL ") for ln in native) == 12
    assert sum(ln.startswith("LAYOUT ") for ln in native) == 2 * len(NATIVE)


@pytest.mark.parametrize("shared", [False, True], ids=["own_heads", "shared_heads"])
@pytest.mark.parametrize("case", sorted(NATIVE))
def test_python_and_cxx_agree_on_runs_and_layout(native, case, shared):
    g = _geo(shared, **NATIVE[case])
    name = case + ("-shared" if shared else "")
    runs = [tuple(int(x) for x in ln.split()[2:]) for ln in native if ln.startswith("RUN %s " % name)]
    assert runs == token_runs(g)
    lay = [ln.split()[2:] for ln in native if ln.startswith("LAYOUT %s " % name)]
    assert len(lay) == 1
    NL, G, Gh, total, pos_layer, wcat, bcat = (int(x) for x in lay[0])
    layout, n = train_param_layout(g)
    at = dict((k, o) for k, o, _ in layout)
    leaves = generated_leaves(g)
    assert (NL, G, Gh, total) == (g.num_layer_tokens, leaves[-1].offset + leaves[-1].size, head_columns(g)[1], n)
    assert (pos_layer, wcat, bcat) == (at["layer_pos_embedding"], at["W_cat"], at["b_cat"])


# ---------------------------------------------------------------------------------------------- 4. the oracle
@pytest.mark.parametrize("shared", [False, True], ids=["own_heads", "shared_heads"])
def test_the_torch_forward_is_the_numpy_restatement(shared):
    """Context and theta of tests/layer_tokens_torch.py against tests/layer_tokens_ref.py on MID to 1e-12."""
    g, B = _geo(shared), 3
    P = syn.synthetic_params(g)
    ins, st = syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g)
    _, rctx, rtheta = LR.create_tasks(P, g, ins, st)
    ctx, theta = LTT.forward(P, g, generated_leaves(g), ins, st)
    assert ctx.shape == rctx.shape and theta.shape == rtheta.shape
    assert np.abs(ctx.numpy() - rctx).max() <= 1e-12 and np.abs(theta.numpy() - rtheta).max() <= 1e-12


def gpu_case(name):
    """The inputs of tests/test_gpu_layer_tokens_train.py's parity cases: (g, B, train_encoder)."""
    return {"own": (_geo(False), 5, False), "shared": (_geo(True), 5, False),
            "language": (_geo(False, lang_in_policy=True), 5, False),
            "differential": (_geo(True, differential=True), 5, False),
            "s48": (_geo(True, layers=4, lang_tokens=38), 3, False),
            "readme": (_geo(True, base=FULL), 2, False),
            "mid_enc": (_geo(False), 2, True)}[name]


def case_inputs(name):
    """(g, B, enc, params, ins, st, x, batch): x = tokens [B, P, E] (encoder frozen) or uint8 images (trained); the seeded inputs of
    tests/train_parity.py's two cases."""
    g, B, enc = gpu_case(name)
    params = syn.synthetic_params(g)
    ins, st = syn.synthetic_instructions(B, g), syn.synthetic_initial_state(B, g)
    batch = syn.synthetic_action_batch(B, g)
    x = syn.synthetic_images(B, g) if enc else np.random.default_rng(9).standard_normal((B, g.patches, g.enc_dim)).astype(np.float32)
    return g, B, enc, params, ins, st, x, batch


def case_reference(name, keep=None):
    from hypervla.config import encoder_leaves
    g, B, enc, params, ins, st, x, batch = case_inputs(name)
    if enc:
        return LTT.train_loss_and_grads(params, g, generated_leaves(g), ins, st, None, batch, images=x, enc_shapes=dict(encoder_leaves(g)),
                                        keep_theta=keep)
    p = {k: v for k, v in params.items() if not k.startswith("encoder_image_encoder_")}
    return LTT.train_loss_and_grads(p, g, generated_leaves(g), ins, st, x, batch, keep_theta=keep)


@pytest.mark.parametrize("name", ["own", "shared", "language", "differential", "s48", "readme", "mid_enc"])
def test_the_oracle_alone_is_not_vacuous_on_the_gpu_cases(name):
    """train_parity.assert_not_vacuous on the oracle's gradients for every input the GPU test uses; token 0's row of layer_pos_embedding
    has gradient exactly 0 (nobody attends it, no leaf reads it) and every other row has not; a shared head is in the dict once."""
    g, B, enc = gpu_case(name)
    keep = {}
    per, loss, grads = case_reference(name, keep)
    above, n = assert_not_vacuous(grads, enc)
    lp = grads["layer_pos_embedding"].numpy()
    assert lp.shape == (1, g.num_layer_tokens, g.ctx_dim) and (lp[0, 0] == 0).all() and (np.abs(lp[0, 1:]).max(1) > 0).all()
    assert (keep["dctx"].numpy()[:, 0] == 0).all()
    heads = {k for k in grads if k.startswith("output_head_")}
    assert heads == {k for k in hypernet_param_shapes(g) if k.startswith("output_head_")}
    print("%s: %d of %d leaves above the floor, loss %.3f .. %.3f" % (name, above, n, float(per.min()), float(per.max())))


# ---------------------------------------------------------------------------------------------- 5. the traced step
@pytest.fixture(scope="module")
def traced(tmp_path_factory):
    if not os.path.exists(X.HIPCC):
        pytest.skip("needs hipcc")
    d = tmp_path_factory.mktemp("layer_tokens_trace")
    exe = os.path.join(str(d), "train_layer_tokens_trace")
    build = subprocess.run([X.HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O1", "-DHVLA_TRAIN_TRACE", "-I", CSRC,
                            os.path.join(ROOT, "tools", "train_layer_tokens_trace.hip"), X.TRAIN_HIP, "-o", exe],
                           cwd=str(d), capture_output=True, text=True, timeout=900)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, timeout=120)
    assert run.returncode == 0, run.stderr
    points = []
    for ln in run.stdout.decode().splitlines():
        w = ln.split(" ")
        if w[0] == "#":
            points.append(dict(title=ln[2:], workspace=None, size={}, plan=[], lines=[]))
        elif w[0] == "workspace":
            points[-1]["workspace"] = int(w[1])
        elif w[0] == "size":
            points[-1]["size"][w[1]] = int(w[2])
        elif w[0] == "plan":
            points[-1]["plan"].append((w[1], int(w[2]), int(w[3])))
        elif w[0] != "step":
            points[-1]["lines"].append(ln)
    return run.stdout, points


def _pinned(out):
    """The lines of the tool's output that a layer-token step adds or changes the shape of: a point's title and workspace, every launch
    of a `_tokens_` / `_groups` kernel and every grouped product.  (The rest of a step is tests/native/train_step_trace.txt's text on
    other offsets; the extent rules below walk all of it.)"""
    keep = [ln for ln in out.split(b"\n") if ln.startswith((b"# ", b"workspace ", b"bgemm_groups ")) or b"_tokens_" in ln.split(b" ")[0]
            or b"_groups" in ln.split(b" ")[0]]
    return b"\n".join(keep) + b"\n"


def test_the_trace_is_the_recorded_one(traced):
    """tests/native/train_layer_tokens_trace.txt is `_pinned` of the tool's output byte for byte (the existing sweep's pin,
    tests/native/train_step_trace.txt, is tests/test_train_launch_trace.py's and does not move)."""
    want = open(os.path.join(ROOT, "tests", "native", "train_layer_tokens_trace.txt"), "rb").read()
    got = _pinned(traced[0])
    if got != want:
        a, b = got.split(b"\n"), want.split(b"\n")
        first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        pytest.fail("line %d differs\nrecorded: %s\nnow:      %s" % (first + 1, b"\n".join(b[first:first + 1]).decode(), b"\n".join(a[first:first + 1]).decode()))


def _kw(title):
    return dict(kv.split("=") for kv in title.split(" ")[1:])


def _geom_of(title):
    name = title.split(" ")[0]
    return {"MID-lt": _geo(False), "MID-lt-shared": _geo(True), "S48-lt": _geo(False, layers=4, lang_tokens=38),
            "LANG-lt": _geo(True, lang_in_policy=True), "DIFF-lt-shared": _geo(True, differential=True),
            "README2-lt": _geo(False, base=FULL)}.get(name)


def test_grouped_launches_and_final_layernorm_rows(traced):
    """Per layer-token point: the three grouped launches once each, with the forward's A the plan's ctx [B][NL C], its C theta, its B
    and bias the heads; NL B rows through ctx_final_tokens_fwd / bwd; no plain weight-generation product and none of the one-token
    kernels; the softmax of the context blocks is softmax_tokens_fwd_kernel with T = S - 1 - NL."""
    on = [pt for pt in traced[1] if "-lt" in pt["title"]]
    assert len(on) == 10
    seen = set()
    for pt in on:
        g, w = _geom_of(pt["title"]), _kw(pt["title"])
        B, NL, C = int(w["B"]), g.num_layer_tokens, g.ctx_dim
        seen.add((pt["title"].split(" ")[0], B, int(w["enc"])))
        layout, total = train_param_layout(g, bool(int(w["enc"])))
        at = dict((k, o) for k, o, _ in layout)
        plan = {n: (o, c) for n, o, c in pt["plan"]}
        G, Gh = generated_leaves(g)[-1].offset + generated_leaves(g)[-1].size, head_columns(g)[1]
        assert plan["ctx"][1] == plan["dctx"][1] == plan["ctxn"][1] == B * NL * C and plan["cmean"][1] == plan["crstd"][1] == B * NL
        assert pt["size"]["theta"] == B * G and pt["size"]["params"] == total
        grp = [ln.split(" ") for ln in pt["lines"] if ln.startswith("bgemm_groups ")]
        assert [(x[1], x[2]) for x in grp] == [("0", "0"), ("1", "0"), ("0", "1")], pt["title"]
        bg = [dict(zip(X.BG_FIELDS, [x[3][3:]] + x[4:3 + len(X.BG_FIELDS) - 1] + [x[3 + len(X.BG_FIELDS) - 1][:-1]])) for x in grp]
        ctx_at, dctx_at = "work+%d" % plan["ctx"][0], "work+%d" % plan["dctx"][0]
        wcat, bcat = "params+%d" % at["W_cat"], "params+%d" % at["b_cat"]
        f, dw, dc = bg
        assert (f["A"], f["B"], f["C"], f["bias"]) == (ctx_at, wcat, "theta+0", bcat), f
        assert (int(f["M"]), int(f["K"]), int(f["lda"]), int(f["ldb"]), int(f["ldc"]), int(f["accumulate"])) == (B, C, NL * C, Gh, G, 0)
        assert (dw["A"], dw["B"], dw["C"], dw["bias"]) == (ctx_at, "dtheta+0", "grads+%d" % at["W_cat"], "null")
        assert (int(dw["M"]), int(dw["K"]), int(dw["lda"]), int(dw["ldb"]), int(dw["ldc"])) == (C, B, NL * C, G, Gh)
        assert int(dw["accumulate"]) == (2 if g.shared_block_heads else 1)               # shared heads: a real sum over the blocks
        assert (dc["A"], dc["B"], dc["C"]) == ("dtheta+0", wcat, dctx_at)
        assert (int(dc["M"]), int(dc["N"]), int(dc["lda"]), int(dc["ldb"]), int(dc["ldc"]), int(dc["accumulate"])) == (B, C, G, Gh, NL * C, 2)
        # the tables: inside the uploaded block, 64-column tiles below B = 96 and 128-column ones from there
        for x, tile_of in zip(grp, (128 if B >= 96 else 64, 128 if C >= 96 else 64, None)):
            tiles, ntiles, tile, nz = X._ptr(x[-5]), int(x[-4]), int(x[-3]), int(x[-2])
            assert tiles[0] == "tiles" and 0 <= tiles[1] and tiles[1] + ntiles <= pt["size"]["tiles"] and ntiles > 0
            if tile_of:
                assert tile == tile_of and nz == 1
            else:
                assert nz == -(-C // tile)
        fin = [ln.split(" ") for ln in pt["lines"] if ln.startswith("ctx_final_tokens_")]
        assert [x[0] for x in fin] == ["ctx_final_tokens_fwd_kernel", "ctx_final_tokens_bwd_kernel"]
        assert all(int(x[-3]) == B * NL and x[1] == "(%d,1,1)" % ((B * NL + 3) // 4) for x in fin)
        names = {ln.split(" ")[0] for ln in pt["lines"]}
        assert not names & {"ctx_rows_kernel", "ctx_rows_bwd_kernel", "ctx_final_fwd_kernel", "ctx_final_bwd_kernel"}
        assert {"ctx_rows_tokens_kernel", "ctx_rows_tokens_bwd_kernel", "colsum_groups_kernel"} <= names
        sm = [ln.split(" ") for ln in pt["lines"] if ln.startswith("softmax_tokens_fwd_kernel")]
        assert len(sm) == g.ctx_layers and all((int(x[5]), int(x[6])) == (g.ctx_seq, g.lang_tokens) for x in sm)
        # no plain product reads or writes the heads or the context rows
        for ln in pt["lines"]:
            if ln.startswith("bgemm "):
                assert wcat not in ln and ctx_at + " " not in ln and dctx_at + " " not in ln, ln
    assert seen == {("MID-lt", 1, 0), ("MID-lt", 5, 0), ("MID-lt-shared", 1, 0), ("MID-lt-shared", 5, 0), ("S48-lt", 3, 0), ("S48-lt", 3, 1),
                    ("LANG-lt", 2, 0), ("DIFF-lt-shared", 2, 0), ("README2-lt", 2, 0), ("MID-lt-shared", 128, 0)}


def test_layer_token_steps_obey_the_extent_rules(traced):
    """The rules of tests/test_train_workspace_extents.py on every layer-token point, S = 48 among them: every GEMM operand, copy and
    memset inside ONE named plan buffer or its vector, nothing beyond the workspace the step reports."""
    on = [pt for pt in traced[1] if "-lt" in pt["title"]]
    assert any(_geom_of(pt["title"]).ctx_seq == 48 for pt in on)
    bad = X.violations(on)
    assert not bad, "%d violations\n%s" % (len(bad), "\n".join(bad[:10]))


def test_flag_off_points_launch_no_layer_token_kernel(traced):
    off = [pt for pt in traced[1] if "-lt" not in pt["title"]]
    assert len(off) == 2
    for pt in off:
        assert not any("_tokens_" in ln or "_groups" in ln for ln in pt["lines"]) and "tiles" not in pt["size"]


# ---------------------------------------------------------------------------------------------- 6. the switch, without a device
class _Model:
    def __init__(self, g):
        self.geometry = g


def test_finetuner_refusals_need_no_device():
    from hypervla.train import FineTuner
    with pytest.raises(ValueError, match="share_layer_index=False is not built; serving is"):
        FineTuner(_Model(_geo()), 2)
    with pytest.raises(ValueError, match="layer_tokens=True needs a model"):
        FineTuner(_Model(MID), 2, layer_tokens=True)


def test_binding_and_header_have_the_setting():
    from hypervla import _native
    assert "hvla_train_layer_tokens" in _native.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "hvla.h")).read()
    assert "int hvla_train_layer_tokens(hvla_ctx* ctx, int32_t on);" in hdr
