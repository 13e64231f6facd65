"""CPU: the host side of the device post-processing (hypervla.postprocess, include/hvla.h hvla_post_*): table rows, refusals before
any launch, the C layout of hvla_post_row, and the ISA of post_slots_kernel (no fused multiply-add: numpy never contracts)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SETUPS = ("libero", "widowx_bridge", "google_robot")


class FakeModel:
    """What InferenceWrapper and DevicePostprocessor read of a HyperVLA, with a recording stand-in for the native context."""

    class Ctx:
        def __init__(self):
            self.calls = []

        def post_create(self, B, stream=0):
            self.calls.append(("create", B))
            return ctypes.c_void_p(1)

        def post_free(self, p):
            self.calls.append(("free",))

        def post_assign(self, p, slots_ptr, K, rows_ptr, ens_ptr, stream=0):
            self.calls.append(("assign", K))

        def post_step(self, *a, **k):
            self.calls.append(("step",))

    def __init__(self, stats, kinds, max_batch=16):
        from hypervla.config import MID
        self.dataset_statistics = stats
        self.config = {"dataset_kwargs": {"dataset_kwargs_list": [
            {"name": n, "action_proprio_normalization_type": k} for n, k in kinds.items()]}}
        self.geometry = MID                                   # horizon 4, action_dim 7
        self.max_batch, self.device, self._ctx = max_batch, "cpu", self.Ctx()

    def _stream(self):
        return 0


def _stats(seed, dtype, gripper_masked):
    rng = np.random.default_rng(seed)
    mean = (0.1 * rng.standard_normal(7)).astype(dtype)
    std = rng.uniform(0.05, 0.5, 7).astype(dtype)
    p01, p99 = (mean - 2.3 * std).astype(dtype), (mean + 2.3 * std).astype(dtype)
    return {"action": {"mean": mean, "std": std, "p01": p01, "p99": p99, "mask": np.array([True] * 6 + [gripper_masked])}}


def _unnormalize_like_the_kernel(row, a):
    """The kernel's un-normalisation of f32 predictions from a table row, in numpy f64 and the kernel's operation order."""
    p0, p1, mask = np.array(row.p0), np.array(row.p1), np.array(row.mask, bool)
    a = a.astype(np.float64)
    if row.normalization == 1:
        return np.where(mask, (a + 1.0) * p1 / 2.0 + p0, a)
    return np.where(mask, a * p1 + p0, a)


@pytest.mark.parametrize("kind", ["normal", "bounds", "NORMAL", "BOUNDS"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("masked", [True, False, None])
def test_table_rows_are_the_wrappers_statistics(kind, dtype, masked):
    """normal and bounds statistics, with a masked gripper, an un-masked one and no mask at all: the row holds the operands
    InferenceWrapper.unnormalize uses, and the kernel's arithmetic on them is bitwise the wrapper's (bounds evaluated literally,
    with p99 - p01 + 1e-8 in the statistics' own dtype)."""
    from hypervla import _native
    from hypervla.interface import InferenceWrapper, action_statistics
    from hypervla.postprocess import table_row
    st = {d: _stats(i, dtype, bool(masked)) for i, d in enumerate(("bridge_dataset", "fractal20220817_data", "libero"))}
    if masked is None:
        for v in st.values():
            del v["action"]["mask"]
    m = FakeModel(st, {"bridge_dataset": kind, "fractal20220817_data": kind, "libero": kind})
    rng = np.random.default_rng(5)
    a = rng.normal(0, 1.5, (4, 7)).astype(np.float32)
    for setup in SETUPS:
        w = InferenceWrapper(m, policy_setup=setup, pred_action_horizon=4, action_ensemble=True)
        stats, nt = action_statistics(m, setup)
        assert stats is w.unnormalization_statistics and nt == w.normalization_type
        row = table_row(setup, stats, nt)
        assert row.setup == {"libero": 0, "widowx_bridge": 1, "google_robot": 2}[setup]
        s = stats
        want_mask = np.ones(7, bool) if masked is None else s["mask"]
        assert np.array(row.mask, bool).tolist() == list(want_mask)
        if kind.lower() == "normal":
            assert row.normalization == _native.HVLA_NORM_NORMAL
            assert np.array(row.p0).tolist() == np.asarray(s["mean"], np.float64).tolist()
            assert np.array(row.p1).tolist() == np.asarray(s["std"], np.float64).tolist()
        else:
            assert row.normalization == _native.HVLA_NORM_BOUNDS
            assert np.array(row.p0).tolist() == np.asarray(s["p01"], np.float64).tolist()
            assert np.array(row.p1).tolist() == np.asarray(s["p99"] - s["p01"] + 1e-8, np.float64).tolist()
        np.testing.assert_array_equal(_unnormalize_like_the_kernel(row, a), w.unnormalize(a.astype(np.float64)))


def test_single_dataset_statistics_and_dataset_kwargs():
    """A checkpoint with one top-level "action" entry and a single `dataset_kwargs`: the lookup InferenceWrapper always did."""
    from hypervla.interface import InferenceWrapper, action_statistics
    m = FakeModel(_stats(1, np.float32, False), {})
    m.config = {"dataset_kwargs": {"dataset_kwargs": {"action_proprio_normalization_type": "bounds"}}}
    stats, nt = action_statistics(m, "google_robot")
    assert stats is m.dataset_statistics["action"] and nt == "bounds"
    w = InferenceWrapper(m, policy_setup="google_robot", pred_action_horizon=4)
    assert w.unnormalization_statistics is stats and w.normalization_type == "bounds"


def _post():
    from hypervla.postprocess import DevicePostprocessor
    st = {d: _stats(i, np.float32, i == 0) for i, d in enumerate(("bridge_dataset", "fractal20220817_data", "libero"))}
    m = FakeModel(st, {"bridge_dataset": "bounds", "fractal20220817_data": "normal", "libero": "normal"})
    return m, DevicePostprocessor(m, 8)


def test_metaworld_and_unknown_setups_are_refused():
    from hypervla.interface import action_statistics
    from hypervla.postprocess import table_row
    m, post = _post()
    for bad in ("metaworld", "franka", ""):
        with pytest.raises(ValueError, match="Unknown policy setup"):
            action_statistics(m, bad)
        with pytest.raises(ValueError, match="Unknown policy setup"):
            table_row(bad, m.dataset_statistics["libero"]["action"], "normal")
        with pytest.raises(ValueError, match="Unknown policy setup"):
            post.assign([0, 1], ["libero", bad])
    with pytest.raises(ValueError, match="Unknown normalization type"):
        table_row("libero", m.dataset_statistics["libero"]["action"], "quantile")
    assert all(c[0] != "assign" for c in m._ctx.calls)


def test_assign_builds_one_row_per_setup_and_checks_its_arguments():
    from hypervla import _native
    m, post = _post()
    post.assign([3, 0, 5], ["google_robot", "libero", "google_robot"], [True, False, True])
    post.assign([1], "widowx_bridge", action_ensemble=False)
    assert post._rows == {"google_robot": 0, "libero": 1, "widowx_bridge": 2}
    assert post._table.numel() == 3 * ctypes.sizeof(_native.hvla_post_row)
    assert [c for c in m._ctx.calls if c[0] == "assign"] == [("assign", 3), ("assign", 1)]
    for slots, setups, ens in (([0, 0], "libero", True), ([8], "libero", True), ([], "libero", True),
                               ([0, 1], ["libero"], True), ([0, 1], "libero", [True])):
        with pytest.raises(ValueError):
            post.assign(slots, setups, ens)
    assert len([c for c in m._ctx.calls if c[0] == "assign"]) == 2


def test_bad_action_shapes_are_refused_before_any_launch():
    m, post = _post()
    with pytest.raises(RuntimeError, match="assign"):
        post.step(np.zeros((2, 4, 7), np.float32), [0, 1])         # no setup yet: no table
    post.assign(range(8), "libero")
    for shape in ((2, 4, 6), (3, 4, 7), (2, 3, 7), (2, 28), (4, 7)):
        with pytest.raises(ValueError, match="actions must be"):
            post.step(np.zeros(shape, np.float32), [0, 1])
    with pytest.raises(ValueError):
        post.step(np.zeros((2, 4, 7), np.float32), [1, 1])
    assert not [c for c in m._ctx.calls if c[0] == "step"]


def test_evaluator_postprocess_keyword():
    """postprocess is 'host' (default) or 'device'; a per-simulator setup list needs 'device'; 'device' refuses unknown setups and a
    pred_action_horizon the model does not predict."""
    from hypervla.evaluate import BatchEvaluator
    m, _ = _post()
    assert BatchEvaluator(m, policy_setup="libero", pred_action_horizon=4).postprocess == "host"
    with pytest.raises(ValueError, match="postprocess"):
        BatchEvaluator(m, postprocess="gpu")
    with pytest.raises(ValueError, match="postprocess='device'"):
        BatchEvaluator(m, policy_setup=["libero", "google_robot"], pred_action_horizon=4)
    ev = BatchEvaluator(m, policy_setup=["libero", "google_robot"], pred_action_horizon=4, postprocess="device")
    assert ev.setups == ["libero", "google_robot"]
    with pytest.raises(ValueError, match="3 simulators"):
        ev._device_post(3)
    for bad in ("metaworld", ["libero", "metaworld"]):
        with pytest.raises(ValueError, match="Unknown policy setup"):
            BatchEvaluator(m, policy_setup=bad, pred_action_horizon=4, postprocess="device")
    with pytest.raises(ValueError, match="horizon"):
        BatchEvaluator(m, policy_setup="libero", pred_action_horizon=2, postprocess="device")


def test_post_row_struct_layout_is_the_header_s(tmp_path):
    """The ctypes mirror of hvla_post_row against the C compiler's view of include/hvla.h."""
    from hypervla import _native
    names = [n for n, _ in _native.hvla_post_row._fields_]
    prog = "#include <stdio.h>\n#include <stddef.h>\n#include \"hvla.h\"\nint main(void) { printf(\"%zu\", sizeof(hvla_post_row));\n"
    prog += "".join(f'printf(" %zu", offsetof(hvla_post_row, {n}));\n' for n in names) + "return 0; }\n"
    (tmp_path / "l.c").write_text(prog)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "l.c"), "-o", str(tmp_path / "l")], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "l")], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == ctypes.sizeof(_native.hvla_post_row)
    assert got[1:] == [getattr(_native.hvla_post_row, n).offset for n in names]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_post_kernel_has_no_fused_multiply_add(tmp_path):
    """post_slots_kernel must round every product before the sum, as numpy does: its body (the rotation's library calls live in
    post_axangle, out of line) has f64 multiplies and adds and no v_fma_f64 / v_fmac_f64."""
    src = os.path.join(ROOT, "hyper-vla_amd", "csrc", "postprocess.hip")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", src, "-save-temps", "-o", "x.o"],
                   cwd=tmp_path, check=True, capture_output=True, timeout=900)
    asm = [f for f in os.listdir(tmp_path) if f.endswith("gfx950.s")]
    assert len(asm) == 1, asm
    text = open(os.path.join(tmp_path, asm[0])).read()
    m = re.search(r"^(\w*post_slots_kernel\w*):", text, re.M)
    assert m, "post_slots_kernel not in the gfx950 assembly"
    body = text[m.end():]
    body = body[:body.index(".Lfunc_end")]
    ops = [ln.split()[0] for ln in body.split("\n") if ln.strip() and not ln.strip().startswith((";", "."))]
    assert "v_mul_f64" in ops and "v_add_f64" in ops
    assert not [o for o in ops if o.startswith(("v_fma_f64", "v_fmac_f64"))]
