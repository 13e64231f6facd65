"""GPU: the fine-tune step's batched GEMM (csrc/train_gemm.hip bgemm(): bgemm3_kernel in 20 instantiations, bgemm_kernel in 4) launch by
launch against float64 -- tools/bgemm_check.py in a fresh process on the bench library, once per module.  The tool's docstring has the
two input classes and the derivation of the precision class's bound; tests/test_train_gemm_reference.py holds a CPU emulation of the
kernel to the same criteria on the same table.

TOOL_SECONDS: the tool's wall time measured on an MI355X host with 16 threads -- 18.1 s, of which its own `summary` line counts
16.3 s from the first case on (717 cases, 743 report lines; almost all of it is the float64 reference on the host) -- rounded up
to 20 s; the subprocess limit is three times that.  A non-zero exit
fails every test of the module; nothing is retried."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOOL_SECONDS = 20         # measured: see the module docstring
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def report():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bgemm_check.py")], capture_output=True, text=True, timeout=3 * TOOL_SECONDS)
    lines = out.stdout.strip().splitlines()
    print("\n".join(ln for ln in lines if not ln.endswith(" ok"))[-6000:])
    print("\n".join(ln for ln in lines if ln.startswith(("coverage", "summary"))))
    assert lines, out.stderr[-3000:]
    return dict(lines=lines, rc=out.returncode, err=out.stderr[-3000:])


def _group(report, prefix, at_least):
    assert report["rc"] in (0, 1), (report["rc"], report["lines"][-3:], report["err"])       # 2 / 3: a launch failed, the calibration failed
    lines = [ln for ln in report["lines"] if ln.startswith(prefix + " | ")]
    assert len(lines) >= at_least, (prefix, len(lines))
    bad = [ln for ln in lines if not ln.endswith(" ok")]
    assert not bad, bad[:8]
    return lines


def test_the_whole_run_is_clean(report):
    assert report["rc"] == 0 and report["lines"][-1] == "ok", (report["rc"], [ln for ln in report["lines"] if not ln.endswith(" ok")][:10], report["err"])


def test_calibration_one_full_tile(report):
    """64 x 64 x 32, NN: the assumption under the exact class -- the bf16 matrix instruction's f32 accumulate is exact when every partial
    sum is representable."""
    _group(report, "calibration", 1)


@pytest.mark.parametrize("group,n", [("forms", 20), ("dword reasons", 72), ("a_padded", 6), ("edges", 70), ("k depth", 200), ("split-K 64", 20), ("split-K 128", 20),
                                     ("modes", 32), ("two batch levels", 4), ("f32 kernel", 12), ("replay B = 1", 40), ("replay B = 32", 40)])
def test_exact_class_bitwise(report, group, n):
    """a + b 2^-10 operands: the device's C buffer, sentinel and all, equals the float64 three-term product bit for bit."""
    for ln in _group(report, group, n):
        assert " | exact | " in ln and "bitwise ok" in ln, ln


@pytest.mark.parametrize("group,n", [("precision forms", 20), ("precision a_padded", 2), ("precision k depth", 24), ("precision split-K", 2), ("precision modes", 32),
                                     ("precision two batch levels", 4), ("precision f32 kernel", 4)])
def test_precision_class_within_the_component_wise_bound(report, group, n):
    """standard-normal operands, K <= 257: |C - C64| <= (2^-14 + K 2^-23) (|alpha| |A| |B|) + 2^-23 |C64|; (K + 2) 2^-24 for the f32 kernel."""
    for ln in _group(report, group, n):
        assert " | precision | " in ln, ln


def test_every_instantiation_is_hit_by_an_exact_class_case(report):
    """from what the launcher reported per case (the table does not restate the dispatch): 20 x bgemm3_kernel, 4 x bgemm_kernel, and a
    launcher- or caller-chosen split of K on both square tiles."""
    lines = _group(report, "coverage", 26)
    assert sum("bgemm3_kernel<" in ln for ln in lines) == 20 and sum("bgemm_kernel<" in ln for ln in lines) == 4
    assert sum("ksplit > 1" in ln for ln in lines) == 2
