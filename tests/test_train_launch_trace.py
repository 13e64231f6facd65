"""What the fine-tune step enqueues, pinned on the CPU (hipcc cross-compiles gfx950 without a GPU): csrc/train.hip built with
-DHVLA_TRAIN_TRACE prints every kernel launch, batched GEMM, memset, copy and event of train_step / train_accumulate / train_apply
instead of enqueueing it (tools/train_launch_trace.h), and tools/train_launch_trace.hip drives it over a sweep of geometries,
batch sizes and options on fake pointers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_train_step_launches_are_the_recorded_trace(tmp_path):
    """tests/native/train_step_trace.txt was recorded from the host sequencing as it stood before the block-leaf table
     with only the seam applied: the MID geometry at B = 1, 5, 32 and the README widths with two encoder layers at
    B = 2, 8, 32 (rows >= 2048: the large-batch kernels), encoder frozen / trained / trained with a position source, forward only
    and not, frozen_buckets 0 / 2 / 4 / 6 with and without a mask, the attention terms off / entropy / both, ema and the shared
    group's weight decay on and off, and the layer-count edges (no context layer and 16 policy layers; 8 and 1).  The tool's
    output is that file byte for byte: one batched QKV product or three, colsum / colsum4 / colsum4b, ln_bwd_shared or the
    two-kernel form, ls_bwd4, scale_add4 and every offset into params / grads / theta / the workspace are where they were."""
    csrc = os.path.join(ROOT, "hyper-vla_amd", "csrc")
    exe = tmp_path / "train_launch_trace"
    build = subprocess.run(
        [HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O1", "-DHVLA_TRAIN_TRACE", "-I", csrc,
         os.path.join(ROOT, "tools", "train_launch_trace.hip"), os.path.join(csrc, "train.hip"), "-o", str(exe)],
        cwd=tmp_path, capture_output=True, text=True, timeout=900)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, timeout=120)
    assert run.returncode == 0, run.stderr
    want = open(os.path.join(ROOT, "tests", "native", "train_step_trace.txt"), "rb").read()
    if run.stdout != want:
        got, ref = run.stdout.split(b"\n"), want.split(b"\n")
        first = next((i for i, (a, b) in enumerate(zip(got, ref)) if a != b), min(len(got), len(ref)))
        point = next((ln for ln in reversed(ref[:first + 1]) if ln.startswith(b"#")), b"")
        pytest.fail("line %d differs (%d lines, recorded %d)\n%s\nrecorded: %s\nnow:      %s" % (
            first + 1, len(got), len(ref), point.decode(), b"\n".join(ref[first:first + 1]).decode(),
            b"\n".join(got[first:first + 1]).decode()))
