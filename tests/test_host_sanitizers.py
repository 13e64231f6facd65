"""The host-side layout / packing code of the C-ABI library under AddressSanitizer + UndefinedBehaviorSanitizer (CPU build;
GPU sanitizers are not available on the pool).  csrc/layout.h and csrc/pack.h hold all the index arithmetic hvla_create
runs on checkpoint tensors; tests/native/pack_sanitize.cpp drives them on the README geometry with exact-size buffers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_layout_and_packing_under_asan_ubsan(tmp_path):
    exe = tmp_path / "pack_sanitize"
    build = subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
         "-Werror", "-I", os.path.join(ROOT, "hyper-vla_amd", "csrc"), os.path.join(ROOT, "tests", "native", "pack_sanitize.cpp"),
         "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    dump = tmp_path / "half.bin"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([str(exe), str(dump)], capture_output=True, text=True, env=env, timeout=600)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith("OK"), run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr
    # the library's software float -> binary16 conversion is numpy's (round to nearest even, subnormals, overflow to inf)
    rec = np.fromfile(dump, dtype=np.uint32).reshape(-1, 2)
    x = rec[:, 0].copy().view(np.float32)
    finite = ~np.isnan(x)
    with np.errstate(over="ignore"):
        want = x.astype(np.float16).view(np.uint16)
    np.testing.assert_array_equal(rec[finite, 1], want[finite])
    assert finite.sum() > 900000


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_launch_plan_arithmetic_under_asan_ubsan(tmp_path):
    """csrc/plan.h: the XCD tile order of the small GEMM kernels is a bijection with one contiguous run per XCD at every grid size
    (a 64-column slice of W / dW on at most two XCDs at the B = 256 launch shapes), and the non-temporal 16-bit epilogue, whose
    stores carry 32-bit BYTE offsets, is only chosen for outputs below 4 GiB (fc1 from B = 2721 on would wrap).  The
    launch plan of an encoder call: the launch counts the committed profiles record, the boundaries between its forms, and, launch
    for launch over a sweep of geometries, batches and CU counts, the trace recorded from the dispatch it replaced.  The three (width,
    batch) pairs at which tests/test_gpu_geometry_contract.py runs the persistent fused LayerNorm take those kernels on 256 CUs.
    The encoder workspace table (WorkspacePlan): byte for byte the allocation sizes and slice offsets recorded from the expressions it
    replaced, over five geometries, nine context sizes and the half points of a two-stream step; there every slice starts on 16
    bytes, the two halves are disjoint and inside the allocation for everything run_encoder touches, and the cut of `g` by S * F
    alone, which once let two streams share rows at the MID geometry, fails the check."""
    exe = tmp_path / "plan_check"
    build = subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
         "-Werror", "-I", os.path.join(ROOT, "hyper-vla_amd", "csrc"), os.path.join(ROOT, "tests", "native", "plan_check.cpp"),
         "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe), os.path.join(ROOT, "tests", "native", "encoder_plan_trace.txt"),
                          os.path.join(ROOT, "tests", "native", "encoder_workspace_trace.txt")], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.strip().endswith("OK"), run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_accepted_geometries_under_asan_ubsan(tmp_path):
    """csrc/accept.h, the predicate hvla_create refuses a geometry by: over a grid of configs -- every pair of fields through its lower
    and upper edges, one step outside each, zero, negative and INT_MAX, from four accepted bases -- the verdict arrives without a
    division by zero or an overflow (a zero heads / patch is HVLA_E_SHAPE), and everything accepted meets the launch-side
    preconditions, computed by the functions the launchers call: context and policy LDS <= 160 KiB (both language forms), context
    head width % 4 == 0, P in {64, 256}, an encoder plan at B = 1.  The largest policy the LDS admits at P = 256 is pinned
    (tests/test_gpu_geometry_contract.py runs it and asserts one step further is refused)."""
    exe = tmp_path / "accept_check"
    build = subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
         "-Werror", "-I", os.path.join(ROOT, "hyper-vla_amd", "csrc"), os.path.join(ROOT, "tests", "native", "accept_check.cpp"),
         "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.strip().endswith("OK"), run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_train_layout_under_asan_ubsan(tmp_path):
    """csrc/train_layout.h, the one table of a transformer block's leaves the fine-tune step binds its pointers from: over the TINY,
    MID and README geometries and the layer-count edges (0 / 8 context layers, 0 / 24 encoder layers, 1 / 16 policy layers) every
    policy member is the offset of the generated leaf of its flax name, nothing is -1 but the LayerScale of blocks without one, the
    members tile [0, total), [0, enc_total) and a row of theta without gap or overlap, and one layer more than a table holds is
    refused by the predicate in front of make_train_layout.  The offsets the program prints for the MID and README vectors are
    hypervla.train.train_param_layout's, name for name."""
    from hypervla.config import MID, Geometry
    from hypervla.train import train_param_layout
    exe = tmp_path / "train_layout_check"
    build = subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
         "-Werror", "-I", os.path.join(ROOT, "hyper-vla_amd", "csrc"), os.path.join(ROOT, "tests", "native", "train_layout_check.cpp"),
         "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.strip().endswith("OK"), run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr
    printed, name = {}, None
    for line in run.stdout.split("\n"):
        if line.startswith("## "):
            _, name, total = line.split()
            printed[name] = ({}, int(total))
        elif line and line != "OK":
            leaf, off = line.rsplit(" ", 1)
            assert leaf not in printed[name][0], leaf
            printed[name][0][leaf] = int(off)
    assert sorted(printed) == ["MID", "README"]
    for name, g in (("MID", MID), ("README", Geometry())):
        layout, total = train_param_layout(g, True)
        assert printed[name][1] == total
        assert printed[name][0] == {leaf: off for leaf, off, _ in layout}, name
