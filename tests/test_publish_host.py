"""CPU: the one layout of the serving buffers (csrc/serving_layout.h, csrc/pack.h) -- the publish tables and the host packer of
hvla_load_weights against a frozen copy of the earlier loader, the packer's refusals -- the value set of the GPU rounding test, and
the publish symbol."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_publish_tables_against_the_host_packer_under_asan_ubsan(tmp_path):
    """tests/native/publish_map_check.cpp: at MID and README geometry a training vector of distinct values through the publish
    tables and the shared rounding functions (what the kernels do) equals, byte for byte, pack::pack_wcat / pack::pack_matrix_t and
    a transcription of the ordering hvla_load_weights had before serving_layout.h, fed the same leaves; every destination element
    is written exactly once.  The real host packer (serving::pack_serving, what hvla_load_weights runs), fed the same leaves by
    checkpoint name, gives the same bytes; the offsets it returns are where the transcription holds each tensor and tile every
    buffer.  At MID geometry a checkpoint with a tensor absent or off by one element is refused with that name and its suffix,
    nothing is written, and of two such tensors the first of the enumeration is named."""
    exe = tmp_path / "publish_map_check"
    build = subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
         "-Werror", "-I", os.path.join(ROOT, "hyper-vla_amd", "csrc"), os.path.join(ROOT, "tests", "native", "publish_map_check.cpp"),
         "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=600)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith("OK"), run.stdout
    assert "README geometry" in run.stdout and "MID geometry (bf16)" in run.stdout, run.stdout
    assert "the packer names the first absent or wrong-sized tensor and writes nothing" in run.stdout, run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr


def _bf16_rne(x):
    u = x.view(np.uint32).astype(np.uint64)
    return (((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)


def _bf16_trunc(x):
    return (x.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)


def _f16_is_tie(x):
    """x lies exactly half way between two neighbouring binary16 values (so round-to-nearest-even has to choose)."""
    h = x.astype(np.float16).astype(np.float64)
    below = np.nextafter(h.astype(np.float16), np.float16(-np.inf)).astype(np.float64)
    above = np.nextafter(h.astype(np.float16), np.float16(np.inf)).astype(np.float64)
    xd = x.astype(np.float64)
    return (xd != h) & ((np.abs(xd - h) == np.abs(xd - below)) | (np.abs(xd - h) == np.abs(xd - above)))


def test_edge_value_set_has_ties_subnormals_and_zeros():
    """The value set of tests/test_gpu_publish.py::test_rounding_edge_values really holds what its docstring says, so that the GPU
    comparison is not an empty one: round-to-nearest-even differs from truncation AND from round-half-up on it, for both 16-bit
    types, at the first rounding and at the rounding of the residue."""
    from publish_edge_values import edge_block, edge_values
    v = edge_values()
    a = np.abs(v)
    assert a.max() < 4.0 and a[a > 0].min() >= 2.0 ** -27 and np.isfinite(v).all()
    assert np.signbit(v[v == 0]).tolist() == [False, True]                       # +0 and -0
    assert (v > 0).sum() > 100 and (v < 0).sum() > 100
    # every value is +-(2m+1) 2^-e: an odd integer after scaling by a power of two
    m, _ = np.frexp(a[a > 0].astype(np.float64))
    k = np.ldexp(m, 24)
    assert np.array_equal(k, np.round(k))
    odd = k.astype(np.int64)
    odd //= (odd & -odd)
    assert (odd % 2 == 1).all()

    # ---- binary16
    with np.errstate(over="raise"):
        h = v.astype(np.float16)
    assert np.isfinite(h).all()
    sub = (np.abs(h) > 0) & (np.abs(h) < np.float16(2.0 ** -14))
    assert sub.sum() >= 50                                                       # binary16 subnormals are produced
    assert ((h == 0) & (v != 0)).sum() >= 20                                     # values that round to zero
    tie16 = _f16_is_tie(v)
    assert tie16.sum() >= 100
    trunc16 = (np.abs(v).view(np.uint32) & np.uint32(0xffffe000)).view(np.float32)       # truncation in the normal range
    normal = np.abs(v) >= 2.0 ** -14
    assert (np.abs(h.astype(np.float32))[normal] != trunc16[normal]).sum() >= 50        # nearest-even differs from truncation
    up = tie16 & normal & (np.abs(h.astype(np.float32)) > np.abs(v))
    down = tie16 & normal & (np.abs(h.astype(np.float32)) < np.abs(v))
    assert up.sum() >= 10 and down.sum() >= 10                                   # ties go both ways: to even, not half-up
    # ties only after the hi part is subtracted: exact-in-f32 residue, scaled as pack_matrix_t does
    res = ((v - h.astype(np.float32)) * np.float32(4096.0)).astype(np.float32)
    second = _f16_is_tie(res) & ~tie16 & (res != 0)
    assert second.sum() >= 50

    # ---- bfloat16 (W_cat's hi / lo split and enc_dtype="bf16")
    b = _bf16_rne(v)
    tieb = (v.view(np.uint32) & np.uint32(0xffff)) == np.uint32(0x8000)
    assert tieb.sum() >= 100
    assert (b != _bf16_trunc(v)).sum() >= 100
    assert (tieb & (np.abs(b) > np.abs(v))).sum() >= 10 and (tieb & (np.abs(b) < np.abs(v))).sum() >= 10
    lo = (v - b).astype(np.float32)
    secondb = ((lo.view(np.uint32) & np.uint32(0xffff)) == np.uint32(0x8000)) & ~tieb
    assert secondb.sum() >= 50

    # the blocks the GPU test overwrites cycle through the whole set
    for shape, off in (((64, 64), 0), ((64, 64), 7), ((128, 64), 13), ((64, 64), 29)):
        assert np.unique(edge_block(shape, off).view(np.uint32)).size == np.unique(v.view(np.uint32)).size


def test_publish_symbol_in_header_binding_and_library():
    from hypervla import _native
    src = open(os.path.join(ROOT, "include", "hvla.h")).read()
    assert "int hvla_train_publish(hvla_ctx* ctx, const float* params, int64_t n_params, int32_t train_encoder, void* stream);" in src
    assert "hvla_train_publish" in _native.EXPORTS
    if not os.path.exists(_native.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    assert hasattr(ctypes.CDLL(_native.lib_path()), "hvla_train_publish")
    assert callable(getattr(_native.Context, "train_publish"))
    from hypervla.train import FineTuner
    assert callable(getattr(FineTuner, "publish"))


def test_pack_params_round_trips_the_edge_blocks():
    """pack_params / unpack_params carry the overwritten blocks bit for bit (the GPU test publishes the packed vector and builds
    its reference from the unpacked one)."""
    from hypervla import synthetic as syn
    from hypervla.config import MID
    from hypervla.train import pack_params, unpack_params
    from publish_edge_values import overwrite_edge_blocks
    P = syn.synthetic_params(MID)
    P2 = overwrite_edge_blocks(P, MID)
    changed = [k for k in P if not np.array_equal(np.asarray(P[k]).reshape(-1), P2[k].reshape(-1))]
    assert len(changed) == 4, changed
    back = unpack_params(MID, pack_params(MID, P2, True), True)
    for k, val in back.items():
        assert np.array_equal(val.reshape(-1).view(np.uint32), np.asarray(P2[k], np.float32).reshape(-1).view(np.uint32)), k
