"""Host side of the fine-tune step's noise (hvla_train_noise_set; csrc/noise.h): the numpy restatement of the
counter-based generator against Random123's known answers and against csrc/noise.h itself, its statistics, the config mapping, and
the workspace extents of a step with every knob on."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from hypervla import train as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KAT = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


def _hex(words):
    return " ".join(f"{int(w):08x}" for w in words)


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10."""
    for ctr, key, want in KAT:
        assert _hex(T.philox4x32(np.array(ctr, np.uint32), np.array(key, np.uint32))) == want
    # vectorised: the three at once
    got = T.philox4x32(np.array([c for c, _, _ in KAT], np.uint32), np.array([k for _, k, _ in KAT], np.uint32))
    assert [_hex(r) for r in got] == [w for _, _, w in KAT]


@pytest.fixture(scope="module")
def noise_check(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("noise_check") / "noise_check"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                            "-Werror", "-I", os.path.join(ROOT, "hyper-vla_amd", "csrc"), os.path.join(ROOT, "tests", "native", "noise_check.cpp"),
                            "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr

    def run(*args):
        r = subprocess.run([str(exe)] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and not r.stderr, r.stdout + r.stderr
        return r.stdout.split("\n")[:-1]
    return run


def test_the_header_is_the_same_generator(noise_check):
    """csrc/noise.h (compiled for the host) gives the known answers, and for a seed above 2^32, a site with a layer and a sample index
    above 2^32 the words the numpy restatement gives; the thresholds agree where rate 2^24 is and is not an integer."""
    assert noise_check("kat") == [w for _, _, w in KAT]
    seed, site, sample, draw, n = 0x1234567890abcdef, T.noise_site(T.NOISE_MLP_HIDDEN, 5), 2 ** 32 + 77, 4000000000, 1031
    got = [int(w, 16) for w in noise_check("words", seed, site, sample, draw, n)]
    assert got == T.noise_words(seed, site, sample, draw, n).tolist()
    assert T.noise_words(seed, site, sample, draw, n).tolist() == T.noise_words(seed, site, 77, draw, n).tolist()      # the low 32 bits
    for rate in (0.0, 0.1, 0.25, 0.5, 1e-8, 0.999):
        assert int(noise_check("thr", repr(rate))[0]) == T.dropout_threshold(rate), rate
    assert T.dropout_threshold(0.25) == 2 ** 22 and T.dropout_threshold(0.0) == 0 and T.dropout_threshold(1e-8) == 1


@pytest.mark.parametrize("rate", [0.1, 0.25])
def test_keep_fraction(rate):
    n = 2 ** 20
    m = T.noise_multipliers(rate, seed=11, site=T.noise_site(T.NOISE_ATTN_OUT, 1), sample_id=3, draw=2, n=n)
    kp = np.float32(1) - np.float32(rate)
    assert set(np.unique(m).tolist()) == {0.0, float(np.float32(1) / kp)}
    p = 1.0 - T.dropout_threshold(rate) / 2.0 ** 24
    kept = float((m > 0).mean())
    sd = np.sqrt(p * (1 - p) / n)
    print(f"rate {rate}: kept {kept:.6f}, expected {p:.6f}, {abs(kept - p) / sd:.2f} sd")
    assert abs(kept - p) <= 5 * sd


def test_normals_mean_and_variance():
    n = 2 ** 20
    z = T.noise_normals(seed=5, site=T.noise_site(T.NOISE_TOKENS), sample_id=9, draw=1, n=n)
    assert z.dtype == np.float64 and z.shape == (n,) and np.isfinite(z).all()
    mean, var = float(z.mean()), float(z.var())
    print(f"normals: mean {mean:.3e} ({abs(mean) * np.sqrt(n):.2f} se), variance {var:.6f} ({abs(var - 1) / np.sqrt(2 / n):.2f} se)")
    assert abs(mean) <= 5 / np.sqrt(n)
    assert abs(var - 1.0) <= 5 * np.sqrt(2.0 / n)


def test_draws_are_a_function_of_every_counter_word():
    base = dict(seed=1, site=T.noise_site(T.NOISE_MLP_OUT, 0), sample_id=0, draw=0, n=64)
    w0 = T.noise_words(**base)
    assert (T.noise_words(**base) == w0).all()
    for change in (dict(seed=2), dict(seed=1 + 2 ** 32), dict(site=T.noise_site(T.NOISE_MLP_OUT, 1)), dict(site=T.noise_site(T.NOISE_ATTN_OUT, 0)),
                   dict(sample_id=1), dict(draw=1)):
        assert (T.noise_words(**dict(base, **change)) != w0).mean() > 0.9, change
    assert (T.noise_words(**dict(base, n=17)) == w0[:17]).all()           # a prefix: element e does not depend on n


def test_train_noise_from_config():
    from hypervla.config import MID, default_config
    cfg = default_config(MID)
    off = dict(dropout_rate=0.0, image_embedding_noise=0.0, embedding_dropout_rate=0.0, image_dropout=0.0)
    assert T.train_noise_from_config(cfg) == off
    cfg["base_net_kwargs"]["vit_kwargs"].update(dropout_rate=0.1, image_embedding_noise=0.05)
    cfg["hypernet_kwargs"].update(embedding_dropout_rate=0.2, image_dropout=0.3)
    want = dict(dropout_rate=0.1, image_embedding_noise=0.05, embedding_dropout_rate=0.2, image_dropout=0.3)
    assert T.train_noise_from_config(cfg) == want
    assert T.train_noise_from_config({"model": cfg}) == want
    # the mapping's keys are FineTuner's keywords
    import inspect
    assert set(want) <= set(inspect.signature(T.FineTuner.__init__).parameters)
    for where, key in ((("hypernet_kwargs", "context_encoder_kwargs"), "dropout_rate"),
                       (("hypernet_kwargs", "context_encoder_kwargs"), "attention_dropout_rate"), (("hypernet_kwargs",), "final_dropout_rate")):
        bad = default_config(MID)
        d = bad
        for k in where:
            d = d[k]
        d[key] = 0.1
        with pytest.raises(ValueError, match=r"\." + key + "="):
            T.train_noise_from_config(bad)
        d[key] = 0.0
        assert T.train_noise_from_config(bad) == off


# ---- workspace extents with every knob on (tools/train_extent_trace.hip's noise=1 points)
@pytest.fixture(scope="module")
def points(tmp_path_factory):
    from test_train_workspace_extents import HIPCC, trace
    if not os.path.exists(HIPCC):
        pytest.skip("needs hipcc")
    return trace(tmp_path_factory.mktemp("noise_extent_trace"))


NOISE_KERNELS = ("dropout_fwd_kernel", "dropout_bwd_kernel", "token_noise_kernel")


def _mid(points, enc, noise):
    tail = " noise=1"
    pts = [p for p in points if p["title"].startswith("MID L=2 ") and f" B=4 enc={enc} " in p["title"] and p["title"].endswith(tail) == noise
           and " forward_only=0 frozen_buckets=0 frozen=0 aux=0 " in p["title"]]
    assert len(pts) == 1, [p["title"] for p in pts]
    return pts[0]


@pytest.mark.parametrize("enc", [0, 1])
def test_noise_points_obey_the_extent_rules(points, enc):
    """MID, B = 4, all four knobs on, encoder frozen and trained: the rules of tests/test_train_workspace_extents.py hold -- the
    branch temporary t.y, the token copy and the CLS copy are whole plan buffers, nothing passes the reported size -- every buffer of
    the noise-off plan keeps its offset, and the size grows by exactly the copies."""
    from test_train_workspace_extents import _Checker
    on, off = _mid(points, enc, True), _mid(points, enc, False)
    bad = _Checker(on).run()
    assert not bad, "\n".join(bad[:10])
    assert on["plan"][:len(off["plan"])] == off["plan"]
    extra = {n: sz for n, _, sz in on["plan"][len(off["plan"]):]}
    B, P, E = 4, 64, 128
    assert extra == ({"ntok": B * P * E, "ncls": B * E} if enc == 0 else {"ncls": B * E}), extra
    assert on["workspace"] - off["workspace"] == sum(extra.values())
    names = [ln.split(" ")[0] for ln in on["lines"]]
    L = 2
    assert names.count("token_noise_kernel") == 1
    # forward: site 1, sites 2-4 per layer, the context, the CLS rows; backward: site 1, sites 2-4 per layer, the context
    assert names.count("dropout_fwd_kernel") == 1 + 3 * L + 2 and names.count("dropout_bwd_kernel") == 1 + 3 * L + 1
    assert not any(ln.split(" ")[0] in NOISE_KERNELS for ln in off["lines"])
    # the policy's residual GEMMs no longer accumulate into a copy of the residual: two copies per layer fewer
    copies = lambda pt: sum(ln.startswith("hipMemcpyAsync ") for ln in pt["lines"])
    assert copies(off) - copies(on) == 2 * L
