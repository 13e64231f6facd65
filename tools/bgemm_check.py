"""Diagnostic (GPU box): ONE launch of the fine-tune path's batched GEMM (csrc/train_gemm.hip bgemm()) per case of a table, every field of
the descriptor BG (csrc/train.h) in the table's hands, against float64 (libhvla_bench.so: hvla_debug_bgemm_once launches once, synchronises
and reports which kernel form bgemm_launch chose).  One line per case, ending in ` ok` or in the failing figures; then the number of
cases per kernel instantiation.  tests/test_gpu_train_gemm.py runs this file once; tests/test_train_gemm_reference.py runs the same
table through a CPU emulation of the kernel's arithmetic (no GPU).

Two input classes per descriptor.

  exact      Operand elements are a + b 2^-10 with a in {-1, +1}, b in {-1, 0, +1}: bf16(x) = a and bf16(x - a) = b 2^-10 exactly, so the
             three products the kernel keeps (hi hi + hi lo + lo hi) are multiples of 2^-10 and every partial sum of them, in ANY order,
             is below 2^24 such units while  depth * 1026 <= 2^24  (depth = K times the batch entries that share one C; K <= 16 352).
             f32 accumulation is then exact, the atomic split-K reduction included.  alpha is a power of two >= 2^-3, bias and the
             initial C are small multiples of 2^-10, so the stored value is exact too (units of 2^-13, asserted per case together with
             the depth condition).  Deeper products (K = 201 500) keep the condition by thinning A to every d-th k (zeros elsewhere).
             Expected = that three-term product in float64 on the restated halves; comparison BITWISE over the whole C buffer.
             With b = 0 the same inputs are exact for the f32 kernel (bgemm_kernel).
  precision  Standard-normal operands, K <= 257.  Component-wise
                 |C - C64| <= tau (|alpha| |A| |B|)_mn + 2^-23 |C64|,   tau = 2^-14 + K 2^-23
             Derivation: x = hi + lo leaves 2^-16 of x per operand (two 8-bit significands with round-to-nearest: 2^-9 x 2^-9 / 4 each
             side of the product, 2 x 2^-17 = 2^-16 together); the dropped lo lo term is at most 2^-9 x 2^-9 / 4 = 2^-20 ... 2^-16 of
             |a||b| depending on where the halves round, bounded by 2^-16; f32 accumulation of K terms is at most K 2^-24 of the sum of
             the magnitudes; a factor below 2 covers the rest (alpha's rounding, second-order terms): 2 x (2^-16 + 2^-16) = 2^-14 and
             2 x K 2^-24.  2^-23 |C64| is the two final roundings (alpha acc + bias, old + v).  K counts every term that reaches one
             C element (batch entries that share a C multiply it).  bgemm_kernel (f32 instruction): tau = (K + 2) 2^-24.
             A product that misses one cross term sits at 7 - 55 x this bound for K <= 257 and INSIDE it from K = 3 072 up, which is
             why deep K belongs to the exact class.

Every case also checks the memory contract: C is pre-filled with a sentinel and must be bit-unchanged outside [M] x [N] of every batch
entry (columns N .. ldc - 1, rows past M, gaps between batch strides, a guard band around the buffer); everything in the operand buffers
that belongs to no batch entry is NaN (row slack up to ld, gaps between batch entries, guard bands of >= 64 floats), except the a_padded
contract's zeros up to the next multiple of 4 inside lda -- an over-read that reaches the matrix cores shows as NaN in C.

    python tools/bgemm_check.py            (GPU)       exit status 0 = every case ok and every instantiation hit
"""
import ctypes as C
import math
import os
import sys
import time
from dataclasses import dataclass, replace
from typing import Optional

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64                     # floats of guard band before and after every buffer (operands: NaN, C: sentinel)
SENTINEL = np.float32(1.2345678)
UNIT = 2.0 ** -10
ORDERS = {"NN": (0, 0), "NT": (0, 1), "TN": (1, 0), "TT": (1, 1)}


@dataclass
class Case:
    name: str
    group: str
    cls: str                   # "exact" | "precision"
    order: str                 # NN / NT / TN / TT
    M: int
    N: int
    K: int
    nb0: int = 1
    nb1: int = 1
    lda: int = 0               # 0 = dense
    ldb: int = 0
    ldc: int = 0
    sA0: Optional[int] = None  # None = dense (behind the inner batch)
    sA1: Optional[int] = None
    sB0: Optional[int] = None
    sB1: Optional[int] = None
    sC0: Optional[int] = None
    sC1: Optional[int] = None
    bias: bool = False
    sBias0: Optional[int] = None
    sBias1: Optional[int] = None
    alpha: float = 1.0
    accumulate: int = 0
    ksplit: int = 1
    allow_split: int = 0
    a_padded: int = 0
    offA: int = 0              # floats added to the (16-byte aligned) operand pointer
    offB: int = 0
    f32: bool = False          # bgemm_kernel (hvla_debug_train_gemm_exact)
    seed: int = 0
    shrink: bool = True        # the CPU companion may cut nb0 (never an edge size)
    expect_ksplit: int = 0     # > 0: the split the case exists for; the launcher's report must say so (the dispatch itself is not restated)
    fold: str = ""             # "M" / "K": that extent is a batch of `fold_rows`-row blocks folded into one matrix (shared weights); the CPU
    fold_rows: int = 0         #            companion may cut the number of blocks (a batch count) to 3

    def __post_init__(self):
        ta, tb = ORDERS[self.order]
        self.ta, self.tb = ta, tb
        self.ar, self.ac = (self.K, self.M) if ta else (self.M, self.K)        # rows x contiguous extent of A in memory
        self.br, self.bc = (self.N, self.K) if tb else (self.K, self.N)
        self.lda = self.lda or self.ac
        self.ldb = self.ldb or self.bc
        self.ldc = self.ldc or self.N
        d = lambda v, dense: dense if v is None else v
        self.sA1 = d(self.sA1, self.ar * self.lda); self.sA0 = d(self.sA0, self.nb1 * self.sA1)
        self.sB1 = d(self.sB1, self.br * self.ldb); self.sB0 = d(self.sB0, self.nb1 * self.sB1)
        self.sC1 = d(self.sC1, self.M * self.ldc); self.sC0 = d(self.sC0, self.nb1 * self.sC1)
        self.sBias1 = d(self.sBias1, self.N); self.sBias0 = d(self.sBias0, self.nb1 * self.sBias1)
        self.a_pad_cols = ((self.ac + 3) & ~3) if (self.a_padded and self.lda >= ((self.ac + 3) & ~3)) else self.ac

    @property
    def shared(self):          # batch entries that add into one C element
        n = 1
        if self.sC0 == 0:
            n *= self.nb0
        if self.sC1 == 0:
            n *= self.nb1
        return n


def _span(nb0, nb1, s0, s1, rows, cols, ld):
    return (nb0 - 1) * s0 + (nb1 - 1) * s1 + (rows - 1) * ld + cols


def _view(buf, off, nb0, nb1, s0, s1, rows, cols, ld):
    return torch.as_strided(buf, (nb0, nb1, rows, cols), (s0, s1, ld, 1), off)


def thinning(c):
    """every d-th k of A keeps its value (exact class): the smallest d with ceil(K / d) * shared * 1026 <= 2^24 - the stored-value head room"""
    d = 1
    while math.ceil(c.K / d) * c.shared * 1026 > 2 ** 24 - 2 ** 16:
        d += 1
    return d


def make_inputs(c):
    """host buffers (float32 torch tensors, guard bands included) and the offsets of element [0] of each operand inside them"""
    rng = np.random.default_rng(1000 + c.seed)

    def draw(shape, lo_terms):
        n = int(np.prod(shape))
        if c.cls == "exact":
            a = rng.integers(0, 2, n).astype(np.float32) * 2 - 1
            b = rng.integers(-1, 2, n).astype(np.float32) if lo_terms else np.zeros(n, np.float32)
            return torch.from_numpy((a + b * np.float32(UNIT)).reshape(shape))
        return torch.from_numpy(rng.standard_normal(n).astype(np.float32).reshape(shape))

    def small(shape):          # bias / initial C
        n = int(np.prod(shape))
        if c.cls == "exact":
            return torch.from_numpy((rng.integers(-8, 9, n).astype(np.float32) * np.float32(UNIT)).reshape(shape))
        return torch.from_numpy(rng.standard_normal(n).astype(np.float32).reshape(shape))

    out = {}
    for nm, off, s0, s1, rows, cols, ld in (("A", c.offA, c.sA0, c.sA1, c.ar, c.ac, c.lda), ("B", c.offB, c.sB0, c.sB1, c.br, c.bc, c.ldb)):
        n = _span(c.nb0, c.nb1, s0, s1, rows, cols if nm == "B" else c.a_pad_cols, ld)
        buf = torch.full((GUARD + off + n + GUARD + 4,), float("nan"), dtype=torch.float32)
        if nm == "A" and c.a_pad_cols != c.ac:
            _view(buf, GUARD + off, c.nb0, c.nb1, s0, s1, rows, c.a_pad_cols, ld).zero_()
        e0, e1 = (1 if s0 == 0 else c.nb0), (1 if s1 == 0 else c.nb1)            # a zero stride: the batch entries read one operand
        vals = draw((e0, e1, rows, cols), not c.f32)
        if nm == "A" and c.cls == "exact":
            d = thinning(c)
            if d > 1:
                k = torch.arange(c.K).reshape((c.K, 1) if c.ta else (1, c.K))
                m = torch.arange(c.M).reshape((1, c.M) if c.ta else (c.M, 1))
                vals = vals * ((k + 7 * m) % d == 0)
        _view(buf, GUARD + off, e0, e1, s0, s1, rows, cols, ld).copy_(vals)
        out[nm], out["o" + nm] = buf, GUARD + off
    n = _span(c.nb0, c.nb1, c.sC0, c.sC1, c.M, c.N, c.ldc)
    cbuf = torch.full((GUARD + n + GUARD,), float(SENTINEL), dtype=torch.float32)
    if c.accumulate:
        e0, e1 = (1 if c.sC0 == 0 else c.nb0), (1 if c.sC1 == 0 else c.nb1)      # batch entries that share a C: one initial value per element
        _view(cbuf, GUARD, e0, e1, c.sC0, c.sC1, c.M, c.N, c.ldc).copy_(small((e0, e1, c.M, c.N)))
    out["C"], out["oC"] = cbuf, GUARD
    if c.bias:
        n = (c.nb0 - 1) * c.sBias0 + (c.nb1 - 1) * c.sBias1 + c.N
        bbuf = torch.full((GUARD + n + GUARD,), float("nan"), dtype=torch.float32)
        e0, e1 = (1 if c.sBias0 == 0 else c.nb0), (1 if c.sBias1 == 0 else c.nb1)
        torch.as_strided(bbuf, (e0, e1, c.N), (c.sBias0, c.sBias1, 1), GUARD).copy_(small((e0, e1, c.N)))
        out["bias"], out["obias"] = bbuf, GUARD
    return out


def split_bf16(x):
    """x (f32) -> hi, lo as the kernel's split1(): hi = bf16(x), lo = bf16(x - hi); both returned as f32"""
    hi = x.to(torch.bfloat16).to(torch.float32)
    lo = (x - hi).to(torch.bfloat16).to(torch.float32)
    return hi, lo


def dense_operands(c, inp):
    """op(A) [nb0][nb1][M][K] and op(B) [nb0][nb1][K][N] gathered through the descriptor's strides (f32)"""
    a = _view(inp["A"], inp["oA"], c.nb0, c.nb1, c.sA0, c.sA1, c.ar, c.ac, c.lda)
    b = _view(inp["B"], inp["oB"], c.nb0, c.nb1, c.sB0, c.sB1, c.br, c.bc, c.ldb)
    return (a.transpose(2, 3) if c.ta else a), (b.transpose(2, 3) if c.tb else b)


def assert_exactness(c, inp):
    """the exact class's condition, from K, the batch entries that share a C and the ranges drawn -- before anything is launched"""
    assert c.cls == "exact"
    a, b = dense_operands(c, inp)
    for x in (a, b):
        hi, lo = split_bf16(x)
        assert bool(((hi.abs() == 1) | (hi == 0)).all()) and bool((lo.abs() <= UNIT).all()) and torch.equal(hi + lo, x.contiguous()), c.name
        if c.f32:
            assert not bool(lo.any()), c.name
    depth = int((a != 0).sum(-1).max()) * c.shared                                        # terms that reach one C element
    la = math.log2(c.alpha)
    assert la == int(la) and -3 <= la <= 0, (c.name, c.alpha)
    # the stored value in units of alpha 2^-10: every product <= 1026, |bias| (once per batch entry) and |C0| <= 8 / alpha <= 64 each
    assert depth * 1026 + 64 * (c.shared + 1) <= 2 ** 24, (c.name, depth)
    return depth


def reference(c, inp):
    """(expected C buffer in float64, tolerance buffer): the float64 product through every stride, transpose and batch field.
    exact class: the three kept terms on the restated halves, tolerance 0.  precision class: the true product and the bound."""
    a, b = dense_operands(c, inp)
    want = inp["C"].to(torch.float64)
    absb = torch.zeros_like(want)
    sh = (1 if c.sC0 == 0 else c.nb0, 1 if c.sC1 == 0 else c.nb1)
    wv = _view(want, inp["oC"], c.nb0, c.nb1, c.sC0, c.sC1, c.M, c.N, c.ldc)
    av = _view(absb, inp["oC"], c.nb0, c.nb1, c.sC0, c.sC1, c.M, c.N, c.ldc)
    bias = torch.as_strided(inp["bias"], (c.nb0, c.nb1, c.N), (c.sBias0, c.sBias1, 1), inp["obias"]).to(torch.float64) if c.bias else None
    for i in range(c.nb0):
        for j in range(c.nb1):
            a32, b32 = a[i, j].contiguous(), b[i, j].contiguous()
            if c.cls == "exact" and not c.f32:
                ah, al = split_bf16(a32)
                bh, _ = split_bf16(b32)
                p = ah.double() @ b32.double() + al.double() @ bh.double()        # hi hi + hi lo + lo hi  (b = bh + bl exactly)
            else:
                p = a32.double() @ b32.double()
            v = c.alpha * p if c.cls == "exact" else float(np.float32(c.alpha)) * p
            if bias is not None:
                v = v + bias[i, j]
            if c.accumulate:
                wv[i, j] += v
            else:
                wv[i, j] = v
            if c.cls == "precision":
                av[i, j] += abs(float(np.float32(c.alpha))) * (a32.double().abs() @ b32.double().abs())
    if c.cls == "exact":
        return want, absb
    depth = c.K * c.shared
    tau = (depth + 2) * 2.0 ** -24 if c.f32 else 2.0 ** -14 + depth * 2.0 ** -23
    tol = tau * absb
    inside = absb > 0
    tol[inside] += 2.0 ** -23 * want[inside].abs()
    return want, tol


def compare(c, got, want, tol):
    """-> (ok, worst err / bound, text).  exact: bit patterns of the whole buffer.  precision: |got - want| <= tol (0 outside [M] x [N]: the sentinel)."""
    if c.cls == "exact":
        w32 = want.to(torch.float32)
        assert torch.equal(w32.double(), want), c.name                       # the expected value is an f32
        bad = got.view(torch.int32) != w32.view(torch.int32)
        nbad = int(bad.sum())
        if nbad == 0:
            return True, 0.0, "bitwise"
        i = int(bad.nonzero()[0])
        d = (got.double() - want).abs()
        d[~torch.isfinite(d)] = float("inf")
        return False, float("inf"), f"{nbad} of {got.numel()} words differ, first at {i - GUARD}: kernel {float(got[i])!r} expected {float(want[i])!r}; max |d| {float(d.max()):.3e}"
    d = (got.double() - want).abs()
    ok = d <= tol                                                            # NaN compares false
    ratio = torch.where(tol > 0, d / tol.clamp_min(1e-300), torch.zeros_like(d))
    worst = float(ratio[torch.isfinite(ratio)].max()) if bool(torch.isfinite(ratio).any()) else 0.0
    if bool(ok.all()):
        return True, worst, f"err/bound {worst:.3f}"
    i = int((~ok).nonzero()[0])
    return False, worst, (f"{int((~ok).sum())} of {got.numel()} outside the bound, first at {i - GUARD}: kernel {float(got[i])!r} expected {float(want[i])!r} "
                          f"bound {float(tol[i]):.3e}; worst err/bound {worst:.2f}")


# ------------------------------------------------------------------------------------------------ CPU emulation of the kernel
def emulate(c, inp, rng, drop=None):
    """The kernel's arithmetic on the CPU: operands split into bf16 halves, f32 accumulation in 16-deep chunks (lo hi, hi lo, hi hi per
    chunk, as mma32_x3), K cut into `ksplit` 32-rounded chunks that are added into C in random order, batch entries in random order;
    the store modes, alpha and bias as the epilogue has them.  `drop` = "lohi": without the a.lo b.hi term; "bias_every_chunk": the
    bias added by every K chunk (the mutations of the pull request's description).  -> C buffer (f32)"""
    a, b = dense_operands(c, inp)
    out = inp["C"].clone()
    cv = _view(out, inp["oC"], c.nb0, c.nb1, c.sC0, c.sC1, c.M, c.N, c.ldc)
    bias = torch.as_strided(inp["bias"], (c.nb0, c.nb1, c.N), (c.sBias0, c.sBias1, 1), inp["obias"]) if c.bias else None
    ks = c.ksplit
    if c.allow_split and c.accumulate and ks == 1 and c.K >= 256:
        ks = min(3, c.K // 128)                                              # any split: the launcher's own choice is not restated here
    step = 16 if not c.f32 else 2
    kchunk = (-(-c.K // ks) + 31) & ~31 if not c.f32 else (-(-c.K // ks) + 15) & ~15
    alpha = torch.tensor(c.alpha, dtype=torch.float32)
    entries = [(i, j, kc) for i in range(c.nb0) for j in range(c.nb1) for kc in range(ks)]
    for n in rng.permutation(len(entries)):
        i, j, kc = entries[n]
        a32, b32 = a[i, j].contiguous(), b[i, j].contiguous()
        acc = torch.zeros((c.M, c.N), dtype=torch.float32)
        k0, k1 = kc * kchunk, min(c.K, (kc + 1) * kchunk)
        if c.f32:
            if k1 > k0:
                acc = a32[:, k0:k1] @ b32[k0:k1]
        else:
            ah, al = split_bf16(a32)
            bh, bl = split_bf16(b32)
            st = step if c.M * c.N * c.K * c.nb0 * c.nb1 <= 1 << 25 else 256    # 16 deep only where that is affordable
            for k in range(k0, k1, st):
                e = min(k + st, k1)
                if drop != "lohi":
                    acc += al[:, k:e] @ bh[k:e]
                acc += ah[:, k:e] @ bl[k:e]
                acc += ah[:, k:e] @ bh[k:e]
        v = alpha * acc
        if bias is not None and (kc == 0 or drop == "bias_every_chunk"):
            v = v + bias[i, j]
        if c.accumulate or ks > 1:
            cv[i, j] += v
        else:
            cv[i, j] = v
    return out


# ------------------------------------------------------------------------------------------------ the case table
def case_table():
    t = []
    seed = [0]

    def add(name, group, cls, order, M, N, K, **kw):
        seed[0] += 1
        t.append(Case(name, group, cls, order, M, N, K, seed=seed[0], **kw))

    # ---- calibration: one full 64 x 64 tile, K = 32, NN (is the bf16 matrix instruction's f32 accumulate exact on representable sums?)
    add("calibration 64x64x32 NN", "calibration", "exact", "NN", 64, 64, 32)
    for cls, g, al in (("exact", "forms", 1.0), ("precision", "precision forms", 0.125)):
        kx = (100, 33, 96, 97, 64)
        for o in ORDERS:
            add(f"{o} 64 vec", g, cls, o, 92, 68, kx[0], alpha=al)
            add(f"{o} 64 dword", g, cls, o, 95, 31, kx[1], alpha=al)
            add(f"{o} 128 vec", g, cls, o, 128, 132, kx[2], alpha=al)
            add(f"{o} 128 dword", g, cls, o, 129, 127, kx[3], alpha=al)
            add(f"{o} 256 vec, M = 384 (half-empty second row tile), nb0 = 100", g, cls, o, 384, 128, kx[4], nb0=100, alpha=al)
    # ---- every way the launcher reaches the all-dword staging (and the a_padded exception), on sizes that would otherwise be float4
    for o in ("NN", "TN", "NT", "TT"):
        for T_, (M, N) in ((64, (64, 64)), (128, (128, 128))):
            g = "dword reasons"
            add(f"{o} {T_} A pointer off by one float", g, "exact", o, M, N, 64, offA=1)
            add(f"{o} {T_} B pointer off by one float", g, "exact", o, M, N, 64, offB=1)
            add(f"{o} {T_} lda % 4 != 0", g, "exact", o, M, N, 64, lda=(M if ORDERS[o][0] else 64) + 1)
            add(f"{o} {T_} ldb % 4 != 0", g, "exact", o, M, N, 64, ldb=(64 if ORDERS[o][1] else N) + 3)
            add(f"{o} {T_} sA0 % 4 != 0", g, "exact", o, M, N, 64, nb0=3, sA0=M * 64 + 2)
            add(f"{o} {T_} sB1 % 4 != 0", g, "exact", o, M, N, 64, nb1=2, sB1=N * 64 + 1)
            add(f"{o} {T_} K % 4 != 0", g, "exact", o, M, N, 66)
            add(f"{o} {T_} M % 4 != 0", g, "exact", o, M + 1, N, 64)
            add(f"{o} {T_} N % 4 != 0", g, "exact", o, M, N + 2, 64)
    for o in ("NN", "TN"):
        ext = dict(NN=dict(M=128, K=257), TN=dict(M=257, K=128))[o]
        add(f"{o} a_padded, lda = 260: float4 staging over the row's end", "a_padded", "exact", o, ext["M"], 128, ext["K"], lda=260, a_padded=1)
        add(f"{o} a_padded, lda = 257 too short for it: dword", "a_padded", "exact", o, ext["M"], 128, ext["K"], lda=257, a_padded=1)
        add(f"{o} a_padded 64 tile, lda = 260", "a_padded", "exact", o, min(ext["M"], 257), 64, ext["K"], lda=260, a_padded=1)
        add(f"{o} a_padded precision, lda = 260", "precision a_padded", "precision", o, ext["M"], 128, ext["K"], lda=260, a_padded=1, alpha=0.125)
    # ---- M, N around the tile and selection edges
    edges = [(1, 128), (31, 129), (64, 64), (95, 96), (96, 95), (96, 96), (127, 128), (128, 127), (129, 257), (257, 31), (257, 257), (384, 128), (128, 384), (1, 1)]
    for o in ORDERS:
        for M, N in edges:
            add(f"{o} M = {M} N = {N} K = 36", "edges", "exact", o, M, N, 36)
        for M, N in ((1, 31), (31, 1), (95, 127), (129, 129)):
            add(f"{o} M = {M} N = {N} K = 33", "edges", "exact", o, M, N, 33)
    add("NN N = 201 500 = 1574 x 128 + 28 column tail, M = 96", "edges", "exact", "NN", 96, 201500, 32)
    add("NN N = 201 500 column tail, M = 1 (64 tile)", "edges", "exact", "NN", 1, 201500, 32)
    # ---- K: short, and around one whole group of register stages (dword: 2 x 32, float4: 3 x 32)
    for K in (1, 3, 4, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 191, 192, 193, 257, 260):
        for T_ in (64, 128):
            g = "k depth"
            add(f"TN {T_} K = {K} (float4 at any K)", g, "exact", "TN", T_, T_, K)
            add(f"TN {T_} K = {K} dword", g, "exact", "TN", T_, T_, K, offA=1)
            add(f"NT {T_} K = {K}", g, "exact", "NT", T_, T_, K)
            add(f"NT {T_} K = {K} dword", g, "exact", "NT", T_, T_, K, offB=1)
            add(f"NN {T_} K = {K}", g, "exact", "NN", T_, T_, K)
            add(f"TT {T_} K = {K}", g, "exact", "TT", T_, T_, K)
    for K in (1, 3, 31, 33, 97, 257):
        for o in ORDERS:
            add(f"{o} K = {K}", "precision k depth", "precision", o, 64, 68, K)
    # ---- split-K chosen by the launcher: 2, 3, K / 128 chunks, and a last chunk that is EMPTY (K = 1 290: kchunk 160, chunk 9 starts past K)
    for T_ in (64, 128):
        for o in ("TN", "NN", "NT", "TT"):
            g = f"split-K {T_}"
            add(f"{o} {T_} launcher split 2 (256 tiles, K = 256)", g, "exact", o, T_, T_, 256, nb0=256, accumulate=1, allow_split=1, expect_ksplit=2)
            add(f"{o} {T_} launcher split 3 (200 tiles, K = 388)", g, "exact", o, T_, T_, 388, nb0=200, accumulate=1, allow_split=1, expect_ksplit=3)
            add(f"{o} {T_} launcher split K / 128 = 10, last chunk empty (K = 1 290)", g, "exact", o, T_, T_, 1290, accumulate=1, allow_split=1, expect_ksplit=10)
            add(f"{o} {T_} launcher split with bias: added once (K = 1 290)", g, "exact", o, T_, T_, 1290, accumulate=1, allow_split=1, bias=True, expect_ksplit=10)
            add(f"{o} {T_} launcher split, K = 16 288 on 3 x 2 tiles", g, "exact", o, 3 * T_ - 5, 2 * T_, 16288, accumulate=2, allow_split=1)
        add(f"TN {T_} explicit ksplit 4, K = 257, bias", f"split-K {T_}", "exact", "TN", T_, T_, 257, accumulate=1, ksplit=4, bias=True)
        add(f"TN {T_} explicit ksplit 5, K = 257, bias", "precision split-K", "precision", "TN", T_, T_ + 4, 257, accumulate=1, ksplit=5, bias=True, alpha=0.125)
    # ---- store modes, bias, alpha, ldc > N, two batch levels
    for o in ORDERS:
        for T_, (M, N) in ((64, (60, 52)), (128, (130, 100))):
            for acc in (0, 1, 2):
                add(f"{o} {T_} accumulate {acc}, bias, ldc = N + 5, alpha 2^-3", "modes", "exact", o, M, N, 40, accumulate=acc, bias=True, ldc=N + 5, alpha=0.125, nb0=3, nb1=2)
                add(f"{o} {T_} accumulate {acc}, bias, ldc = N + 5, alpha 1/sqrt(48)", "precision modes", "precision", o, M, N, 40, accumulate=acc, bias=True, ldc=N + 5,
                    alpha=1 / math.sqrt(48.0), nb0=3, nb1=2)
            add(f"{o} {T_} accumulate 2, 5 batch entries share one C (sC0 = 0)", "modes", "exact", o, M, N, 36, accumulate=2, nb0=5, sC0=0)
            add(f"{o} {T_} accumulate 2, 5 batch entries share one C (sC0 = 0)", "precision modes", "precision", o, M, N, 36, accumulate=2, nb0=5, sC0=0)
    # sub-matrix strides: the heads of one [S][D] row block interleave inside a row (sA1 = hd inside lda = D), C as [H][S][Sp]
    S, H, hd = 65, 4, 16
    D, Sp = H * hd, (S + 3) & ~3
    for cls, al in (("exact", 0.25), ("precision", 1 / math.sqrt(hd))):
        g = "two batch levels" if cls == "exact" else "precision two batch levels"
        add("NT scores: sA1 = hd inside lda = D, sC1 = S Sp, ldc = Sp", g, cls, "NT", S, S, hd, nb0=3, nb1=H, lda=D, ldb=D, ldc=Sp, sA0=S * D, sA1=hd, sB0=S * D, sB1=hd,
            sC0=H * S * Sp, sC1=S * Sp, alpha=al)
        add("NN p v: A [H][S][Sp] padded, B and C interleaved heads", g, cls, "NN", S, hd, S, nb0=3, nb1=H, lda=Sp, ldb=D, ldc=D, sA0=H * S * Sp, sA1=S * Sp, sB0=S * D, sB1=hd,
            sC0=S * D, sC1=hd, a_padded=1, alpha=al)
        add("TN p^T do: A [H][S][Sp] padded", g, cls, "TN", S, hd, S, nb0=3, nb1=H, lda=Sp, ldb=D, ldc=D, sA0=H * S * Sp, sA1=S * Sp, sB0=S * D, sB1=hd, sC0=S * D, sC1=hd,
            a_padded=1, alpha=al)
        add("NN three products in one launch: sB1, sC1, sBias1 (bias with two batch strides)", g, cls, "NN", 70, 64, 64, nb0=2, nb1=3, sA1=0, sA0=70 * 64, sB1=64 * 64 + 64,
            sB0=3 * (64 * 64 + 64) + 8, sC1=2 * 70 * 64 + 4, sC0=70 * 64, bias=True, sBias1=64 * 64 + 64, sBias0=7, alpha=al)
    # ---- the f32 kernel (hvla_debug_train_gemm_exact): integer inputs
    for o in ORDERS:
        add(f"{o} f32 kernel 95 x 129 x 33", "f32 kernel", "exact", o, 95, 129, 33, f32=True)
        add(f"{o} f32 kernel accumulate 1, bias, batches", "f32 kernel", "exact", o, 64, 64, 48, f32=True, accumulate=1, bias=True, nb0=2, nb1=2, alpha=0.5)
        add(f"{o} f32 kernel split 10 with an empty chunk, K = 1 290", "f32 kernel", "exact", o, 70, 64, 1290, f32=True, accumulate=1, allow_split=1, bias=True)
        add(f"{o} f32 kernel K = 97", "precision f32 kernel", "precision", o, 95, 129, 97, f32=True, bias=True, alpha=1 / math.sqrt(16.0))
    # ---- call-site replay: the descriptors train_step issues at the README geometry with the encoder trained
    for B in (1, 32):
        t.extend(replay_cases(B, seed))
    return t


def replay_cases(B, seed):
    """csrc/train.hip train_step / block_fwd / block_bwd, by formula from the README geometry (Geometry() of hypervla/config.py)."""
    sys.path.insert(0, os.path.join(ROOT, "hyper-vla_amd"))
    from hypervla.config import FULL as g, generated_leaves
    P, S, D, H, F, E = g.patches, g.seq, g.dim, g.heads, g.mlp, g.enc_dim
    He, Fe, Kp = g.enc_heads, g.enc_mlp, g.patch_in
    Cx, Hc, Fc, T, Sc, lang = g.ctx_dim, g.ctx_heads, g.ctx_mlp, g.lang_tokens, g.ctx_seq, g.lang_dim
    G = sum(l.size for l in generated_leaves(g))
    assert (G, S, Kp) == (201500, 257, 588)
    out = []
    grp = f"replay B = {B}"

    def add(name, order, M, N, K, **kw):
        seed[0] += 1
        kw.setdefault("alpha", 1.0)
        out.append(Case(f"B = {B}: {name}", grp, "exact", order, M, N, K, seed=seed[0], **kw))

    def blocks(tag, nb, S_, D_, H_, F_, shared, big):
        hd, Sp, rows = D_ // H_, (S_ + 3) & ~3, nb * S_
        al = 2.0 ** round(math.log2(1.0 / math.sqrt(hd)))                     # exact class: the power of two next to 1 / sqrt(hd) (hd = 32: 2^-2)
        att = dict(nb0=nb if not big else 2, nb1=H_, shrink=True)
        ss0, ss1 = H_ * S_ * Sp, S_ * Sp
        qk = dict(lda=D_, ldb=D_, sA0=S_ * D_, sA1=hd, sB0=S_ * D_, sB1=hd)
        pa = dict(lda=Sp, ldb=D_, ldc=D_, sA0=ss0, sA1=ss1, sB0=S_ * D_, sB1=hd, sC0=S_ * D_, sC1=hd, a_padded=1)
        add(f"{tag} scores = q k^T / sqrt(hd)", "NT", S_, S_, hd, ldc=Sp, sC0=ss0, sC1=ss1, alpha=al, **qk, **att)
        add(f"{tag} o = p v", "NN", S_, hd, S_, **pa, **att)
        add(f"{tag} dp = do v^T", "NT", S_, S_, hd, ldc=Sp, sC0=ss0, sC1=ss1, **qk, **att)
        add(f"{tag} dv = p^T do", "TN", S_, hd, S_, **pa, **att)
        add(f"{tag} dq = ds k / sqrt(hd)", "NN", S_, hd, S_, alpha=al, **pa, **att)
        add(f"{tag} dk = ds^T q / sqrt(hd)", "TN", S_, hd, S_, alpha=al, **pa, **att)
        if shared:
            lin = [("wo", D_, D_, 0), ("fc1", D_, F_, 0), ("fc2", F_, D_, 0)]
            fm, fk = dict(fold="M", fold_rows=S_), dict(fold="K", fold_rows=S_)
            for nm, K, N, acc in lin:
                add(f"{tag} linear {nm} (rows folded into M)", "NN", rows, N, K, bias=True, accumulate=acc, **fm)
                add(f"{tag} linear_dx {nm}", "NT", rows, K, N, **fm)
                add(f"{tag} wgrad {nm} = X^T dY (launcher split-K)", "TN", K, N, rows, accumulate=1, allow_split=1, **fk)
            add(f"{tag} linear_dx accumulate 1 (dh += dk Wk^T)", "NT", rows, D_, D_, accumulate=1, **fm)
            ws = D_ * D_ + D_                                                  # kb | kk | qb | qk | vb | vk: leaves of one layer, bias in front of kernel
            ys = (rows * D_ + 3) & ~3
            add(f"{tag} q, k, v in one launch (nb1 = 3)", "NN", rows, D_, D_, nb1=3, sA1=0, sB1=ws, sC1=ys, bias=True, sBias1=ws, **fm)
            add(f"{tag} wgrad q, k, v in one launch (nb1 = 3, launcher split-K)", "TN", D_, D_, rows, nb1=3, sA1=0, sB1=ys, sC1=ws, accumulate=1, allow_split=1, **fk)
        else:
            nbb = nb if not big else 2
            for nm, K, N in (("wq", D_, D_), ("fc1", D_, F_), ("fc2", F_, D_)):
                add(f"{tag} linear {nm} (per-episode weights, stride G)", "NN", S_, N, K, nb0=nbb, sA0=S_ * K, sB0=G, sC0=S_ * N, bias=True, sBias0=G, accumulate=1 if nm != "fc1" else 0)
                add(f"{tag} linear_dx {nm}", "NT", S_, K, N, nb0=nbb, sA0=S_ * N, sB0=G, sC0=S_ * K)
                add(f"{tag} wgrad {nm} into dtheta (stride G)", "TN", K, N, S_, nb0=nbb, sA0=S_ * K, sB0=S_ * N, sC0=G, accumulate=1)

    big = B > 1
    nbb = B if not big else 3
    add("patch embedding", "NN", P, E, Kp, nb0=nbb, sA0=P * Kp, sB0=0, sC0=S * E, bias=True, sBias0=0)
    blocks("encoder", B, S, E, He, Fe, True, big)
    add("language tokens -> context rows", "NN", T, Cx, lang, nb0=B, sA0=T * lang, sB0=0, sC0=Sc * Cx, bias=True, sBias0=0)
    add("CLS projection, M = 1", "NN", 1, Cx, E, nb0=B, sA0=E, sB0=0, sC0=Sc * Cx, bias=True, sBias0=0)
    blocks("context encoder", B, Sc, Cx, Hc, Fc, True, False)
    add("theta = ctx W_cat + b_cat, N = G", "NN", B, G, Cx, bias=True, shrink=False)
    add("policy patch projection (weights per episode)", "NN", P, D, E, nb0=nbb, sA0=S * E, sB0=G, sC0=S * D, bias=True, sBias0=G)
    blocks("policy", B, S, D, H, F, False, big)
    add("dWp = tokens^T dx0, K = P", "TN", E, D, P, nb0=nbb, sA0=S * E, sB0=S * D, sC0=G, accumulate=1)
    add("d tokens = dx0 Wp^T", "NT", P, E, D, nb0=nbb, sA0=S * D, sB0=G, sC0=S * E)
    add("patch-embedding gradient, every image into one C (mode 2)", "TN", Kp, E, P, nb0=nbb, sA0=P * Kp, sB0=S * E, sC0=0, accumulate=2)
    add("dW_cat = ctx^T dtheta, K = B, N = G", "TN", Cx, G, B, accumulate=1, shrink=False)
    add("dctx = dtheta W_cat^T, K = G (launcher split-K; A thinned to keep the sums exact)", "NT", B, Cx, G, accumulate=1, allow_split=1, shrink=False)
    add("w_tok gradient, every episode into one C (mode 2), K = T", "TN", lang, Cx, T, nb0=B, sA0=T * lang, sB0=Sc * Cx, sC0=0, accumulate=2)
    add("w_img gradient, K = 1 (mode 2)", "TN", E, Cx, 1, nb0=B, sA0=E, sB0=Sc * Cx, sC0=0, accumulate=2)
    return out


def shrunk(c):
    """the CPU companion's copy of a case: fewer batch entries of the outer level, no edge size touched"""
    if c.shrink and c.nb0 > 3 and c.sC0 != 0:
        c = replace(c, nb0=3)                             # (the strides are already resolved: they stay)
    if c.fold and getattr(c, c.fold) > 3 * c.fold_rows:
        c = replace(c, **{c.fold: 3 * c.fold_rows})
    return c


# ------------------------------------------------------------------------------------------------ GPU driver
class hvla_bgemm_desc(C.Structure):
    _fields_ = [("A", C.c_void_p), ("B", C.c_void_p), ("C", C.c_void_p), ("bias", C.c_void_p)] + \
               [(n, C.c_int32) for n in ("M", "N", "K", "lda", "ldb", "ldc")] + \
               [(n, C.c_int64) for n in ("sA0", "sA1", "sB0", "sB1", "sC0", "sC1", "sBias0", "sBias1")] + \
               [("nb1", C.c_int32), ("alpha", C.c_float)] + [(n, C.c_int32) for n in ("accumulate", "ksplit", "allow_split", "a_padded", "ta", "tb", "nb0")]


def instantiation(c, chosen):
    tile, vec, ksplit, exact = chosen
    if exact:
        return f"bgemm_kernel<{c.order}>"
    return f"bgemm3_kernel<{c.order}, {tile}, {'vec' if vec else 'dword'}>"


def all_instantiations():
    return [f"bgemm3_kernel<{o}, {tl}, {v}>" for o in ORDERS for tl, v in ((64, "vec"), (64, "dword"), (128, "vec"), (128, "dword"), (256, "vec"))] + \
           [f"bgemm_kernel<{o}>" for o in ORDERS]


def main():
    os.environ["HVLA_LIBRARY_FLAVOUR"] = "bench"        # libhvla_bench.so: the product library has no hvla_debug_* entry points
    sys.path.insert(0, os.path.join(ROOT, "hyper-vla_amd"))
    from hypervla import _native
    lib = _native.load_library()
    lib.hvla_debug_bgemm_once.argtypes = [C.POINTER(hvla_bgemm_desc), C.POINTER(C.c_int32)]
    lib.hvla_debug_bgemm_once.restype = C.c_int
    lib.hvla_debug_train_gemm_exact.argtypes = [C.c_int]
    only = sys.argv[1] if len(sys.argv) > 1 else None
    t0 = time.time()
    hits = {k: 0 for k in all_instantiations()}
    split_tiles = set()
    worst = {"exact": 0.0, "precision": 0.0}
    all_ok = True
    dev = torch.device("cuda:0")
    for c in case_table():
        if only and only not in c.group:
            continue
        inp = make_inputs(c)
        if c.cls == "exact":
            assert_exactness(c, inp)
        d = {k: inp[k].to(dev) for k in ("A", "B", "C") + (("bias",) if c.bias else ())}
        ptr = lambda k: d[k].data_ptr() + 4 * inp["o" + k]
        desc = hvla_bgemm_desc(ptr("A"), ptr("B"), ptr("C"), ptr("bias") if c.bias else None, c.M, c.N, c.K, c.lda, c.ldb, c.ldc, c.sA0, c.sA1, c.sB0, c.sB1,
                               c.sC0, c.sC1, c.sBias0, c.sBias1, c.nb1, c.alpha, c.accumulate, c.ksplit, c.allow_split, c.a_padded, c.ta, c.tb, c.nb0)
        chosen = (C.c_int32 * 4)()
        torch.cuda.synchronize()
        assert lib.hvla_debug_train_gemm_exact(1 if c.f32 else 0) == 0
        rc = lib.hvla_debug_bgemm_once(C.byref(desc), chosen)
        lib.hvla_debug_train_gemm_exact(0)
        if rc != 0:
            print(f"{c.group} | {c.cls} | {c.name}: HIP status {rc}", flush=True)
            sys.exit(2)                                   # nothing more is launched behind a failed launch
        got = d["C"].cpu()
        want, tol = reference(c, inp)
        ok, ratio, text = compare(c, got, want, tol)
        inst = instantiation(c, tuple(chosen))
        if c.expect_ksplit and chosen[2] != c.expect_ksplit:
            ok, text = False, f"the launcher split K {chosen[2]} ways, the case exists for {c.expect_ksplit}; " + text
        if c.cls == "exact":
            hits[inst] += 1
            if chosen[2] > 1 and not chosen[3]:
                split_tiles.add(chosen[0])
        if ok:
            worst[c.cls] = max(worst[c.cls], ratio)
        all_ok &= ok
        print(f"{c.group} | {c.cls} | {c.name} | {inst} ksplit {chosen[2]}: {text} {'ok' if ok else 'MISMATCH'}", flush=True)
        if c.group == "calibration" and not ok:
            print("calibration failed: the exact class's assumption does not hold; nothing else was run")
            sys.exit(3)
    if not only:
        for k, n in hits.items():
            good = n > 0
            all_ok &= good
            print(f"coverage | {k}: {n} exact-class cases {'ok' if good else 'MISSING'}")
        for tl in (64, 128):
            good = tl in split_tiles
            all_ok &= good
            print(f"coverage | ksplit > 1 with the {tl} tile: {'ok' if good else 'MISSING'}")
    print(f"summary | worst err/bound precision class {worst['precision']:.3f}; exact class bitwise; {time.time() - t0:.1f} s")
    print("ok" if all_ok else "MISMATCH")
    sys.exit(0 if all_ok else 1)


if __name__ == "__main__":
    main()
