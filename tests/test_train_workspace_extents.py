"""What every launch of the fine-tune step may touch, pinned on the CPU at the edges of the accepted set (csrc/accept.h minus
train_refusal).  csrc/train.hip built with -DHVLA_TRAIN_TRACE prints instead of launching; tools/train_extent_trace.hip drives it
over the geometries of tests/test_gpu_train_geometry.py (encoder frozen and trained, at the GPU case's batch size and at B = 1), with
MID, the README widths and the recorded sweep of tests/native/train_step_trace.txt as controls, and prints the workspace plan in
front of every step.  A GEMM whose output runs into one of its own operands gives gradients that depend on the order in which
workgroups run: a parity run passes most of the time, this check cannot."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
TRAIN_HIP = os.path.join(ROOT, "hyper-vla_amd", "csrc", "train.hip")
PTR = re.compile(r"^([a-z_0-9]+)([+-]\d+)$")
# the fields of BG in the order tools/train_launch_trace.h prints them
BG_FIELDS = ("A B C bias M N K lda ldb ldc sA0 sA1 sB0 sB1 sC0 sC1 sBias0 nb1 alpha accumulate ksplit allow_split a_padded sBias1").split()


def trace(tmp_path, train_hip=TRAIN_HIP):
    """Build tools/train_extent_trace.hip against `train_hip` (the tree's; a scratch copy to show that the rules bite) and parse its
    output: a list of points {title, workspace, size{buffer: elements}, plan[(name, offset, floats)], lines[str]}."""
    csrc = os.path.join(ROOT, "hyper-vla_amd", "csrc")
    exe = os.path.join(str(tmp_path), "train_extent_trace")
    build = subprocess.run(
        [HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O1", "-DHVLA_TRAIN_TRACE", "-I", csrc,
         os.path.join(ROOT, "tools", "train_extent_trace.hip"), train_hip, "-o", exe],
        cwd=str(tmp_path), capture_output=True, text=True, timeout=900)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr
    points = []
    for ln in run.stdout.splitlines():
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
    return points


def _ptr(tok):
    m = PTR.match(tok)
    return (m.group(1), int(m.group(2))) if m else None


class _Checker:
    def __init__(self, point):
        self.pt, self.bad, self.top = point, [], 0
        self.bufs = sorted((off, off + n, name) for name, off, n in point["plan"])

    def fail(self, rule, ln, what):
        self.bad.append(f"[{self.pt['title']}] ({rule}) {what}\n    {ln}")

    def plan_buffer(self, lo, hi):
        for b in self.bufs:
            if b[0] <= lo and hi <= b[1]:
                return b
        return None

    def inside(self, rule, ln, what, buf, start, pieces, length):
        """`pieces` (offsets from start) of `length` elements each in `buf`: in `work` every piece inside ONE plan buffer (the whole
        extent first: one look-up for all pieces), elsewhere inside [0, size) where the driver printed the buffer's size."""
        lo, hi = start + min(pieces), start + max(pieces) + length
        if buf == "work":
            self.top = max(self.top, hi)
            if self.plan_buffer(lo, hi):
                return
            for p in pieces:
                if not self.plan_buffer(start + p, start + p + length):
                    at = [b for b in self.bufs if b[0] <= start + p < b[1]]
                    self.fail(rule, ln, f"{what} [work{start + p:+d}, work{start + p + length:+d}) is inside no single plan buffer"
                              + (f" (starts in {at[0][2]} [{at[0][0]}, {at[0][1]}))" if at else ""))
                    return
        elif buf in self.pt["size"]:
            if lo < 0 or hi > self.pt["size"][buf]:
                self.fail(rule, ln, f"{what} [{buf}{lo:+d}, {buf}{hi:+d}) leaves [0, {self.pt['size'][buf]})")

    def bgemm(self, ln):
        w = ln.split(" ")
        ta, tb, nb0 = int(w[1]), int(w[2]), int(w[3])
        assert w[4].startswith("BG{") and w[-1].endswith("}") and len(w) == 4 + len(BG_FIELDS), ln
        f = dict(zip(BG_FIELDS, [w[4][3:]] + w[5:-1] + [w[-1][:-1]]))
        g = {k: (v if k in ("A", "B", "C", "bias") else float(v) if k == "alpha" else int(v)) for k, v in f.items()}
        M, N, K, nb1 = g["M"], g["N"], g["K"], g["nb1"]
        shape = {"A": (K, M) if ta else (M, K), "B": (N, K) if tb else (K, N), "C": (M, N)}
        ld = {"A": g["lda"], "B": g["ldb"], "C": g["ldc"]}
        ext = {}
        for op in "ABC":
            p = _ptr(g[op])
            assert p, ln
            s0, s1 = g["s" + op + "0"], g["s" + op + "1"]
            rows, cols = shape[op]
            assert s0 >= 0 and s1 >= 0 and ld[op] >= cols, ln
            length = (rows - 1) * ld[op] + cols
            pieces = sorted({b0 * s0 + b1 * s1 for b0 in range(nb0) for b1 in range(nb1)})
            ext[op] = (p[0], p[1], p[1] + pieces[-1] + length)
            self.inside("b", ln, f"operand {op}", p[0], p[1], pieces, length)
        c = ext["C"]
        for op in "AB":
            o = ext[op]
            if o[0] == c[0] and o[1] < c[2] and c[1] < o[2]:
                self.fail("a", ln, f"C extent [{c[0]}{c[1]:+d}, {c[0]}{c[2]:+d}) overlaps {op} extent [{o[0]}{o[1]:+d}, {o[0]}{o[2]:+d})")

    def run(self):
        pt = self.pt
        names = [n for n, _, _ in pt["plan"]]
        assert pt["workspace"] and pt["plan"] and "?" not in names and len(set(names)) == len(names), pt["title"]
        for (lo, hi, name), nxt in zip(self.bufs, self.bufs[1:] + [(pt["workspace"], 0, "the end")]):
            assert 0 <= lo < hi <= nxt[0], (pt["title"], name, lo, hi, nxt)
        gemms = 0
        for ln in pt["lines"]:
            w = ln.split(" ")
            if w[0] == "bgemm":
                gemms += 1
                self.bgemm(ln)
            elif w[0] in ("hipMemcpyAsync", "hipMemsetAsync"):
                nbytes = int(w[3])
                assert nbytes % 4 == 0, ln
                for what, tok in (("destination", w[1]),) + ((("source", w[2]),) if w[0] == "hipMemcpyAsync" else ()):
                    p = _ptr(tok)
                    assert p, ln
                    self.inside("c", ln, what, p[0], p[1], [0], nbytes // 4)
        assert gemms > 0, pt["title"]
        if self.top > pt["workspace"]:
            self.fail("d", "", f"highest float touched work+{self.top} is beyond the workspace of {pt['workspace']} floats")
        return self.bad


def violations(points):
    return [v for pt in points for v in _Checker(pt).run()]


@pytest.fixture(scope="module")
def points(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("needs hipcc")
    return trace(tmp_path_factory.mktemp("extent_trace"))


def _is_control(pt):
    return pt["title"].split(" ")[0] in ("MID", "README", "README2", "MID-L16", "MID-L1")


def test_the_sweep_is_the_one_the_gpu_cases_name(points):
    """Every case of tests/test_gpu_train_geometry.py, each frozen and trained, at its batch size and at B = 1; the F < D cases are in it."""
    seen = {}
    for pt in points:
        w = dict(kv.split("=") for kv in pt["title"].split(" ")[1:])
        seen.setdefault(pt["title"].split(" ")[0], set()).add((int(w["B"]), int(w["enc"])))
    cases = {"P1": 5, "P2": 5, "P3": 5, "P4": 5, "P5": 5, "P6": 2, "C1": 5, "C1n": 5, "C2": 5, "C3": 5, "C4": 5, "C5": 5, "E1": 5,
             "E1-B128": 128, "E2": 3, "E3": 5, "E4": 3, "E5": 2, "E6": 2, "E7": 3, "E8": 2, "E9": 9, "MID": 4, "README": 2}
    for name, B in cases.items():
        assert seen.get(name, set()) >= {(B, 0), (B, 1), (1, 0), (1, 1)}, (name, seen.get(name))
    assert {"README2", "MID-L16", "MID-L1"} <= set(seen)


def test_controls_obey_the_extent_rules(points):
    """MID, the README widths and the nine points of the recorded sweep (position source, attention terms, frozen buckets, forward
    only, the layer-count edges): the rules forbid nothing the step does on purpose."""
    ctl = [pt for pt in points if _is_control(pt)]
    assert len(ctl) >= 8 + 9
    bad = violations(ctl)
    assert not bad, "%d violations\n%s" % (len(bad), "\n".join(bad[:10]))


def test_edge_geometries_obey_the_extent_rules(points):
    """(a) no GEMM's C extent meets its A or B extent; (b) each operand extent in `work` lies in one plan buffer, each in params /
    grads / theta / dtheta / tok / cls / tokens inside the vector's length; (c) every copy's and memset's range likewise; (d) nothing
    is touched beyond the workspace size the step reports."""
    edge = [pt for pt in points if not _is_control(pt)]
    assert len(edge) == 22 * 4
    bad = violations(edge)
    assert not bad, "%d violations\n%s" % (len(bad), "\n".join(bad[:10]))


def test_the_rules_see_a_temporary_that_is_too_small(points):
    """Not vacuous: with t.g of P1 (policy mlp 32 under dim 64) cut back to rows x F -- the size it had while it was `rf`, the largest
    rows x MLP width -- rule (b) reports dh2 = du W1^T, the three dh products and nothing in the forward pass."""
    pt = next(p for p in points if p["title"].startswith("P1 ") and " B=5 enc=0 " in p["title"])
    rf, rd = max(5 * 65 * 32, 5 * 14 * 256), max(5 * 65 * 64, 5 * 14 * 128)      # policy and context encoder: rows x F, rows x D
    assert rf == 17920 < rd == 20800
    cut = dict(pt, plan=[(n, off, rf if n == "t.g" else sz) for n, off, sz in pt["plan"]])
    bad = _Checker(cut).run()
    assert bad and all("(b)" in v and "operand C" in v for v in bad), bad[:3]
    assert len(bad) == 2 * (1 + 3), len(bad)      # two policy layers x (dh2 + three dh)
