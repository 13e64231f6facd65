"""Compare two device-assembly files function by function (mangled name): instruction streams with comment lines, directives
and trailing comments stripped and the function's index taken out of its local labels, and the code-object notes of every kernel.

  hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC [-DHVLA_BENCH_HOOKS] --cuda-device-only -S csrc/policy.hip -o new.s
  python tools/isa_compare.py old.s new.s [--diff]

One line per function: identical, or the instruction counts and the number of differing lines; --diff prints those lines."""
import difflib
import re
import sys

NOTES = ("vgpr_count", "sgpr_count", "agpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size",
         "group_segment_fixed_size")


def functions(path):
    """{name: [instruction or label lines]}, {kernel: {note: value}}"""
    text = open(path).read().split("\n")
    is_func = {m.group(1) for m in (re.match(r"^\s+\.type\s+([\w$.]+),@function", l) for l in text) if m}
    funcs, cur = {}, None
    for line in text:
        m = re.match(r"^([A-Za-z_][\w$.]*):", line)
        if m and m.group(1) in is_func:
            cur = funcs.setdefault(m.group(1), [])
            continue
        if re.match(r"^\.Lfunc_end\d+:", line):
            cur = None
            continue
        if cur is None:
            continue
        s = line.split(";")[0].strip()
        if not s or (s.startswith(".") and not s.startswith(".LBB")):
            continue
        cur.append(re.sub(r"\.LBB\d+_", ".LBB_", s))
    notes, rec = {}, None                       # amdhsa.kernels: a record per kernel, its own keys at four columns
    for line in text:
        m = re.match(r"^  (- | {2})\.(\w+):\s+(\S+)\s*$", line)
        if not m:
            continue
        if m.group(1) == "- ":
            rec = {}
        if rec is None:
            continue
        if m.group(2) in NOTES:
            rec[m.group(2)] = int(m.group(3))
        elif m.group(2) == "name":
            notes[m.group(3)] = rec
    return {k: v for k, v in funcs.items() if v}, notes


def main():
    old_f, old_n = functions(sys.argv[1])
    new_f, new_n = functions(sys.argv[2])
    show = "--diff" in sys.argv
    for name in sorted(set(old_f) | set(new_f)):
        if name not in new_f or name not in old_f:
            print(f"{name}: {'gone' if name in old_f else 'new'}")
            continue
        a, b = old_f[name], new_f[name]
        ins = lambda x: sum(1 for l in x if not l.endswith(":"))
        notes = "notes equal" if old_n.get(name) == new_n.get(name) else f"NOTES {old_n.get(name)} -> {new_n.get(name)}"
        if name not in old_n:
            notes = "no kernel"
        if a == b:
            print(f"{name}: identical ({ins(a)} instructions; {notes})")
            continue
        d = [l for l in difflib.unified_diff(a, b, lineterm="", n=0) if l[:1] in "+-" and l[:3] not in ("+++", "---")]
        print(f"{name}: {ins(a)} -> {ins(b)} instructions, {len(d)} differing lines; {notes}")
        if show:
            for l in d:
                print("    " + l)
    return 0


if __name__ == "__main__":
    sys.exit(main())
