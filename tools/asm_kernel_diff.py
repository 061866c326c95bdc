#!/usr/bin/env python3
"""Per-kernel comparison of two device assembly files (hipcc --offload-device-only -S).

    python tools/asm_kernel_diff.py before.s after.s [--list]

For every `.amdhsa_kernel NAME` it compares (a) the kernel's text from `NAME:` to its `.Lfunc_end` label, with `;` comments
removed and the function index taken out of local labels, and (b) its `.amdhsa_kernel ... .end_amdhsa_kernel` descriptor block.
Prints one verdict per kernel that differs (every kernel with --list), a count per kernel family and a one-line JSON summary;
exits 1 unless both files hold the same kernels with identical text and descriptors.  Used for refactors that must not change
a single instruction (profiles/gemm_epilogue_refactor.jsonl).
"""
import collections
import json
import re
import sys

LOCAL = re.compile(r"\.(LBB|Lfunc_end|Lfunc_begin|LJTI|Ltmp)\d+")


def clean(lines):
    out = []
    for ln in lines:
        ln = LOCAL.sub(r".\1", ln.split(";", 1)[0]).strip()
        if ln:
            out.append(ln)
    return out


def kernels(path):
    lines = open(path, errors="replace").read().splitlines()
    start = {}   # label -> line index
    for i, ln in enumerate(lines):
        ln = ln.split(";", 1)[0].rstrip()
        if ln.endswith(":") and not ln.startswith((".", " ", "\t")):
            start.setdefault(ln[:-1], i)
    found = {}
    for i, ln in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if not m:
            continue
        name = m.group(1)
        j = i
        while ".end_amdhsa_kernel" not in lines[j]:
            j += 1
        b = start[name]
        e = b
        while not lines[e].startswith(".Lfunc_end"):
            e += 1
        found[name] = (clean(lines[b + 1:e]), clean(lines[i + 1:j]))
    return found


def family(name):   # the function name inside an Itanium-mangled symbol: _ZN<len><namespace><len><function>...
    m = re.match(r"_ZN?(?:\d+_GLOBAL__N_1)?(\d+)", name)
    return name[m.end():m.end() + int(m.group(1))] if m else name


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if len(args) != 2:
        sys.exit(__doc__)
    a, b = kernels(args[0]), kernels(args[1])
    per = collections.defaultdict(lambda: [0, 0])   # family -> [identical, total]
    bad = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            verdict = "only in " + (args[0] if name in a else args[1])
        elif a[name] == b[name]:
            verdict = "identical"
        else:
            verdict = "DIFFERS:" + (" text (%d -> %d lines)" % (len(a[name][0]), len(b[name][0])) if a[name][0] != b[name][0] else "") + (
                " descriptor" if a[name][1] != b[name][1] else "")
        per[family(name)][0] += verdict == "identical"
        per[family(name)][1] += 1
        bad += verdict != "identical"
        if verdict != "identical" or "--list" in sys.argv:
            print("%-12s %s" % (verdict, name))
    for fam, (same, total) in sorted(per.items()):
        print("%-28s %d / %d identical" % (fam, same, total))
    print(json.dumps({"kernels_before": len(a), "kernels_after": len(b), "identical": sum(s for s, _ in per.values()),
                      "families": {f: {"identical": s, "total": t} for f, (s, t) in sorted(per.items())}}))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
