"""Pins the engines' launch sequences: writes ``tests/golden/launch_trace.json``, per case of tests/launch_trace.py the C-ABI calls of
one forward (+ backward), one call per line, so that a later diff of the file shows which launch moved.

    python tools/gen_launch_trace_golden.py

Needs neither a GPU nor the library (the recorder stands in for both).  Run it on the engine code whose sequences are to be pinned,
BEFORE a host-side refactor; tests/test_04_launch_trace_cpu.py then holds the refactored engines to the file.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "bioscan-clip_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "launch_trace.json"))
    a = ap.parse_args()
    from launch_trace import CASES, trace_case
    out = {}
    for name in sorted(CASES):
        out[name] = trace_case(name)
        print(f"{name}: {len(out[name])} calls")
    with open(a.out, "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
