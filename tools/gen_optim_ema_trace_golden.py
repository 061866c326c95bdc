"""Pins ``FusedAdamW``'s eager launch sequences with the weight average (EMA) on: writes ``tests/golden/optim_ema_trace.json``, per
scenario of tests/optim_ema_trace.py the C-ABI calls of its steps, one call per line, and the host-visible state after every step, the
average included.

    python tools/gen_optim_ema_trace_golden.py [--out FILE]

Needs neither a GPU nor the library (the recorder stands in for both).
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
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "optim_ema_trace.json"))
    a = ap.parse_args()
    from bioscanclip.hip.optim import FusedAdamW
    from optim_ema_trace import SCENARIOS, trace
    out = {}
    for name in sorted(SCENARIOS):
        out[name] = trace(name, FusedAdamW, setattr)      # the patches stay: this process does nothing else
        print(f"{name}: {len(out[name]['calls'])} calls, {len(out[name]['steps'])} steps" + (", raises" if out[name]["raises"] else ""))
    with open(a.out, "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
