"""Pins ``FusedAdamW``'s eager launch sequences: writes ``tests/golden/optim_trace.json``, per scenario of tests/optim_trace.py the C-ABI
calls of its steps, one call per line, and the host-visible state after every step.

    python tools/gen_optim_trace_golden.py [--optim PATH] [--out FILE]

``--optim PATH`` loads the optimizer module from another file (an earlier commit's ``hip/optim.py`` saved aside): a refactor of the
optimizer is right when both give the same bytes.  Needs neither a GPU nor the library (the recorder stands in for both).
"""
import argparse
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "bioscan-clip_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--optim", help="file to load the optimizer module from (default: bioscanclip/hip/optim.py)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "optim_trace.json"))
    a = ap.parse_args()
    import bioscanclip.hip.optim as optim
    if a.optim:      # under the package's name space, so that its relative imports resolve
        spec = importlib.util.spec_from_file_location("bioscanclip.hip.optim_from_file", a.optim)
        optim = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(optim)
    from optim_trace import SCENARIOS, trace
    out = {}
    for name in sorted(SCENARIOS):
        out[name] = trace(name, optim.FusedAdamW, setattr)      # the patches stay: this process does nothing else
        print(f"{name}: {len(out[name]['calls'])} calls, {len(out[name]['steps'])} steps" + (", raises" if out[name]["raises"] else ""))
    with open(a.out, "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
