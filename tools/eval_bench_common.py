"""What tools/retrieval_eval_bench.py, method_one_bench.py and method_two_bench.py share: the hash of the product sources, the clock,
the synthetic taxonomy, the host / GPU comparison driver of the two method benches and the JSON line."""
import contextlib
import glob
import hashlib
import io
import json
import os
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE_KEYS = ("micro_acc", "macro_acc", "per_class_acc")


def tree_hash():
    """sha256 over the product sources (kernels, header, package, scripts) and the retrieval bench with this module: names and
    contents, in sorted order."""
    pats = ["bioscan-clip_amd/csrc/*.hip", "bioscan-clip_amd/csrc/*.h", "bioscan-clip_amd/csrc/Makefile", "include/*.h",
            "bioscan-clip_amd/bioscanclip/**/*.py", "bioscan-clip_amd/scripts/*.py", "tools/retrieval_eval_bench.py",
            "tools/eval_bench_common.py"]
    files = sorted({f for p in pats for f in glob.glob(os.path.join(ROOT, p), recursive=True)})
    h = hashlib.sha256()
    for f in files:
        h.update(os.path.relpath(f, ROOT).encode() + b"\0")
        with open(f, "rb") as fh:
            h.update(fh.read() + b"\0")
    return h.hexdigest()[:16]


def label(s):
    return {"order": f"o{s % 19}", "family": f"f{s % 494}", "genus": f"g{s % 3441}", "species": f"s{s}"}


def timed(fn, *a, **kw):
    """(seconds, what ``fn`` returned, what it printed): host clock around the whole call, device synchronised."""
    sink = io.StringIO()
    torch.cuda.synchronize()
    t = time.perf_counter()
    with contextlib.redirect_stdout(sink):
        result = fn(*a, **kw)
    torch.cuda.synchronize()
    return time.perf_counter() - t, result, sink.getvalue()


def compare_and_time(host_path, gpu_path, small, large, repeats):
    """The driver of the two method benches.  ``small`` / ``large``: the argument tuples of both paths, each path returning
    ``(output dictionaries, membership shares)``.  One untimed GPU run, then host and GPU alternate on ``small`` and must agree; the
    GPU path alone is then timed on ``large``.  Returns the fields of the JSON line both benches share."""
    timed(gpu_path, *small)                                       # untimed: code objects, allocator
    host_s, gpu_s, tables_equal, threshold_equal = [], [], True, True
    for _ in range(repeats):
        th, (out_h, share_h), _ = timed(host_path, *small)
        tg, (out_g, share_g), _ = timed(gpu_path, *small)
        tables_equal &= all(g[k] == h[k] for h, g in zip(out_h, out_g) for k in TABLE_KEYS) and share_h == share_g
        threshold_equal &= all(g["best_threshold"] == h["best_threshold"] for h, g in zip(out_h, out_g))
        host_s.append(th)
        gpu_s.append(tg)
    if not (tables_equal and threshold_equal):
        raise RuntimeError("the GPU path's outputs differ from the host path's: nothing to time")
    timed(gpu_path, *large)
    big_s = [timed(gpu_path, *large)[0] for _ in range(repeats)]
    return {"host_s": min(host_s), "gpu_s": min(gpu_s), "host_over_gpu": min(host_s) / min(gpu_s), "host_runs_s": host_s,
            "gpu_runs_s": gpu_s, "splits": 2, "gpu_large_s": min(big_s), "gpu_large_runs_s": big_s, "k_list": [1, 3, 5],
            "tables_equal": bool(tables_equal), "best_threshold_equal": bool(threshold_equal),
            "best_threshold": float(out_h[0]["best_threshold"]),
            "top1_species": [out_h[0]["micro_acc"][1]["species"], out_h[1]["micro_acc"][1]["species"]]}


def append_line(path, line):
    """Append ``line`` plus the tree hash to ``path`` as one JSON line and print it."""
    line = dict(line, tree_hash=tree_hash())
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "a") as f:
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line))
