"""JPEG shards against raw shards of the same pixels: what the storage saves and whether the loader keeps up.

Makes N seeded 256 x 341 images, encodes them with Pillow (4:2:0, quality 90 -- the bench is skipped with a message where Pillow is
absent), decodes them ON THE GPU for the raw twin, writes both shards into a temporary directory and reports, per decode thread
count 1 / 2 / 4 / 8:

  * host entropy decode, images/s (the thread pool alone, pinned destination, no device work);
  * bsclip_jpeg_pixels for B = 256, device-event time (median of --reps launches after a warm-up);
  * ShardLoader samples/s end to end (training chain, batch 256, one warm-up epoch then --epochs timed, a device synchronise inside
    the timed window) on the JPEG shard and -- once, it has no decode threads -- on the raw shard, which is what the loader did
    before the codec existed.

The bar (README): the step consumes 6 540 samples/s per GPU.  Writes profiles/jpeg_loader_bench.json.

    python tools/jpeg_loader_bench.py [--n 1024] [--epochs 2] [--reps 20]

``--entropy both`` adds the entropy axis and writes profiles/jpeg_loader_bench_gpu_entropy.json instead: the host path at 1 / 2 / 4 / 8
decode threads and the GPU path (``ShardLoader(entropy="gpu")``) at sync_mcus 2 / 4 / 8 / 16 / 32 take turns, one epoch each, inside the
same run -- one warm-up round, then --epochs timed rounds -- and each configuration reports end-to-end samples/s, the producer
thread's CPU seconds per 1 000 samples (``time.thread_time``; the decode pool's threads are not in it, so the process's CPU seconds
are reported next to it), the image path's H2D bytes per sample counted from the shapes, and for the GPU path the index's share of
the stream bytes and the entropy kernel's device-event time for B images.  The issue's workload is ``--n 4096 --epochs 4``.
``--kernel-only`` only launches the entropy kernel (B images, default sync_mcus, --reps times): the program to put behind
``rocprofv3 --kernel-trace --stats --``.
"""
import argparse
import io
import json
import os
import shutil
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bioscan-clip_amd")]
STEP_RATE = 6540.0    # samples/s per GPU the training step consumes (README)
H, W = 256, 341


def make_images(n, seed):
    """Seeded specimen-like pictures: a bright smooth background, a darker textured blob, sensor noise."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    out = []
    for _ in range(n):
        cx, cy, rx, ry = rng.uniform(100, 240), rng.uniform(80, 180), rng.uniform(40, 110), rng.uniform(30, 90)
        blob = np.exp(-(((x - cx) / rx) ** 2 + ((y - cy) / ry) ** 2) * 1.5)
        tex = np.sin(x * rng.uniform(0.1, 0.6) + y * rng.uniform(0.1, 0.6)) * 0.5 + 0.5
        bg = 225 + 20 * np.sin(x / W * 3 + rng.uniform(0, 6)) * np.cos(y / H * 2)
        tint = rng.uniform(0.3, 0.9, size=3).astype(np.float32)
        img = bg[..., None] * (1 - blob[..., None]) + (60 + 120 * tex[..., None] * tint) * blob[..., None]
        img += rng.normal(0, 4, size=(H, W, 3))
        out.append(np.clip(np.rint(img), 0, 255).astype(np.uint8))
    return out


def entropy_kernel_us(streams, sync_mcus, reps):
    """Device-event times (us) of bsclip_jpeg_entropy_device over ``streams`` (copies and memset of the records included)."""
    import torch
    from bioscanclip.hip import lib, ops
    B = len(streams)
    idx = [ops.jpeg_sync_index(s, sync_mcus) for s in streams]
    huff = np.zeros((B, 4 * lib.JPEG_HUFF_BYTES), dtype=np.uint8)
    qtab, rec, seg = np.zeros((B, 3, 64), dtype=np.uint16), np.zeros((B, 16), dtype=np.int32), np.zeros((B, 8), dtype=np.int32)
    blob, eo, co = bytearray(), 0, 0
    for k, s in enumerate(streams):
        src = np.frombuffer(s, dtype=np.uint8)
        ops.jpeg_device_tables(src.ctypes.data, src.size, huff[k].ctypes.data, qtab[k].ctypes.data, rec[k].ctypes.data)
        rec[k, 0] = co
        seg[k] = (len(blob), len(s), eo, len(idx[k]), sync_mcus, k, 0, 0)
        blob += s
        eo, co = eo + len(idx[k]), co + 64 * int(rec[k, 12])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    bytes_dev, sync_dev, huff_dev = dev(np.frombuffer(bytes(blob), dtype=np.uint8).copy()), dev(np.concatenate(idx)), dev(huff)
    rec_host, seg_host = torch.from_numpy(rec).pin_memory(), torch.from_numpy(seg).pin_memory()
    rec_dev, seg_dev = torch.empty((B, 16), dtype=torch.int32, device="cuda"), torch.empty((B, 8), dtype=torch.int32, device="cuda")
    coef, status = torch.empty(co, dtype=torch.int16, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
    times = []
    for r in range(reps + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.jpeg_entropy_device(bytes_dev, sync_dev, huff_dev, rec_host, seg_host, rec_dev, seg_dev, B, coef, co, status)
        e1.record()
        torch.cuda.synchronize()
        if r >= 3:
            times.append(e0.elapsed_time(e1) * 1e3)
    assert int(status.abs().sum()) == 0, "the bench pictures must decode with status 0"
    return times


def entropy_axis(args, tmp, sample_streams, common, count):
    """Host path at 1 / 2 / 4 / 8 threads and GPU path at each sync_mcus, alternating epoch by epoch in one run."""
    import torch
    from bioscanclip.hip import lib
    from bioscanclip.util import shards
    n, B = args.n, args.batch
    stream_bytes = sum(len(s) for s in sample_streams) / n
    configs = []
    for T in (1, 2, 4, 8):
        configs.append({"name": f"host_t{T}", "entropy": "host", "decode_threads": T, "path": os.path.join(tmp, "jpeg"),
                        "h2d_bytes_per_sample": 2 * count + 384 + 64})
    for s in (2, 4, 8, 16, 32):
        path = os.path.join(tmp, f"jpeg_sync{s}")
        shards.write_shard(path, sample_streams, image_codec="jpeg", jpeg_sync_mcus=s, **common)
        entries = len(np.load(os.path.join(path, "image_sync.npy"))) / n
        kt = entropy_kernel_us(sample_streams[:B], s, args.reps)
        configs.append({"name": f"gpu_sync{s}", "entropy": "gpu", "sync_mcus": s, "path": path, "index_entries_per_image": entries,
                        "index_over_stream_bytes": 16 * entries / stream_bytes,
                        "h2d_bytes_per_sample": stream_bytes + 16 * entries + 4 * lib.JPEG_HUFF_BYTES + 384 + 2 * 64 + 32,
                        "entropy_kernel_us_median": statistics.median(kt), "entropy_kernel_us_min": min(kt), "entropy_kernel_B": B})
    for c in configs:
        kw = {"decode_threads": c["decode_threads"]} if c["entropy"] == "host" else {"entropy": "gpu"}
        c["loader"] = shards.ShardLoader(c["path"], batch_size=B, shuffle=True, seed=1, for_training=True, with_text=True, **kw)
        c["rates"], c["producer_cpu"], c["process_cpu"] = [], [], []
    for epoch in range(args.epochs + 1):        # round 0 warms every configuration up
        for c in configs:
            ld = c["loader"]
            ld.set_epoch(epoch)
            torch.cuda.synchronize()
            t0, p0, seen = time.perf_counter(), time.process_time(), 0
            for batch in ld:
                seen += batch[1].shape[0]
            torch.cuda.synchronize()
            if epoch:
                c["rates"].append(seen / (time.perf_counter() - t0))
                c["producer_cpu"].append(ld.producer_cpu_seconds / seen * 1e3)
                c["process_cpu"].append((time.process_time() - p0) / seen * 1e3)
    out = {}
    for c in configs:
        out[c["name"]] = {k: v for k, v in c.items() if k not in ("loader", "path", "name", "rates", "producer_cpu", "process_cpu")}
        out[c["name"]].update({"samples_per_s": {"median": statistics.median(c["rates"]), "runs": c["rates"]},
                               "producer_thread_cpu_s_per_1000": statistics.median(c["producer_cpu"]),
                               "process_cpu_s_per_1000": statistics.median(c["process_cpu"]),
                               "feeds_the_step": statistics.median(c["rates"]) >= STEP_RATE})
    ok = [c for c in configs if c["entropy"] == "gpu" and c["index_over_stream_bytes"] <= 0.10]
    best = max(ok, key=lambda c: statistics.median(c["rates"]))
    out["chosen_sync_mcus"] = best["sync_mcus"]
    out["gpu_reaches_host_at_two_threads"] = statistics.median(best["rates"]) >= statistics.median(configs[1]["rates"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=64, help="distinct pictures; the shard cycles through them")
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--streams", default=None, help="directory that keeps the bench's JPEG files: written when Pillow is here, read "
                    "when it is not (a GPU box without Pillow then measures the files made elsewhere)")
    ap.add_argument("--entropy", choices=("host", "both"), default="host", help="both: the host / GPU entropy axis (see above)")
    ap.add_argument("--kernel-only", action="store_true", help="launch the entropy kernel alone, for a profiler")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "jpeg_loader_bench.json" if args.entropy == "host" else "jpeg_loader_bench_gpu_entropy.json")
    cached = sorted(f for f in os.listdir(args.streams) if f.endswith(".jpg")) if args.streams and os.path.isdir(args.streams) else []
    try:
        from PIL import Image
        streams = []
        for im in make_images(args.distinct, 7):
            buf = io.BytesIO()
            Image.fromarray(im).save(buf, format="JPEG", quality=90, subsampling="4:2:0")
            streams.append(buf.getvalue())
        if args.streams:
            os.makedirs(args.streams, exist_ok=True)
            for k, s in enumerate(streams):
                with open(os.path.join(args.streams, f"bench{k:03d}.jpg"), "wb") as f:
                    f.write(s)
    except ImportError:
        if not cached:
            print("jpeg_loader_bench: skipped, Pillow is not installed (it writes the bench's JPEG files) and --streams holds none")
            return 0
        streams = [open(os.path.join(args.streams, f), "rb").read() for f in cached]
    import torch
    if not torch.cuda.is_available():
        print("jpeg_loader_bench: needs a GPU (no fall-back: a CPU timing says nothing about the loader)")
        return 1
    from bioscanclip.hip import ops
    from bioscanclip.util import shards
    assert len(streams) <= args.batch
    n, B = args.n, args.batch
    sample_streams = [streams[i % len(streams)] for i in range(n)]
    jpeg_bytes, raw_bytes = sum(len(s) for s in sample_streams), n * H * W * 3
    info = ops.jpeg_probe(streams[0])
    count = int(info.coef_count)
    if args.kernel_only:
        t = entropy_kernel_us(sample_streams[:B], shards.DEFAULT_JPEG_SYNC_MCUS, args.reps)
        print(json.dumps({"entropy_kernel_us_median": statistics.median(t), "B": B, "sync_mcus": shards.DEFAULT_JPEG_SYNC_MCUS}))
        return 0

    # ---- host entropy decode alone ------------------------------------------------------------------------------------------
    result = {"images": f"{H}x{W} 4:2:0 quality 90 (Pillow), {len(streams)} distinct, shard of {n}", "jpeg_bytes_per_image": jpeg_bytes / n,
              "raw_bytes_per_image": raw_bytes / n, "raw_over_jpeg_bytes": raw_bytes / jpeg_bytes, "step_samples_per_s": STEP_RATE,
              "threads": {}}
    coef_host = torch.empty(B * count, dtype=torch.int16).pin_memory()
    qtab_host = torch.empty((3 * B, 64), dtype=torch.int16).pin_memory()
    rec_host = torch.empty((B, 16), dtype=torch.int32).pin_memory()
    srcs = [np.frombuffer(s, dtype=np.uint8) for s in sample_streams[:B]]

    def decode_chunk(chunk):
        for k in chunk:
            ops.jpeg_entropy_decode(srcs[k].ctypes.data, srcs[k].size, coef_host.data_ptr() + 2 * k * count, count,
                                    qtab_host.data_ptr() + 384 * k, rec_host.data_ptr() + 64 * k)
    for T in (1, 2, 4, 8):
        with ThreadPoolExecutor(max_workers=T) as pool:
            chunks = [range(t, B, T) for t in range(T)]
            list(pool.map(decode_chunk, chunks))
            t0, rounds = time.perf_counter(), 0
            while time.perf_counter() - t0 < 1.5:
                list(pool.map(decode_chunk, chunks))
                rounds += 1
            result["threads"][T] = {"entropy_decode_images_per_s": rounds * B / (time.perf_counter() - t0)}

    # ---- the pixel kernels, B images --------------------------------------------------------------------------------------
    rec = rec_host.numpy()
    offs = np.arange(B, dtype=np.int64)
    rec[:, 0], rec[:, 1] = ((offs * count) & 0xFFFFFFFF).astype(np.uint32).view(np.int32), ((offs * count) >> 32).astype(np.int32)
    rec[:, 2], rec[:, 3] = ((offs * H * W * 3) & 0xFFFFFFFF).astype(np.uint32).view(np.int32), ((offs * H * W * 3) >> 32).astype(np.int32)
    rec[:, 9:12] += 3 * np.arange(B, dtype=np.int32)[:, None]
    coef_dev, qtab_dev, rec_dev = coef_host.cuda(), qtab_host.cuda(), torch.empty((B, 16), dtype=torch.int32, device="cuda")
    planes = torch.empty(ops.jpeg_pixels_workspace_bytes(B * count), dtype=torch.uint8, device="cuda")
    pix = torch.empty(B * H * W * 3, dtype=torch.uint8, device="cuda")
    times = []
    for r in range(args.reps + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.jpeg_pixels(coef_dev, B * count, qtab_dev, rec_host, rec_dev, B, planes, pix)
        e1.record()
        torch.cuda.synchronize()
        if r >= 3:
            times.append(e0.elapsed_time(e1) * 1e3)
    moved = B * count * (2 + 1 + 1) + B * H * W * 3   # coefficients in (int16), planes out and back in (uint8), pixels out
    result["pixels_kernel"] = {"B": B, "us_median": statistics.median(times), "us_min": min(times), "us_max": max(times), "reps": len(times),
                               "images_per_s": B / statistics.median(times) * 1e6, "algorithmic_GB_per_s": moved / statistics.median(times) / 1e3}

    # ---- the loader end to end ----------------------------------------------------------------------------------------------
    decoded = pix.view(B, H, W, 3).cpu().numpy()
    tmp = tempfile.mkdtemp(prefix="bsclip_jpeg_bench_")
    try:
        rng = np.random.default_rng(3)
        barcodes = ["".join(rng.choice(list("ACGT"), size=658)) for _ in range(64)]
        common = dict(barcodes=[barcodes[i % 64] for i in range(n)], input_ids=rng.integers(0, 30000, size=(n, 20)),
                      token_type_ids=np.zeros((n, 20), dtype=np.int64), attention_mask=np.ones((n, 20), dtype=np.int64),
                      processid=[f"B{i:06d}" for i in range(n)])
        shards.write_shard(os.path.join(tmp, "jpeg"), sample_streams, image_codec="jpeg", **common)
        shards.write_shard(os.path.join(tmp, "raw"), (decoded[i % len(streams)] for i in range(n)), **common)

        def rate(path, **kw):
            ld = shards.ShardLoader(path, batch_size=B, shuffle=True, seed=1, for_training=True, with_text=True, **kw)
            rates = []
            for epoch in range(args.epochs + 1):
                ld.set_epoch(epoch)
                torch.cuda.synchronize()
                t0, seen = time.perf_counter(), 0
                for batch in ld:
                    seen += batch[1].shape[0]
                torch.cuda.synchronize()
                if epoch:
                    rates.append(seen / (time.perf_counter() - t0))
            return rates
        raw_rates = rate(os.path.join(tmp, "raw"))
        result["raw_loader_samples_per_s"] = {"median": statistics.median(raw_rates), "runs": raw_rates}
        for T in (1, 2, 4, 8):
            r = rate(os.path.join(tmp, "jpeg"), decode_threads=T)
            result["threads"][T]["jpeg_loader_samples_per_s"] = {"median": statistics.median(r), "runs": r}
            result["threads"][T]["feeds_the_step"] = statistics.median(r) >= STEP_RATE
        if args.entropy == "both":
            result["entropy_axis"] = entropy_axis(args, tmp, sample_streams, common, count)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    result["where"] = f"{torch.cuda.get_device_name(0)}, {torch.get_num_threads()} torch CPU threads, one process"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
