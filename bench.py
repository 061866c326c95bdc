"""Headline benchmark: paired samples/s of the BIOSCAN-CLIP contrastive training step on MI355X.

    python bench.py --gpus 1 --steps 20 --warmup 5
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

Workload: what BASELINE.json's metric names -- Image + DNA + Text (configs[2]'s per-GPU shape: LoRA ViT-B/16 + LoRA BarcodeBERT +
LoRA BERT-small), bf16 MFMA GEMMs with f32 accumulation, local batch 256 per GPU, synthetic 224x224 images + 133-token barcodes
+ 20-token texts resident in HBM, InfoNCE over the (all-gathered, for N > 1) batch, backward, gradient all-reduce, fused AdamW.
--no-text runs configs[1] (Image + DNA, the configuration north_star's 40 % target is stated on); the single-GPU --full line
carries that configuration (and configs[4]'s fp8 shape) as `extra`, measured in the same run on the same number of steps.
One "step" = zero_grad + forward + loss + backward + (all-reduce) + optimizer step; nothing is skipped or cached.

One JSON line is printed by rank 0.  A plain run sets up, warms up, times --steps steps and prints the headline (`metric`, `value`,
`unit`, `higher_is_better`, `dtype`, `ms_per_step`) with `config`, `host`, for N > 1 `dist`, and
  step_roofline -- algorithmic FLOPs of the whole step (118.3 GFLOP per I+D pair) / measured step time
                   against the dense bf16 MFMA peak (no run of its own: derived from the timed steps and the engine clock over them).
--dump-outputs DIR writes, after the timed steps, what the last timed step computed as DIR/<name>.npy (float32): `loss` and
`param.<parameter name>` for every trainable parameter after the last optimizer step.  Inputs and weights are seeded, so two runs
with the same arguments compare output for output.  Above 60 MB in all (full fine-tuning), each tensor larger than 4096 elements
is written as a fixed, seeded sample of its flattened elements.
--full adds what takes runs of its own (the same keys as before the option existed; --no-extras / --no-cpu-baseline trim it):
  roofline      -- the DOMINANT kernel family of the step by time: the bias-free dX GEMMs (dfc1, dproj, dqkv: 70 launches per step,
                   gemm_nt_pers_kernel<EPI_BF16, no bias>), timed live with HIP events on the launch stream in the step's launch mix;
                   `traffic` from the rocprofv3 --pmc passes of that mix (profiles/*.json, --pmc-traffic), never a constant.
  roofline_lowest -- the LOWEST-fraction GEMM family (fc1 + bias + GELU, 24 launches per step), same method.
  roofline_families -- every kernel family that takes more than 2 % of the step (the GEMM families by epilogue, attention forward /
                   backward), each timed live in its own launch mix: TFLOP/s and fraction of the dense bf16 MFMA peak.
  extra, parity_mode_ms_per_step, exact_mode_ms_per_step, numerics_modes -- the other single-GPU BASELINE shapes and numerics
                   modes, each a model of its own timed on the same number of steps (default I+D+T line at local batch 256).
  cpu_baseline  -- the CPU oracle (a port; the reference's Python cannot travel to the GPU box) timed on the host
                   cores on a bounded sample of BASELINE configs[0] (I+D, B=8).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "bioscan-clip_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

PEAK_BF16_TFLOPS = 2500.0  # dense bf16 MFMA, MI355X (MI355X_MICROARCH.md chip table)
GFLOP_PER_PAIR_ID = 118.3   # fwd 58.8 + LoRA-regime bwd
GFLOP_PER_TRIPLE_IDT = 119.3
# HBM-side bytes per launch (roofline.traffic) cannot be measured by this process (PMC passes need rocprofv3 around it): they are read
# from the JSON that tools/scripts/r05_dx_pmc.sh writes from separate --pmc passes (FETCH_SIZE doubled per MI355X_MICROARCH.md's gfx950
# correction + WRITE_SIZE, KB -> bytes) over the SAME launch mix (tools/family_one.py), and labelled with the tree they were taken on.
DEFAULT_PMC_TRAFFIC = {"dx": os.path.join(ROOT, "profiles", "r05_dx_pmc.json"), "fc1": os.path.join(ROOT, "profiles", "r05_fc1_pmc.json")}
METRIC = "paired samples/sec/node (I+D+T, global batch) + step MFMA-roofline % at 1/2/4/8 GPU"   # BASELINE.json:metric, verbatim


class _Cfg:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def build_model(with_text, device, seed=1234, full_ft=False):
    from bioscanclip.model.simple_clip import load_clip_model
    torch.manual_seed(seed)
    mc = _Cfg(image=_Cfg(input_type="image", model="lora_vit"),
              dna=_Cfg(input_type="sequence", model="lora_barcode_bert"), output_dim=768)
    if with_text:
        mc.language = _Cfg(input_type="sequence", model="lora_bert")
    if full_ft:
        mc.disable_lora = True   # reference config/model_config/full_fine_tuning/**: every parameter trained
    args = _Cfg(model_config=mc, bioscan_bert_checkpoint=None, allow_random_init=True)
    model = load_clip_model(args, device=None)
    # LoRA-B is zero-initialised in the reference (image_encoder.py:102-106), which would make the LoRA branch a
    # numerical no-op; re-seed it so the benchmark exercises live branches.
    g = torch.Generator().manual_seed(seed + 1)
    for enc in (model.image_encoder, model.dna_encoder, model.language_encoder):
        if enc is None:
            continue
        for w_b in enc.w_Bs:
            w_b.weight.data.copy_(torch.randn(w_b.weight.shape, generator=g) * 0.02)
    return model.to(device)


def synthetic_batch(B, with_text, device, seed):
    g = torch.Generator().manual_seed(seed)
    image = torch.rand(B, 3, 224, 224, generator=g)
    dna = torch.randint(3, 1027, (B, 133), generator=g)
    dna[:, 0] = 0
    text = None
    if with_text:
        ids = torch.randint(1000, 30522, (B, 20), generator=g)
        lens = torch.randint(6, 21, (B,), generator=g)
        mask = (torch.arange(20)[None] < lens[:, None]).long()
        ids = ids * mask
        ids[:, 0] = 101
        ids[torch.arange(B), lens - 1] = 102
        text = {"input_ids": ids.to(device), "token_type_ids": torch.zeros_like(ids).to(device),
                "attention_mask": mask.to(device)}
    return image.to(device), dna.to(device), text


# GFLOP per image that the reference spends on rows 1..196 of the last ViT block after its QKV GEMM (they cannot reach the
# head, which reads token 0): forward proj + fc1 + fc2 (2*196*768*(768+2*3072)) + attention for 196 of 197 queries, and the
# same set of dX GEMMs + attention backward (2.5x forward) in the backward pass.
VIT_LAST_BLOCK_SKIPPED_GFLOP = (2 * 196 * 768 * (768 + 2 * 3072) * 2 + 4 * 196 * 197 * 768 * 3.5) / 1e9


def family_shapes(B):
    """(M, N, K, launches per step) of the two GEMM families the roofline objects describe, at local batch B (I+D step: ViT rows
    B*197 -- its 12th block runs on the token-0 rows and goes to the small-grid kernel --, BarcodeBERT rows B*133)."""
    Mv, Md = B * 197, B * 133
    return {"dx": [(Mv, 768, 3072, 11), (Mv, 768, 768, 11), (Mv, 768, 2304, 11), (Md, 768, 3072, 12), (Md, 768, 768, 12), (Md, 768, 2304, 12)],
            "fc1": [(Mv, 3072, 768, 11), (Md, 3072, 768, 12), (Md, 768, 768, 1)]}


def _pmc_traffic(path, B):
    """(bytes per launch, provenance) from a tools/scripts/r05_dx_pmc.sh JSON, or (None, why not)."""
    try:
        d = json.load(open(path))
    except Exception as exc:   # noqa: BLE001
        return None, f"no PMC file ({type(exc).__name__}: {path})"
    if d.get("local_batch") != B:
        return None, f"PMC passes were taken at local batch {d.get('local_batch')}, this run is at {B}"
    kb = 2.0 * d["fetch_size_kb_sum"] + d["write_size_kb_sum"]     # FETCH_SIZE counts 64 B per 128-B request on gfx950: doubled
    return kb * 1024.0 / d["launches"], (f"offline: rocprofv3 --pmc FETCH_SIZE (x2, gfx950 correction) and WRITE_SIZE passes over this launch mix, "
                                         f"{os.path.relpath(path, ROOT)} (tree {d.get('tree', '?')}, {d.get('date', '?')}); not collected by this run")


def time_gemm_family(which, B, device, pmc_path, reps=4):
    """One GEMM family of the step, timed live with HIP events on the launch stream in the step's own launch mix, so that the average
    duration is directly comparable with the kernel's row in the rocprofv3 --stats summary of this command (profiles/).
    "dx": the bias-free dX GEMMs gemm_nt_pers_kernel<EPI_BF16, no bias> -- dfc1 [M, 768, 3072], dproj [M, 768, 768], dqkv [M, 768, 2304]
    of 11 ViT blocks and 12 BarcodeBERT layers: the largest family by time (19 % of the step's kernel time).
    "fc1": fc1 + bias + exact GELU (writes gelu(z) and 8-bit gelu'(z)) gemm_nt_pers_kernel<EPI_GELU_BF16, bias>: the lowest fraction."""
    from bioscanclip.hip import ops
    from bioscanclip.hip.lib import EPI_BF16, EPI_GELU_BF16
    shapes = family_shapes(B)[which]
    epi = EPI_BF16 if which == "dx" else EPI_GELU_BF16
    bufs = []
    for M, N, K, _ in shapes:
        kw = {}
        if which == "fc1":
            kw = {"bias": torch.randn(N, device=device), "aux": torch.empty(M, N, device=device, dtype=torch.uint8)}
        bufs.append((torch.randn(M, K, device=device).bfloat16(), (torch.randn(N, K, device=device) * 0.03).bfloat16(),
                     torch.empty(M, N, device=device, dtype=torch.bfloat16), kw))

    def mix():
        for (M, N, K, cnt), (a, w, out, kw) in zip(shapes, bufs):
            for _ in range(cnt):
                ops.gemm(a, w, out, epi, **kw)

    mix()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        mix()
    e1.record()
    torch.cuda.synchronize()
    launches = sum(c for *_, c in shapes)
    mean_ms = e0.elapsed_time(e1) / (reps * launches)
    flops = sum(2.0 * M * N * K * c for M, N, K, c in shapes) / launches
    achieved = flops / (mean_ms * 1e-3) / 1e12
    traffic, source = _pmc_traffic(pmc_path, B)
    out_bytes = 2.0 if which == "dx" else 3.0      # bf16 out; fc1: gelu bf16 + gelu' 8-bit
    algo = sum(((M * K + N * K) * 2.0 + out_bytes * M * N) * c for M, N, K, c in shapes) / launches
    res = {"bound": "mfma", "achieved": round(achieved, 1), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
           "frac": round(achieved / PEAK_BF16_TFLOPS, 4),
           "traffic": None if traffic is None else round(traffic, 0), "traffic_source": source,
           "algorithmic_bytes_per_launch": round(algo, 0),
           "kernel": ("gemm_nt_pers_kernel<0 = EPI_BF16, false, false, true> (bias-free dX GEMMs: dfc1, dproj, dqkv; 70 launches per step)" if which == "dx"
                      else "gemm_nt_pers_kernel<2 = EPI_GELU_BF16, true, false, true> (fc1 + bias + GELU; 24 launches per step)"),
           "kernel_role": ("the dominant kernel family of the step by time" if which == "dx" else
                           "the LOWEST-fraction GEMM family of the step (its two-output GELU epilogue)"),
           "launch_mix_MNK_count": [list(x) for x in shapes],
           "algorithmic_gflop_per_launch": round(flops / 1e9, 2), "avg_launch_ms": round(mean_ms, 4)}
    del bufs
    torch.cuda.empty_cache()
    return res


def time_families(B, device, reps=3):
    """Live HIP-event timing of every kernel family above 2 % of the step, each in the launch mix the I+D step has at local batch B
    (ViT rows B*197, BarcodeBERT rows B*133; the text tower's launches are latency-sized and left out): algorithmic FLOPs per launch
    / mean launch time against the dense bf16 MFMA peak.  Attention: 4 S^2 64 FLOP per head forward, 2.5 x that backward (5 products)."""
    from bioscanclip.hip import ops
    from bioscanclip.hip.lib import EPI_BF16, EPI_DGELU_BF16, EPI_GELU_BF16, EPI_RESID_BF16
    Mv, Md = B * 197, B * 133

    def gemm_family(shapes, epi, bias):
        bufs = []
        for M, N, K, _ in shapes:
            a = torch.randn(M, K, device=device).bfloat16()
            w = (torch.randn(N, K, device=device) * 0.03).bfloat16()
            kw = {"bias": torch.randn(N, device=device)} if bias else {}
            out = torch.empty(M, N, device=device, dtype=torch.bfloat16)
            if epi == EPI_RESID_BF16:
                kw["resid"] = torch.randn(M, N, device=device).bfloat16()
            if epi in (EPI_GELU_BF16, EPI_DGELU_BF16):
                kw["aux"] = torch.randint(0, 256, (M, N), device=device, dtype=torch.uint8)
            bufs.append((a, w, out, kw))

        def mix():
            for (M, N, K, cnt), (a, w, out, kw) in zip(shapes, bufs):
                for _ in range(cnt):
                    ops.gemm(a, w, out, epi, **kw)
        n = sum(c for *_, c in shapes)
        return mix, n, sum(2.0 * M * N * K * c for M, N, K, c in shapes) / n

    def attn_family(bwd):
        bufs = []
        for S, p, cnt in ((197, 0.0, 11), (133, 0.1, 12)):   # the 12th ViT block runs the token-0 form: a different, cheap launch
            qkv = (torch.randn(B * S, 2304, device=device) * 0.5).bfloat16()
            ctx = torch.empty(B * S, 768, device=device, dtype=torch.bfloat16)
            lse = torch.empty(B, 12, S, device=device)
            dctx = torch.randn(B * S, 768, device=device).bfloat16()
            dqkv = torch.empty(B * S, 2304, device=device, dtype=torch.bfloat16)
            drop = (p, 1234) if p else None
            # with dropout the forward leaves its keep decisions as bit words and the backward reads them: the engines' path (round 5)
            bits = torch.zeros(B * 12 * S * ops.KEEP_WORDS, device=device, dtype=torch.int32) if p else None
            ops.attn_fwd(qkv, B, S, 12, 0.125, ctx, lse, dropout=drop, keep_bits=bits)
            # the backward also leaves the LoRA gradients' dt / dB partial sums (bsclip_attn_bwd_lora): the engines' path (round 5)
            lora = (torch.randn(B * S, 64, device=device).bfloat16(), torch.randn(2, 768, 4, device=device) * 0.1,
                    torch.empty(12, 2, B * S, 4, device=device), torch.empty(B * 12, 2, 4, 64, device=device))
            bufs.append((S, qkv, ctx, lse, dctx, dqkv, drop, bits, lora, cnt))

        def mix():
            for S, qkv, ctx, lse, dctx, dqkv, drop, bits, lora, cnt in bufs:
                for _ in range(cnt):
                    if bwd:
                        ops.attn_bwd(qkv, dctx, lse, B, S, 12, 0.125, dqkv, dropout=drop, keep_bits=bits, lora=lora)
                    else:
                        ops.attn_fwd(qkv, B, S, 12, 0.125, ctx, lse, dropout=drop, keep_bits=bits)
        n = sum(b[-1] for b in bufs)
        fl = sum(4.0 * B * 12 * b[0] * b[0] * 64 * b[-1] for b in bufs) / n * (2.5 if bwd else 1.0)
        return mix, n, fl

    fams = [
        ("qkv + bias (K = 768 + 64: LoRA rides in K)", *gemm_family([(Mv, 2304, 832, 12), (Md, 2304, 832, 12)], EPI_BF16, True)),
        ("fc1 + bias + GELU (+ 8-bit gelu')", *gemm_family([(Mv, 3072, 768, 11), (Md, 3072, 768, 12), (Md, 768, 768, 1)], EPI_GELU_BF16, True)),
        ("out-projection / fc2 + bias + residual", *gemm_family([(Mv, 768, 768, 11), (Mv, 768, 3072, 11), (Md, 768, 768, 12), (Md, 768, 3072, 12)],
                                                               EPI_RESID_BF16, True)),
        ("dfc2 x gelu' (dX of fc2)", *gemm_family([(Mv, 3072, 768, 11), (Md, 3072, 768, 12)], EPI_DGELU_BF16, False)),
        ("bias-free dX (dfc1, dproj, dqkv)", *gemm_family([(Mv, 768, 3072, 11), (Mv, 768, 768, 11), (Mv, 768, 2304, 11), (Md, 768, 3072, 12),
                                                         (Md, 768, 768, 12), (Md, 768, 2304, 12)], EPI_BF16, False)),
        ("attention forward (S = 197; S = 133 with dropout)", *attn_family(False)),
        ("attention backward (+ LoRA dt / dB partial sums)", *attn_family(True)),
    ]
    out = []
    for name, mix, n, flops in fams:
        mix()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            mix()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) / (reps * n) * 1e3
        tf = flops / (us * 1e-6) / 1e12
        out.append({"family": name, "launches_per_step": n, "gflop_per_launch": round(flops / 1e9, 2), "avg_launch_us": round(us, 1),
                    "ms_per_step": round(us * n / 1e3, 3), "tflops": round(tf, 1), "frac_of_bf16_mfma_peak": round(tf / PEAK_BF16_TFLOPS, 4)})
        torch.cuda.empty_cache()
    return out


def parity_distances():
    """Distances to the f32 reference of the three numerics configurations, as the GPU parity tests measured them at depth 12
    (tests/test_20_encoders_gpu.py appends them to gpurun_out/parity.jsonl; the copy under profiles/ travels with the tree): this process
    times the configurations, it does not re-measure their distances (the f32 oracle of a 12-layer tower is a minute of CPU time)."""
    path = os.path.join(ROOT, "profiles", "parity_latest.jsonl")
    rec = {}
    try:
        for line in open(path):
            d = json.loads(line)
            if "emb_vs_f32_oracle" in d and "worst_grad" in d:
                rec[d["test"]] = {"embedding": float("%.3g" % d["emb_vs_f32_oracle"]), "worst_gradient_tensor": float("%.3g" % d["worst_grad"])}
    except Exception as exc:   # noqa: BLE001
        return {"error": f"{type(exc).__name__}: {exc}"}
    pick = lambda keys: {k.split("_", 2)[-1] if k.startswith(("parity_mode_", "exact_forward_")) else k: rec[k] for k in keys if k in rec}
    return {"default": pick(["vit_L12", "dna_L12", "txt_L4"]), "parity1": pick(["parity_mode_vit_L12", "parity_mode_dna_L12"]),
            "exact": pick(["exact_forward_vit_L12", "exact_forward_dna_L12", "exact_forward_txt_L4"]),
            "source": "relative L2 distance to the f32 CPU oracle (= the imported reference's fixtures, tests/golden) of the full-depth encoders' "
                      "embeddings and of the worst trainable-gradient tensor, measured by the -m gpu parity tests: profiles/parity_latest.jsonl"}


def thread_cpu_seconds():
    """{tid: (name, user + system CPU seconds)} of every thread of this process (/proc/self/task): who burns the host."""
    out = {}
    tick = os.sysconf("SC_CLK_TCK")
    try:
        for tid in os.listdir("/proc/self/task"):
            with open(f"/proc/self/task/{tid}/stat") as f:
                raw = f.read()
            name = raw[raw.index("(") + 1:raw.rindex(")")]
            fields = raw[raw.rindex(")") + 2:].split()
            out[int(tid)] = (name, (int(fields[11]) + int(fields[12])) / tick)
    except Exception:   # noqa: BLE001
        pass
    return out


def usable_cores():
    """Cores this process may really use: affinity mask capped by the cgroup CPU quota (a GPU box exposes every
    host CPU in the mask but grants a 16-CPU share; oversubscribing the torch pool makes the baseline meaningless)."""
    n = os.cpu_count() or 1
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except Exception:
        pass
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    n = min(n, max(1, int(int(txt[0]) / int(txt[1]))))
            else:
                q = int(txt[0])
                if q > 0:
                    p = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
                    n = min(n, max(1, q // p))
            break
        except Exception:
            continue
    return max(1, min(n, 16))


def cpu_baseline(seconds_budget=20.0):
    """CPU oracle (port of the reference path) on BASELINE configs[0]: I+D, B=8, f32, AdamW; bounded sample."""
    from oracle import refcpu, synth
    from bioscanclip.model import arch
    from bioscanclip.model.dna_encoder import LoRA_barcode_bert
    from bioscanclip.model.image_encoder import LoRA_ViT_timm
    from bioscanclip.model.simple_clip import SimpleCLIP
    cores = usable_cores()
    torch.set_num_threads(cores)
    model = SimpleCLIP(LoRA_ViT_timm(arch.vit_base_patch16_224(), r=4, num_classes=768),
                       LoRA_barcode_bert(arch.BertForMaskedLMParams(arch.barcode_bert_config()), r=4, num_classes=768),
                       None)
    state = refcpu.StepState(synth.synth_state_dict(synth.shapes_of(model), seed=31))
    B, done, t_total = 8, 0, 0.0
    for s in range(12):
        image, dna, _, label = synth.synth_batch(B, seed=100 + s)
        t0 = time.perf_counter()
        refcpu.train_step(state, image, dna, None, label)
        dt = time.perf_counter() - t0
        print(f"[bench] cpu_baseline step {s}: {dt:.2f} s", file=sys.stderr, flush=True)
        if s >= 1:  # first step warms the allocator / thread pool
            done += 1
            t_total += dt
        if done >= 1 and t_total + dt > seconds_budget:
            break
    cpu = "unknown"
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    cpu = line.split(":", 1)[1].strip()
                    break
    except Exception:
        pass
    return {"value": round(B * done / t_total, 3), "unit": "paired samples/s", "cores": cores, "kind": "port",
            "sample": f"{done} steps of Image+DNA B=8 fp32 (BASELINE configs[0]) after 1 warm-up step, "
                      f"{t_total:.1f} s, torch CPU threads={cores}, {cpu}"}


def side_measurement(device, with_text, fp8, B, steps=20, parity=0):
    """ms/step of another BASELINE configuration's per-GPU shape on this one GPU (same step, same launch path: captured
    hipGraph), reported as extra keys of the line so that they are driver-run numbers too: configs[2]'s I+D+T at local batch 256
    and configs[4]'s fp8 trunks at its own local batch 512."""
    from bioscanclip.hip.graph import GraphedStep
    from bioscanclip.hip.optim import FusedAdamW
    from bioscanclip.model.loss_func import ContrastiveLoss
    from bioscanclip.hip import engine as _engine
    prev = _engine.set_parity_mode(parity) if parity else None   # 1: f32 streams (BSCLIP_PARITY=1); 2: + the exact forward
    model = build_model(with_text, device)
    if fp8:
        from bioscanclip.hip.engine import set_precision
        set_precision(model, "fp8")
    model.train()
    image, dna, text = synthetic_batch(B, with_text, device, seed=4321)
    label = torch.arange(B, device=device)
    opt = FusedAdamW(model.parameters(), lr=1e-3)
    g = GraphedStep(model, opt, ContrastiveLoss(torch.nn.CrossEntropyLoss(), 1 / 0.07), warmup=2)
    for _ in range(5):      # two eager steps, the capture (+ its replay), two more replays
        loss = g(image, dna, text, label)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = g(image, dna, text, label)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    per = GFLOP_PER_TRIPLE_IDT if with_text else GFLOP_PER_PAIR_ID
    nmod = 3 if with_text else 2
    tflop = (per * B + (nmod * (nmod - 1) // 2) * 3 * 2.0 * B * B * 768 / 1e9) / 1e3
    out = {"ms_per_step": round(ms, 3), "paired_samples_per_s": round(B / (ms * 1e-3), 1), "local_batch": B, "steps": steps,
           "final_loss": round(loss.item(), 5),
           "step_roofline_frac": round(tflop / (ms * 1e-3) / PEAK_BF16_TFLOPS, 4), "algorithmic_tflop_per_gpu_step": round(tflop, 3)}
    del g, opt, model
    torch.cuda.empty_cache()
    if prev is not None:
        _engine.set_parity_mode(0)
        _engine.GRAD_STREAM_BF16, _engine.RESID_STREAM_BF16 = prev
    return out


DUMP_BUDGET_BYTES = 60 << 20   # array data of --dump-outputs; with the .npy headers the directory stays under 64 MB


def dump_outputs(path, loss, model):
    """--dump-outputs: what the last timed step computed, as a caller of the step receives it -- the loss and every trainable
    parameter after the optimizer step -- as <path>/<name>.npy in float32.  When the set exceeds DUMP_BUDGET_BYTES (full
    fine-tuning trains every parameter), each tensor larger than 4096 elements is written as a sample of its flattened elements:
    indices drawn from a generator seeded by the tensor's name, as many as keep the set within the budget, so that two runs with
    the same arguments write the same elements."""
    import zlib

    import numpy as np
    os.makedirs(path, exist_ok=True)
    arrays = [("loss", loss.detach().reshape(1))]
    arrays += [("param." + n, p.detach()) for n, p in model.named_parameters() if p.requires_grad]
    small = sum(t.numel() for _, t in arrays if t.numel() <= 4096)
    large = sum(t.numel() for _, t in arrays if t.numel() > 4096)
    keep = 1.0 if 4 * (small + large) <= DUMP_BUDGET_BYTES else (DUMP_BUDGET_BYTES - 4 * small) / (4 * large)
    for name, t in arrays:
        flat = t.float().reshape(-1)
        if keep < 1.0 and flat.numel() > 4096:
            g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
            idx = torch.randint(0, flat.numel(), (max(1, int(flat.numel() * keep)),), generator=g).sort().values
            arr = flat[idx.to(flat.device)].cpu().numpy()
        else:
            arr = t.float().cpu().numpy()
        np.save(os.path.join(path, name + ".npy"), arr)
    print(f"[bench] wrote {len(arrays)} arrays to {path}" + ("" if keep == 1.0 else f" (tensors over 4096 elements sampled at {keep:.3f})"),
          file=sys.stderr, flush=True)


def main():
    # stdout carries exactly one line, the JSON result.  Native libraries print there too (RCCL writes a version banner to
    # fd 1 when the first communicator is created), so fd 1 is pointed at stderr for the duration of the run and the result
    # is written to the saved descriptor.
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256, help="local (per-GPU) batch")
    ap.add_argument("--text", action="store_true", help="(default) Image + DNA + Text: what BASELINE.json's metric names (configs[2]'s per-GPU shape)")
    ap.add_argument("--no-text", action="store_true", help="Image + DNA only (BASELINE configs[1], the shape of north_star's 40 %% target)")
    ap.add_argument("--fp8", action="store_true", help="fp8 e4m3 frozen-trunk GEMMs for ViT + BarcodeBERT (BASELINE configs[4])")
    ap.add_argument("--full-ft", action="store_true", help="disable_lora: true -- train every parameter (SURVEY 8f-4; not a BASELINE config)")
    ap.add_argument("--lr", type=float, default=None, help="AdamW lr (default 1e-3; 1e-6 with --full-ft, the reference's full fine-tuning base lr: random-init towers on noise images collapse under larger steps, tools/ft_dynamics_probe.py)")
    ap.add_argument("--no-graph", action="store_true", help="enqueue every launch from Python instead of replaying the captured hipGraph")
    ap.add_argument("--full", action="store_true", help="after the headline, also run what takes runs of its own: the roofline / "
                    "roofline_lowest / roofline_families kernel timings, the side measurements (extra, parity and exact mode) and the "
                    "CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write the last timed step's loss and trainable parameters "
                    "as DIR/<name>.npy (float32, at most 64 MB in all; larger sets as fixed seeded samples)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the side measurements (configs[1] I+D at B=256, fp8 trunks "
                    "at B=512, parity and exact mode) and roofline_families")
    ap.add_argument("--pmc-traffic", default=None, help="JSON of the rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes over the dominant kernel's "
                    "launch mix (tools/scripts/r05_dx_pmc.sh); default profiles/r05_dx_pmc.json")
    a = ap.parse_args()
    a.text = not a.no_text

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # Rehearsal knobs (one-GPU box): BSCLIP_DIST_BACKEND=gloo + BSCLIP_SINGLE_DEVICE=1 runs N ranks on cuda:0 so the whole
    # multi-rank code path (all-gather loss with row0/n_local, flat-gradient all-reduce) executes without an 8-GPU node.
    backend = os.environ.get("BSCLIP_DIST_BACKEND", "nccl")
    if os.environ.get("BSCLIP_SINGLE_DEVICE", "0") == "1":
        local_rank = 0
    force_dist = os.environ.get("BSCLIP_FORCE_DIST", "0") == "1"  # world_size 1 through the real collectives (rehearsal)
    if world > 1 or force_dist:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29531")
        torch.cuda.set_device(local_rank)
        dist.init_process_group(backend, rank=rank, world_size=world)
    if world > 1:
        torch.set_num_threads(2)  # N ranks share the host: the step has no CPU tensor math worth a wide intra-op pool
    device = torch.device("cuda", local_rank if world > 1 else 0)
    torch.cuda.set_device(device)
    assert world == a.gpus, f"--gpus {a.gpus} but WORLD_SIZE={world}"

    from bioscanclip.hip import dist as hdist
    from bioscanclip.hip import engine as _engine
    from bioscanclip.hip.optim import FusedAdamW
    from bioscanclip.model.loss_func import ContrastiveLoss, GlobalBatchContrastiveLoss

    model = build_model(a.text, device, full_ft=a.full_ft)
    if a.fp8:
        from bioscanclip.hip.engine import set_precision
        set_precision(model, "fp8")
    model.train()
    nodrop = os.environ.get("BSCLIP_BENCH_NODROP", "0") == "1"  # diagnostic: what the dropout masks cost (not a valid bench line)
    if nodrop:
        model.eval()
    B = a.batch
    image, dna, text = synthetic_batch(B, a.text, device, seed=1234 + rank)
    label = (torch.arange(B) + rank * B).to(device)
    crit = (GlobalBatchContrastiveLoss if world > 1 or force_dist else ContrastiveLoss)(torch.nn.CrossEntropyLoss(), 1 / 0.07)
    opt = FusedAdamW(model.parameters(), lr=a.lr if a.lr is not None else (1e-6 if a.full_ft else 1e-3))

    # One process, one GPU: the whole step is captured once into a hipGraph and replayed (bioscanclip/hip/graph.py) -- the
    # host does three calls per step instead of ~1 500.
    graphed = None
    if not a.no_graph:
        from bioscanclip.hip.graph import GraphedDistStep, GraphedStep
        # with a process group: per-tower captured graphs (forward_k | loss | backward_k | AdamW), each tower's all-gather and
        # all-reduce issued eagerly from that tower's stream between them (hip/graph.py GraphedDistStep) -- a rank's host work
        # drops from ~35 ms to ~1 ms per step and the collectives run beside the other towers' kernels
        graphed = (GraphedDistStep if world > 1 or force_dist else GraphedStep)(model, opt, crit, warmup=2)
        if world > 1 or force_dist:
            graphed.profile_waits = True     # event pairs around the waits for the collectives (read after the timed region)

    def step():
        nonlocal graphed
        if graphed is not None:
            return graphed(image, dna, text, label)
        opt.zero_grad()
        if hasattr(crit, "prefetch_labels"):
            crit.prefetch_labels(label)  # global batch: label all-gather at the top of the step (as train_epoch does)
        io, do, to = model(image, dna, text)
        loss = crit(io, do, to, label)
        loss.backward()
        hdist.allreduce_grads(model)
        if opt.needs_attach():
            opt.attach(model)
        opt.step()
        return loss

    loss = step()  # builds engines / workspaces
    torch.cuda.synchronize()
    if rank == 0:
        print(f"[bench] first step done, loss {loss.item():.5f}", file=sys.stderr, flush=True)
    hdist.broadcast_trainable(model)
    if graphed is not None:   # 1 more eager step, the capture, one replay -- all untimed; an eager fallback if the capture fails
        try:
            for _ in range(3):
                loss = step()
            torch.cuda.synchronize()
        except Exception as exc:   # noqa: BLE001 - the measurement must not die with the launch path
            print(f"[bench] hipGraph capture failed ({type(exc).__name__}: {exc}); continuing with the eager launch path",
                  file=sys.stderr, flush=True)
            graphed = None
            opt.enable_device_hyper(False)
            torch.cuda.synchronize()
    for _ in range(a.warmup):
        loss = step()

    def park(ev, nap=2e-4):
        """Wait for a HIP event WITHOUT burning a core.  Every synchronising call of this runtime spins -- torch.cuda.synchronize(),
        and (measured, round 4) hipEventSynchronize on an event created with hipEventBlockingSync too: the enqueue thread showed
        100 % CPU either way, and a second runtime thread beside it.  Round 3's 38.8 ms of host CPU per 38.1 ms step was that spin;
        the enqueue of a replayed step itself costs well under a millisecond.  So: poll hipEventQuery between short sleeps."""
        while not ev.query():
            time.sleep(nap)

    def wait_idle():
        ev = torch.cuda.Event()
        ev.record()
        park(ev)

    def fence():
        wait_idle()
        if world > 1 or force_dist:
            dist.barrier()
        wait_idle()

    # the engine clock the chip actually runs at over the timed steps (per-XCD s_memtime against the 100 MHz real-time counter):
    # sampled just outside the timed region, so the K steps are timed exactly as before
    from bioscanclip.hip import ops as _ops
    clk0, clk1 = torch.zeros(32, dtype=torch.int64, device=device), torch.zeros(32, dtype=torch.int64, device=device)
    _ops.clock_probe(clk0)
    fence()
    if graphed is not None and hasattr(graphed, "wait_events"):
        graphed.wait_events.clear()          # only the timed steps
    # The host stays at most two steps ahead of the device (as train_epoch does by reading the loss one step late): with an
    # unbounded run-ahead the K launches are enqueued in microseconds and the thread then sits in the runtime's queue back-pressure
    # -- a spin.  The throttle polls an event between sleeps: the GPU never idles (a step is always queued behind the running one).
    ring = [torch.cuda.Event() for _ in range(3)]
    th0 = thread_cpu_seconds()
    t0 = time.perf_counter()
    c0 = time.process_time()
    tc0 = time.thread_time()
    for i in range(a.steps):
        if i >= 2:
            park(ring[(i - 2) % 3], nap=1e-3)
        loss = step()
        ring[i % 3].record()
    t_enq = time.perf_counter() - t0
    fence()
    elapsed = time.perf_counter() - t0
    host_cpu_s = time.process_time() - c0   # CPU time of every thread of this process over the timed region (enqueue + waits)
    main_cpu_s = time.thread_time() - tc0   # ... and of this (the enqueueing) thread alone
    th1 = thread_cpu_seconds()
    busiest = sorted(((th1[t][1] - th0.get(t, (None, 0.0))[1], th1[t][0], t) for t in th1), reverse=True)[:4]
    if rank == 0:
        print("[bench] busiest threads over the timed steps (CPU s, name, tid): " +
              ", ".join(f"{d:.2f} {n} {t}{' (enqueue thread)' if t == os.getpid() else ''}" for d, n, t in busiest), file=sys.stderr, flush=True)
    _ops.clock_probe(clk1)
    torch.cuda.synchronize()
    clock_ghz = _ops.engine_clock_ghz(clk0, clk1)
    dist_info = None
    if world > 1 or force_dist:
        # per-rank wall time of the K steps (the line's value uses the MAX, as the contract says) and what each rank's main stream
        # spent waiting for collectives AFTER its own towers were done -- so that the first SCALE record explains itself
        waits = graphed.collective_wait_ms() if graphed is not None and hasattr(graphed, "collective_wait_ms") else None
        mine = torch.tensor([elapsed / a.steps * 1e3, -1.0 if waits is None else waits[0], -1.0 if waits is None else waits[1]],
                            device=device, dtype=torch.float64)
        allv = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allv, mine)
        per_rank = torch.stack(allv).cpu()
        dist_info = {"ranks": world, "ms_per_step_per_rank": [round(v, 3) for v in per_rank[:, 0].tolist()],
                     "ms_per_step_min": round(per_rank[:, 0].min().item(), 3), "ms_per_step_max": round(per_rank[:, 0].max().item(), 3),
                     "exposed_allgather_wait_ms_per_step": None if waits is None else round(per_rank[:, 1].max().item(), 4),
                     "exposed_allreduce_wait_ms_per_step": None if waits is None else round(per_rank[:, 2].max().item(), 4),
                     "note": "exposed wait = time a rank's main stream waited for the step's all-gathers (before the loss graph) / gradient "
                             "all-reduces (before the optimizer graph) after its own tower graphs had finished: the collective time the "
                             "overlap did not hide, max over ranks; a straggler rank shows as ms_per_step_min << max on the others' waits"}
        t = torch.tensor([elapsed], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = t.item()
    final_loss = loss.item()

    if rank == 0:
        ms = elapsed / a.steps * 1e3
        N = B * world
        nmod = 3 if a.text else 2
        pairs = nmod * (nmod - 1) // 2
        per = GFLOP_PER_TRIPLE_IDT if a.text else GFLOP_PER_PAIR_ID
        skipped = VIT_LAST_BLOCK_SKIPPED_GFLOP
        if a.full_ft:   # fwd + dX + dW of every linear = 3 x F_fwd (58.79 G I+D, + 0.51 G text)
            per = 3 * (58.79 + (0.51 if a.text else 0.0))
            skipped += 196 * 768 * (768 + 2 * 3072) * 2 / 1e9      # the token-1..196 rows' dW of the last block's proj / MLP
        loss_gflop = pairs * 3 * 2.0 * N * N * 768 / 1e9  # fwd + 2x bwd on the distinct matrices
        step_tflop_per_gpu = (per * B + loss_gflop) / 1e3
        achieved = step_tflop_per_gpu / (ms * 1e-3)
        out = {
            # BASELINE.json's metric string; which towers THIS line ran is in config.workload (configs[1] = I+D is the
            # single-GPU configuration the metric is quoted on; --text runs configs[2]'s I+D+T)
            "metric": METRIC,
            "value": round(N / (ms * 1e-3), 1), "unit": "paired samples/s", "n_gpus": world, "steps": a.steps,
            "warmup": a.warmup, "ms_per_step": round(ms, 3), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "fp8" if a.fp8 else "bf16", "data": "synthetic",
            "config": {"workload": "%s: Image+DNA%s (LoRA ViT-B/16 + LoRA BarcodeBERT%s), local batch %d, "
                                   "224x224 images + 133-token barcodes, %s InfoNCE, fused AdamW"
                                   % ("full fine-tuning (disable_lora: true, every parameter trained; not a BASELINE config)"
                                      if a.full_ft else "configs[%d]" % (4 if a.fp8 else 2 if a.text else 1), "+Text" if a.text else "",
                                      (" + BERT-small" if a.text else "") + (", fp8 e4m3 QKV/fc1/fc2 forward GEMMs with bf16 LoRA, "
                                                                             "attention, backward and loss" if a.fp8 else ""), B,
                                      "RCCL all-gather global-batch" if world > 1 else "local-batch"),
                       "local_batch": B, "global_batch": N, "parallelism": f"dp{world}",
                       "dropout": ("DISABLED (diagnostic run, not the benchmark configuration)" if nodrop else
                                   "HF defaults active (BERT hidden 0.1, attention-probs 0.1; timm ViT drop 0), train mode"),
                       "launch_path": ("eager (Python enqueue)" if graphed is None else
                                       "per-tower captured hipGraphs (forward_k | loss | backward_k | AdamW), each tower's all-gather / all-reduce issued from its stream between them"
                                       if world > 1 or force_dist else "hipGraph replay (one captured step)"),
                       "collectives": ("none (one process, local-batch loss)" if not (world > 1 or force_dist) else
                                       "C-ABI entry points (bsclip_allgather_* / bsclip_allreduce_grads): one RCCL communicator and stream per tower, event-ordered (BSCLIP_NATIVE_COMM=1)"
                                       if getattr(graphed, "native", False) else "torch.distributed (ProcessGroupNCCL = RCCL), issued from the tower streams"),
                       "numerics": {0: "default: bf16 GEMM / attention operands, bf16 residual and residual-gradient streams",
                                    1: "BSCLIP_PARITY=1: f32 residual / residual-gradient streams (diagnostic run)",
                                    2: "BSCLIP_PARITY=2: exact mode -- split-bf16 operands on every GEMM and attention product (diagnostic run: "
                                       "1e-3 parity with the f32 reference, not the benchmark configuration)"}[
                                        2 if _engine.EXACT_FORWARD else 0 if _engine.GRAD_STREAM_BF16 else 1],
                       "final_loss": round(final_loss, 6)},
            "step_roofline": {"bound": "mfma", "achieved": round(achieved, 1), "peak": PEAK_BF16_TFLOPS,
                              "unit": "TFLOP/s", "frac": round(achieved / PEAK_BF16_TFLOPS, 4),
                              "algorithmic_tflop_per_gpu_step": round(step_tflop_per_gpu, 3),
                              # the reference's work (SURVEY 8d model).  The build skips what cannot reach the result: the last
                              # ViT block's proj / MLP / attention rows other than token 0, forward and backward
                              "executed_tflop_per_gpu_step": round(step_tflop_per_gpu - skipped * B / 1e3, 3),
                              "executed_frac": round((step_tflop_per_gpu - skipped * B / 1e3)
                                                     / (ms * 1e-3) / PEAK_BF16_TFLOPS, 4),
                              # `peak` is the data-sheet figure at the 2.4 GHz peak engine clock.  The clock the chip held over
                              # the timed steps is measured (s_memtime / s_memrealtime); the matrix pipe's ceiling scales with it
                              "measured_engine_clock_ghz": None if clock_ghz is None else round(clock_ghz, 3),
                              "frac_of_peak_at_measured_clock": None if clock_ghz is None else
                              round(achieved / (PEAK_BF16_TFLOPS * clock_ghz / 2.4), 4)},
        }
        out["host"] = {"cpu_ms_per_step_all_threads": round(host_cpu_s / a.steps * 1e3, 3),
                       "cpu_ms_per_step_enqueue_thread": round(main_cpu_s / a.steps * 1e3, 3),
                       "enqueue_wall_ms_per_step": round(t_enq / a.steps * 1e3, 3),
                       "note": "the enqueueing thread sleeps between hipEventQuery polls (at most two steps queued ahead); what is left is "
                               "the HIP / ROCr runtime's own helper threads"}
        if dist_info is not None:
            out["dist"] = dist_info
        if a.dump_outputs:
            dump_outputs(a.dump_outputs, loss, model)
        if a.full:
            out["roofline"] = time_gemm_family("dx", B, device, a.pmc_traffic or DEFAULT_PMC_TRAFFIC["dx"])
            out["roofline_lowest"] = time_gemm_family("fc1", B, device, DEFAULT_PMC_TRAFFIC["fc1"])
        if a.full and world == 1 and not (a.fp8 or a.full_ft or a.no_extras):
            try:
                out["roofline_families"] = time_families(B, device)
            except Exception as exc:   # noqa: BLE001
                out["roofline_families"] = {"error": f"{type(exc).__name__}: {exc}"}
        if a.full and world == 1 and not force_dist and not (a.no_extras or a.no_text or a.fp8 or a.full_ft or nodrop or B != 256):
            # the other single-GPU-measurable BASELINE shapes, so that they are driver-run numbers
            graphed = None
            del opt, model
            torch.cuda.empty_cache()
            try:
                out["extra"] = {"configs[1] (I+D, bf16, local batch 256: the shape of north_star's 40 % target)":
                                side_measurement(device, False, False, 256, steps=a.steps),
                                "configs[4] per-GPU shape (fp8 trunks, I+D, local batch 512)": side_measurement(device, False, True, 512, steps=a.steps)}
                pm = side_measurement(device, True, False, 256, steps=a.steps, parity=1)
                out["parity_mode_ms_per_step"] = pm["ms_per_step"]
                xm = side_measurement(device, True, False, 256, steps=max(4, a.steps // 4), parity=2)
                out["exact_mode_ms_per_step"] = xm["ms_per_step"]
                out["exact_mode"] = ("BSCLIP_PARITY=2: the step that meets north_star's 1e-3 against the f32 reference on embeddings, loss and every "
                                     "gradient (forward AND backward GEMMs and every attention product on split-bf16 operands = 3 x the MFMA work, "
                                     "LoRA folded in f32, exact-erf GELU, f32 softmax / LayerNorm / LoRA-gradient arithmetic; golden 10-step "
                                     "trajectory within 1e-3, tests/test_20_encoders_gpu.py); same workload as the headline: what bf16 operands "
                                     "buy is the headline's ms_per_step against this (round 4: 158 ms with f32-operand MFMA attention)")
                dist_ = parity_distances()
                out["numerics_modes"] = {   # the three configurations on one line, time beside distance
                    "default (bf16 operands, bf16 streams)": {"ms_per_step": out["ms_per_step"], "rel_err_vs_f32_reference": dist_.get("default")},
                    "BSCLIP_PARITY=1 (f32 streams)": {"ms_per_step": pm["ms_per_step"], "rel_err_vs_f32_reference": dist_.get("parity1")},
                    "BSCLIP_PARITY=2 (exact: split-bf16 operands everywhere)": {"ms_per_step": xm["ms_per_step"], "rel_err_vs_f32_reference": dist_.get("exact")},
                    "no_cheaper_middle": "tools/site_sensitivity.py / profiles/r05_site_sensitivity.log: no subset of rounding sites carries the "
                                         "default's distance (every site within +-15 % of it; everything but the MLP still 5.6e-3), so no "
                                         "BSCLIP_PARITY=3 exists (DESIGN.md 4)",
                    "distances_source": dist_.get("source", dist_.get("error"))}
                out["parity_mode"] = ("BSCLIP_PARITY=1: f32 residual and residual-gradient streams + split-bf16 patch embedding, same workload "
                                      "as the headline (what the default's bf16 streams buy: headline ms_per_step vs this); trunk GEMM and "
                                      "attention operands stay bf16 in both (DESIGN.md 4)")
            except Exception as exc:   # noqa: BLE001 - the headline line must not die with a side measurement
                out["extra"] = {"error": f"{type(exc).__name__}: {exc}"}
        print(f"[bench] gpu: {ms:.2f} ms/step, {out['value']} pairs/s; host enqueue wall {t_enq / a.steps * 1e3:.2f} ms/step, "
              f"host cpu {host_cpu_s / a.steps * 1e3:.2f} ms/step", file=sys.stderr, flush=True)
        if a.full and world == 1 and not a.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline()
        sys.stdout.flush()
        os.write(real_stdout, (json.dumps(out) + "\n").encode())
    if world > 1 or force_dist:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
