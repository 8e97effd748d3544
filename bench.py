#!/usr/bin/env python3
"""Benchmark of the hot path: 6-view frames/s through the EVA-02 ViT-L + ToC3D token-compression backbone.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--full] [--dump-outputs DIR]      (N > 1: launched by torch.distributed.run)

One "step" = one pass of the hot path over one synthetic 6-view frame per rank: patch-embed -> 24 blocks with the
three query-guided scorers and per-window token compression (ToC3D_faster, ratios 0.5/0.4/0.3, 6 x 3 x 320 x 800,
BASELINE.json configs[1]) -> CPFPN neck; with N > 1 ranks every rank processes its own frame (weak scaling, no
data-path collective inside the backbone) and the per-frame neck features are all-gathered over RCCL where the
detection head would consume them.  Inputs are resident in HBM before the timed region.  Rank 0 prints ONE JSON
line: the headline (metric, value, unit, higher_is_better, dtype, ms_per_step of the K timed steps).  With --full the
line also carries `roofline` for the dominant kernel (the bf16 MFMA GEMM behind every linear layer), the box
calibration, the side legs, the norm2-fold A/B and `cpu_baseline` (the oracle's eager-PyTorch fp32 port, timed on
the host cores).  --dump-outputs DIR writes what the last timed step computed as .npy files (inputs and weights are
seeded: the same arguments give the same inputs on every run).
"""
from __future__ import annotations

import argparse
import json
import os
import re
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import toc3d_amd  # noqa: E402
from toc3d_amd import configs, lib, synth  # noqa: E402

PEAK_BF16_TFLOPS = 2500.0       # MI355X dense bf16 MFMA peak (MI355X_MICROARCH.md, chip-level parameters)
PAPER_FPS = 1000.0 / 209.0      # ToC3D-Faster ViT-L 6x(800x320) backbone 209.0 ms, fp32, GPU unstated


def flop_model(cfg, V, h, w):
    """GEMM FLOPs per frame: (algorithmic, issued).  Algorithmic = as the reference executes (BASELINE.md section 2:
    padded window rows in dense blocks, k+1 rows per window in accelerated blocks); issued = what our launches do
    (dense blocks skip the zero-padded rows analytically; accelerated blocks give kept *padded* slots no row)."""
    C, Hd = cfg["embed_dim"], synth.hidden_dim(cfg)
    T = h * w
    per_attn = 2 * 4 * C * C            # q,k,v,proj per row
    per_mlp = 2 * 3 * C * Hd            # w1,w2,w3 per row
    alg = iss = 2.0 * V * T * (3 * 16 * 16) * C     # patch embed
    n_launch = 1
    stage = -1
    for i in range(cfg["depth"]):
        L = cfg["global_window_size"] if i in cfg["global_attn_indexes"] else cfg["window_size"]
        nW = V * (-(-h // L)) * (-(-w // L))
        if synth.is_toc3d(cfg) and i in cfg["pruning_loc"]:
            stage += 1
        if synth.is_toc3d(cfg) and stage >= 0:
            k = int(L * L * cfg["token_ratio"][stage])
            alg += nW * (k + 1) * (per_attn + per_mlp)                    # the reference runs k+1 rows per window, pads included
            iss += int(lib.load().toc3d_window_topk_rows(V, h, w, L, k)) * (per_attn + per_mlp)   # we run kept real tokens + 1
        else:
            alg += nW * L * L * per_attn + V * T * per_mlp
            iss += V * T * (per_attn + per_mlp)
        n_launch += 4
    return alg, iss, n_launch


def cpu_baseline(cfg, sd_cpu, inp, name):
    """Oracle (CPU eager fp32 port of the reference path) on the host cores, SURVEY.md 8d / BASELINE.md section 3 protocol: 1 warm-up + the MEDIAN of
    3 frames of the same workload (the warm-up is a 1-view forward: it pages the weights in and spins the thread pool up at a sixth of a frame's cost)."""
    from oracle import toc3d_oracle as O
    args = lambda d: (d["x"], d["temp_queries"], d["temp_ref_points"], d["temp_vel"], d["temp_timestamp"], d["temp_ego_pose"], d["ego_pose_inv"])
    ncpu = os.cpu_count() or 1
    # SURVEY.md 8d says "all host cores".  Measured on the pool's 256-thread hosts in round 6 (profiles/r06_cpu_baseline_all_cores.json, this protocol with
    # torch.set_num_threads(256)): 188.7 / 189.0 / 186.3 s per frame = 0.0053 frames/s against 3.9-4.3 s = 0.24 frames/s on 32 threads -- eager PyTorch on 6000-row ops
    # collapses under a 256-way fork/join per op (and the run takes 25 minutes).  The baseline a reader would tune is the 32-thread one: that is `value`, `cores` says so,
    # `host_cores` is the box's count, and the all-cores figure is quoted in `all_cores_note`.
    # (no more threads than this process may run on: the CPUs it is pinned to, and OMP_NUM_THREADS where that is set)
    usable = min(len(os.sched_getaffinity(0)), int(os.environ.get("OMP_NUM_THREADS") or ncpu))
    torch.set_num_threads(min(usable, 32))
    ts = []
    with torch.no_grad():
        warm = dict(inp, x=inp["x"][:1], gumbel=[g[:1] for g in inp["gumbel"]])
        O.forward_toc3d(sd_cpu, cfg, *args(warm), True, warm["gumbel"])               # warm-up
        for _ in range(3):
            t0 = time.perf_counter()
            O.forward_toc3d(sd_cpu, cfg, *args(inp), True, inp["gumbel"])
            ts.append(time.perf_counter() - t0)
    dt = sorted(ts)[1]
    return {"value": 1.0 / dt, "unit": "frames/s", "cores": torch.get_num_threads(), "host_cores": ncpu, "kind": "port", "config": name,
            "seconds_per_frame_each": [round(t, 3) for t in ts],
            "sample": f"median of 3 frames (6 views @ 800x320 each) of the {name} workload after a 1-view warm-up, eager PyTorch fp32 oracle",
            "all_cores_note": "threads capped at 32: with all 256 host threads the same protocol reads 0.0053 frames/s (188 s per frame; measured in round 6, "
                              "profiles/r06_cpu_baseline_all_cores.json) against 0.24 on 32 -- eager PyTorch does not scale past a few tens of threads on these ops"}


DUMP_BUDGET_BYTES = 63_000_000          # (the .npy headers stay well inside 64 MB)


def dump_outputs(out_dir, outs):
    """--dump-outputs: the arrays the timed step handed its caller -- the neck features and the backbone's return (features, per-stage token masks, kept /
    dropped token indices) -- as DIR/<name>.npy, floats in float32, indices in float64 (exact).  At most DUMP_BUDGET_BYTES in all: an array that does not
    fit its share is replaced by a fixed sample of its flattened elements (seeded by the name, sorted positions), the same on every run and build."""
    import zlib

    import numpy as np
    bb = outs["backbone"]
    arrays = {"neck_features": outs["neck"]}
    if isinstance(bb, dict):
        arrays.update(bb)
    else:
        arrays.update(bb.img_feats)
        for key in ("token_masks", "keep_idx", "drop_idx"):
            for s, t in enumerate(getattr(bb, key) or []):
                arrays[f"{key}_stage{s}"] = t
    host = {}
    for name, t in arrays.items():
        t = t.detach()
        host[name] = t.cpu().double().numpy() if not t.is_floating_point() else t.float().cpu().numpy()
    os.makedirs(out_dir, exist_ok=True)
    left, todo = DUMP_BUDGET_BYTES, sorted(host, key=lambda n: host[n].nbytes)
    for i, name in enumerate(todo):
        a = host[name]
        share = left // (len(todo) - i)
        if a.nbytes > share:
            k = share // a.itemsize
            idx = np.sort(np.random.default_rng(zlib.crc32(name.encode())).choice(a.size, size=k, replace=False))
            a = a.reshape(-1)[idx]
            print(f"[bench] --dump-outputs: {name} {tuple(host[name].shape)} sampled to {k} elements", file=sys.stderr)
        np.save(os.path.join(out_dir, f"{name}.npy"), a)
        left -= a.nbytes


def read_clocks():
    """Shader / memory clock in MHz while a kernel loop is in flight, or None.  hwmon's freq{1,2}_input (the instantaneous clock the SMU reports, in Hz) is the
    only sysfs source that moves with load on MI355X: pp_dpm_sclk lists the DPM levels and stars the LOWEST one in the fine-grained mode these boxes run in
    (it read 94 MHz under a GEMM loop in r04 -- the field was wrong and is no longer read).  Best effort, no tool is spawned; None when the file is absent."""
    import glob
    out = {"sclk_mhz": None, "mclk_mhz": None}
    # the node's other cards are visible in sysfs (and busy with other tenants' work): only the card whose PCI address is this process's device counts
    try:
        pr = torch.cuda.get_device_properties(torch.cuda.current_device())
        want = f"{pr.pci_domain_id:04x}:{pr.pci_bus_id:02x}:{pr.pci_device_id:02x}."
    except (AttributeError, RuntimeError):
        return out
    for card in sorted(glob.glob("/sys/class/drm/card*/device")):
        if not os.path.basename(os.path.realpath(card)).startswith(want):
            continue
        for key, fn in (("sclk_mhz", "freq1_input"), ("mclk_mhz", "freq2_input")):
            for path in sorted(glob.glob(f"{card}/hwmon/hwmon*/{fn}")):
                try:
                    out[key] = int(open(path).read().strip()) / 1e6
                except (OSError, ValueError):
                    continue
    return out


def calibrate(dev):
    """What THIS box does on two fixed yardsticks, measured before the timed region, so that a slow box is a number in the JSON line and not a sentence
    in DESIGN.md (the pool's boxes differ by 4-8 % on identical code):
      * GEMM: the library's own tile variant 16 on 6016 x 3072 x 1024 bf16 (bias epilogue, random operands), 30 back-to-back launches, TFLOP/s;
      * copy: a 256 MiB 16-byte-per-lane copy (toc3d_copy_bytes), read + write bytes per second;
      * clocks sampled while the GEMM loop is in flight."""
    M, N, K = 6016, 3072, 1024
    g = torch.Generator(device="cpu").manual_seed(1234)
    A = torch.randn(M, K, generator=g).to(dev).to(torch.bfloat16)
    W = (torch.randn(N, K, generator=g) * K ** -0.5).to(dev).to(torch.bfloat16)
    b = torch.randn(N, generator=g).to(dev)
    out = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
    s = lib.stream_ptr()
    run = lambda: lib.call("toc3d_linear_ex", lib.BF16, lib.EPI_BIAS, 16, A, K, W, K, b, out, N, None, 0, 0, None, None, M, N, K, 0, s)
    for _ in range(10):
        run()
    torch.cuda.synchronize()
    tf, clocks = [], None
    for r in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(30):
            run()
        e1.record()
        if r == 2:
            # the loop (30 x ~50 us) is still running on the GPU: sample a few times while it does and keep the highest reading
            samples = []
            while not e1.query() and len(samples) < 8:
                samples.append(read_clocks())
            best = lambda k: max([c[k] for c in samples if c[k] is not None], default=None)
            clocks = {"sclk_mhz": best("sclk_mhz"), "mclk_mhz": best("mclk_mhz"), "clock_samples_under_load": len(samples)}
        e1.synchronize()
        tf.append(2.0 * M * N * K * 30 / (e0.elapsed_time(e1) * 1e-3) / 1e12)
    nbytes = 256 << 20
    src = torch.empty(nbytes, dtype=torch.uint8, device=dev).random_(0, 255)
    dst = torch.empty_like(src)
    for _ in range(3):
        lib.call("toc3d_copy_bytes", dst, src, nbytes, s)
    torch.cuda.synchronize()
    gb = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(4):
            lib.call("toc3d_copy_bytes", dst, src, nbytes, s)
        e1.record()
        e1.synchronize()
        gb.append(2.0 * nbytes * 4 / (e0.elapsed_time(e1) * 1e-3) / 1e9)
    del A, W, out, src, dst
    torch.cuda.empty_cache()
    med = lambda v: sorted(v)[len(v) // 2]
    return {"gemm_yardstick_tflops": med(tf), "gemm_yardstick": "toc3d_linear_ex variant 16, 6016x3072x1024 bf16 + bias, 30 back-to-back launches, median of 5",
            "copy_gb_s": med(gb), "copy": "toc3d_copy_bytes 256 MiB (read + write bytes), 4 back-to-back launches, median of 5",
            "note": "this box's own yardsticks (the pool's boxes spread ~5 % on identical code; profiles/r0*_bench_*.json carry the same fields for the boxes the "
                    "committed numbers were taken on)",
            **(clocks or {"sclk_mhz": None, "mclk_mhz": None})}


def hbm_bytes(name, a, ctx):
    """Algorithmic HBM bytes of one launch of a token-level (HBM-bound) kernel from its C-ABI arguments, or None.
    ctx: tokens = V*h*w rows of the residual stream, rows_fn = toc3d_window_topk_rows, V / h / w."""
    esz = lambda dt: 2 if dt == lib.BF16 else 4
    if name == "toc3d_layernorm_rows":                    # read the f32 row, write the act row
        M, C = a[10], a[11]
        return M * C * (4 + esz(a[0]))
    if name == "toc3d_rebase_layernorm_rows":
        C, rows = a[2], a[15]
        return rows * C * (4 + esz(a[0]))
    if name in ("toc3d_gather_merge_ln_ex", "toc3d_gather_merge_ln", "toc3d_gather_merge_ln_split"):
        C, nW, rows = a[2], a[7], a[10]
        kept_copy = 1 if name == "toc3d_gather_merge_ln" else a[17]
        # every real token is read once (kept: copied, dropped: merged); kept rows leave in the act dtype (+ the f32 copy when asked for),
        # representative rows in both
        return ctx["tokens"] * C * 4 + rows * C * esz(a[0]) + (rows if kept_copy else nW) * C * 4
    if name == "toc3d_scatter_update":
        C, nW, N, k = a[1], a[4], a[5], a[6]
        L = int(round(N ** 0.5))
        kept = int(ctx["rows_fn"](ctx["V"], ctx["h"], ctx["w"], L, k)) - nW
        nrep = 4 if a[10] is not None else 2
        # kept rows: read the compact row, write the token row; dropped rows: read-modify-write; the windows' representative updates are read
        return kept * C * 8 + (ctx["tokens"] - kept) * C * 8 + nrep * nW * C * 4
    return None


def instrument(step, set_eager, cfg, V, h, w, precision, n_inst, want_block_loop=False, verbose=False):
    """Dominant-kernel timing of one leg: HIP events around every launch of each C-ABI op in an eager, single-stream pass of `step` (the models are switched
    by `set_eager(True / False)`), the cost of the bracketing event pair calibrated in the same pass, FLOPs from flop_model.  Returns (roofline dict,
    block-loop ms or None).  The GEMM family (every toc3d_linear* launch) is the dominant kernel of every leg."""
    orig_call = lib.call
    rec = []
    gemm_calls = {}                                    # tag -> (entry point, arguments) of every distinct GEMM launch: replayed below to calibrate the event cost
    hbm_ctx = dict(tokens=V * h * w, rows_fn=lib.load().toc3d_window_topk_rows, V=V, h=h, w=w)

    def timed_call(name, *a):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        orig_call(name, *a)
        e1.record()
        if name in ("toc3d_linear_fused", "toc3d_linear_qkv_rope"):
            gemm_calls.setdefault((name,) + tuple(a[15:18] if name == "toc3d_linear_fused" else a[9:12]), (name, a))
        if name in ("toc3d_linear_ex", "toc3d_linear_fused", "toc3d_linear_fused_ws"):
            tag = f"[epi{a[1]} v{a[2]} M={a[15]} N={a[16]} K={a[17]}]"
        elif name == "toc3d_linear":
            tag = f"[epi{a[1]} M={a[14]} N={a[15]} K={a[16]}]"
        elif name == "toc3d_linear_qkv_rope":
            tag = f"[epi9 v{a[1]} M={a[9]} N={a[10]} K={a[11]}]"
        elif name == "toc3d_conv3x3_nhwc":
            tag = f"[epi8 v{a[1]} M={a[9] * a[10] * a[11]} N={a[12]} K={9 * a[3]}]"
        elif name.startswith("toc3d_window_attention"):
            tag = f"[stride={a[11]} nwin={a[12]} maxq={a[13]}]"
        else:
            tag = ""
        rec.append((name, tag, e0, e1, hbm_bytes(name, a, hbm_ctx)))

    # the paper times the backbone's block loop only (toc3d_eva_vit.py:262,293): two events per step, one behind the
    # patch-embedding GEMM and one in front of the neck's first launch (single stream, no per-launch instrumentation)
    marks, state = [], {"stem": False}

    def marking_call(name, *a):
        if name == "toc3d_pack_weight" and marks and len(marks[-1]) == 1:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            marks[-1].append(e)
        orig_call(name, *a)
        if name in ("toc3d_im2col_patches", "toc3d_im2col_patches_u8"):
            state["stem"] = True
        elif state["stem"] and name in ("toc3d_linear_ex", "toc3d_linear_fused"):
            state["stem"] = False
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            marks.append([e])

    set_eager(True)                                    # one stream, one host call per launch: per-launch events, durations not inflated by co-running kernels
    block_loop_ms = None
    try:
        for _ in range(2):
            step()                                     # builds / autotunes the single-group plan outside the instrumented pass
        torch.cuda.synchronize()
        if want_block_loop:
            try:
                lib.call = marking_call
                for _ in range(max(n_inst, 5)):
                    step()
                torch.cuda.synchronize()
            finally:
                lib.call = orig_call
            loops = sorted(m[0].elapsed_time(m[1]) for m in marks if len(m) == 2)
            block_loop_ms = loops[len(loops) // 2] if loops else None
        try:
            lib.call = timed_call
            for _ in range(n_inst):
                step()
            torch.cuda.synchronize()
        finally:
            lib.call = orig_call
    finally:
        set_eager(False)
    # What an event pair adds to a launch it brackets (the pair's own packets between two kernels): every distinct GEMM launch of the frame replayed
    # R times back to back, once inside ONE event pair and once with a pair around every launch -- same kernels, same (warm) operands, so the
    # difference of the two per-launch times is the event cost alone.  It is subtracted from the GEMM launches' times below, which is what makes
    # roofline.avg_launch_ms comparable with the average kernel duration of `rocprofv3 --kernel-trace --stats` (profiles/r0*_kernel_stats.csv).
    ev_cost = []
    R_ = 12
    for key_, (nm_, a_) in list(gemm_calls.items()):
        for _ in range(3):
            orig_call(nm_, *a_)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(R_):
            orig_call(nm_, *a_)
        e1.record()
        pairs = []
        for _ in range(R_):
            p0, p1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            p0.record()
            orig_call(nm_, *a_)
            p1.record()
            pairs.append((p0, p1))
        torch.cuda.synchronize()
        ev_cost.append(sum(p0.elapsed_time(p1) for p0, p1 in pairs) / R_ - e0.elapsed_time(e1) / R_)
    event_cost_ms = max(0.0, sorted(ev_cost)[len(ev_cost) // 2]) if ev_cost else 0.0
    # ... and for the SHORT kernels (2-15 us row kernels) the same calibration on a short launch of their own size class -- a 64 KB toc3d_copy_bytes --, not
    # the GEMMs' figure ("pairs minus back-to-back" also contains whatever launch gap a long kernel hides and a short one does not: ADVICE r04)
    cs, cd = torch.empty(65536, dtype=torch.uint8, device="cuda"), torch.empty(65536, dtype=torch.uint8, device="cuda")
    sp = lib.stream_ptr()
    for _ in range(5):
        orig_call("toc3d_copy_bytes", cd, cs, 65536, sp)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(40):
        orig_call("toc3d_copy_bytes", cd, cs, 65536, sp)
    e1.record()
    pairs = []
    for _ in range(40):
        p0, p1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        p0.record()
        orig_call("toc3d_copy_bytes", cd, cs, 65536, sp)
        p1.record()
        pairs.append((p0, p1))
    torch.cuda.synchronize()
    short_event_cost_ms = max(0.0, sum(p0.elapsed_time(p1) for p0, p1 in pairs) / 40 - e0.elapsed_time(e1) / 40)
    detail, hbm, breakdown = {}, {}, {}
    for name, tag, e0, e1, nbytes in rec:
        t = e0.elapsed_time(e1)
        if nbytes is not None:
            hk = hbm.setdefault(name, [0, 0.0, 0.0])
            hk[0] += 1
            hk[1] += t
            hk[2] += nbytes
        d = breakdown.setdefault(name, [0, 0.0])
        d[0] += 1
        d[1] += t
        if tag:
            d = detail.setdefault(name + tag, [0, 0.0])
            d[0] += 1
            d[1] += t
    is_gemm = lambda k: k.startswith("toc3d_linear") or k.startswith("toc3d_conv3x3")
    # algorithmic HBM bytes of the GEMM launches: A + W + bias read once, the output written once (+ the f32 residual read for the
    # residual epilogues), in the element sizes the launch uses
    esz = 2 if precision == "bf16" else 4
    gemm_bytes = 0.0
    for name, tag, _, _, _ in rec:
        mnk = re.search(r"epi(\d+) .*M=(\d+) N=(\d+) K=(\d+)", tag) if is_gemm(name) else None
        if mnk:
            e, M_, N_, K_ = (int(v) for v in mnk.groups())
            out_b = 2 * M_ * N_ * 4 + (M_ * N_ * esz if e == 6 else 0) if e in (1, 5, 6) else (M_ * (N_ // 2) * esz if e in (2, 4, 7) else M_ * N_ * esz)
            gemm_bytes += (M_ * K_ + N_ * K_) * esz + N_ * 4 + out_b
    gemm_ms = sum(v[1] for k, v in breakdown.items() if is_gemm(k))
    gemm_n = sum(v[0] for k, v in breakdown.items() if is_gemm(k))
    alg, iss, n_launch = flop_model(cfg, V, h, w)
    # backbone GEMM launches only carry the model's FLOPs; the two neck GEMMs are counted on top
    neck_flops = 2.0 * V * h * w * 256 * (cfg["embed_dim"] + 9 * 256)
    avg_ms_raw = gemm_ms / gemm_n
    avg_ms = avg_ms_raw - event_cost_ms            # the launches' own time: event-timed minus the calibrated cost of the event pair
    per_launch = (alg + neck_flops) / (gemm_n / n_inst)
    peak = {"bf16": PEAK_BF16_TFLOPS, "fp32x3": PEAK_BF16_TFLOPS / 3, "fp32x6": PEAK_BF16_TFLOPS / 6}.get(precision, 157.3)
    peak_note = {"bf16": "dense bf16 MFMA peak (MI355X_MICROARCH.md)",
                 "fp32x3": "CONVENTION, not a hardware peak: the bf16 MFMA peak / 3 (three bf16 MFMAs per f32-operand product); against the bf16 peak itself frac is a third of this",
                 "fp32x6": "CONVENTION, not a hardware peak: the bf16 MFMA peak / 6 (six bf16 MFMAs per f32-operand product)"}.get(precision, "f32 MFMA peak (v_mfma_f32_16x16x4_f32, MI355X_MICROARCH.md)")
    roof = {"bound": "mfma", "kernel": "gemm_kernel<bf16|f32, epilogue> (all toc3d_linear / toc3d_conv3x3 launches)",
            "achieved": per_launch / (avg_ms * 1e-3) / 1e12, "peak": peak, "peak_note": peak_note,
            "unit": "TFLOP/s", "traffic": None,
            "avg_launch_ms": avg_ms, "avg_launch_ms_event_timed": avg_ms_raw, "event_pair_cost_ms": event_cost_ms,
            "frac_event_timed": per_launch / (avg_ms_raw * 1e-3) / 1e12 / peak,
            "launches_per_step": gemm_n / n_inst,
            "gemm_ms_per_step": gemm_ms / n_inst - event_cost_ms * gemm_n / n_inst,
            "algorithmic_flop_per_step": alg + neck_flops, "issued_flop_per_step": iss + neck_flops,
            "note": "HIP events around each launch in an eager, single-stream instrumented pass of the same step run right after the timed region; avg_launch_ms = "
                    "that average minus event_pair_cost_ms (what a bracketing event pair adds, calibrated in the same pass on the same launches: < 10 % of a GEMM launch) and is the number "
                    "to hold against the average gemm_kernel duration of profiles/r0*_kernel_stats.csv; frac_event_timed is the uncorrected form"}
    roof["frac"] = roof["achieved"] / roof["peak"]
    roof["frac_issued"] = roof["frac"] * (iss + neck_flops) / (alg + neck_flops)      # on the FLOPs the launches actually issue (pads skipped)
    # north_star: achieved HBM GB/s of the gather / scatter / LayerNorm row kernels = algorithmic bytes per launch / event time (same instrumented pass),
    # against the 8 TB/s HBM3E peak.  PRIMARY = the raw event-timed figure (a lower bound: it contains the event pair); the corrected figure subtracts the
    # short-launch calibration and is only given when that correction is under 30 % of the measured time (an unbounded correction on 2-10 us kernels inflates)
    hk_out = {}
    for k, v in sorted(hbm.items()):
        raw_ms = v[1] / v[0]
        ent = {"launches_per_step": v[0] // n_inst, "avg_us_event_timed": 1e3 * raw_ms, "algorithmic_mb_per_launch": v[2] / v[0] / 1e6,
               "achieved_gb_s": v[2] / v[0] / (raw_ms * 1e-3) / 1e9, "frac_of_8tb_s": v[2] / v[0] / (raw_ms * 1e-3) / 8e12}
        if short_event_cost_ms < 0.3 * raw_ms:
            c_ms = raw_ms - short_event_cost_ms
            ent.update({"avg_us_corrected": 1e3 * c_ms, "achieved_gb_s_corrected": v[2] / v[0] / (c_ms * 1e-3) / 1e9, "frac_of_8tb_s_corrected": v[2] / v[0] / (c_ms * 1e-3) / 8e12})
        hk_out[k.replace("toc3d_", "")] = ent
    roof["hbm_kernels"] = hk_out
    roof["hbm_kernels_note"] = f"raw event-timed figures are primary; *_corrected subtract the event-pair cost calibrated on a 64 KB copy launch ({1e3 * short_event_cost_ms:.2f} us) where that is < 30 % of the launch"
    roof["algorithmic_bytes_per_launch"] = gemm_bytes / gemm_n
    # Per distinct GEMM launch: the COMBINED floor max(FLOPs / MFMA peak, algorithmic bytes / 6.3 TB/s) and the fraction of it the launch reaches (the
    # MFMA fraction alone is the wrong roof for the N = 1024 residual GEMMs, whose f32 read-modify-write of the residual stream is a third of the launch).  6.3 TB/s = the
    # achievable HBM3E rate of MI355X_MICROARCH.md (8 TB/s nominal); times are event-timed minus the calibrated event-pair cost.
    per_shape = []
    for k, v in sorted(detail.items(), key=lambda kv: -kv[1][1]):
        mnk = re.search(r"epi(\d+) .*M=(\d+) N=(\d+) K=(\d+)", k)
        if not (is_gemm(k) and mnk):
            continue
        e, M_, N_, K_ = (int(x) for x in mnk.groups())
        out_b = 2 * M_ * N_ * 4 + (M_ * N_ * esz if e == 6 else 0) if e in (1, 5, 6) else (M_ * (N_ // 2) * esz if e in (2, 4, 7) else M_ * N_ * esz)
        nbytes = (M_ * K_ + N_ * K_) * esz + N_ * 4 + out_b
        fl = 2.0 * M_ * N_ * K_
        t_us = max(1e-3, 1e3 * (v[1] / v[0] - event_cost_ms))
        floor_us = max(fl / (peak * 1e12), nbytes / 6.3e12) * 1e6
        per_shape.append({"launch": k.replace("toc3d_", ""), "per_step": v[0] // n_inst, "us": round(t_us, 2), "tflops": round(fl / t_us / 1e6, 1),
                          "mb": round(nbytes / 1e6, 2), "floor_us": round(floor_us, 2), "floor": "mfma" if fl / (peak * 1e12) >= nbytes / 6.3e12 else "hbm",
                          "frac_of_floor": round(floor_us / t_us, 3)})
    roof["per_shape"] = per_shape
    roof["per_shape_note"] = "floor_us = max(2MNK / peak, algorithmic bytes / 6.3 TB/s); frac_of_floor = floor_us / us; FLOPs as issued by the launch (pads skipped)"
    if verbose:
        tot = sum(v[1] for v in breakdown.values())
        print("[bench] per-op GPU time per step (ms), event-timed eager pass:", file=sys.stderr)
        for k, v in sorted(breakdown.items(), key=lambda kv: -kv[1][1]):
            print(f"   {k:34s} {v[1] / n_inst:8.3f} ms  {v[0] // n_inst:4d} launches  {100 * v[1] / tot:5.1f}%", file=sys.stderr)
        print(f"   {'sum':34s} {tot / n_inst:8.3f} ms", file=sys.stderr)
        print("[bench] per-shape detail (us per launch, launches per step):", file=sys.stderr)
        for k, v in sorted(detail.items(), key=lambda kv: -kv[1][1]):
            mnk = re.search(r"M=(\d+) N=(\d+) K=(\d+)", k)
            tf = f"  {2.0 * int(mnk[1]) * int(mnk[2]) * int(mnk[3]) / (v[1] / v[0] * 1e-3) / 1e12:6.0f} TF issued" if mnk else ""
            print(f"   {k:70s} {1e3 * v[1] / v[0]:8.1f} us x {v[0] // n_inst:3d}  = {v[1] / n_inst:6.3f} ms{tf}", file=sys.stderr)
    return roof, block_loop_ms


def leg_roofline(roof):
    """The per-leg subset of instrument()'s dictionary (other_configs, batched, parity paths): enough to recompute frac from the line."""
    keep = ("kernel", "achieved", "peak", "peak_note", "unit", "frac", "frac_issued", "avg_launch_ms", "avg_launch_ms_event_timed", "event_pair_cost_ms",
            "launches_per_step", "gemm_ms_per_step", "algorithmic_flop_per_step", "issued_flop_per_step")
    return {"bound": "mfma", **{k: roof[k] for k in keep}}


def side_leg(config, H, W, args, dev, sd_cpu, tdist, steps=5, precision=None):
    """A short, separately built and timed run of another BASELINE.json configuration (same protocol, `steps` steps), reported beside the headline.
    ``precision``: another arithmetic than the headline's (the default precision fp32x3 at the hi-res input)."""
    if precision is not None:
        import argparse
        args = argparse.Namespace(**dict(vars(args), precision=precision))
    cfg = configs.get(config)
    if config == args.config:
        sd = sd_cpu
    else:                                                 # synthetic weights are drawn per parameter name: a sub-model shares the headline model's values
        sd = {k: sd_cpu[k] for k in synth.state_dict_spec(cfg) if k in sd_cpu}
        if len(sd) != len(synth.state_dict_spec(cfg)):
            sd = synth.make_state_dict(cfg)
    m = toc3d_amd.build_backbone(dict(cfg, precision=args.precision))
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    m.alias_outputs, m.launch_mode = True, args.launch
    n = toc3d_amd.build_neck(dict(configs.CPFPN_CFG, precision=args.precision))
    n.load_state_dict(synth.neck_state_dict(configs.CPFPN_CFG))
    n = n.to(dev).eval()
    n.alias_outputs, n.launch_mode = True, args.launch
    tpath = os.path.join(ROOT, "toc3d_amd", "tuned", f"{config}_{H}x{W}_{args.precision}.json")
    if os.path.exists(tpath):
        m.load_tuning(tpath)
        n._tuned.update(m._tuned)
    d = synth.make_inputs(cfg, n_frames=1, views_per_frame=6, hw=(H, W), seed=7)
    d = {k: ([t.to(dev) for t in v] if isinstance(v, list) else v.to(dev)) for k, v in d.items()}
    toc = synth.is_toc3d(cfg)

    def step():
        if toc:
            f = m(d["x"], temp_queries=d["temp_queries"], prev_exists=True, temp_ref_points=d["temp_ref_points"], temp_vel=d["temp_vel"],
                  temp_timestamp=d["temp_timestamp"], temp_ego_pose=d["temp_ego_pose"], ego_pose_inv=d["ego_pose_inv"], gumbel_noise=d["gumbel"]).img_feats["last_feat"]
        else:
            f = m(d["x"])["last_feat"]
        return n([f])[0]

    step()                                                # eager: packs (and tunes what the shipped table does not hold)
    torch.cuda.synchronize()
    el = tdist.timed_steps(step, steps, 3, dev)           # 2 more untimed steps record + replay the launch plan
    out = step()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out.float()).all())
    roof = None
    if not args.no_breakdown:
        def set_eager(on):
            m.launch_mode = n.launch_mode = "eager" if on else args.launch
        roof, _ = instrument(step, set_eager, cfg, 6, H // 16, W // 16, args.precision, 3)
    del m, n
    torch.cuda.empty_cache()
    return {"config": f"{config} EVA-02 ViT-L backbone + CPFPN neck, 6 views x 3x{H}x{W}", "value": steps / el, "unit": "frames/s", "ms_per_step": 1e3 * el / steps,
            "steps": steps, "dtype": "bf16" if args.precision == "bf16" else "f32", "tuned_table": os.path.exists(tpath),
            "roofline": None if roof is None else leg_roofline(roof)}


def dry_run(args, rank, world, tdist):
    """See main(): the script's multi-rank control flow with a stand-in step (CPU, gloo).  Not a benchmark."""
    import torch.distributed as dist
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo", rank=rank, world_size=world)
    assert not args.frames_total or args.frames_total % world == 0
    my_frames = list(tdist.frames_for_rank(args.frames_total, rank, world)) if args.frames_total else [rank]
    frames_per_step = args.frames_total if args.frames_total else world
    # strong scaling: a rank's frames are ONE forward of B = frames per rank (main()); --sequential-frames keeps one forward per frame
    batch = len(my_frames) if (args.frames_total and len(my_frames) > 1 and not args.sequential_frames) else 1
    forwards = [my_frames] if batch > 1 else [[f] for f in my_frames]
    gather = tdist.FeatureGather((6 * batch, 4, 2, 5), "cpu", dtype=torch.float32) if world > 1 and not args.sync_gather else None
    seen = []

    def step():
        for fw in forwards:
            time.sleep(0.002 * (1 + rank))
            n0 = torch.cat([torch.full((6, 4, 2, 5), float(f)) for f in fw], 0)     # (B * 6 views, ...): view 6 b belongs to frame fw[b]
            if gather is not None:
                t = gather.submit(n0)
                if t >= 1:
                    seen.append(gather.wait(t - 1)[:, ::6, 0, 0, 0].flatten().tolist())
            elif world > 1:
                seen.append(tdist.all_gather_features(n0, dtype=torch.float32)[:, ::6, 0, 0, 0].flatten().tolist())

    elapsed = tdist.timed_steps(step, args.steps, max(0, args.warmup), "cpu", finish=gather.drain if gather is not None else None)
    census = tdist.exchange_census(torch.full((6, 4, 2, 5), float(rank) + 0.5), "cpu") if world > 1 else None     # (one frame's worth: the byte count the test pins)
    if rank == 0:
        print(json.dumps({"metric": "LAUNCHER DRY RUN -- not a measurement", "value": frames_per_step * args.steps / elapsed, "unit": "frames/s", "n_gpus": world,
                          "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True,
                          "scaling": "strong" if args.frames_total else "weak", "vs_baseline": None, "dtype": "none", "data": "stand-in step, no kernels (TOC3D_BENCH_DRY_RUN=1)",
                          "config": {"workload": "dry run", "frames_per_step": frames_per_step, "frames_per_forward": batch, "last_exchange": seen[-1] if seen else None,
                                     "ranks_seen": census["ranks_seen"] if census else [0], "gather_bytes": census["gather_bytes"] if census else 0,
                                     "gather_verified": census["verified"] if census else None}}))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)           # 50 warm-up + 200 timed iterations (the driver passes its own)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--config", default="toc3d_faster")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32", "fp32x3", "fp32x6"])
    ap.add_argument("--hw", default="320x800")
    ap.add_argument("--groups", type=int, default=1, help="concurrent view groups (independent views on separate lanes / HIP streams); "
                    "measured r02: one lane replayed from a launch plan is as fast as two eagerly issued ones and steadier than two replayed ones")
    ap.add_argument("--launch", default="plan", choices=["plan", "graph", "eager"],
                    help="plan: the frame's launch sequence recorded once and replayed from C on HIP streams (toc3d_plan_run); "
                         "graph: the same recording as an explicitly built hipGraph; eager: every launch issued from Python")
    ap.add_argument("--frames-total", type=int, default=0, help="strong-scaling mode (SURVEY.md 8d C5): this many frames per step in total, "
                    "split over the ranks like the reference's DistributedSampler (contiguous chunks); 0 = one frame per rank per step (weak scaling)")
    ap.add_argument("--sequential-frames", action="store_true", help="--frames-total: run a rank's frames one forward after the other instead of as ONE forward "
                    "with B = frames per rank (the reference's own batch dimension, toc3d_eva_vit.py:230-242); the A/B leg of the batched form")
    ap.add_argument("--sync-gather", action="store_true", help="N > 1: all-gather the neck features on the compute stream instead of overlapped on a side stream")
    ap.add_argument("--tune-cache", default=None, help="JSON file: load the GEMM variant table if present, save it after warm-up "
                    "(default: the table shipped in toc3d_amd/tuned/ for this config, if any)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-batched", action="store_true", help="skip the short run with two frames per forward that is reported beside the headline")
    ap.add_argument("--no-parity-path", action="store_true", help="skip the short run of the strict-parity fp32 (exact-f32 MFMA) path that is reported beside the headline")
    ap.add_argument("--no-breakdown", action="store_true")
    ap.add_argument("--reps", type=int, default=None, help="the K-step timed region is repeated this many times (default 1, with --full 3); value / ms_per_step are "
                    "the MEDIAN repetition (every one is listed)")
    ap.add_argument("--no-other-configs", action="store_true", help="skip the short legs of BASELINE.json configs 3 (dense EVA_ViT) and 4 (ToC3D_faster @ 6x1600x640)")
    ap.add_argument("--no-ab", action="store_true", help="skip the interleaved in-run A/B of the norm2 fold (the shipped default against schedule=dict(fold_norm2=False))")
    ap.add_argument("--no-calibration", action="store_true", help="skip the box calibration (GEMM yardstick, copy bandwidth, clocks) in front of the timed region")
    ap.add_argument("--packed", default=None, help="a packed-weight file written BEFORE the launch (python bench.py --write-packed PATH, or model.save_packed): every rank "
                    "restores it (toc3d_amd/packed_io.py) instead of rank 0 drawing and packing a synthetic checkpoint while the other ranks wait at a barrier")
    ap.add_argument("--write-packed", default=None, help="draw the synthetic checkpoint, write the packed weights to this path and exit (one process, before an N > 1 launch)")
    ap.add_argument("--full", action="store_true", help="everything beside the headline: box calibration, per-kernel roofline, the side legs (batched, parity "
                    "paths, other configs), the norm2-fold A/B and the CPU baseline, and --reps 3 by default; the --no-* options switch single parts off again. "
                    "Without it a run sets up, warms up, times --steps steps once and prints the headline line")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR", help="after the timed region, write what the last timed step computed (rank 0's neck features "
                    "and the backbone outputs they came from) to DIR/<name>.npy in float32 / float64")
    args = ap.parse_args()
    if not args.full:
        args.no_calibration = args.no_breakdown = args.no_batched = args.no_parity_path = True
        args.no_other_configs = args.no_ab = args.no_cpu_baseline = True
    if args.reps is None:
        args.reps = 3 if args.full else 1

    rank = int(os.environ.get("RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    local = int(os.environ.get("LOCAL_RANK", 0))
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world} (launch with torch.distributed.run)"
    from toc3d_amd import dist as tdist
    if os.environ.get("TOC3D_BENCH_DRY_RUN") == "1":
        # LAUNCHER DRY RUN (tests/test_cpu_dist.py only): no model, no kernel, no measurement -- a stand-in step on the CPU over gloo, so that
        # the N > 1 control flow of this script (rank env, frame sharding, overlapped exchange, barriers, max over ranks, the one JSON line of
        # rank 0) can be exercised where there is no GPU.  The line it prints says so in "data" and can never be mistaken for a result.
        return dry_run(args, rank, world, tdist)
    assert torch.cuda.is_available(), "bench.py needs a GPU (the HIP extension is the only compute path)"
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        tdist.pin_rank_to_cores(local, int(os.environ.get("LOCAL_WORLD_SIZE", world)))   # one slice of host cores per rank
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    H, W = (int(v) for v in args.hw.split("x"))
    cfg = configs.get(args.config)
    is_toc = synth.is_toc3d(cfg)
    model = toc3d_amd.build_backbone(dict(cfg, precision=args.precision))
    if args.write_packed:
        assert world == 1, "--write-packed is a single-process preparation step"
        model.load_state_dict(synth.make_state_dict(cfg))
        model = model.to(dev).eval()
        model.save_packed(args.write_packed)
        print(json.dumps({"wrote_packed": args.write_packed, "config": args.config, "precision": args.precision}))
        return
    if args.packed:
        # the file exists before the launch: no rank draws a checkpoint, no rank waits for another (the world starts in step)
        sd_cpu = synth.make_state_dict(cfg) if world == 1 else None      # (one process: the side legs and the CPU baseline build their models from the state dict)
        model = model.to(dev).eval()
        model.load_packed(args.packed)
    elif world > 1:
        # one converter run for the node: rank 0 draws the synthetic checkpoint and writes the PACKED weights (toc3d_amd/packed_io.py, what the
        # kernels read); the other ranks restore that file instead of drawing and packing 1.2 GB each (eight host-bound minutes on one socket).
        # (rank 0's draw + pack serialises the start-up: `--packed PATH` with a file written beforehand avoids it)
        import tempfile
        packed_path = os.path.join(tempfile.gettempdir(), f"toc3d_bench_packed_{os.environ.get('MASTER_PORT', '0')}_{args.config}_{args.precision}.safetensors")
        sd_cpu = None
        model = model.to(dev).eval()
        if rank == 0:
            sd_cpu = synth.make_state_dict(cfg)
            model.load_state_dict(sd_cpu)
            model.save_packed(packed_path)
        tdist.barrier(dev)
        if rank != 0:
            model.load_packed(packed_path)
        tdist.barrier(dev)
        if rank == 0:
            os.remove(packed_path)
    else:
        sd_cpu = synth.make_state_dict(cfg)
        model.load_state_dict(sd_cpu)
        model = model.to(dev).eval()
    model.alias_outputs = True
    model_schedule = {k_: getattr(model, k_) for k_ in toc3d_amd.backbone.schedule_defaults(args.precision)}
    model.view_groups = args.groups
    model.launch_mode = args.launch
    neck = toc3d_amd.build_neck(dict(configs.CPFPN_CFG, precision=args.precision))
    neck.load_state_dict(synth.neck_state_dict(configs.CPFPN_CFG))
    neck = neck.to(dev).eval()
    neck.alias_outputs = True
    neck.launch_mode = args.launch

    main_model, main_neck = model, neck
    # weak scaling (default): every rank gets its own frame (seed = rank) -- independent units, one per rank per step.
    # strong scaling (--frames-total F): F frames per step in total, rank r owns the reference sampler's contiguous chunk
    # (datasets/samplers/distributed_sampler.py:41-44), every frame its own inputs (seed = frame id).
    assert not args.frames_total or args.frames_total % world == 0, \
        "--frames-total must be a multiple of the rank count: every rank issues one feature exchange per frame, uneven chunks would not pair up"
    my_frames = list(tdist.frames_for_rank(args.frames_total, rank, world)) if args.frames_total else [rank]
    frames_per_step = args.frames_total if args.frames_total else world
    to_dev = lambda d: {k: ([t.to(dev) for t in v] if isinstance(v, list) else v.to(dev)) for k, v in d.items()}
    inp_cpu = synth.make_inputs(cfg, n_frames=1, views_per_frame=6, hw=(H, W), seed=my_frames[0] if my_frames else rank)
    inps = [to_dev(inp_cpu)] + [to_dev(synth.make_inputs(cfg, n_frames=1, views_per_frame=6, hw=(H, W), seed=f)) for f in my_frames[1:]]
    inp = inps[0]
    V, h, w = 6, H // 16, W // 16
    # Strong scaling: a rank's F / world frames are ONE forward with B = frames per rank -- the reference's own batch dimension
    # (B = temp_queries.shape[0], 6 views per sample, samplers/distributed_sampler.py:41-44 + toc3d_eva_vit.py:230-242): every GEMM is B times as
    # tall, the per-launch floors are paid once per step instead of once per frame.  --sequential-frames keeps the per-frame loop (the A/B of this).
    batch_frames = len(inps) if (args.frames_total and len(inps) > 1 and not args.sequential_frames) else 1
    if batch_frames > 1:
        inps = [synth.stack_frames(inps)]
        V = 6 * batch_frames
    # the one exchange (BASELINE.json config 5): per-frame neck features for the head, all-gathered over RCCL on a side stream
    # while the next frame's backbone runs (toc3d_amd/dist.py); the head would wait on the ticket where it reads them
    gather = tdist.FeatureGather((V, 256, h, w), dev) if world > 1 and not args.sync_gather else None
    gathered = torch.empty(world, V, 256, h, w, dtype=torch.bfloat16, device=dev) if world > 1 and args.sync_gather else None

    last_outputs = {}                                        # what the most recent forward returned (aliases the workspace): --dump-outputs

    def one_frame(d):
        if is_toc:
            out = model(d["x"], temp_queries=d["temp_queries"], prev_exists=True, temp_ref_points=d["temp_ref_points"],
                        temp_vel=d["temp_vel"], temp_timestamp=d["temp_timestamp"], temp_ego_pose=d["temp_ego_pose"],
                        ego_pose_inv=d["ego_pose_inv"], gumbel_noise=d["gumbel"])
            feat = out.img_feats["last_feat"]
        else:
            out = model(d["x"])
            feat = out["last_feat"]
        n0 = neck([feat])[0]
        last_outputs["backbone"], last_outputs["neck"] = out, n0
        if world > 1 and my_frames:
            if gather is not None:
                gather.submit(n0)
            else:
                tdist.all_gather_features(n0, gathered)
        return n0

    def step():
        n0 = None
        for d in (inps if my_frames else []):
            n0 = one_frame(d)
        return n0

    def barrier():
        tdist.barrier(dev)

    # ---- warm-up (also packs weights / builds plans / autotunes the GEMM tiles) + timed region --------------
    shipped = os.path.join(ROOT, "toc3d_amd", "tuned", f"{args.config}_{H}x{W}_{args.precision}.json")
    tune_path = args.tune_cache or (shipped if os.path.exists(shipped) else None)
    if tune_path and os.path.exists(tune_path):
        model.load_tuning(tune_path)
        neck._tuned.update(model._tuned)                     # one (epilogue, M, N, K) -> variant table serves backbone and neck
    calibration = None if (args.no_calibration or rank != 0) else calibrate(dev)     # rank 0 only (collective-free; the timed region starts behind a barrier anyway)
    step()                                                   # first forward: packs, tunes shapes the table does not hold
    torch.cuda.synchronize()
    if args.tune_cache and rank == 0:
        model._tuned.update(neck._tuned)
        model.save_tuning(args.tune_cache)
    # W untimed steps, barrier + sync, EXACTLY K timed steps (the overlapped exchange drained inside the timed region), barrier + sync,
    # max over ranks -- toc3d_amd/dist.py:timed_steps, the same function the world-2 gloo test drives
    fin = gather.drain if gather is not None else None
    runs = [tdist.timed_steps(step, args.steps, max(0, args.warmup - 1), dev, finish=fin)]
    for _ in range(max(1, args.reps) - 1):                   # the same region again (no further warm-up): a 0.25 s region moves with the box's clocks
        runs.append(tdist.timed_steps(step, args.steps, 0, dev, finish=fin))
    elapsed = sorted(runs)[len(runs) // 2]
    if args.dump_outputs and rank == 0 and last_outputs:
        dump_outputs(args.dump_outputs, last_outputs)       # the timed region ended in a device sync: the buffers hold the last timed step

    last = step()
    torch.cuda.synchronize()
    assert last is None or bool(torch.isfinite(last.float()).all()), "non-finite neck features after the timed region"
    # N > 1: one verified exchange of the features just computed -- rank census + per-rank checksums through the same collective (toc3d_amd/dist.py)
    census = tdist.exchange_census(last, dev) if world > 1 and last is not None else None
    if census is not None:
        assert census["verified"], f"feature exchange failed its checksum census: {census}"

    # ---- dominant-kernel timing: HIP events around every launch of each C-ABI op (eager, same stream) ------
    roof = None
    block_loop_ms = None
    n_inst = min(args.steps, 5)

    def set_eager(on, models=None):
        nonlocal world, inps
        for m_ in (models or [model, neck]):
            m_.launch_mode = "eager" if on else args.launch
        if models is None:
            model.view_groups = 1 if on else args.groups
        if on:
            set_eager.saved = (world, inps)
            world, inps = 1, inps[:1]                  # no collective in the instrumented pass, one forward per instrumented step
        else:
            world, inps = set_eager.saved

    if rank == 0 and not args.no_breakdown:
        roof, block_loop_ms = instrument(step, set_eager, cfg, V, h, w, args.precision, n_inst, want_block_loop=True, verbose=True)
        # memory-side bytes per launch of the same kernel family from the committed rocprofv3 --pmc passes (FETCH_SIZE x 2 on
        # gfx950 + WRITE_SIZE, see profiles/r01_gemm_hbm_traffic.json); only valid for the profiled workload
        for tag_ in ("r06", "r05", "r04", "r03", "r02", "r01"):               # newest committed PMC pass of this workload (tools/gpu/profile.sh + tools/summarize_prof.py)
            tpath = os.path.join(ROOT, "profiles", f"{tag_}_gemm_hbm_traffic.json")
            if os.path.exists(tpath) and args.config == "toc3d_faster" and (H, W) == (320, 800) and args.precision == "bf16":
                tj = json.load(open(tpath))
                # counters cannot be collected inside the run: the committed pass is only quoted while it describes THIS launch schedule
                # (a switch that did not exist when the pass was taken and is OFF in this model changes nothing: only the recorded keys must agree)
                rec_s = tj.get("schedule") or {}
                if rec_s and all(model_schedule.get(k) == v for k, v in rec_s.items()) and not any(model_schedule[k] for k in model_schedule if k not in rec_s):
                    roof["traffic"] = tj["hbm_bytes_per_launch"]
                    roof["traffic_source"] = f"profiles/{tag_}_gemm_hbm_traffic.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command; not collected inside this run)"
                else:
                    roof["traffic_source"] = f"profiles/{tag_}_gemm_hbm_traffic.json was taken with another launch schedule ({tj.get('schedule')}): stale, not quoted"
                break

    if rank == 0:
        world_report = world
        ms = 1e3 * elapsed / args.steps
        value = frames_per_step * args.steps / elapsed
        alg, iss, _ = flop_model(cfg, V, h, w)
        res = {
            "metric": "multi-view frames/sec through ViT+ToC3D backbone, 6x(800x320)" if (H, W) == (320, 800) else f"multi-view frames/sec through ViT+ToC3D backbone, 6x({W}x{H})",
            "value": value, "unit": "frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms,
            "repetitions": {"n": len(runs), "ms_per_step_each": [1e3 * r / args.steps for r in runs], "reported": "median"},
            "higher_is_better": True, "scaling": "strong" if args.frames_total else "weak",
            "vs_baseline": (value / PAPER_FPS) if (args.config == "toc3d_faster" and (H, W) == (320, 800)) else None,
            "dtype": "bf16" if args.precision == "bf16" else "f32", "data": "synthetic",
            "config": {"workload": f"{args.config} EVA-02 ViT-L backbone + CPFPN neck, 6 views x 3x{H}x{W} per frame, "
                                   + (f"{args.frames_total} frames per step split over the ranks"
                                      + (f" (each rank's {batch_frames} frames as ONE forward, B = {batch_frames}), " if batch_frames > 1 else " (one forward per frame), ")
                                      if args.frames_total else "1 frame per rank per step, ")
                                   + "random-init weights, prev_exists=True, injected Gumbel noise",
                       "frames_per_step": frames_per_step, "frames_per_forward": batch_frames,
                       "feature_exchange": None if world_report == 1 else ("all-gather on the compute stream" if args.sync_gather else "all-gather overlapped on a side stream"),
                       "launch": {"plan": "recorded launch plan replayed from C (toc3d_plan_run, HIP streams)", "graph": "recorded launch plan as an explicit hipGraph",
                                  "eager": "eager (Python issues every launch)"}[args.launch],
                       "view_groups": args.groups,
                       "alias_outputs": True,           # NOT the module default: the returned tensors alias the reused workspace (the default clones 24.6 MB through torch, ~0.2 %)
                       "schedule": model_schedule,
                       "ranks_seen": census["ranks_seen"] if census else [0], "gather_bytes": census["gather_bytes"] if census else 0,
                       "gather_verified": census["verified"] if census else None,
                       "baseline_note": "vs_baseline divides by the paper's 4.78 backbone-frames/s (fp32, GPU model unstated, BASELINE.md section 1)"},
            "whole_path_tflops": (flop_model(cfg, 6, h, w)[0] * frames_per_step / world_report / (ms * 1e-3)) / 1e12,      # per GPU (algorithmic FLOPs of ONE frame x frames)
            "paper_protocol": None if roof is None or block_loop_ms is None else {
                "block_loop_ms": block_loop_ms, "block_loop_frames_per_s": 1e3 / block_loop_ms,
                "note": "block loop only, single stream, event-timed (the span the paper's 209 ms covers); the headline value also "
                        "includes patch embedding, the scorer-side query preparation and the CPFPN neck"},
        }
        if calibration is not None:
            res["calibration"] = calibration
        if roof is not None:
            res["roofline"] = roof
        if not args.no_batched and is_toc and world == 1 and not args.frames_total:
            # throughput mode, reported BESIDE the headline (which stays one 6-view frame per forward, BASELINE.json configs[1]): two frames of
            # different sequences per forward -- the reference's own batch dimension (B = temp_queries.shape[0], toc3d_eva_vit.py:230-242;
            # samples_per_gpu > 1) -- doubles M of every GEMM and halves the per-launch floors per frame
            Bf = 2
            inp2 = to_dev(synth.make_inputs(cfg, n_frames=Bf, views_per_frame=6, hw=(H, W), seed=1000 + rank))
            inps_1, inps = inps, [inp2]
            step()
            torch.cuda.synchronize()
            kb = max(5, min(args.steps, 30))
            eb = tdist.timed_steps(step, kb, 3, dev)
            res["batched"] = {"frames_per_forward": Bf, "value": Bf * kb / eb, "unit": "frames/s", "ms_per_forward": 1e3 * eb / kb, "steps": kb,
                              "note": "same model and kernels, 12 views per forward (two sequences); not the headline configuration"}
            if not args.no_breakdown:
                res["batched"]["roofline"] = leg_roofline(instrument(step, set_eager, cfg, 6 * Bf, h, w, args.precision, 3)[0])
            inps = inps_1
        if not args.no_parity_path and args.precision == "bf16" and world == 1:
            # the path that meets the 1e-3 parity bar (exact-f32 MFMA, rel. max err 5e-6 vs the reference, tests/test_gpu_e2e.py), timed
            # with the same protocol on the same inputs: what the bf16 headline costs in accuracy is reported next to what parity costs in speed
            m32 = toc3d_amd.build_backbone(dict(cfg, precision="fp32"))
            m32.load_state_dict(sd_cpu)
            m32 = m32.to(dev).eval()
            m32.alias_outputs, m32.launch_mode = True, args.launch
            n32 = toc3d_amd.build_neck(dict(configs.CPFPN_CFG, precision="fp32"))
            n32.load_state_dict(synth.neck_state_dict(configs.CPFPN_CFG))
            n32 = n32.to(dev).eval()
            n32.alias_outputs, n32.launch_mode = True, args.launch
            t32 = os.path.join(ROOT, "toc3d_amd", "tuned", f"{args.config}_{H}x{W}_fp32.json")
            if os.path.exists(t32):
                m32.load_tuning(t32)
                n32._tuned.update(m32._tuned)
            model, neck = m32, n32
            step()
            torch.cuda.synchronize()
            k32 = max(3, min(args.steps, 10))
            e32 = tdist.timed_steps(step, k32, 2, dev)
            res["parity_path"] = {"precision": "fp32 (v_mfma_f32_16x16x4_f32, exact f32 products)", "value": frames_per_step * k32 / e32, "unit": "frames/s",
                                  "ms_per_step": 1e3 * e32 / k32, "steps": k32,
                                  "parity": "rel. max err 5e-6 vs the reference's fp32 features, kept-token IoU 1.0 (tests/test_gpu_e2e.py, tests/golden/vitl_*.npz)"}
            if not args.no_breakdown:
                res["parity_path"]["roofline"] = leg_roofline(instrument(step, set_eager, cfg, V, h, w, "fp32", 2)[0])
        if not args.no_parity_path and args.precision == "bf16" and world == 1:
            # ... and the parity-grade FAST path: the same f32 buffers and kernels, the linear layers' products as three bf16 MFMAs on (hi, lo)
            # operand splits (precision="fp32x3"; <= 1e-3 vs the reference on every golden case, tests/test_gpu_e2e.py / test_gpu_parity_bf16.py)
            mx3 = toc3d_amd.build_backbone(dict(cfg, precision="fp32x3"))
            mx3.load_state_dict(sd_cpu)
            mx3 = mx3.to(dev).eval()
            mx3.alias_outputs, mx3.launch_mode = True, args.launch
            nx3 = toc3d_amd.build_neck(dict(configs.CPFPN_CFG, precision="fp32x3"))
            nx3.load_state_dict(synth.neck_state_dict(configs.CPFPN_CFG))
            nx3 = nx3.to(dev).eval()
            nx3.alias_outputs, nx3.launch_mode = True, args.launch
            tx3 = os.path.join(ROOT, "toc3d_amd", "tuned", f"{args.config}_{H}x{W}_fp32x3.json")
            if os.path.exists(tx3):
                mx3.load_tuning(tx3)
                nx3._tuned.update(mx3._tuned)
            model, neck = mx3, nx3
            step()
            torch.cuda.synchronize()
            kx3 = max(3, min(args.steps, 40))                # (the default precision's leg: 40 steps behind 6 warm-up steps -- 10 behind 2 read 3 % low against a standalone run)
            ex3 = tdist.timed_steps(step, kx3, 6, dev)
            res["parity_path_fast"] = {"precision": "fp32x3 (f32 buffers; a.w = hi.hi + hi.lo + lo.hi on v_mfma_f32_16x16x32_bf16, f32 accumulate)",
                                       "value": frames_per_step * kx3 / ex3, "unit": "frames/s", "ms_per_step": 1e3 * ex3 / kx3, "steps": kx3,
                                       "parity": "<= 1e-3 rel. max err vs the reference's fp32 features on the 800x320 golden cases (tests/test_gpu_e2e.py::test_vitl_fp32_matches_reference[fp32x3]: "
                                                 "3e-5); at 1600-wide inputs the bound is on the kept sets (tests/test_gpu_parity_bf16.py::test_vitl_1600_fp32_matches_reference: one top-k near-tie per "
                                                 "input may break the other way than the reference's CPU summation order -- that window's tokens then differ by up to 0.15 rel. max --, every other token <= 1e-3)"}
            if not args.no_breakdown:
                res["parity_path_fast"]["roofline"] = leg_roofline(instrument(step, set_eager, cfg, V, h, w, "fp32x3", 3)[0])
        if not args.no_parity_path and args.precision == "bf16" and world == 1:
            # ... and the f32-GRADE form of the same idea: a three-way split, six bf16 MFMAs per product (dropped terms <= 2^-26: as accurate as the exact-f32 MFMA
            # in tests/test_gpu_ops.py::test_linear_bf16x3_products_on_f32_operands), every other kernel in its exact-f32 form
            mx6 = toc3d_amd.build_backbone(dict(cfg, precision="fp32x6"))
            mx6.load_state_dict(sd_cpu)
            mx6 = mx6.to(dev).eval()
            mx6.alias_outputs, mx6.launch_mode = True, args.launch
            nx6 = toc3d_amd.build_neck(dict(configs.CPFPN_CFG, precision="fp32x6"))
            nx6.load_state_dict(synth.neck_state_dict(configs.CPFPN_CFG))
            nx6 = nx6.to(dev).eval()
            nx6.alias_outputs, nx6.launch_mode = True, args.launch
            tx6 = os.path.join(ROOT, "toc3d_amd", "tuned", f"{args.config}_{H}x{W}_fp32x6.json")
            if os.path.exists(tx6):
                mx6.load_tuning(tx6)
                nx6._tuned.update(mx6._tuned)
            model, neck = mx6, nx6
            step()
            torch.cuda.synchronize()
            kx6 = max(3, min(args.steps, 10))
            ex6 = tdist.timed_steps(step, kx6, 2, dev)
            res["parity_path_x6"] = {"precision": "fp32x6 (f32 buffers; a.w from six bf16 MFMAs on (hi, mid, lo) splits: f32-grade products; exact-f32 attention)",
                                     "value": frames_per_step * kx6 / ex6, "unit": "frames/s", "ms_per_step": 1e3 * ex6 / kx6, "steps": kx6,
                                     "parity": "<= 1e-3 rel. max err vs the reference's fp32 features on the 800x320 golden cases (tests/test_gpu_e2e.py::test_vitl_fp32_matches_reference[fp32x6]: 6e-6); "
                                               "1600-wide inputs: bounded through the kept sets like fp32x3 (tests/test_gpu_parity_bf16.py::test_vitl_1600_fp32_matches_reference)"}
            if not args.no_breakdown:
                res["parity_path_x6"]["roofline"] = leg_roofline(instrument(step, set_eager, cfg, V, h, w, "fp32x6", 2)[0])
        if not args.no_other_configs and world == 1 and args.config == "toc3d_faster" and (H, W) == (320, 800) and not args.frames_total:
            # BASELINE.json configs 3 and 4, driver-timed in the same line: the dense EVA_ViT baseline (keep ratio 1.0) and ToC3D_faster at 6 x 1600 x 640
            # ... and at 6 x 1600 x 800, the reference's real hi-res input (ToC3D_1600_resolution/ToC3D_faster_1600.py:176-177; SURVEY.md 8d C4 "benchmark both")
            res["other_configs"] = [side_leg("eva_dense", 320, 800, args, dev, sd_cpu, tdist), side_leg("toc3d_faster", 640, 1600, args, dev, sd_cpu, tdist),
                                    side_leg("toc3d_faster", 800, 1600, args, dev, sd_cpu, tdist, steps=4)]
            if args.precision == "bf16" and not args.no_parity_path:
                # ... and what an unchanged reference config gets there: the default precision (fp32x3) at BASELINE.json config 4's input
                res["parity_path_fast_1600x640"] = side_leg("toc3d_faster", 640, 1600, args, dev, sd_cpu, tdist, steps=4, precision="fp32x3")
        if not args.no_ab and args.precision == "bf16" and is_toc and world == 1 and not args.frames_total:
            # One round only: the norm2 fold became the default on +0.3 % evidence; here the shipped schedule and the explicit
            # LayerNorm launch alternate >= 5 times IN THIS RUN, on the driver's box.  Rule for every default from now on: no flip on < 1 % from < 5
            # same-box alternations.
            # Both legs are models built NOW (a twin of the shipped schedule and the other schedule): a process's first model measures ~2 % faster than
            # any identical model built later (its side streams do not share a hardware queue with the caller's stream, profiles/r04_stream_priority.txt),
            # so the headline model itself must not be a leg.
            def ab_model(sched):
                mb = toc3d_amd.build_backbone(dict(cfg, precision="bf16", schedule=sched))
                mb.load_state_dict(sd_cpu)
                mb = mb.to(dev).eval()
                mb.alias_outputs, mb.launch_mode = True, args.launch
                if tune_path and os.path.exists(tune_path):
                    mb.load_tuning(tune_path)
                nb_ = toc3d_amd.build_neck(dict(configs.CPFPN_CFG, precision="bf16"))
                nb_.load_state_dict(synth.neck_state_dict(configs.CPFPN_CFG))
                nb_ = nb_.to(dev).eval()
                nb_.alias_outputs, nb_.launch_mode = True, args.launch
                nb_._tuned.update(mb._tuned)
                return mb, nb_
            legs = {"shipped": ab_model(dict(model_schedule)), "other": ab_model(dict(model_schedule, fold_norm2=not model_schedule["fold_norm2"]))}
            times = {"shipped": [], "other": []}
            for which in ("other", "shipped"):              # warm both: pack, (tune), record, replay
                model, neck = legs[which]
                for _ in range(4):
                    step()
            torch.cuda.synchronize()
            for _ in range(5):
                for which in ("shipped", "other"):
                    model, neck = legs[which]
                    times[which].append(tdist.timed_steps(step, args.steps, 1, dev))
            med = lambda v: sorted(v)[len(v) // 2]
            fps = lambda t: frames_per_step * args.steps / t
            res["ab_norm2_fold"] = {"shipped": {"fold_norm2": model_schedule["fold_norm2"], "frames_per_s_each": [fps(t) for t in times["shipped"]], "median": fps(med(times["shipped"]))},
                                    "other": {"fold_norm2": not model_schedule["fold_norm2"], "frames_per_s_each": [fps(t) for t in times["other"]], "median": fps(med(times["other"]))},
                                    "shipped_over_other": med(times["other"]) / med(times["shipped"]),
                                    "protocol": f"5 alternations of {args.steps}-step timed regions in this run between two models built for this leg (same weights, same tile "
                                                "table, replayed launch plans); neither is the headline model, which as the process's first model runs ~2 % faster than either"}
            model, neck = main_model, main_neck
            del legs
            torch.cuda.empty_cache()
        if not args.no_cpu_baseline and is_toc and (H, W) == (320, 800) and world == 1:
            res["cpu_baseline"] = cpu_baseline(cfg, sd_cpu, inp_cpu, "ToC3D_faster (ratio 5/4/3), BASELINE.json configs[1]")
            if args.config == "toc3d_faster":
                # BASELINE.json configs[0] exists only as a CPU row: ToC3D_fast (ratio 7/5/5) on the same synthetic frame and weights
                res["cpu_baseline_configs0"] = cpu_baseline(configs.get("toc3d_fast"), sd_cpu, inp_cpu, "ToC3D_fast (ratio 7/5/5), BASELINE.json configs[0]")
        # Top-level SCALAR copies of what a reader needs to hold this line against another box or another round (a driver that keeps only known
        # top-level keys drops the nested dictionaries): the box's yardsticks, every side leg's frames/s and GEMM roofline fraction.
        def hoist(key, node, *path):
            for p_ in path:
                node = node.get(p_) if isinstance(node, dict) else None
            if isinstance(node, (int, float)):
                res[key] = node
        hoist("roofline_frac", res, "roofline", "frac")
        hoist("calibration_gemm_yardstick_tflops", res, "calibration", "gemm_yardstick_tflops")
        hoist("calibration_copy_gb_s", res, "calibration", "copy_gb_s")
        hoist("calibration_sclk_mhz", res, "calibration", "sclk_mhz")
        for leg in ("batched", "parity_path", "parity_path_fast", "parity_path_x6"):
            hoist(f"{leg}_value", res, leg, "value")
            hoist(f"{leg}_roofline_frac", res, leg, "roofline", "frac")
        for oc, tag in zip(res.get("other_configs") or [], ("dense_eva_vit", "toc3d_faster_1600x640", "toc3d_faster_1600x800")):
            hoist(f"{tag}_value", oc, "value")
            hoist(f"{tag}_roofline_frac", oc, "roofline", "frac")
        hoist("parity_path_fast_1600x640_value", res, "parity_path_fast_1600x640", "value")
        hoist("cpu_baseline_value", res, "cpu_baseline", "value")
        hoist("cpu_baseline_cores", res, "cpu_baseline", "cores")
        print(json.dumps(res))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
