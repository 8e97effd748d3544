"""Time of one frame of the assembled toc3d_amd.StreamPETRHead at the shipped sizes (batch 1, 6 x 20 x 50 tokens, 644 + 256 queries, 1024 memory entries, six decoder
layers) in ``fp32x3`` and ``bf16``: the whole ``forward`` and its stages one by one (events between the stages of the same composition), next to the sum of the
per-module figures already under profiles/ (decoder_time.json, head_queries_time.json, head_outputs_time.json).  A leg = one forward on a populated bank with the
frame's inputs on the device; warm-up 50, then the median of 200 event-timed legs (the benchmark's protocol).

Token-side A/B in the same file: ``HeadTokenEmbedding`` in ``"fp32"`` (two launches per Linear + ReLU, exact-f32 products: what it ran before ``"fp32x3"`` existed)
against ``"fp32x3"`` and ``"bf16"``; and, on the four GEMMs that carry a ReLU (M = 6000), ``EPI_BIAS`` + ``toc3d_relu_inplace`` against ``EPI_BIAS_RELU`` on the same
operands, dtype and tile -- five repeats of (warm-up 50, median of 200) each; ``spread_ms`` = the larger min-max range of the two forms over the repeats, and
``fused_not_slower`` says whether the fused median of medians lies within that spread of the two-launch one (a leg is bracketed by events and followed by a
synchronisation, so the two-launch legs include one inter-launch issue gap: margins of a few microseconds are of that order).  One JSON line on stdout, also written to --out.

  python tools/head_time.py
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import toc3d_amd                                  # noqa: E402
from toc3d_amd import gemm, lib, synth            # noqa: E402
from tools.decoder_time import timed              # noqa: E402

DEV = "cuda:0"
STAGES = ("tokens", "pre_update_memory", "queries", "decoder", "outputs", "post_update_memory")


def staged_frame(h, data, metas):
    """StreamPETRHead.forward, stage by stage, with an event between the stages -> ms per stage."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(STAGES) + 1)]
    ev[0].record()
    memory, pos_embed, _ = h._tokens(data["img_feats"], data["intrinsics"], data["lidar2img"], metas[0]["pad_shape"][0])
    ev[1].record()
    bank = h._memory(DEV)
    bank.pre_update_memory(data)
    ev[2].record()
    tgt, query_pos, reference_points, temp_memory, temp_pos, rec_ego_pose = h._queries.forward_from(bank)
    ev[3].record()
    outs_dec, _, _ = h.transformer(memory, tgt, query_pos, pos_embed, None, temp_memory, temp_pos)
    ev[4].record()
    outs_dec, cls, box = h._outputs(outs_dec, reference_points)
    ev[5].record()
    bank.post_update_memory(data, rec_ego_pose, cls, box, outs_dec)
    ev[6].record()
    ev[6].synchronize()
    return [ev[i].elapsed_time(ev[i + 1]) for i in range(len(STAGES))]


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def head_times(precision, warmup, steps):
    h = toc3d_amd.build_head(synth.head_cfg(), precision=precision)
    h.load_state_dict(synth.head_state_dict())
    h = h.to(DEV).eval()
    inp = synth.head_inputs()
    frames = [{k: v.to(DEV) for k, v in d.items()} for d in inp["frames"]]
    metas = inp["img_metas"]
    h(None, metas, None, **frames[0])                                  # scene start: from here on the bank is populated
    whole = timed(lambda: h(None, metas, None, **frames[1]), warmup, steps)
    for _ in range(warmup):
        staged_frame(h, frames[1], metas)
    per = [staged_frame(h, frames[1], metas) for _ in range(steps)]
    stages = {s: round(median([p[i] for p in per]), 4) for i, s in enumerate(STAGES)}
    return dict(forward=whole, stages_median_ms=stages, stages_sum_ms=round(sum(stages.values()), 4))


def per_module_profiles(precision):
    """The per-module figures measured earlier (one module at a time, replayed plans), where their files exist."""
    out = {}
    for name in ("decoder_time", "head_queries_time", "head_outputs_time"):
        path = os.path.join(ROOT, "profiles", name + ".json")
        if os.path.exists(path):
            d = json.loads(open(path).read().strip().splitlines()[-1])
            v = d.get(f"hip_{precision}", d.get(f"hip_{precision}_all"))          # (head_outputs_time.json: levels "all", the drop-in setting)
            if isinstance(v, dict) and "median_ms" in v:
                out[name] = v["median_ms"]
    if len(out) == 3:
        out["sum_ms"] = round(sum(out.values()), 4)
    return out


def token_side(warmup, steps):
    cfg = synth.HEAD_TOKENS_CFG
    inp = synth.head_tokens_inputs(cfg, 1, 6, 20, 50, seed=1)
    args = (inp["feats"].to(DEV), inp["intrinsics"].to(DEV), inp["lidar2img"].to(DEV), (320, 800, 3))
    res = {}
    for precision in ("fp32", "fp32x3", "bf16"):
        m = toc3d_amd.HeadTokenEmbedding(precision=precision, **cfg)
        m.load_state_dict(synth.head_tokens_state_dict(cfg, seed=1))
        m = m.to(DEV).eval()
        res[precision] = timed(lambda: m(*args), warmup, steps)
    return res


def relu_gemms(warmup, steps, repeats=5):
    """The four Linear + ReLU of the token side at M = 6000: (name, N, K)."""
    M, s = 6000, lib.stream_ptr
    out = {}
    for form, dt, pdt, tdt, planes in (("fp32x3", lib.F32X3WA, lib.F32, torch.float32, True), ("bf16", lib.BF16, lib.BF16, torch.bfloat16, False)):
        for name, N, K in (("position_encoder.0", 1024, 192), ("memory_embed.0", 256, 256), ("spatial_alignment.reduce.0", 256, 64), ("featurized_pe.conv_reduce", 256, 256)):
            g = torch.Generator().manual_seed(N + K)
            A = torch.randn(M, K, generator=g).to(DEV).to(tdt).contiguous()
            W = gemm.pack_weight(torch.randn(N, K, generator=g) * K ** -0.5, gemm.dtypes("fp32x3" if planes else "bf16"), DEV)
            b = (0.1 * torch.randn(N, generator=g)).to(DEV)
            if planes:
                lib.call("toc3d_x3_planes", A, K, A, K, M, K, s())
            o = torch.empty(M, N, dtype=tdt, device=DEV)
            v = gemm.small_m_variant(M, N, K, False)

            def launch(epi):
                lib.call("toc3d_linear_fused", dt, epi, v, A, K, W, W.shape[1], b, o, N, None, 0, 0, None, None, M, N, K, 0, *lib.NO_FUSED, s())

            def two():
                launch(lib.EPI_BIAS)
                lib.call("toc3d_relu_inplace", pdt, o, o.numel(), s())
            runs = {"bias_then_relu": [], "bias_relu": []}
            for _ in range(repeats):                                   # interleaved: both forms see the same drift of the card
                runs["bias_then_relu"].append(timed(two, warmup, steps)["median_ms"])
                runs["bias_relu"].append(timed(lambda: launch(lib.EPI_BIAS_RELU), warmup, steps)["median_ms"])
            spread = max(max(r) - min(r) for r in runs.values())
            m2, m1 = median(runs["bias_then_relu"]), median(runs["bias_relu"])
            out[f"{form} {name} M={M} N={N} K={K} v{v}"] = dict(bias_then_relu_ms=runs["bias_then_relu"], bias_relu_ms=runs["bias_relu"], median_two_ms=m2, median_fused_ms=m1,
                                                                 spread_ms=round(spread, 4), fused_not_slower=bool(m1 <= m2 + spread))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_time.json"))
    a = ap.parse_args()
    res = dict(tool="head_time", device=torch.cuda.get_device_name(0), sizes={k: v for k, v in synth.HEAD_FULL.items() if k != "decoder"}, shape=synth.HEAD_FULL_SHAPE,
               warmup=a.warmup, steps=a.steps)
    for precision in ("fp32x3", "bf16"):
        res[f"head_{precision}"] = head_times(precision, a.warmup, a.steps)
        res[f"per_module_profiles_{precision}"] = per_module_profiles(precision)
    res["token_side"] = token_side(a.warmup, a.steps)
    res["relu_gemms"] = relu_gemms(a.warmup, a.steps)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
