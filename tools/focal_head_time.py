"""Time of one toc3d_amd.FocalHead frame at the shipped size (6 views of 20 x 50 tokens, 256 channels, ten classes), for ``infer_ratio`` 1.0 and 0.5 in both
precisions: the whole ``forward`` (staging copies, ``toc3d_nchw_to_rows``, the four launches replayed from the recorded plan, the clones of the outputs), the
same with eager launches, ``forward_rows`` (no NCHW tensor), and each of the four launches on its own (event-timed back to back on the module's workspace, so a
launch's figure holds its launch overhead).  Next to that, torch eager running the restatement of tests/focal_head_cases.py on the same card in the same run
(f32 next to fp32x3; the conv operands rounded to bf16 next to bf16).  Warm-up 50, then the median of 200 event-timed legs.  One JSON line on stdout, also
written to --out (default profiles/focal_head_time.json).

  python tools/focal_head_time.py                  # the timing
  python tools/focal_head_time.py --frames 20 --precision fp32x3     # just run frames (under `rocprofv3 --kernel-trace --stats -- python ...`)
  python tools/focal_head_time.py --select         # select_rows against forward_rows -> profiles/focal_select_time.json

``--select``: the selection-only frame (``FocalHead.select_rows``: the class tower's conv, one-branch statistics, ``toc3d_focal_sample_weight``, the ranking)
against ``forward_rows`` of the same module on the same rows at ``infer_ratio`` 0.5, in both precisions: warm-up 50, the median of 200 legs, three repetitions
alternating the two forms so both see the same drift of the card; per form the three medians, their median and their spread (max - min).
``select_not_slower``: the selection's median lies within ``forward_rows``' own spread of it.  Then each form launch by launch (event-timed back to back, so a
launch's figure holds its launch overhead).
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import focal_head_cases as FC            # noqa: E402
import toc3d_amd                         # noqa: E402
from toc3d_amd import lib, synth         # noqa: E402
from tools.decoder_time import timed     # noqa: E402

DEV = "cuda:0"


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def run_select(a, module, inp, sizes, shape):
    B, N, h, w, C = shape["B"], shape["N"], shape["h"], shape["w"], sizes["in_channels"]
    key, K = (B, N, h, w), int(N * h * w * 0.5)
    res = dict(tool="focal_head_time --select", device=torch.cuda.get_device_name(0), sizes=dict(sizes, infer_ratio=0.5), shape=shape, warmup=a.warmup, steps=a.steps,
               repeats=3)
    for precision in ("fp32x3", "bf16"):
        m = module(precision, 0.5)
        full = m(inp["location"], img_feats=inp["img_feats"])
        rows = m._ws[key]["rows"].clone()
        legs = dict(forward_rows=lambda: m.forward_rows(inp["location"], rows, C, B, N, h, w), select_rows=lambda: m.select_rows(inp["location"], rows, C, B, N, h, w))
        got = legs["select_rows"]()
        same = bool(torch.equal(got["topk_indexes"], full["topk_indexes"]) and torch.equal(got["sample_weight"], full["sample_weight"]))
        runs = {name: [] for name in legs}
        for _ in range(3):                                                 # alternating: both forms see the same drift of the card
            for name, fn in legs.items():
                runs[name].append(timed(fn, a.warmup, a.steps)["median_ms"])
        r = dict(same_bits=same)
        for name, ms in runs.items():
            r[name] = dict(rounds_ms=ms, median_ms=median(ms), spread_ms=round(max(ms) - min(ms), 4))
        f, s = r["forward_rows"], r["select_rows"]
        r["select_minus_forward_ms"] = round(s["median_ms"] - f["median_ms"], 4)
        r["select_not_slower"] = bool(s["median_ms"] <= f["median_ms"] + f["spread_ms"])
        r["select_faster_beyond_spread"] = bool(s["median_ms"] + max(f["spread_ms"], s["spread_ms"]) < f["median_ms"])
        me = module(precision, 0.5, "eager")
        me(inp["location"], img_feats=inp["img_feats"])
        me.select(inp["location"], img_feats=inp["img_feats"])
        W = me._ws[key]
        for form, launches in (("forward_rows", me._launches(key, W, W["rows"], K)), ("select_rows", me._select_launches(key, W, W["rows"], K))):
            per = {name: timed(launch, a.warmup, a.steps) for name, launch in launches}
            r[form + "_launches"] = per
            r[form + "_launch_sum_ms"] = round(sum(v["median_ms"] for v in per.values()), 4)
        res[precision] = r
        print(f"[{precision}] forward_rows {f['median_ms']} ms (spread {f['spread_ms']}), select_rows {s['median_ms']} ms (spread {s['spread_ms']})", file=sys.stderr, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--frames", type=int, default=0, help="run this many forwards of --precision and exit (for a profiler)")
    ap.add_argument("--precision", default="fp32x3")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch-eager control")
    ap.add_argument("--select", action="store_true", help="time select_rows against forward_rows instead (default --out: profiles/focal_select_time.json)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "focal_select_time.json" if a.select else "focal_head_time.json")
    sizes, shape = synth.FOCAL_HEAD_FULL, synth.FOCAL_HEAD_FULL_SHAPE
    B, N, h, w, C = shape["B"], shape["N"], shape["h"], shape["w"], sizes["in_channels"]
    sd = synth.focal_head_state_dict(sizes)
    inp = {k: v.to(DEV) for k, v in synth.focal_head_inputs(sizes, shape).items()}

    def module(precision, ratio, launch_mode="plan"):
        m = toc3d_amd.FocalHead(**dict(sizes, infer_ratio=ratio), precision=precision, launch_mode=launch_mode)
        m.load_state_dict(sd)
        return m.to(DEV)

    if a.frames:
        m = module(a.precision, sizes["infer_ratio"])
        for _ in range(a.frames):
            m(inp["location"], img_feats=inp["img_feats"])
        torch.cuda.synchronize()
        return
    if a.select:
        res = run_select(a, module, inp, sizes, shape)
        line = json.dumps(res)
        print(line)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
        return
    res = dict(tool="focal_head_time", device=torch.cuda.get_device_name(0), sizes=sizes, shape=shape, warmup=a.warmup, steps=a.steps)
    for precision in ("fp32x3", "bf16"):
        for ratio in (1.0, 0.5):
            tag = f"hip_{precision}_ratio{ratio}"
            m = module(precision, ratio)
            res[tag] = timed(lambda: m(inp["location"], img_feats=inp["img_feats"]), a.warmup, a.steps)
            me = module(precision, ratio, "eager")
            res[tag + "_eager_launches"] = timed(lambda: me(inp["location"], img_feats=inp["img_feats"]), a.warmup, a.steps)
            rows = m._ws[(B, N, h, w)]["rows"].clone()
            res[tag + "_forward_rows"] = timed(lambda: m.forward_rows(inp["location"], rows, C, B, N, h, w), a.warmup, a.steps)
            if ratio == 1.0:                             # the launches do not depend on the ratio: the ranking is always the full one
                key = (B, N, h, w)
                for name, launch in me._launches(key, me._ws[key], me._ws[key]["rows"], N * h * w):
                    res[f"hip_{precision}_launch_{name}"] = timed(launch, a.warmup, a.steps)
                res[f"hip_{precision}_launch_sum_ms"] = round(sum(res[f"hip_{precision}_launch_{n}"]["median_ms"] for n in ("conv3x3", "gn_stats", "heads", "rank_desc")), 4)
    if not a.no_torch:
        dsd = {k: v.to(DEV) for k, v in sd.items()}
        with torch.no_grad():
            for tag, contract in (("f32", None), ("bf16", torch.bfloat16)):
                for ratio in (1.0, 0.5):
                    res[f"torch_eager_{tag}_ratio{ratio}"] = timed(lambda: FC.restated_forward(dsd, inp, ratio, contract=contract), min(a.warmup, 10), a.steps)
        res["hip_faster_than_torch_eager"] = {f"{p}_ratio{r}": res[f"hip_{p}_ratio{r}"]["median_ms"] < res[f"torch_eager_{t}_ratio{r}"]["median_ms"]
                                              for p, t in (("fp32x3", "f32"), ("bf16", "bf16")) for r in (1.0, 0.5)}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
