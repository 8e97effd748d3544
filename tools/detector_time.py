"""Time of one frame of the assembled toc3d_amd.Petr3D at the shipped sizes (ViT-L ToC3D_faster at 6 x 320 x 800, CPFPN 1024 -> 256, StreamPETRHead with 644 + 256
queries, 1024 memory entries, six decoder layers; batch 1) in ``fp32x3`` and ``bf16``, next to the hand-written chain of INTEGRATION.md on separately built modules
with the same weights -- backbone, neck, head, ``get_bboxes``, the bank's proposals handed to the next frame's backbone -- in the same run on the same card.

A leg = one continuation frame (``prev_exists`` true, a populated bank) from the frame's tensors on the device to the decoded lists on the host (both forms end with
the three device-to-host copies of ``bbox3d2result``), bracketed by events and followed by a synchronisation.  Warm-up 50 legs, then the median of 200; repeated three
times, alternating chain and detector, so both see the same drift of the card.  There is no fixed bar: ``detector_not_slower`` says whether the detector's median of
medians lies within the chain's own spread (max - min of its three medians) of the chain's.  ``split_ms`` is the chain's frame stage by stage (events between the
stages, medians over the same number of legs).  The two forms differ by the neck-to-head hand-off alone (``toc3d_neck_rows_fanout`` against ``toc3d_nhwc_to_nchw`` +
a copy + ``toc3d_nchw_to_rows``) and return the same bits (tests/test_gpu_detector.py).  One JSON line on stdout, also written to --out.

  python tools/detector_time.py

``--streams 1 2 4``: instead, B camera streams per step through ``Petr3D.simple_test_streams`` (stream b = ``synth.detector_inputs(seed=b)``), same warm-up, median
and alternation scheme, written to profiles/detector_streams_time.json.  Per B: a steady step (every stream continues) and, for B >= 2, a mixed step (stream 0 is
forgotten with ``reset_streams([0])`` in front of every step, so it starts a scene while the others continue; the call is inside the bracket).  B = 1 goes through the
unchanged ``simple_test`` -- the baseline, checked against profiles/detector_time.json within that file's own spread -- and also gives the first-frame step (a scene
start every step) that the two-forward alternative to a mixed step would add to a steady one.  Peak device memory (``torch.cuda.max_memory_allocated``) per B.

``--sampling``: instead, the detector with token selection (``aux_2d_only=False``: FocalHead's selection-only frame, the head on the ``infer_ratio`` = 0.5 best
tokens, 3000 of 6000) against the full-token detector (``aux_2d_only=True``) with the same weights, in the same run: the continuation frame, same warm-up, median
and alternation scheme, written to profiles/detector_sampled_time.json.  ``sampled_faster``: the sampled frame's median lies below the full-token one's by more
than the larger of the two spreads; ``sampled_not_slower``: within the full-token form's own spread of it.  Reported either way.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import toc3d_amd                                  # noqa: E402
from toc3d_amd import synth                       # noqa: E402
from toc3d_amd.detector import bbox3d2result      # noqa: E402
from tools.decoder_time import timed              # noqa: E402

DEV = "cuda:0"
STAGES = ("backbone_queries", "backbone", "neck", "head", "get_bboxes")


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def tuned(sizes, precision, backbone, neck):
    path = os.path.join(ROOT, "toc3d_amd", "tuned", f"{sizes['backbone']}_{sizes['hw'][0]}x{sizes['hw'][1]}_{precision}.json")
    if os.path.exists(path):
        backbone.load_tuning(path)
        neck._tuned.update(backbone._tuned)               # one (epilogue, M, N, K) -> variant table serves backbone and neck (as bench.py)
    return os.path.exists(path)


class Chain:
    """The loop INTEGRATION.md asked the user to write, before the detector existed."""

    def __init__(self, sizes, sd, precision):
        cfg = synth.detector_cfg(sizes)
        pick = lambda pre: {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}
        self.backbone = toc3d_amd.build_backbone(dict(cfg["img_backbone"], precision=precision))
        self.neck = toc3d_amd.build_neck(dict(cfg["img_neck"], precision=precision))
        self.head = toc3d_amd.build_head(cfg["pts_bbox_head"], precision=precision)
        for m, pre in ((self.backbone, "img_backbone."), (self.neck, "img_neck."), (self.head, "pts_bbox_head.")):
            m.load_state_dict(pick(pre), strict=True)
            m.to(DEV).eval()
        self.tuned = tuned(sizes, precision, self.backbone, self.neck)
        self.scene = None

    def frame(self, metas, data, events=None):
        mark = (lambda: None) if events is None else (lambda: events.pop(0).record())
        mark()
        prev = metas[0]["scene_token"] == self.scene
        self.scene = metas[0]["scene_token"]
        q = self.head.backbone_queries(self.backbone.pruning_num_queries, prev, 1)
        mark()
        out = self.backbone(data["img"][0], ego_pose_inv=data["ego_pose_inv"], **q)
        mark()
        feats = self.neck(list(out.img_feats.values()))[0]
        mark()
        if not prev:
            self.head.reset_memory()
        d = dict(data, img_feats=feats.view(1, *feats.shape), prev_exists=data["img"].new_ones(1) if prev else data["img"].new_zeros(1))
        outs = self.head(None, metas, None, **d)
        mark()
        res = [bbox3d2result(*b) for b in self.head.get_bboxes(outs, metas)]
        mark()
        return res


def run(precision, warmup, steps, repeats=3):
    sizes = synth.DETECTOR_FULL
    sd = synth.detector_state_dict(sizes)
    frames = synth.detector_inputs(sizes)
    metas = frames[0]["img_metas"]
    data = [{k: v.to(DEV) for k, v in f["data"].items()} for f in frames]
    det = toc3d_amd.build_detector(synth.detector_cfg(sizes), precision=precision)
    det.load_state_dict(sd, strict=True)
    det.to(DEV)
    has_table = tuned(sizes, precision, det.img_backbone, det.img_neck)
    chain = Chain(sizes, sd, precision)
    # scene start, then the continuation frame that is timed; the two forms agree on it before anything is timed
    a = [det.simple_test(metas, **data[f])[0]["pts_bbox"] for f in (0, 1)][1]
    b = [chain.frame(metas, data[f]) for f in (0, 1)][1][0]
    same = all(torch.equal(a[k], b[k]) for k in ("boxes_3d", "scores_3d", "labels_3d"))
    legs = dict(chain=lambda: chain.frame(metas, data[1]), detector=lambda: det.simple_test(metas, **data[1]))
    runs = dict(chain=[], detector=[])
    for _ in range(repeats):                                           # alternating: both forms see the same drift of the card
        for name in ("chain", "detector"):
            runs[name].append(timed(legs[name], warmup, steps)["median_ms"])
    spread = max(runs["chain"]) - min(runs["chain"])
    mc, md = median(runs["chain"]), median(runs["detector"])
    # the chain's frame, stage by stage
    per = []
    for i in range(warmup + steps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(STAGES) + 1)]
        chain.frame(metas, data[1], list(ev))
        ev[-1].synchronize()
        if i >= warmup:
            per.append([ev[j].elapsed_time(ev[j + 1]) for j in range(len(STAGES))])
    split = {s: round(median([p[j] for p in per]), 4) for j, s in enumerate(STAGES)}
    return dict(chain_ms=runs["chain"], detector_ms=runs["detector"], chain_median_ms=mc, detector_median_ms=md, chain_spread_ms=round(spread, 4),
                detector_minus_chain_ms=round(md - mc, 4), detector_not_slower=bool(md <= mc + spread), same_decoded_lists=bool(same), tuned_table=bool(has_table and chain.tuned),
                split_ms=split, split_sum_ms=round(sum(split.values()), 4))


def run_streams(precision, counts, warmup, steps, repeats=3):
    sizes = synth.DETECTOR_FULL
    sd = synth.detector_state_dict(sizes)
    res = {}
    for B in counts:
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        det = toc3d_amd.build_detector(synth.detector_cfg(sizes), precision=precision)
        det.load_state_dict(sd, strict=True)
        det.to(DEV)
        has_table = tuned(sizes, precision, det.img_backbone, det.img_neck)
        per = [synth.detector_inputs(sizes, seed=b) for b in range(B)]
        frames = [synth.stack_detector_frames([p[f] for p in per]) for f in range(2)]
        metas = frames[0]["img_metas"]
        data = [{k: v.to(DEV) for k, v in f["data"].items()} for f in frames]
        if B == 1:                                                         # the unchanged simple_test: the baseline, and the scene start of the two-forward alternative
            def first():
                det.prev_scene_token = None
                return det.simple_test(metas, **data[1])
            legs = dict(steady=lambda: det.simple_test(metas, **data[1]), first=first)
            det.simple_test(metas, **data[0])
        else:
            def mixed():
                det.reset_streams([0])
                return det.simple_test_streams(metas, **data[1])
            legs = dict(steady=lambda: det.simple_test_streams(metas, **data[1]), mixed=mixed)
            det.simple_test_streams(metas, **data[0])
        runs = {name: [] for name in legs}
        for _ in range(repeats):                                           # alternating: every leg sees the same drift of the card
            for name, fn in legs.items():
                runs[name].append(timed(fn, warmup, steps)["median_ms"])
        r = dict(tuned_table=bool(has_table), peak_memory_mib=round(torch.cuda.max_memory_allocated() / 2 ** 20, 1))
        for name, ms in runs.items():
            r[name + "_ms"] = ms
            r[name + "_median_ms"] = median(ms)
            r[name + "_spread_ms"] = round(max(ms) - min(ms), 4)
        r["steady_frames_per_s"] = round(1000.0 * B / r["steady_median_ms"], 2)
        res[str(B)] = r
        print(f"[{precision}] B = {B}: " + ", ".join(f"{name} {r[name + '_median_ms']} ms" for name in legs), file=sys.stderr, flush=True)
        del det, legs
    one = res.get("1")
    for B, r in res.items():
        if one is None or B == "1":
            continue
        r["steady_frames_per_s_over_b1"] = round(r["steady_frames_per_s"] / one["steady_frames_per_s"], 4)
        r["mixed_over_steady"] = round(r["mixed_median_ms"] / r["steady_median_ms"], 4)
        r["two_forwards_ms"] = round(r["steady_median_ms"] + one["first_median_ms"], 4)          # the alternative: the steady step + one B = 1 first-frame step
        r["mixed_over_two_forwards"] = round(r["mixed_median_ms"] / r["two_forwards_ms"], 4)
        r["mixed_beats_two_forwards"] = bool(r["mixed_median_ms"] < r["two_forwards_ms"])
    return res


def run_sampling(precision, warmup, steps, repeats=3):
    sizes = dict(synth.DETECTOR_FULL, roi=dict(infer_ratio=0.5))
    sd = synth.detector_state_dict(sizes)
    frames = synth.detector_inputs(sizes)
    metas = frames[0]["img_metas"]
    data = [{k: v.to(DEV) for k, v in f["data"].items()} for f in frames]
    dets, has_table = {}, True
    for name, aux in (("full_tokens", True), ("sampled", False)):
        det = toc3d_amd.build_detector(dict(synth.detector_cfg(sizes), aux_2d_only=aux), precision=precision)
        det.load_state_dict(sd, strict=True)
        det.to(DEV)
        has_table = tuned(sizes, precision, det.img_backbone, det.img_neck) and has_table
        for f in (0, 1):                                                   # scene start, then the continuation frame that is timed
            det.simple_test(metas, **data[f])
        dets[name] = det
    legs = {name: (lambda det=det: det.simple_test(metas, **data[1])) for name, det in dets.items()}
    runs = {name: [] for name in legs}
    for _ in range(repeats):                                               # alternating: both forms see the same drift of the card
        for name, fn in legs.items():
            runs[name].append(timed(fn, warmup, steps)["median_ms"])
    r = dict(tuned_table=bool(has_table), tokens=6000, kept_tokens=int(6000 * 0.5))
    for name, ms in runs.items():
        r[name] = dict(rounds_ms=ms, median_ms=median(ms), spread_ms=round(max(ms) - min(ms), 4))
    f, s = r["full_tokens"], r["sampled"]
    r["sampled_minus_full_ms"] = round(s["median_ms"] - f["median_ms"], 4)
    r["sampled_faster"] = bool(s["median_ms"] + max(f["spread_ms"], s["spread_ms"]) < f["median_ms"])
    r["sampled_not_slower"] = bool(s["median_ms"] <= f["median_ms"] + f["spread_ms"])
    print(f"[{precision}] full tokens {f['median_ms']} ms (spread {f['spread_ms']}), sampled {s['median_ms']} ms (spread {s['spread_ms']})", file=sys.stderr, flush=True)
    return r


def main_sampling(a):
    res = dict(tool="detector_time --sampling", device=torch.cuda.get_device_name(0), sizes=dict(backbone="toc3d_faster", image=[6, 320, 800], neck="CPFPN 1024 -> 256",
                                                                                                   head={k: v for k, v in synth.HEAD_FULL.items() if k != "decoder"},
                                                                                                   roi=dict(synth.FOCAL_HEAD_FULL)),
               warmup=a.warmup, steps=a.steps, repeats=3)
    for precision in a.precisions.split(","):
        res[precision] = run_sampling(precision, a.warmup, a.steps)
    line = json.dumps(res)
    print(line)
    out = a.out or os.path.join(ROOT, "profiles", "detector_sampled_time.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write(line + "\n")


def main_streams(a):
    res = dict(tool="detector_time --streams", device=torch.cuda.get_device_name(0), sizes=dict(backbone="toc3d_faster", image=[6, 320, 800], neck="CPFPN 1024 -> 256",
                                                                                                  head={k: v for k, v in synth.HEAD_FULL.items() if k != "decoder"}),
               streams=a.streams, warmup=a.warmup, steps=a.steps, repeats=3)
    base_path = os.path.join(ROOT, "profiles", "detector_time.json")
    base = json.load(open(base_path)) if os.path.exists(base_path) else {}
    for precision in a.precisions.split(","):
        r = run_streams(precision, a.streams, a.warmup, a.steps)
        if "1" in r and precision in base:                                  # B = 1 is the parent's code: within the earlier file's own spread of its figure?
            b = base[precision]
            spread = max(b["detector_ms"]) - min(b["detector_ms"])
            r["1"]["baseline_file_ms"], r["1"]["baseline_file_spread_ms"] = b["detector_median_ms"], round(spread, 4)
            r["1"]["within_baseline_file_spread"] = bool(abs(r["1"]["steady_median_ms"] - b["detector_median_ms"]) <= spread)
        res[precision] = r
    line = json.dumps(res)
    print(line)
    out = a.out or os.path.join(ROOT, "profiles", "detector_streams_time.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--precisions", default="fp32x3,bf16")
    ap.add_argument("--out", default=None, help="default: profiles/detector_time.json; profiles/detector_streams_time.json with --streams, profiles/detector_sampled_time.json with --sampling")
    ap.add_argument("--streams", type=int, nargs="+", default=None, help="camera streams per step to time through simple_test_streams, e.g. 1 2 4")
    ap.add_argument("--sampling", action="store_true", help="time aux_2d_only=False at infer_ratio 0.5 against aux_2d_only=True (profiles/detector_sampled_time.json)")
    a = ap.parse_args()
    if a.sampling:
        return main_sampling(a)
    if a.streams:
        return main_streams(a)
    a.out = a.out or os.path.join(ROOT, "profiles", "detector_time.json")
    res = dict(tool="detector_time", device=torch.cuda.get_device_name(0), sizes=dict(backbone="toc3d_faster", image=[6, 320, 800], neck="CPFPN 1024 -> 256",
                                                                                        head={k: v for k, v in synth.HEAD_FULL.items() if k != "decoder"}),
               warmup=a.warmup, steps=a.steps, repeats=3)
    for precision in a.precisions.split(","):
        res[precision] = run(precision, a.warmup, a.steps)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
