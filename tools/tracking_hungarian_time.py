"""Time of the tracking step with hungarian=True (toc3d_tracks_step_hungarian) beside the greedy step (toc3d_tracks_step) IN THE SAME RUN, warm, many repetitions,
with the spread (min, p10, median, p90), and the solver's scan rounds -- the unit the Hungarian kernel's time is read in: it is a dependent chain of rounds, each a
walk over the list, a pick across the workgroup and one barrier.  Recorded, not gated.
* ``entry``: one call of each entry point on the same steady state and frame -- the state the Hungarian restatement of tests/tracking_hungarian_cases.py leaves
  after five frames of a scene of tests/tracking_cases.py -- at K = 300, max_age = 3 for B = 1, 2, 4 streams over all classes, for the crowded one-label case, and
  for the case at the caps (512 rows on 2048 tracks, one label); device events around the call, so the call's host side is inside.  ms per round = the Hungarian
  median minus the greedy median of the same state (the filter and the state write, which the two share, and the launch), over the rounds.
* the detector's frame (the tiny synthetic detector, fp32x3) without tracking, with the greedy tracker and with the Hungarian one, alternating in the same run.
Every timed configuration is first checked against the restatements: a time is reported only for the right ids and the right rounds.
A development build of the kernel with another workgroup size (make EXTRA=-DTOC3D_ASSIGN_THREADS=64 BUILD=... LIB=..., selected with TOC3D_LIB) is timed by
running this tool under it with --out elsewhere; ``workgroup_threads`` names what was timed (--threads).  The reference with scipy was not timed on this host:
no ratio to it.  One JSON line on stdout, also written to --out (default profiles/tracking_hungarian_time.json).

  python tools/tracking_hungarian_time.py
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tracking_cases as TC              # noqa: E402
import tracking_hungarian_cases as HC    # noqa: E402
from tools.tracking_time import K, MAX_AGE, THR, spread, steady   # noqa: E402

DEV = "cuda:0"

def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--detector-frames", type=int, default=30)
    ap.add_argument("--threads", type=int, default=256, help="the workgroup size of the library timed (what TOC3D_ASSIGN_THREADS it was built with)")
    ap.add_argument("--no-detector", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracking_hungarian_time.json"))
    a = ap.parse_args()

    import torch

    import toc3d_amd
    from toc3d_amd import lib, synth, tracking
    assert torch.cuda.is_available(), "tracking_hungarian_time needs the GPU: the matching has no CPU path to time"
    dv = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return spread(ts)

    def both(states, lasts, fr, Kc, cap, max_age):
        """The two entry points on the same states and frame, each checked against its restatement -> the record of a configuration."""
        B = len(states)
        sin = dv(np.stack([TC.state_to_bytes(s, l, cap) for s, l in zip(states, lasts)]))
        sout = torch.zeros_like(sin)
        args = [dv(fr[k]) for k in ("rec", "score", "name", "kept")]
        label, gate, ts, first = dv(TC.track_label_table()), dv(TC.max_diff_table()), dv(fr["timestamp"]), dv(fr["first"])
        out = dict(track_id=torch.empty(B, Kc, dtype=torch.int32, device=DEV), active=torch.empty(B, Kc, dtype=torch.int32, device=DEV),
                   order=torch.empty(B, Kc, dtype=torch.int32, device=DEV), num_out=torch.empty(B, dtype=torch.int64, device=DEV), rounds=torch.empty(B, dtype=torch.int32, device=DEV))
        rec = dict(tracks_held_before=[len(s["label"]) for s in states])
        for name, entry, keys, cls in (("greedy", "toc3d_tracks_step", TC.OUT_KEYS, TC.Tracker), ("hungarian", "toc3d_tracks_step_hungarian", HC.OUT_KEYS, HC.Tracker)):
            fn = lambda: lib.call(entry, *args, B, Kc, label, 10, gate, 7, fr["thr"], max_age, ts, first, sin, sout, cap, *[out[k] for k in keys], lib.stream_ptr())
            fn()
            torch.cuda.synchronize()
            want = []
            for b in range(B):
                t = cls(max_age)
                t.set_state(states[b], lasts[b])
                want.append(t.step(fr["rec"][b], fr["score"][b], fr["name"][b], fr["kept"][b], fr["timestamp"][b], fr["first"][b], fr["thr"]))
            for k in keys:
                assert np.array_equal(out[k].cpu().numpy(), np.stack([w[k] for w in want])), f"{name}: {k} differs from the restatement"
            rec[name] = dict(timed(fn), launches=1)
            rec["detections_surviving"] = [int(w["num_out"]) for w in want]
            if name == "hungarian":
                rec["rounds"] = [int(w["rounds"]) for w in want]
        most = max(rec["rounds"])
        rec["rounds_per_row"] = [round(r / max(1, min(n, m)), 3) for r, n, m in zip(rec["rounds"], rec["detections_surviving"], rec["tracks_held_before"])]
        rec["us_per_round"] = round((rec["hungarian"]["median_ms"] - rec["greedy"]["median_ms"]) * 1e3 / most, 3) if most else None
        return rec

    res = dict(tool="tracking_hungarian_time", device=torch.cuda.get_device_name(0), library=os.path.basename(lib.LIB_PATH), workgroup_threads=a.threads, K=K, max_age=MAX_AGE,
               score_threshold=THR, warmup=a.warmup, steps=a.steps, sizes={},
               us_per_round_is="(the Hungarian entry's median - the greedy entry's median on the same state) / the rounds of the stream with the most: the streams of a launch run "
                               "side by side on their own CUs; what the two entries share (launch, filter, state write) cancels, greedy's own matching does not and is small")
    for tag, B, classes, spacing in [(f"B{B}_all_classes", B, TC.ALL_CLASSES, 2.0) for B in (1, 2, 4)] + [("B1_one_label_crowded", 1, (TC.CAR,), 1.0)]:
        _, trackers, fr = steady(B, classes, spacing, tracker=HC.Tracker)
        res["sizes"][tag] = both([t.state for t in trackers], [t.last for t in trackers], dict(fr, thr=THR), K, tracking.capacity_for(K, MAX_AGE), MAX_AGE)
    c = HC.build_case(HC.CAPS_CASE)
    res["sizes"]["caps_512_rows_2048_tracks_one_label"] = both(c["init"], c["init_last"], dict(c["frames"][0], thr=c["thr"]), c["K"], HC.MAX_TRACKS, c["max_age"])
    c = HC.build_case("n128_m128_one_label")
    st = HC.run_case(dict(c, frames=c["frames"][:1]))[1][0]
    res["sizes"]["crowded_128_on_128_one_label"] = both(st, [float(c["frames"][0]["timestamp"][0])], dict(c["frames"][1], thr=c["thr"]), c["K"], 512, c["max_age"])
    res["expectation_from_the_cpu_count"] = "1.2 to 1.6 rounds per row on scene-like input (374 to 481 rounds at 300 rows): compare rounds_per_row of the all-classes sizes"

    if not a.no_detector:
        import nusc_results_cases as NC
        sizes = synth.DETECTOR_TINY
        dets = {}
        for mode in ("off", "greedy", "hungarian"):
            det = toc3d_amd.build_detector(synth.detector_cfg(sizes), precision="fp32x3")
            det.load_state_dict(synth.detector_state_dict(sizes), strict=True)
            det = det.to(DEV).enable_nusc_results()
            det.img_backbone.autotune = det.img_neck.autotune = False
            dets[mode] = det if mode == "off" else det.enable_tracking(max_age=MAX_AGE, score_threshold=0.0, hungarian=mode == "hungarian")
        pose = NC.pose_records(NC.random_poses(np.random.default_rng(5), 1))[0]
        frames = [dict(img_metas=[dict(fr["img_metas"][0], sample_idx=f"s{f}", **pose)], gumbel=fr["gumbel"], dev={k: v.to(DEV) for k, v in fr["data"].items()})
                  for f, fr in enumerate(synth.detector_inputs(dict(sizes, new_scene_at=None))[:2])]
        times = {mode: [] for mode in dets}
        for i in range(a.detector_frames + 10):
            for mode in dets:
                fr = frames[i % 2]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                dets[mode].simple_test(fr["img_metas"], gumbel_noise=fr["gumbel"], **fr["dev"])
                torch.cuda.synchronize()
                if i >= 10:
                    times[mode].append((time.perf_counter() - t0) * 1e3)
        sp = {mode: spread(ts, 3) for mode, ts in times.items()}
        band = round(sp["off"]["p90_ms"] - sp["off"]["p10_ms"], 3)
        res["detector_frame"] = dict(sizes="DETECTOR_TINY, fp32x3, records on in all three", **{f"tracking_{m}": s for m, s in sp.items()}, p10_p90_band_of_off_ms=band,
                                     median_difference_greedy_ms=round(sp["greedy"]["median_ms"] - sp["off"]["median_ms"], 3),
                                     median_difference_hungarian_ms=round(sp["hungarian"]["median_ms"] - sp["off"]["median_ms"], 3),
                                     records_tracked_last_frame=len(dets["hungarian"].tracking_results.get("s1", [])),
                                     note="wall clock, synchronised, alternating off / greedy / hungarian frame by frame; a difference inside the band of the frames without tracking "
                                          "is not resolved by this run")
    res["not_measured"] = "the reference's tracker with scipy on this host: no ratio to it; no counter run and no kernel trace"
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
