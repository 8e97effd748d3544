"""Time of the tracking step (toc3d_amd.PubTracker, toc3d_tracks_step), warm, many repetitions, with the spread (min, p10, median, p90):
* ``entry``: one call of the entry point on a steady state -- the state a scene of tests/tracking_cases.py leaves after five frames, read again by every
  repetition (a step reads one state and writes the other, so every repetition does the same work) -- at K = 300, max_age = 3, for B = 1, 2, 4 streams of
  real-looking tracks over all classes, for the one-label worst case (every detection and track a car, one metre apart: one greedy chain), and at K = 2048 on the
  full state of 8192 tracks, one label and spread over the labels; device events around the call, so the call's host side is inside;
* ``step_fixed``: the class's call on the same frames (its uploads of timestamps and flags and its output allocations included);
* the detector's frame (the tiny synthetic detector, fp32x3) with tracking on against off, alternating in the same run, wall clock and synchronised; the difference
  of the medians is named as inside or outside that run's own spread (the p10 .. p90 band of the frames without tracking);
* the tests' numpy restatement on this host, one thread -- LABELLED A STAND-IN, not the reference's loop.
Every timed configuration is first checked against the restatement: a time is reported only for the right ids.  No bar is set.

The reference's own tracker exists only where the reference tree does, which is another host: ``--reference DIR`` (no GPU needed) times its step_centertrack on the
same K = 300 steady-state frame there and merges the figure into --out under ``reference_on_its_own_host`` with the host named.  NO RATIO ACROSS THE TWO HOSTS MAY
BE QUOTED.  One JSON line on stdout, also written to --out (default profiles/tracking_time.json).

  python tools/tracking_time.py
"""
import argparse
import contextlib
import io
import json
import os
import platform
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tracking_cases as TC              # noqa: E402

DEV = "cuda:0"
K, MAX_AGE, THR, WARM_FRAMES = 300, 3, 0.25, 5


def spread(ts, digits=4):
    ts = sorted(ts)
    q = lambda p: round(ts[min(len(ts) - 1, int(len(ts) * p))], digits)
    return dict(median_ms=q(0.5), min_ms=round(ts[0], digits), p10_ms=q(0.1), p90_ms=q(0.9), reps=len(ts))


def steady(B, classes=TC.ALL_CLASSES, spacing=2.0, seed=31, tracker=TC.Tracker):
    """-> (case, the trackers of the restatement ``tracker`` after WARM_FRAMES frames, the next frame)."""
    c = TC.scene_case(seed, K, WARM_FRAMES + 1, 330, MAX_AGE, thr=THR, classes=classes, spacing=spacing, B=B)
    trackers = [tracker(MAX_AGE) for _ in range(B)]
    for fr in c["frames"][:WARM_FRAMES]:
        for b, t in enumerate(trackers):
            t.step(fr["rec"][b], fr["score"][b], fr["name"][b], fr["kept"][b], fr["timestamp"][b], fr["first"][b], THR)
    return c, trackers, c["frames"][WARM_FRAMES]


def time_reference(ref_dir, out_path):
    sys.path.insert(0, os.path.join(ref_dir, "nusc_tracking"))
    import pub_tracker
    c, trackers, fr = steady(1)
    dets = lambda f: [dict(translation=f["rec"][0, i, 0:3].tolist(), velocity=f["rec"][0, i, 10:12].tolist(), detection_name=TC.CLASS_NAMES[int(f["name"][0, i])],
                           detection_score=float(f["score"][0, i])) for i in range(int(f["kept"][0]))]
    ts = []
    for _ in range(30):
        with contextlib.redirect_stdout(io.StringIO()):
            trk = pub_tracker.PubTracker(max_age=MAX_AGE)
        for f in c["frames"][:WARM_FRAMES]:
            trk.step_centertrack(dets(f), 0.5, THR)
        d = dets(fr)
        t0 = time.perf_counter()
        trk.step_centertrack(d, 0.5, THR)
        ts.append((time.perf_counter() - t0) * 1e3)
    cpu = next((l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name")), platform.processor()) if os.path.exists("/proc/cpuinfo") else platform.processor()
    res = json.load(open(out_path)) if os.path.exists(out_path) else dict(tool="tracking_time")
    res["reference_on_its_own_host"] = dict(spread(ts, 3), host=f"{cpu} ({platform.machine()}), one Python thread", tracks_held=len(trk.tracks),
                                            note="the reference's PubTracker.step_centertrack on the K = 300 steady-state frame, dicts already built; ANOTHER HOST than the "
                                                 "one the other figures of this file were taken on: no ratio across the two may be quoted")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--host-reps", type=int, default=20)
    ap.add_argument("--detector-frames", type=int, default=40)
    ap.add_argument("--reference", default=None, help="the reference tree: time its tracker on this host (no GPU) and merge the figure into --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracking_time.json"))
    a = ap.parse_args()
    if a.reference:
        res = time_reference(a.reference, a.out)
    else:
        res = time_device(a)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


def time_device(a):
    import torch

    import toc3d_amd
    from toc3d_amd import lib, synth, tracking
    assert torch.cuda.is_available(), "tracking_time needs the GPU: the matching has no CPU path to time"
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

    def entry(trackers, fr, Kc, cap):
        """The entry point on the trackers' state and the frame ``fr`` -> (the timed closure, outputs)."""
        B = len(trackers)
        sin = dv(np.stack([TC.state_to_bytes(t.state, t.last, cap) for t in trackers]))
        sout = torch.zeros_like(sin)
        args = [dv(fr[k]) for k in ("rec", "score", "name", "kept")]
        label, gate, ts, first = dv(TC.track_label_table()), dv(TC.max_diff_table()), dv(fr["timestamp"]), dv(fr["first"])
        out = dict(track_id=torch.empty(B, Kc, dtype=torch.int32, device=DEV), active=torch.empty(B, Kc, dtype=torch.int32, device=DEV),
                   order=torch.empty(B, Kc, dtype=torch.int32, device=DEV), num_out=torch.empty(B, dtype=torch.int64, device=DEV))
        fn = lambda: lib.call("toc3d_tracks_step", *args, B, Kc, label, 10, gate, 7, fr["thr"], MAX_AGE, ts, first, sin, sout, cap, out["track_id"], out["active"], out["order"],
                              out["num_out"], lib.stream_ptr())
        fn()
        torch.cuda.synchronize()
        want = [t.step(fr["rec"][b], fr["score"][b], fr["name"][b], fr["kept"][b], fr["timestamp"][b], fr["first"][b], fr["thr"]) for b, t in enumerate(trackers)]
        for k in TC.OUT_KEYS:
            assert np.array_equal(out[k].cpu().numpy(), np.stack([w[k] for w in want])), f"{k} differs from the restatement"
        return fn, want

    res = dict(tool="tracking_time", device=torch.cuda.get_device_name(0), K=K, max_age=MAX_AGE, score_threshold=THR, warmup=a.warmup, steps=a.steps, sizes={})
    configs = [(f"B{B}_all_classes", B, TC.ALL_CLASSES, 2.0) for B in (1, 2, 4)] + [("B1_one_label_worst_case", 1, (TC.CAR,), 1.0)]
    for tag, B, classes, spacing in configs:
        c, trackers, fr = steady(B, classes, spacing)
        fr = dict(fr, thr=THR)
        held = [len(t.state["label"]) for t in trackers]
        copies = [TC.Tracker(MAX_AGE) for _ in range(B)]
        for t, s in zip(copies, trackers):
            t.set_state(s.state, s.last)
        reps = max(3, a.host_reps // 4)
        host = []
        for _ in range(reps):
            for t, s in zip(copies, trackers):
                t.set_state(s.state, s.last)
            t0 = time.perf_counter()
            for b, t in enumerate(copies):
                t.step(fr["rec"][b], fr["score"][b], fr["name"][b], fr["kept"][b], fr["timestamp"][b], fr["first"][b], THR)
            host.append((time.perf_counter() - t0) * 1e3)
        fn, want = entry(trackers, fr, K, tracking.capacity_for(K, MAX_AGE))
        trk = toc3d_amd.PubTracker(max_age=MAX_AGE, num_streams=B)
        for f in c["frames"][:WARM_FRAMES + 1]:
            dev = [dv(f[k]) for k in ("rec", "score", "name", "kept")]
            got = trk.step_fixed(*dev, dv(f["timestamp"]), dv(f["first"]), THR)
        assert np.array_equal(got["track_id"].cpu().numpy(), np.stack([w["track_id"] for w in want]))
        res["sizes"][tag] = dict(tracks_held_before=held, detections_surviving=[int(w["num_out"]) for w in want],
                                 entry=dict(timed(fn), launches=1, note="device events around one call of the entry point on the steady state"),
                                 step_fixed=dict(timed(lambda: trk.step_fixed(*dev, dv(fr["timestamp"]), dv(fr["first"]), THR)), launches=1,
                                                 note="the class's call on the same frame again and again (every detection then matches its own track): uploads of "
                                                      "timestamps and flags and the output allocations included"),
                                 numpy_restatement_one_thread=dict(spread(host, 3), note="STAND-IN, not the reference's loop: the tests' restatement, one vector "
                                                                                         "operation per detection, arrays in, arrays out"))
    for name in ("large_one_label", "large_spread"):
        c = TC.build_case(name)
        t = TC.Tracker(MAX_AGE)
        t.set_state(c["init"][0], c["init_last"][0])
        fr = dict(c["frames"][0], thr=c["thr"])
        fn, want = entry([t], fr, 2048, 8192)
        res["sizes"][f"K2048_full_state_{name}"] = dict(tracks_held_before=[8192], detections_surviving=[int(want[0]["num_out"])],
                                                        entry=dict(timed(fn), launches=1, note="K = 2048 on a state of 8192 tracks"))
    res["kernel_variants"] = "one: a wavefront per tracking label (the single-chain form was not built; the one-label case above is what a single chain costs)"

    # the detector's frame with tracking on against off, alternating in the same run
    import nusc_results_cases as NC
    sizes = synth.DETECTOR_TINY
    dets = {}
    for mode in ("off", "on"):
        det = toc3d_amd.build_detector(synth.detector_cfg(sizes), precision="fp32x3")
        det.load_state_dict(synth.detector_state_dict(sizes), strict=True)
        det = det.to(DEV).enable_nusc_results()
        det.img_backbone.autotune = det.img_neck.autotune = False
        dets[mode] = det.enable_tracking(max_age=MAX_AGE, score_threshold=0.0) if mode == "on" else det
    pose = NC.pose_records(NC.random_poses(np.random.default_rng(5), 1))[0]
    frames = [dict(img_metas=[dict(fr["img_metas"][0], sample_idx=f"s{f}", **pose)], gumbel=fr["gumbel"], dev={k: v.to(DEV) for k, v in fr["data"].items()})
              for f, fr in enumerate(synth.detector_inputs(dict(sizes, new_scene_at=None))[:2])]
    times = dict(off=[], on=[])
    for i in range(a.detector_frames + 10):
        for mode in ("off", "on"):
            fr = frames[i % 2]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dets[mode].simple_test(fr["img_metas"], gumbel_noise=fr["gumbel"], **fr["dev"])
            torch.cuda.synchronize()
            if i >= 10:
                times[mode].append((time.perf_counter() - t0) * 1e3)
    off, on = spread(times["off"], 3), spread(times["on"], 3)
    diff = round(on["median_ms"] - off["median_ms"], 3)
    band = round(off["p90_ms"] - off["p10_ms"], 3)
    res["detector_frame"] = dict(sizes="DETECTOR_TINY, fp32x3, records on in both", tracking_off=off, tracking_on=on, median_difference_ms=diff, p10_p90_band_of_off_ms=band,
                                 difference_is=("inside" if abs(diff) <= band else "outside") + " the run's own spread (the p10 .. p90 band of the frames without tracking)",
                                 records_tracked_last_frame=len(dets["on"].tracking_results.get("s1", [])),
                                 note="wall clock, synchronised, alternating off / on frame by frame; tracking adds one launch, the upload of B flags and one copy of the outputs to the host")
    res["not_measured"] = ("the reference's tracker on this host (its tree is not here): see reference_on_its_own_host if present, taken on another host -- no ratio across hosts; "
                           "no counter run and no kernel trace")
    if os.path.exists(a.out):
        old = json.load(open(a.out))
        if "reference_on_its_own_host" in old:
            res["reference_on_its_own_host"] = old["reference_on_its_own_host"]
    return res


if __name__ == "__main__":
    main()
