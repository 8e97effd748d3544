"""Time of the nuScenes submission records (toc3d_amd.NuScenesResults) at B = 1, 2 and 4 samples of 300 boxes each, about half of them beyond their class range:
* ``format_fixed``: the one launch and its call (poses already on the device) -- warm-up 50, then the median of 200 event-timed calls, as the other timing tools do;
* ``format``: packing the lists, the launch, the copy of the records to the host and the dict building (wall clock, synchronised, the median of --host-reps);
and, in the same run, the per-box float64 restatement of tests/nusc_results_cases.py on one host thread, from ``.cpu().numpy()`` of the same device tensors to the
same dicts -- LABELLED A STAND-IN: the reference's loop builds a pyquaternion object and a NuScenesBox per detection, and neither package is installed where this
runs, so NO FIGURE FOR THE REFERENCE'S LOOP IS GIVEN and no ratio to it may be quoted until someone runs it where those packages exist.  The kept sets and
attributes are compared with the restatement's first: a time is reported only for the right records.  No bar is set.  One JSON line on stdout, also written to
--out (default profiles/nusc_results_time.json).

  python tools/nusc_results_time.py
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nusc_results_cases as NC          # noqa: E402
import toc3d_amd                         # noqa: E402
from tools.decoder_time import timed     # noqa: E402

DEV = "cuda:0"
N = 300


def wall(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return dict(median_ms=round(ts[len(ts) // 2], 3), min_ms=round(ts[0], 3))


def case(B, seed=7):
    rng = np.random.default_rng(seed + B)
    poses = NC.random_poses(rng, B)
    parts = [NC.random_sample(rng, N, N, "random", poses[b, 0]) for b in range(B)]
    return dict(boxes=np.stack([p[0] for p in parts]), scores=np.stack([p[1] for p in parts]), labels=np.stack([p[2] for p in parts]),
                counts=np.full(B, N, dtype=np.int64), poses=poses)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--host-reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nusc_results_time.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "nusc_results_time needs the GPU: the records have no CPU path to time"
    dv = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    res = dict(tool="nusc_results_time", device=torch.cuda.get_device_name(0), boxes_per_sample=N, warmup=a.warmup, steps=a.steps, host_reps=a.host_reps, sizes={})
    fmt = toc3d_amd.NuScenesResults()
    for B in (1, 2, 4):
        c = case(B)
        boxes, scores, labels, counts, poses = dv(c["boxes"]), dv(c["scores"]), dv(c["labels"]), dv(c["counts"]), dv(c["poses"])
        records = NC.pose_records(c["poses"])
        lists = [[boxes[b], scores[b], labels[b]] for b in range(B)]
        want = NC.restate(c["boxes"], c["scores"], c["labels"], c["counts"], c["poses"])
        got = fmt.format_fixed(boxes, scores, labels, counts, poses)
        for k in ("kept", "src", "name", "attr"):
            assert np.array_equal(got[k].cpu().numpy(), want[k]), f"B = {B}: {k} differs from the restatement"
        assert np.abs(got["rec"].cpu().numpy() - want["rec"]).max() < 1e-9

        def host_route():
            b, s, l, n = (t.cpu().numpy() for t in (boxes, scores, labels, counts))
            r = NC.restate(b, s, l, n, c["poses"])
            return fmt.records_to_annos(r["rec"], r["score"], r["name"], r["attr"], r["kept"])
        res["sizes"][f"B{B}"] = dict(
            kept=want["kept"].tolist(),
            format_fixed=dict(timed(lambda: fmt.format_fixed(boxes, scores, labels, counts, poses), a.warmup, a.steps), launches=1,
                              note="device events around the call: the launch and its host side, poses on the device"),
            format=dict(wall(lambda: fmt.format(lists, records), a.host_reps), note="packing, pose upload, the launch, one copy of the records to the host, the dicts"),
            numpy_restatement_one_thread=dict(wall(host_route, max(3, a.host_reps // 4)),
                                              note="STAND-IN, not the reference's loop: the tests' per-box float64 restatement on Python floats, host copy and dicts included"))
    res["not_measured"] = ("the reference's pyquaternion / NuScenesBox loop (packages not installed): no figure for it, no ratio to it; no counter run and no kernel "
                           "trace: format_fixed is the events' time around one call")
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
