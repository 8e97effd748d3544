"""Time of the box overlays (toc3d_amd.BoxVis) at six 320 x 800 views with 300 boxes at the shipped pc_range, thickness 2, in its parts:
* ``render`` with and without the top-down panel: the four / two launches that make views (6, 320, 800, 3) and bev (640, 640, 3) on the device -- warm-up 50,
  then the median of 200 event-timed calls, as the other timing tools do;
* the device-to-host copy of the finished bytes (wall clock, synchronised, the median of --host-reps);
* the PNG writing of the seven files (wall clock, the median of --host-reps; into a temporary directory);
and, in the same run, the numpy restatement of tests/box_vis_cases.py to the same arrays on one host thread: ``.cpu().numpy()`` of the same device tensors, the
float64 geometry (Python loops over views, boxes and edges), the denormalised base and the integer render (wall clock, the median of --host-reps).  The rendered
bytes are compared with the restatement's render of the device's own tables first: a time is reported only for the right bytes.  No bar is set.  One JSON line on
stdout, also written to --out (default profiles/box_vis_time.json).

  python tools/box_vis_time.py
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import box_vis_cases as BC               # noqa: E402
import token_vis_cases as TC             # noqa: E402
import toc3d_amd                         # noqa: E402
from tools.decoder_time import timed     # noqa: E402

DEV = "cuda:0"


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "box_vis_time.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "box_vis_time needs the GPU: the pixels have no CPU path to time"
    c, norm = BC.big_case(), TC.SHIPPED_NORM
    dv = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    img, boxes, scores, labels, proj = dv(c["img"]), dv(c["boxes"]), dv(c["scores"]), dv(c["labels"]), dv(c["proj"])
    vis = toc3d_amd.BoxVis(thickness=2)
    with_bev = lambda: vis.render(img, boxes, scores, labels, proj, norm, bev=True)
    without = lambda: vis.render(img, boxes, scores, labels, proj, norm, bev=False)
    r = with_bev()
    base = BC.base_f32(c["img"], norm)
    want = BC.render_restated(base, r["segi"].cpu().numpy().reshape(6, -1, 4), r["cidx"].cpu().numpy().reshape(6, -1), BC.PALETTE, 2)
    white = np.full((1, 640, 640, 3), 255, dtype=np.uint8)
    want_bev = BC.render_restated(white, r["bev_segi"].cpu().numpy().reshape(1, -1, 4), r["bev_cidx"].cpu().numpy().reshape(1, -1), BC.PALETTE, 2)
    diff = int((r["views"].cpu().numpy() != want).sum()) + int((r["bev"].cpu().numpy() != want_bev[0]).sum())
    assert diff == 0, f"{diff} bytes differ from the restatement"
    out_bytes = r["views"].numel() + r["bev"].numel()
    res = dict(tool="box_vis_time", device=torch.cuda.get_device_name(0), images=list(c["img"].shape), boxes=int(boxes.shape[0]), thickness=2,
               camera_segments_drawn=int((r["cidx"] != 255).sum().item()), bev_segments_drawn=int((r["bev_cidx"] != 255).sum().item()),
               pixels_coloured=int(BC.coloured(want, base).sum()), warmup=a.warmup, steps=a.steps, host_reps=a.host_reps, differing_bytes=diff, output_bytes=out_bytes)
    res["render_with_bev"] = dict(timed(with_bev, a.warmup, a.steps), launches=4)
    res["render_without_bev"] = dict(timed(without, a.warmup, a.steps), launches=2)
    r = with_bev()
    res["device_to_host_copy"] = wall(lambda: [r[k].cpu() for k in ("views", "bev")], a.host_reps)
    with tempfile.TemporaryDirectory() as tmp:
        n = [0]

        def write():
            n[0] += 1
            return vis.write(r, os.path.join(tmp, str(n[0])))
        w = wall(write, a.host_reps)
        files = write()
        res["png_writing"] = dict(w, files=len(files), file_bytes=sum(os.path.getsize(f) for f in files),
                                  note="includes the device-to-host copy above: write() is one copy, then the encoder")

    def host_route():
        i, b, s, l, p = (t.cpu().numpy() for t in (img, boxes, scores, labels, proj))
        cam = BC.camera_segments64(b, s, l, p, c["H"], c["W"])
        bev = BC.bev_segments64(b, s, l, 640)
        views = BC.render_restated(BC.base_f32(i, norm), np.rint(cam["segf"]).reshape(6, -1, 4), cam["cidx"].reshape(6, -1), BC.PALETTE, 2)
        return views, BC.render_restated(white, np.rint(bev["segf"]).reshape(1, -1, 4), bev["cidx"].reshape(1, -1), BC.PALETTE, 2)
    res["numpy_restatement_one_thread"] = dict(wall(host_route, a.host_reps), note="float64 geometry in Python loops, integer coverage per segment window in numpy")
    res["restatement_over_render"] = round(res["numpy_restatement_one_thread"]["median_ms"] / res["render_with_bev"]["median_ms"], 1)
    res["not_measured"] = "no counter run (memory traffic, occupancy, LDS) and no kernel trace: the render times are the events' around the launches of a call"
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
