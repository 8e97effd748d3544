"""Time of the token selection overlays (toc3d_amd.TokenVis) at 6 x 320 x 800 with three stages, in its three parts:
* ``render``: the L + 1 = 4 launches that make ori (6, 320, 800, 3) and six RGBA planes (6, 320, 800, 4) on the device -- warm-up 50, then the median of 200
  event-timed calls, as the other timing tools do;
* the device-to-host copy of the finished bytes (wall clock, synchronised, the median of --host-reps);
* the PNG writing of the 54 files (wall clock, the median of --host-reps; into a temporary directory);
and, in the same run, the host route the reference takes to the same arrays: ``.cpu().numpy()`` of the same device tensors (images, masks, index lists), then the
numpy restatement of tests/token_vis_cases.py up to the uint8 arrays (wall clock, the median of --host-reps; one thread).  The rendered bytes are compared with the
restatement first: a time is reported only for the right bytes.  No bar is set.  One JSON line on stdout, also written to --out (default
profiles/token_vis_time.json).

  python tools/token_vis_time.py
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
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "token_vis_time.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "token_vis_time needs the GPU: the pixels have no CPU path to time"
    c = TC.BIG
    inp = TC.inputs(c, TC.case_seed("big"))
    dv = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    img, masks, keeps, drops = dv(inp["img"]), [dv(m) for m in inp["masks"]], [dv(k) for k in inp["keeps"]], [dv(k) for k in inp["drops"]]
    vis = toc3d_amd.TokenVis(c["patch"])
    render = lambda: vis.render(img, masks, keeps, drops, c["norm"])
    r = render()
    want = TC.planes(TC.restated(inp["img"], inp["masks"], inp["keeps"], inp["drops"], c["norm"], c["patch"]), c["V"], 3, True)
    diff = sum(int((r[k].cpu().numpy() != w).sum()) for k, w in zip(("ori", "masks", "keepidx"), want))
    assert diff == 0, f"{diff} bytes differ from the restatement"
    out_bytes = sum(r[k].numel() for k in ("ori", "masks", "keepidx"))
    res = dict(tool="token_vis_time", device=torch.cuda.get_device_name(0), images=list(inp["img"].shape), stages=3, planes=6, launches_per_call=4,
               warmup=a.warmup, steps=a.steps, host_reps=a.host_reps, differing_bytes=diff, output_bytes=out_bytes)
    res["render"] = dict(timed(render, a.warmup, a.steps))
    res["render"]["written_GB_per_s"] = round(out_bytes / (res["render"]["median_ms"] * 1e-3) / 1e9, 1)
    res["device_to_host_copy"] = wall(lambda: [r[k].cpu() for k in ("ori", "masks", "keepidx")], a.host_reps)
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
        i = img.cpu().numpy()
        m, k, d = [t.cpu().numpy() for t in masks], [t.cpu().numpy() for t in keeps], [t.cpu().numpy() for t in drops]
        return [TC.to_bytes(arr) for _, arr in TC.restated(i, m, k, d, c["norm"], c["patch"])]
    res["host_route_to_uint8_arrays"] = wall(host_route, a.host_reps)
    res["host_route_over_render"] = round(res["host_route_to_uint8_arrays"]["median_ms"] / res["render"]["median_ms"], 1)
    res["not_measured"] = "no counter run (memory traffic, occupancy) and no kernel trace: the render time is the events' around the four launches"
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
