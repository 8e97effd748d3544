"""Time of the camera ingest (toc3d_amd.ResizeCropFlipRotImage: one toc3d_resize_crop_u8 launch) on 6 x 900 x 1600 raw frames, to 320 x 800 and to 800 x 1600.
Warm-up 50, then the median of 200 event-timed calls, as the other timing tools do.  Beside each figure: the bytes the launch must move (the source rows its
vertical taps need, once, plus the destination), the time a device-to-device copy of the same run needs for that many bytes (the card's copy bandwidth, measured
here on a 64 MiB buffer with the same warm-up and steps), and -- where PIL imports -- host Pillow on the same host's CPU (one thread, the median of --host-reps
frames of six images).  The outputs are compared with the numpy restatement of tests/ingest_cases.py first: a time is reported only for the right bytes.  One
JSON line on stdout, also written to --out (default profiles/ingest_time.json).

  python tools/ingest_time.py
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
import ingest_cases as IC                # noqa: E402
import toc3d_amd                         # noqa: E402
from tools.decoder_time import timed     # noqa: E402

DEV = "cuda:0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest_time.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ingest_time needs the GPU: there is no CPU path to time"
    img = IC.big_frames()
    x = torch.from_numpy(img).to(DEV)
    res = dict(tool="ingest_time", device=torch.cuda.get_device_name(0), frames=list(img.shape), warmup=a.warmup, steps=a.steps)
    # the yardstick: a device-to-device copy moves 2 bytes per byte copied
    n = 64 << 20
    s, d = torch.zeros(n, dtype=torch.uint8, device=DEV), torch.empty(n, dtype=torch.uint8, device=DEV)
    cp = timed(lambda: d.copy_(s), a.warmup, a.steps)
    gbps = 2 * n / (cp["median_ms"] * 1e-3) / 1e9
    res["copy_64MiB"] = dict(cp, moved_GB_per_s=round(gbps, 1))
    try:
        from PIL import Image
        import PIL
        res["pillow"] = PIL.__version__
    except ImportError:
        Image = None
        res["pillow"] = None
    for tag, (fH, fW) in IC.BIG.items():
        m = toc3d_amd.ResizeCropFlipRotImage(IC.conf(900, 1600, (fH, fW)), training=False)
        ref = IC.restated_case(IC.conf(900, 1600, (fH, fW)), img)
        diff = int((m(x).cpu().numpy() != ref).sum())
        assert diff == 0, f"{tag}: {diff} bytes differ from the restatement"
        t = m.host_tables()
        bv = t["v"][1]
        rows = int((bv[:, 0] + bv[:, 1]).max() - bv[0, 0])
        moved = 6 * (rows * 1600 * 3 + fH * fW * 3)
        r = dict(timed(lambda: m(x), a.warmup, a.steps), differing_bytes=diff, ksize=[t["h"][2], t["v"][2]], source_rows_needed=rows, bytes_moved=moved)
        r["copy_time_for_those_bytes_ms"] = round(moved / (gbps * 1e9) * 1e3, 4)
        r["times_the_copy"] = round(r["median_ms"] / r["copy_time_for_those_bytes_ms"], 2)
        r["moved_GB_per_s"] = round(moved / (r["median_ms"] * 1e-3) / 1e9, 1)
        if Image is not None:
            _, dims, crop = m.geometry()
            ts = []
            for _ in range(a.host_reps):
                t0 = time.perf_counter()
                for f in img:
                    np.array(Image.fromarray(f).resize(dims).crop(crop))
                ts.append((time.perf_counter() - t0) * 1e3)
            r["host_pillow_six_images_ms"] = round(sorted(ts)[len(ts) // 2], 2)
            r["host_pillow_over_hip"] = round(r["host_pillow_six_images_ms"] / r["median_ms"], 1)
        res[tag] = r
        print(f"[{tag}] {r}", file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
