"""Time of one toc3d_amd.FocalHead frame at the shipped size (6 views of 20 x 50 tokens, 256 channels, ten classes), for ``infer_ratio`` 1.0 and 0.5 in both
precisions: the whole ``forward`` (staging copies, ``toc3d_nchw_to_rows``, the four launches replayed from the recorded plan, the clones of the outputs), the
same with eager launches, ``forward_rows`` (no NCHW tensor), and each of the four launches on its own (event-timed back to back on the module's workspace, so a
launch's figure holds its launch overhead).  Next to that, torch eager running the restatement of tests/focal_head_cases.py on the same card in the same run
(f32 next to fp32x3; the conv operands rounded to bf16 next to bf16).  Warm-up 50, then the median of 200 event-timed legs.  One JSON line on stdout, also
written to --out (default profiles/focal_head_time.json).

  python tools/focal_head_time.py                  # the timing
  python tools/focal_head_time.py --frames 20 --precision fp32x3     # just run frames (under `rocprofv3 --kernel-trace --stats -- python ...`)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--frames", type=int, default=0, help="run this many forwards of --precision and exit (for a profiler)")
    ap.add_argument("--precision", default="fp32x3")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch-eager control")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "focal_head_time.json"))
    a = ap.parse_args()
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
