"""Time of one toc3d_amd.HeadOutputs forward plus NMS-free decoding at the shipped sizes (6 levels, batch 1, 900 queries, E 256, 10 classes, max_num 300), for
``levels="all"`` and ``levels="last"`` in both precisions, next to a torch-eager control of the same math on the same card: the branches on stock ``nn.Linear`` /
``nn.LayerNorm`` modules with the same weights (f32 next to fp32x3, bf16 next to bf16), ``torch.nan_to_num``, the reference-point add, sigmoid, pc_range, and the
coder's top-k / gather / denormalise / mask in eager torch ops.  A leg = forward + decode of the last level, decode output left on the device (no host
synchronisation in either path).  Warm-up 50, then the median of 200 event-timed legs.  One JSON line on stdout, also written to --out
(default profiles/head_outputs_time.json).

  python tools/head_outputs_time.py                  # the timing
  python tools/head_outputs_time.py --frames 20 --precision fp32x3 --levels all    # just run legs (under `rocprofv3 --kernel-trace --stats -- python ...`)
"""
import argparse
import json
import os
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import toc3d_amd                         # noqa: E402
from toc3d_amd import synth              # noqa: E402
from tools.decoder_time import timed     # noqa: E402

DEV = "cuda:0"


class TorchHeadOutputs(nn.Module):
    """get_transformer_outputs behind the transformer call and NMSFreeCoder.decode_single on stock torch ops."""

    def __init__(self, sizes, sd, coder_cfg):
        super().__init__()
        E, NC, CS = sizes["embed_dims"], sizes["num_classes"], sizes["code_size"]
        self.cls = nn.Sequential(nn.Linear(E, E), nn.LayerNorm(E), nn.ReLU(), nn.Linear(E, E), nn.LayerNorm(E), nn.ReLU(), nn.Linear(E, NC))
        self.reg = nn.Sequential(nn.Linear(E, E), nn.ReLU(), nn.Linear(E, E), nn.ReLU(), nn.Linear(E, CS))
        self.cls.load_state_dict({k[len("cls_branches.0."):]: v for k, v in sd.items() if k.startswith("cls_branches.0.")})
        self.reg.load_state_dict({k[len("reg_branches.0."):]: v for k, v in sd.items() if k.startswith("reg_branches.0.")})
        self.register_buffer("pc", torch.tensor(coder_cfg["pc_range"]))
        self.register_buffer("pcr", torch.tensor(coder_cfg["post_center_range"]))
        self.max_num, self.NC = coder_cfg["max_num"], NC

    @torch.no_grad()
    def forward(self, outs_dec, reference_points, last_only):
        x = torch.nan_to_num(outs_dec[-1:] if last_only else outs_dec)
        ref = reference_points.clamp(0, 1)
        ref = torch.log(ref.clamp(min=1e-5) / (1 - ref).clamp(min=1e-5))
        cls, box = self.cls(x), self.reg(x)
        box[..., 0:3] = (box[..., 0:3] + ref).sigmoid() * (self.pc[3:6] - self.pc[0:3]) + self.pc[0:3]
        out = []
        for b in range(cls.shape[1]):                                          # nms_free_coder.py:39-90
            scores, idx = cls[-1, b].float().sigmoid().view(-1).topk(self.max_num)
            labels, q = idx % self.NC, torch.div(idx, self.NC, rounding_mode="floor")
            p = box[-1, b].float()[q]
            dec = torch.cat([p[:, 0:3], p[:, 3:6].exp(), torch.atan2(p[:, 6:7], p[:, 7:8]), p[:, 8:10]], -1)
            mask = (dec[:, :3] >= self.pcr[:3]).all(1) & (dec[:, :3] <= self.pcr[3:]).all(1)
            out.append((dec, scores, labels, mask))                            # (boolean indexing would synchronise with the host: the mask is handed out instead)
        return x, cls, box, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--frames", type=int, default=0, help="run this many legs of --precision / --levels and exit (for a profiler)")
    ap.add_argument("--precision", default="fp32x3")
    ap.add_argument("--levels", default="all")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_outputs_time.json"))
    a = ap.parse_args()
    sizes, shape = synth.HEAD_OUTPUTS_FULL, synth.HEAD_OUTPUTS_FULL_SHAPE
    sd, coder_cfg = synth.head_outputs_state_dict(sizes), synth.bbox_coder_cfg()
    inp = {k: v.to(DEV) for k, v in synth.head_outputs_inputs(sizes, shape).items()}

    def module(precision, levels, launch_mode="plan"):
        m = toc3d_amd.HeadOutputs(precision=precision, levels=levels, launch_mode=launch_mode, pc_range=coder_cfg["pc_range"], bbox_coder=coder_cfg, **sizes)
        m.load_state_dict(sd)
        m = m.to(DEV).eval()

        def leg():
            _, cls, box = m(inp["outs_dec"], inp["reference_points"])
            return m.bbox_coder.decode_fixed(cls[-1], box[-1], sub_half_height=True)
        return leg

    if a.frames:
        f = module(a.precision, a.levels)
        for _ in range(a.frames):
            f()
        torch.cuda.synchronize()
        return
    res = dict(tool="head_outputs_time", device=torch.cuda.get_device_name(0), sizes=sizes, shape=shape, max_num=coder_cfg["max_num"], warmup=a.warmup, steps=a.steps)
    ctl = {tag: TorchHeadOutputs(sizes, sd, coder_cfg).to(DEV).to(tdt).eval() for tag, tdt in (("f32", torch.float32), ("bf16", torch.bfloat16))}
    beats = {}
    for levels in ("all", "last"):
        for precision, tag in (("fp32x3", "f32"), ("bf16", "bf16")):
            hip = res[f"hip_{precision}_{levels}"] = timed(module(precision, levels), a.warmup, a.steps)
            res[f"hip_{precision}_{levels}_eager_launches"] = timed(module(precision, levels, "eager"), a.warmup, a.steps)
            args = (inp["outs_dec"].to(ctl[tag].pc.dtype), inp["reference_points"].to(ctl[tag].pc.dtype), levels == "last")
            tor = res[f"torch_eager_{tag}_{levels}"] = timed(lambda: ctl[tag](*args), a.warmup, a.steps)
            beats[f"{precision}_{levels}"] = hip["median_ms"] < tor["median_ms"]
    res["hip_faster_than_torch_eager"] = beats
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
