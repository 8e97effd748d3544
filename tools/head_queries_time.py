"""Time of one toc3d_amd.HeadQueries forward at the shipped sizes (batch 1, 644 learned + 256 propagated queries, 1024 memory entries, E 256) in ``fp32x3`` and
``bf16``, as a replayed launch plan and as eager launches, next to a torch-eager control of the same math on the same card: ``temporal_alignment`` and the lines in
front of it on stock ``nn.Linear`` / ``nn.LayerNorm`` modules with the same weights (f32 next to fp32x3, bf16 linear layers next to bf16), the encodings and the
concatenations in eager torch ops.  The control recomputes the learned queries' half every frame, as the reference does; ``torch_eager_*_memory_half`` is the same
control with that half cached, i.e. on the rows the module works on per frame.  A leg = one forward on a bank that stays on the device.  Warm-up 50, then the
median of 200 event-timed legs.  One JSON line on stdout, also written to --out (default profiles/head_queries_time.json).

  python tools/head_queries_time.py                  # the timing
  python tools/head_queries_time.py --frames 20 --precision fp32x3    # just run legs (under `rocprofv3 --kernel-trace --stats -- python ...`)
"""
import argparse
import json
import math
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import toc3d_amd                                  # noqa: E402
from toc3d_amd import synth                       # noqa: E402
from toc3d_amd.head_queries import dim_t          # noqa: E402
from tools.decoder_time import timed              # noqa: E402

DEV = "cuda:0"
BANK = ("memory_embedding", "memory_reference_point", "memory_timestamp", "memory_egopose", "memory_velo")


class _MLN(nn.Module):
    def __init__(self, E):
        super().__init__()
        self.reduce, self.gamma, self.beta, self.ln = nn.Sequential(nn.Linear(180, E), nn.ReLU()), nn.Linear(E, E), nn.Linear(E, E), nn.LayerNorm(E, elementwise_affine=False)

    def forward(self, x, c):
        c = self.reduce(c.to(self.gamma.weight.dtype))
        return self.gamma(c).float() * self.ln(x) + self.beta(c).float()


class TorchHeadQueries(nn.Module):
    """streampetr_head.py:641-652 with temporal_alignment :424-453 on stock torch ops; ``lin_dtype``: dtype of the linear layers (LayerNorms and encodings in f32)."""

    def __init__(self, sizes, sd, lin_dtype):
        super().__init__()
        E = sizes["embed_dims"]
        self.nq, self.np, self.E, self.dt = sizes["num_query"], sizes["num_propagated"], E, lin_dtype
        self.reference_points = nn.Embedding(self.nq, 3)
        self.query_embedding = nn.Sequential(nn.Linear(E * 3 // 2, E), nn.ReLU(), nn.Linear(E, E))
        self.time_embedding = nn.Sequential(nn.Linear(E, E), nn.LayerNorm(E))
        self.ego_pose_pe, self.ego_pose_memory = _MLN(E), _MLN(E)
        self.load_state_dict(sd, strict=True)
        for m in (self.query_embedding, self.time_embedding[0], self.ego_pose_pe.reduce, self.ego_pose_pe.gamma, self.ego_pose_pe.beta, self.ego_pose_memory.reduce,
                  self.ego_pose_memory.gamma, self.ego_pose_memory.beta):
            m.to(lin_dtype)
        self.register_buffer("pc", torch.tensor(synth.PC_RANGE))
        self.register_buffer("d3", dim_t(128))
        self.register_buffer("d1", dim_t(256))
        self.cache = None

    @staticmethod
    def _emb(pos, d):
        a = (pos * (2 * math.pi))[..., None] / d
        return torch.stack((a[..., 0::2].sin(), a[..., 1::2].cos()), -1).flatten(-2)

    def _pos3d(self, x):
        return torch.cat([self._emb(x[..., 1], self.d3), self._emb(x[..., 0], self.d3), self._emb(x[..., 2], self.d3)], -1)

    @staticmethod
    def _nerf(x):
        return torch.cat([f(x * 2.0 ** k) for k in range(6) for f in (torch.sin, torch.cos)], -1)

    def _qemb(self, x):
        return self.query_embedding(self._pos3d(x).to(self.dt)).float()

    def _temb(self, ts):
        return self.time_embedding[1](self.time_embedding[0](self._emb(ts[..., 0], self.d1).float().to(self.dt)).float())

    def _fresh(self, B, dev):
        ref = self.reference_points.weight[None].repeat(B, 1, 1)
        query_pos = self._qemb(ref)
        tgt = torch.zeros_like(query_pos)
        rec = torch.eye(4, device=dev)[None, None].repeat(B, self.nq, 1, 1)
        motion = self._nerf(torch.cat([torch.zeros_like(ref), rec[..., :3, :].flatten(-2)], -1))
        tgt, query_pos = self.ego_pose_memory(tgt, motion), self.ego_pose_pe(query_pos, motion)
        return tgt, query_pos + self._temb(torch.zeros_like(ref[..., :1])), ref

    @torch.no_grad()
    def forward(self, emb, ref_pt, ts, pose, velo, cache_fresh=False):
        B, dev = emb.shape[0], emb.device
        if cache_fresh:
            if self.cache is None:
                self.cache = self._fresh(B, dev)
            tgt, query_pos, ref = self.cache
        else:
            tgt, query_pos, ref = self._fresh(B, dev)
        tref = (ref_pt - self.pc[:3]) / (self.pc[3:6] - self.pc[0:3])
        temp_pos, temp_memory = self._qemb(tref), emb
        motion = self._nerf(torch.cat([velo, ts, pose[..., :3, :].flatten(-2)], -1).float())
        temp_pos, temp_memory = self.ego_pose_pe(temp_pos, motion), self.ego_pose_memory(temp_memory, motion)
        temp_pos = temp_pos + self._temb(ts)
        np_ = self.np
        tgt, query_pos, ref = torch.cat([tgt, temp_memory[:, :np_]], 1), torch.cat([query_pos, temp_pos[:, :np_]], 1), torch.cat([ref, tref[:, :np_]], 1)
        rec = torch.eye(4, device=dev)[None, None].repeat(B, query_pos.shape[1], 1, 1)
        return tgt, query_pos, ref, temp_memory[:, np_:], temp_pos[:, np_:], rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--frames", type=int, default=0, help="run this many legs of --precision and exit (for a profiler)")
    ap.add_argument("--precision", default="fp32x3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_queries_time.json"))
    a = ap.parse_args()
    sizes = synth.HEAD_QUERIES_FULL
    sd = synth.head_queries_state_dict(sizes)
    bank = [synth.head_queries_bank(sizes, 1, 1)[k].to(DEV) for k in BANK]

    def module(precision, launch_mode="plan"):
        m = toc3d_amd.HeadQueries(precision=precision, launch_mode=launch_mode, pc_range=synth.PC_RANGE, **sizes)
        m.load_state_dict(sd)
        m = m.to(DEV).eval()
        return lambda: m(*bank)

    if a.frames:
        f = module(a.precision)
        for _ in range(a.frames):
            f()
        torch.cuda.synchronize()
        return
    res = dict(tool="head_queries_time", device=torch.cuda.get_device_name(0), sizes=sizes, B=1, warmup=a.warmup, steps=a.steps)
    beats = {}
    for precision, tag, tdt in (("fp32x3", "f32", torch.float32), ("bf16", "bf16", torch.bfloat16)):
        ctl = TorchHeadQueries(sizes, sd, tdt).to(DEV).eval()
        hip = res[f"hip_{precision}"] = timed(module(precision), a.warmup, a.steps)
        res[f"hip_{precision}_eager_launches"] = timed(module(precision, "eager"), a.warmup, a.steps)
        tor = res[f"torch_eager_{tag}"] = timed(lambda: ctl(*bank), a.warmup, a.steps)
        half = res[f"torch_eager_{tag}_memory_half"] = timed(lambda: ctl(*bank, cache_fresh=True), a.warmup, a.steps)
        beats[precision] = dict(vs_torch_eager=hip["median_ms"] < tor["median_ms"], vs_torch_eager_memory_half=hip["median_ms"] < half["median_ms"])
    res["hip_faster_than_torch_eager"] = beats
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
