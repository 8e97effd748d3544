"""Time of one toc3d_amd.PETRTemporalTransformer forward at the shipped sizes (E 256, 8 heads, FFN 2048, 6 layers, 900 queries, 768 memory entries, 6000
image tokens, batch 1), both precisions, next to a torch-eager control on the same card: the same layer built from ``nn.MultiheadAttention`` / ``nn.Linear`` /
``nn.LayerNorm`` modules with the same weights, in f32 and in bf16.  Warm-up 50 forwards, then the median of 200 event-timed forwards.  One JSON line on
stdout, also written to --out (default profiles/decoder_time.json).

  python tools/decoder_time.py                       # the timing
  python tools/decoder_time.py --frames 20 --precision fp32x3     # just run frames (under `rocprofv3 --kernel-trace --stats -- python tools/decoder_time.py ...`)
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

DEV = "cuda:0"


class TorchDecoder(nn.Module):
    """The eval-time dataflow of the reference's decoder on stock torch modules (sequence-first, as the reference runs it)."""

    def __init__(self, sizes, sd):
        super().__init__()
        E, H, F, L = sizes["embed_dims"], sizes["num_heads"], sizes["feedforward_channels"], sizes["num_layers"]
        self.attn = nn.ModuleList([nn.ModuleList([nn.MultiheadAttention(E, H) for _ in range(2)]) for _ in range(L)])
        self.fc0, self.fc1 = nn.ModuleList([nn.Linear(E, F) for _ in range(L)]), nn.ModuleList([nn.Linear(F, E) for _ in range(L)])
        self.norms = nn.ModuleList([nn.ModuleList([nn.LayerNorm(E) for _ in range(3)]) for _ in range(L)])
        self.post = nn.LayerNorm(E)
        for i in range(L):
            p = f"decoder.layers.{i}."
            for a in range(2):
                self.attn[i][a].load_state_dict({k[len(p) + 18:]: v for k, v in sd.items() if k.startswith(p + f"attentions.{a}.attn.")})
            self.fc0[i].load_state_dict(dict(weight=sd[p + "ffns.0.layers.0.0.weight"], bias=sd[p + "ffns.0.layers.0.0.bias"]))
            self.fc1[i].load_state_dict(dict(weight=sd[p + "ffns.0.layers.1.weight"], bias=sd[p + "ffns.0.layers.1.bias"]))
            for n in range(3):
                self.norms[i][n].load_state_dict(dict(weight=sd[p + f"norms.{n}.weight"], bias=sd[p + f"norms.{n}.bias"]))
        self.post.load_state_dict(dict(weight=sd["decoder.post_norm.weight"], bias=sd["decoder.post_norm.bias"]))

    @torch.no_grad()
    def forward(self, memory, tgt, query_pos, pos_embed, temp_memory, temp_pos):
        t = lambda a: a.transpose(0, 1).contiguous()
        memory, x, qpos, pos, tmem, tpos = t(memory), t(tgt), t(query_pos), t(pos_embed), t(temp_memory), t(temp_pos)
        outs = []
        for i in range(len(self.attn)):
            keys, kpos = torch.cat([x, tmem], 0), torch.cat([qpos, tpos], 0)
            x = self.norms[i][0](x + self.attn[i][0](x + qpos, keys + kpos, keys, need_weights=False)[0])
            x = self.norms[i][1](x + self.attn[i][1](x + qpos, memory + pos, memory)[0])        # the reference takes the attention maps of the cross-attention
            x = self.norms[i][2](x + self.fc1[i](torch.relu(self.fc0[i](x))))
            outs.append(self.post(x))
        return torch.stack(outs).transpose(1, 2)


def timed(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return dict(median_ms=round(ts[len(ts) // 2], 4), min_ms=round(ts[0], 4), p90_ms=round(ts[int(len(ts) * 0.9)], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--frames", type=int, default=0, help="run this many forwards of --precision and exit (for a profiler)")
    ap.add_argument("--precision", default="fp32x3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decoder_time.json"))
    a = ap.parse_args()
    sizes, shape = synth.DECODER_FULL, synth.DECODER_FULL_SHAPE
    sd = synth.decoder_state_dict(sizes)
    inp = {k: v.to(DEV) for k, v in synth.decoder_inputs(sizes, shape).items()}

    def module(precision, launch_mode="plan"):
        m = toc3d_amd.build_transformer(dict(synth.decoder_cfg(**sizes), precision=precision, launch_mode=launch_mode))
        m.load_state_dict(sd)
        m = m.to(DEV).eval()
        return lambda: m(inp["memory"], inp["tgt"], inp["query_pos"], inp["pos_embed"], None, inp["temp_memory"], inp["temp_pos"])

    if a.frames:
        f = module(a.precision)
        for _ in range(a.frames):
            f()
        torch.cuda.synchronize()
        return
    res = dict(tool="decoder_time", device=torch.cuda.get_device_name(0), sizes=sizes, shape=shape, warmup=a.warmup, steps=a.steps)
    for precision in ("fp32x3", "bf16"):
        res[f"hip_{precision}"] = timed(module(precision), a.warmup, a.steps)
        res[f"hip_{precision}_eager_launches"] = timed(module(precision, "eager"), a.warmup, a.steps)
    for tag, tdt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
        ctl = TorchDecoder(sizes, sd).to(DEV).to(tdt).eval()
        args = [inp[k].to(tdt) for k in ("memory", "tgt", "query_pos", "pos_embed", "temp_memory", "temp_pos")]
        res[f"torch_eager_{tag}"] = timed(lambda: ctl(*args), a.warmup, a.steps)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
