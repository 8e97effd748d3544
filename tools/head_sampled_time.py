"""Time of the head on SAMPLED tokens (``topk_indexes``) at the shipped sizes -- batch 1, 6 x 20 x 50 = 6000 tokens, 644 + 256 queries, 1024 memory entries, six
decoder layers -- in ``fp32x3`` and ``bf16``: the token side alone (``HeadTokenEmbedding``) and one whole frame of ``StreamPETRHead(token_sampling=True)`` on a
populated bank, for ``None`` (every token: the full-token path), K = 3000 (the ``infer_ratio`` 0.5 of the shipped ``FocalHead``) and K = 6000 (every token through
the sampled kernels: what the gather itself costs).  The three legs of a comparison run in the SAME process on the same module, alternating over ``--repeats``
rounds of (warm-up 50, median of 200 event-timed legs: tools/head_time.py's protocol); a figure here is only ever compared with the ``None`` leg beside it.
``median_ms`` = the median of the rounds' medians, ``spread_ms`` = their min-max range; ``faster_than_full`` says whether a sampled leg's median lies below the
full path's by more than the larger of the two spreads.  The lists are seeded random subsets in random order (``FocalHead``'s lists are sorted by score, not by
position, so neither are theirs).  One JSON line on stdout, also written to --out.

  python tools/head_sampled_time.py
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import toc3d_amd                                  # noqa: E402
from toc3d_amd import synth                       # noqa: E402
from tools.decoder_time import timed              # noqa: E402

DEV = "cuda:0"
LEN = 6000
LEGS = (("full", None), ("k3000", 3000), ("k6000", 6000))


def index_list(K):
    g = torch.Generator().manual_seed(K)
    return torch.randperm(LEN, generator=g)[:K].view(1, K, 1).to(DEV)


def compare(fns, warmup, steps, repeats):
    """{leg: callable} -> per leg the rounds' medians, their median and spread, and the verdict against "full"."""
    runs = {k: [] for k in fns}
    for _ in range(repeats):                                           # alternating: every leg sees the same drift of the card
        for k, fn in fns.items():
            runs[k].append(timed(fn, warmup, steps)["median_ms"])
    med = {k: sorted(v)[len(v) // 2] for k, v in runs.items()}
    spread = {k: round(max(v) - min(v), 4) for k, v in runs.items()}
    out = {}
    for k in fns:
        out[k] = dict(rounds_ms=runs[k], median_ms=med[k], spread_ms=spread[k])
        if k != "full":
            out[k]["ratio_to_full"] = round(med[k] / med["full"], 4)
            out[k]["faster_than_full"] = bool(med[k] < med["full"] - max(spread[k], spread["full"]))
    return out


def token_side(precision, warmup, steps, repeats):
    cfg = synth.HEAD_TOKENS_CFG
    inp = synth.head_tokens_inputs(cfg, 1, 6, 20, 50, seed=1)
    args = (inp["feats"].to(DEV), inp["intrinsics"].to(DEV), inp["lidar2img"].to(DEV), (320, 800, 3))
    m = toc3d_amd.HeadTokenEmbedding(precision=precision, **cfg)
    m.load_state_dict(synth.head_tokens_state_dict(cfg, seed=1))
    m = m.to(DEV).eval()
    lists = {k: None if K is None else index_list(K) for k, K in LEGS}
    return compare({k: (lambda t=t: m(*args, topk_indexes=t)) for k, t in lists.items()}, warmup, steps, repeats)


def head_frame(precision, warmup, steps, repeats):
    h = toc3d_amd.build_head(synth.head_cfg(), precision=precision, token_sampling=True)
    h.load_state_dict(synth.head_state_dict())
    h = h.to(DEV).eval()
    inp = synth.head_inputs()
    frames = [{k: v.to(DEV) for k, v in d.items()} for d in inp["frames"]]
    metas = inp["img_metas"]
    h(None, metas, None, **frames[0])                                  # scene start: from here on the bank is populated
    lists = {k: None if K is None else index_list(K) for k, K in LEGS}
    return compare({k: (lambda t=t: h(None, metas, t, **frames[1])) for k, t in lists.items()}, warmup, steps, repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_sampled_time.json"))
    a = ap.parse_args()
    res = dict(tool="head_sampled_time", device=torch.cuda.get_device_name(0), sizes={k: v for k, v in synth.HEAD_FULL.items() if k != "decoder"},
               shape=synth.HEAD_FULL_SHAPE, warmup=a.warmup, steps=a.steps, repeats=a.repeats)
    for precision in ("fp32x3", "bf16"):
        res[f"token_side_{precision}"] = token_side(precision, a.warmup, a.steps, a.repeats)
        res[f"head_{precision}"] = head_frame(precision, a.warmup, a.steps, a.repeats)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
