"""Generates the fixtures of the assembled head on SAMPLED tokens from the REAL reference: tests/golden/head_sampled_tiny.npz, head_sampled_tiny_f64.npz and
head_sampled_full_frame0.npz.

Everything is tools/gen_golden_head_e2e.py's -- its holder, its stable top-k, its f32 / f64 pair, its seed search, its near-tie condition (a gap of at least
100 x the f32 / f64 error at every cut; the first seed below MAX_SEEDS that meets it) and its LIMITATION (mmcv's FFN and MultiheadAttention are stood in) --
with one change: the reference's ``forward`` is called as ``head.forward(m, centers, metas, topk, **data)``, with a seeded index list per frame and sample
(``index_lists``: unsorted, no repeats, different per sample and frame), stored in the archive as ``f<frame>_topk_indexes``.  The reference then gathers the
per-token geometry and the feature rows before any arithmetic (``dense_heads/streampetr_head.py:379-422``, :627-639) and its decoder cross-attends to K keys.

The kept ORDER is a condition of this fixture as well.  ``post_update_memory`` puts the kept proposals in front of the bank in the order of their scores, and
tests/test_gpu_head_sampled.py compares the bank entry for entry -- so wherever two kept scores lie closer than the arithmetic can tell them apart, the
reference's row order is an accident of its rounding and not something an implementation can be held to.  That is not hypothetical: the first seed that met
the cut condition alone (seed 0) has, in frame 3 of sample 1, two kept scores 2.9e-7 apart in f64 while f32 differs from f64 by 2e-6 on those scores; the head
on the GPU matched every output of that frame to 7e-5 and had the two bank rows the other way round (memory_embedding off by 3.6e-2).  So ``kept_order``
asks of every frame and sample that f32 and f64 keep the same ORDER and that every gap between neighbouring kept scores of the f64 run is at least the same
100 x the largest |f32 - f64| over the proposal scores; the stored ``order_margins`` [frame, sample, (smallest gap, error)] state it.

Tiny sizes (``synth.HEAD_TINY``, B = 2, four frames): K = 7 of the 24 tokens of a sample.  Should no seed meet the condition, frame 0 alone is written
(``head_sampled_tiny_frame0.npz``), as that file does for the shipped sizes.  Shipped sizes: K = 3000 of 6000, frame 0 only (seed 0; the last level whole, every
8th query row of the others, f32 and f64) -- the search at these sizes is the one that file reports as fruitless.  Fixed zip timestamps: a second run reproduces
the archives byte for byte.  Runs only where the reference tree exists; nothing of it is copied."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_decoder as GD                  # noqa: E402
import gen_golden_head_e2e as GE                 # noqa: E402
import gen_golden_head_outputs as GO             # noqa: E402
from toc3d_amd import synth                      # noqa: E402

K_TINY, K_FULL = 7, 3000


def index_lists(seed, shape, K):
    """Per frame (B, K, 1) int64: K of the N*h*w tokens of each sample, in random order."""
    g = torch.Generator().manual_seed(17000 + seed)
    B, LEN = shape["B"], shape["N"] * shape["h"] * shape["w"]
    return [torch.stack([torch.randperm(LEN, generator=g)[:K] for _ in range(B)]).view(B, K, 1) for _ in range(shape["frames"])]


def kept_order(f32, f64, K):
    """The condition on the ORDER of the kept proposals (module docstring) -> (met, text), and the [frame, sample, (smallest gap, error)] behind it."""
    rows, same = [], True
    for a, b in zip(f32, f64):
        v64, i64 = GE.stable_topk(b["proposal_score"], K, dim=1)
        same &= torch.equal(i64, GE.stable_topk(a["proposal_score"], K, dim=1)[1])
        gap = (v64[:, :-1] - v64[:, 1:]).min(1).values
        err = (a["proposal_score"].double() - b["proposal_score"]).abs().max(1).values
        rows.append(torch.stack([gap, err], 1))
    mg = torch.stack(rows)
    ok = same and bool((mg[..., 0] >= GE.MARGIN * mg[..., 1]).all())
    return ok, f"kept order: smallest gap / error = {float((mg[..., 0] / mg[..., 1]).min()):.1f} (need {GE.MARGIN:.0f}); f32 and f64 keep the same order: {same}", mg


def frame0(head, Coder, TR, sizes, shape, K, rows, path):
    m, holder = GE.build(head, Coder, TR, sizes, 0)
    lists = index_lists(0, shape, K)
    a = GE.pack(GE.run_stream(head, m, holder, sizes, shape, 0, torch.float32, first_frame_outputs_only=True, topk=lists), rows)
    b = GE.pack(GE.run_stream(head, m, holder, sizes, shape, 0, torch.float64, first_frame_outputs_only=True, topk=lists), rows)
    for k in a:
        print(f"  frame 0 {k}: f32 vs f64 max-abs / max-abs {float(np.abs(a[k].astype(np.float64) - b[k]).max() / np.abs(b[k]).max()):.2e}")
    extra = {} if rows is None else dict(row_step=np.array(rows))
    GO.save_npz(path, seed=np.array(0), f0_topk_indexes=lists[0].numpy(), **extra, **a, **{"f64_" + k: v for k, v in b.items()})


def main():
    pt, TR = GD.load_petr_transformer()
    head, Coder = GO.load()
    written = []
    sizes, shape = synth.HEAD_TINY, synth.HEAD_TINY_SHAPE
    print("tiny")
    found = GE.find_seed(head, Coder, TR, sizes, shape, topk=lambda seed: index_lists(seed, shape, K_TINY),
                         extra=lambda f32, f64: kept_order(f32, f64, sizes["topk_proposals"])[:2])
    if found is None:
        stale = [f for f in ("head_sampled_tiny.npz", "head_sampled_tiny_f64.npz") if os.path.exists(os.path.join(GE.GOLDEN, f))]
        assert not stale, f"no seed below {GE.MAX_SEEDS} meets the near-tie condition, yet {stale} exist: remove them"
        print(f"  no seed below {GE.MAX_SEEDS} meets the near-tie condition: frame 0 only")
        frame0(head, Coder, TR, sizes, shape, K_TINY, None, os.path.join(GE.GOLDEN, "head_sampled_tiny_frame0.npz"))
        written.append("head_sampled_tiny_frame0.npz")
    else:
        seed, holder, f32, f64, mg = found
        lists = index_lists(seed, shape, K_TINY)
        met, _, order = kept_order(f32, f64, sizes["topk_proposals"])
        assert met
        meta = dict(seed=np.array(seed), margins=mg.numpy(), order_margins=order.numpy(), margin_required=np.array(GE.MARGIN), **{f"f{f}_topk_indexes": t.numpy() for f, t in enumerate(lists)})
        for a, b in zip(f32, f64):
            for k in ("all_cls_scores", "all_bbox_preds") + GE.BANK:
                print(f"  {k}: f32 vs f64 max-abs / max-abs {float((a[k].double() - b[k]).abs().max() / b[k].abs().max().clamp_min(1e-30)):.2e}")
        GO.save_npz(os.path.join(GE.GOLDEN, "head_sampled_tiny.npz"), **meta, **GE.pack(f32))
        GO.save_npz(os.path.join(GE.GOLDEN, "head_sampled_tiny_f64.npz"), **GE.pack(f64))
        written += ["head_sampled_tiny.npz", "head_sampled_tiny_f64.npz"]
    print("full")
    frame0(head, Coder, TR, synth.HEAD_FULL, synth.HEAD_FULL_SHAPE, K_FULL, GE.FULL_STEP, os.path.join(GE.GOLDEN, "head_sampled_full_frame0.npz"))
    written.append("head_sampled_full_frame0.npz")
    for fn in written:
        size = os.path.getsize(os.path.join(GE.GOLDEN, fn))
        print(fn, size, "bytes")
        assert size < 1 << 20


if __name__ == "__main__":
    main()
