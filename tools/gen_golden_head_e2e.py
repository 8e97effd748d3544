"""Generates the end-to-end fixtures of the assembled head from the REAL reference: tests/golden/head_tiny.npz, head_tiny_f64.npz, head_full.npz,
head_full_f64.npz and head_state_dict_spec.json.

The reference's own ``StreamPETRHead.forward`` (``dense_heads/streampetr_head.py:604-680``) runs, unbound, on a holder object -- with its own
``position_embeding``, ``prepare_for_dn``, ``temporal_alignment``, ``get_transformer_outputs``, ``pre_update_memory`` / ``post_update_memory`` and ``get_bboxes``
bound to the same holder -- over a stream of frames, twice: in f32, and in f64 as the arbiter (``Tensor.float`` is the identity while the f64 run is on, as in
tools/gen_golden_head_queries.py, so the two ``.float()`` casts of ``temporal_alignment`` do not round it).  ``torch.topk`` / ``Tensor.topk`` are stable for the
whole run (ties to the lowest index, as ``oracle.ref_harness.ReferenceMemory`` pins them).  The decoder is the reference's ``PETRTemporalTransformer`` loaded
as tools/gen_golden_decoder.py loads it, and the LIMITATION stated there holds here word for word: mmcv is not installed, so mmcv's ``FFN`` and mmcv's
``MultiheadAttention`` are stood in by that file's stand-ins; every other line that computes is the reference's.  The box coder is the reference's ``NMSFreeCoder``.

The reference's ``__init__`` cannot run under the stubs (it builds losses, an assigner and a sampler through mmdet), so the holder is built from the reference's
``_init_layers`` (:236-298) plus the reference transformer, and the five frozen parameters are listed by the expressions of :207-231 (``frozen_parameters``
below); the state-dict spec is read off that holder.  Weights and inputs: ``toc3d_amd.synth.head_cfg`` / ``head_state_dict`` / ``head_inputs``.

The near-tie condition is a condition of the fixture: for every frame and sample, the gap between the ``topk_proposals``-th and the next proposal score of the
f64 run must be at least 100 x the largest |f32 - f64| over those scores, and likewise for the coder's ``max_num`` cut wherever fewer candidates than scores
survive.  The first seed, counting from 0, that meets it is taken, asserted and stored with the gaps and the errors; a size at which no seed below MAX_SEEDS
meets it gets no archive.  Runs only where the reference tree exists; nothing of it is copied.  The archives carry fixed zip timestamps: a second run reproduces
them byte for byte.

Outcome with the seeded weights of ``toc3d_amd.synth``: the tiny sizes meet the condition at seed 5 (smallest gap 146 x the error).  At the shipped sizes (900 queries,
256 kept; 9000 class scores, 300 kept) the proposal scores of a head with random weights lie within ~1e-5 of their neighbours around the cut while f32 differs
from f64 by ~1e-7 on them: of the seeds 0 .. 272 none reaches 100 x (best: 64 x), a few dozen have exact f32 ties among the decoded scores.  So ``head_full.npz`` is
not committed and the full-size streaming test that would read it does not exist.  What no cut has touched is committed instead: ``head_full_frame0.npz``, both
outputs of frame 0 at seed 0 (the last level whole, every 8th query row of the others, f32 and f64), which ``tests/test_gpu_head.py`` holds the head to; the shipped sizes are covered per module (decoder_full, head_queries_full,
head_outputs_full); the composition test holds the head to the chain of those modules bit for bit at the tiny sizes.
"""
import collections
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_decoder as GD                  # noqa: E402
import gen_golden_head_outputs as GO             # noqa: E402
from oracle import ref_harness as R              # noqa: E402
from toc3d_amd import synth                      # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
BANK = ("memory_embedding", "memory_reference_point", "memory_timestamp", "memory_egopose", "memory_velo")
FULL_STEP = 8
MARGIN = 100.0
MAX_SEEDS = 273                                  # the search that was run (4 s a seed at the shipped sizes); see the outcome in the module docstring


_TopK = collections.namedtuple("topk", ["values", "indices"])


def stable_topk(input, k, dim=-1, largest=True, sorted=True):
    v, i = torch.sort(input, dim=dim, descending=largest, stable=True)
    return _TopK(v.narrow(dim, 0, k), i.narrow(dim, 0, k))


def frozen_parameters(cfg, code_size=10, depth_num=64, depth_start=1):
    """code_weights, match_costs, pc_range, position_range, coords_d by the expressions of streampetr_head.py:119-129 and :207-231 (LID = True)."""
    cw = list(cfg["code_weights"])[:code_size]
    p = lambda v: nn.Parameter(torch.tensor(v), requires_grad=False)
    position_range = p(cfg["position_range"])
    index = torch.arange(start=0, end=depth_num, step=1).float()
    index_1 = index + 1
    bin_size = (position_range[3] - depth_start) / (depth_num * (1 + depth_num))
    coords_d = depth_start + bin_size * index * index_1
    return dict(code_weights=p(cw), match_costs=p(cw), pc_range=p(cfg["bbox_coder"]["pc_range"]), position_range=position_range,
                coords_d=nn.Parameter(coords_d, requires_grad=False))


class Holder(R.ReferenceMemory):
    """What ``self`` is while the reference's methods run: the memory attributes of ReferenceMemory plus the modules of ``_init_layers``."""

    def post_update_memory(self, data, rec_ego_pose, all_cls_scores, all_bbox_preds, outs_dec, mask_dict=None):
        assert mask_dict is None
        self._cls.post_update_memory(self, data, rec_ego_pose, all_cls_scores, all_bbox_preds, outs_dec, None)


def build(head, Coder, TR, sizes, seed):
    cfg = synth.head_cfg(sizes)
    m = Holder(memory_len=sizes["memory_len"], topk_proposals=sizes["topk_proposals"], num_propagated=sizes["num_propagated"], embed_dims=256,
               pc_range=synth.PC_RANGE, pseudo_reference_points=None)
    for k, v in dict(num_reg_fcs=2, normedlinear=False, cls_out_channels=10, code_size=10, num_pred=6, position_dim=192, in_channels=sizes["in_channels"],
                     num_query=sizes["num_query"], with_ego_pos=True, with_dn=False).items():
        setattr(m, k, v)
    head._init_layers(m)
    m.transformer = TR.build(cfg["transformer"])
    m.bbox_coder = Coder(**{k: v for k, v in cfg["bbox_coder"].items() if k != "type"})
    holder = nn.Module()
    for name in ("cls_branches", "reg_branches", "position_encoder", "memory_embed", "featurized_pe", "reference_points", "pseudo_reference_points",
                 "query_embedding", "spatial_alignment", "time_embedding", "ego_pose_pe", "ego_pose_memory", "transformer"):
        setattr(holder, name, getattr(m, name))
    for name, prm in frozen_parameters(cfg).items():
        setattr(holder, name, prm)
        setattr(m, name, prm)
    holder.load_state_dict(synth.head_state_dict(sizes, seed=seed), strict=True)
    holder.eval()
    for name in ("position_embeding", "prepare_for_dn", "temporal_alignment", "get_transformer_outputs", "get_bboxes"):
        setattr(m, name, types.MethodType(getattr(head, name), m))
    return m, holder


def run_stream(head, m, holder, sizes, shape, seed, dtype, first_frame_outputs_only=False, topk=None):
    """The reference's forward and get_bboxes over the frames of synth.head_inputs -> per frame a dict of tensors (outputs, bank, decoded lists, cut margins).
    ``first_frame_outputs_only``: frame 0 alone and its two output tensors alone -- what no top-k cut has touched yet.  ``topk``: per frame the ``topk_indexes``
    (B, K, 1) handed to the forward (tools/gen_golden_head_sampled.py); None: every token, as the shipped configs run at eval."""
    ref = R.load_reference()
    inp = synth.head_inputs(sizes, shape, seed=seed)
    holder.to(dtype)
    head.reset_memory(m)
    NC, K, max_num = 10, sizes["topk_proposals"], sizes["max_num"]
    metas = [dict(meta, box_type_3d=lambda t, d: t) for meta in inp["img_metas"]]
    pad_h, pad_w, _ = metas[0]["pad_shape"][0]
    cast = lambda t: t.to(dtype) if t.dtype == torch.float32 else t          # (the timestamps are f64 in both runs)
    frames = []
    orig = (torch.topk, torch.Tensor.topk, torch.Tensor.to, torch.Tensor.float)
    torch.topk = torch.Tensor.topk = stable_topk
    torch.Tensor.to = lambda self, *a, **k: self if (a and a[0] in ("cuda", "cpu")) else orig[2](self, *a, **k)      # position_embeding hops cpu -> cuda (:407)
    if dtype == torch.float64:
        torch.Tensor.float = lambda t, *a, **k: t
    try:
        with torch.no_grad():
            for f, data in enumerate(inp["frames"]):
                data = {k: cast(v) for k, v in data.items()}
                B, N = data["img_feats"].shape[:2]
                centers = cast(ref.misc.locations(data["img_feats"].flatten(0, 1), 16, pad_h, pad_w)[None].repeat(B * N, 1, 1, 1))
                out = head.forward(m, centers, metas, None if topk is None else topk[f], **data)
                assert out["dn_mask_dict"] is None
                cls, box = out["all_cls_scores"], out["all_bbox_preds"]
                if first_frame_outputs_only:
                    return [dict(all_cls_scores=cls.clone(), all_bbox_preds=box.clone())]
                fr = dict(all_cls_scores=cls.clone(), all_bbox_preds=box.clone(), **{k: getattr(m, k).clone() for k in BANK})
                score = cls[-1].sigmoid().max(-1).values                                  # rec_score of post_update_memory (:359)
                fr["proposal_score"] = score
                fr["proposal_set"] = stable_topk(score, K, dim=1)[1].sort(1).values
                flat = cls[-1].sigmoid().flatten(1)
                fr["flat_score"] = flat
                dec = m.get_bboxes(dict(all_cls_scores=cls.clone(), all_bbox_preds=box.clone()), metas)
                for b, (bboxes, scores, labels) in enumerate(dec):
                    top_v, top_i = stable_topk(flat[b], min(max_num, flat.shape[1]))
                    assert bool((top_v[:-1] > top_v[1:]).all()), "ties among the decoded scores: another seed"
                    pos = torch.searchsorted(-top_v, -scores)                                # the survivors are a subsequence of the top max_num
                    assert pos.numel() == 0 or (int(pos.max()) < top_v.numel() and torch.equal(top_v[pos], scores) and torch.equal(top_i[pos] % NC, labels)), \
                        "the decoded list is not a subsequence of the stable top max_num: another seed"
                    fr[f"b{b}_bboxes"], fr[f"b{b}_scores"], fr[f"b{b}_labels"] = bboxes, scores, labels
                    fr[f"b{b}_query"] = torch.div(top_i[pos], NC, rounding_mode="floor")
                frames.append(fr)
    finally:
        torch.topk, torch.Tensor.topk, torch.Tensor.to, torch.Tensor.float = orig
    return frames


def margins(f32, f64, K, max_num):
    """Per frame and sample: (gap of the proposal cut in f64, max |f32 - f64| over the proposal scores, gap of the max_num cut, its error); a cut that keeps
    everything has an infinite gap."""
    rows = []
    for a, b in zip(f32, f64):
        for key, k in (("proposal_score", K), ("flat_score", max_num)):
            s64 = torch.sort(b[key], dim=1, descending=True).values
            gap = (s64[:, k - 1] - s64[:, k]) if k < s64.shape[1] else torch.full((s64.shape[0],), float("inf"), dtype=torch.float64)
            err = (a[key].double() - b[key]).abs().max(1).values
            rows.append(torch.stack([gap, err], 1))
    return torch.stack(rows).view(len(f32), 2, -1, 2)          # [frame, cut, sample, (gap, err)]


def find_seed(head, Coder, TR, sizes, shape, topk=None, extra=None):
    """``topk``: seed -> the per-frame index lists of that seed's stream (run_stream), or None.  ``extra``: a further condition of the fixture,
    (f32 frames, f64 frames) -> (met, text for the log), asked of a seed beside the near-tie condition."""
    for seed in range(MAX_SEEDS):
        m, holder = build(head, Coder, TR, sizes, seed)
        try:
            lists = None if topk is None else topk(seed)
            f32 = run_stream(head, m, holder, sizes, shape, seed, torch.float32, topk=lists)
            f64 = run_stream(head, m, holder, sizes, shape, seed, torch.float64, topk=lists)
        except AssertionError as e:
            print(f"  seed {seed}: {e}")
            continue
        mg = margins(f32, f64, sizes["topk_proposals"], sizes["max_num"])
        ok = bool((mg[..., 0] >= MARGIN * mg[..., 1]).all())
        same = all(torch.equal(a["proposal_set"], b["proposal_set"]) and all(torch.equal(a[k], b[k]) for k in a if k.endswith(("_labels", "_query"))) for a, b in zip(f32, f64))
        print(f"  seed {seed}: smallest gap / error = {float((mg[..., 0] / mg[..., 1]).min()):.1f} (need {MARGIN:.0f}); f32 and f64 keep the same sets: {same}")
        if ok and extra is not None:
            ok, text = extra(f32, f64)
            print(f"  seed {seed}: {text}")
        if ok:
            assert same, "the margin holds and the sets differ: the condition does not mean what it should"
            return seed, holder, f32, f64, mg
    return None


def pack(frames, rows=None, last_whole=True):
    """Frames -> flat dict of numpy arrays.  ``rows``: keep every ``rows``-th query / bank row (the last level whole when ``last_whole``)."""
    out = {}
    for f, fr in enumerate(frames):
        for k, v in fr.items():
            if k in ("proposal_score", "flat_score"):
                continue
            if rows and k in ("all_cls_scores", "all_bbox_preds"):
                out[f"f{f}_{k}_last"] = v[-1].numpy()
                v = v[:-1, :, ::rows]
            elif rows and k in BANK:
                v = v[:, ::rows]
            out[f"f{f}_{k}"] = v.numpy()
    return out


def main():
    pt, TR = GD.load_petr_transformer()
    head, Coder = GO.load()
    cases = (("tiny", synth.HEAD_TINY, synth.HEAD_TINY_SHAPE, None), ("full", synth.HEAD_FULL, synth.HEAD_FULL_SHAPE, FULL_STEP))
    spec = {tag: {k: list(v.shape) for k, v in build(head, Coder, TR, sizes, 0)[1].state_dict().items()} for tag, sizes, _, _ in cases}
    json.dump(spec, open(os.path.join(GOLDEN, "head_state_dict_spec.json"), "w"), indent=1)
    written = ["head_state_dict_spec.json"]
    for tag, sizes, shape, rows in cases:
        print(tag)
        found = find_seed(head, Coder, TR, sizes, shape)
        if found is None:
            # a fixture that does not meet its condition is not written (and one written earlier must not survive a generator that no longer stands behind it)
            stale = [f for f in (f"head_{tag}.npz", f"head_{tag}_f64.npz") if os.path.exists(os.path.join(GOLDEN, f))]
            assert not stale, f"no seed below {MAX_SEEDS} meets the near-tie condition at the {tag} sizes, yet {stale} exist: remove them"
            print(f"  no seed below {MAX_SEEDS} meets the near-tie condition at the {tag} sizes: head_{tag}.npz is NOT written")
            # ... what no cut has touched is written all the same: both outputs of frame 0 (a scene start: the bank holds the pseudo reference points), seed 0,
            # f32 and f64 in one archive -- the token side, the six-layer decoder and the branches at these sizes against the reference itself
            m, holder = build(head, Coder, TR, sizes, 0)
            a = pack(run_stream(head, m, holder, sizes, shape, 0, torch.float32, first_frame_outputs_only=True), rows)
            b = pack(run_stream(head, m, holder, sizes, shape, 0, torch.float64, first_frame_outputs_only=True), rows)
            for k in a:
                print(f"  frame 0 {k}: f32 vs f64 max-abs / max-abs {float(np.abs(a[k].astype(np.float64) - b[k]).max() / np.abs(b[k]).max()):.2e}")
            GO.save_npz(os.path.join(GOLDEN, f"head_{tag}_frame0.npz"), seed=np.array(0), row_step=np.array(rows), **a, **{"f64_" + k: v for k, v in b.items()})
            written.append(f"head_{tag}_frame0.npz")
            continue
        seed, holder, f32, f64, mg = found
        meta = dict(seed=np.array(seed), margins=mg.numpy(), margin_required=np.array(MARGIN))
        if rows:
            meta["row_step"] = np.array(rows)
        for a, b in zip(f32, f64):
            for k in ("all_cls_scores", "all_bbox_preds") + BANK:
                print(f"  {k}: f32 vs f64 max-abs / max-abs {float((a[k].double() - b[k]).abs().max() / b[k].abs().max().clamp_min(1e-30)):.2e}")
        GO.save_npz(os.path.join(GOLDEN, f"head_{tag}.npz"), **meta, **pack(f32, rows))
        GO.save_npz(os.path.join(GOLDEN, f"head_{tag}_f64.npz"), **pack(f64, rows))
        written += [f"head_{tag}.npz", f"head_{tag}_f64.npz"]
    for fn in written:
        size = os.path.getsize(os.path.join(GOLDEN, fn))
        print(fn, size, "bytes")
        assert size < 1 << 20


if __name__ == "__main__":
    main()
