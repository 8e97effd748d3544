"""Output side of ``StreamPETRHead`` on the GPU: the class / box branches behind the temporal decoder and NMS-free box decoding.

:class:`HeadOutputs` is the second half of the reference's ``StreamPETRHead.get_transformer_outputs`` (``dense_heads/streampetr_head.py:582-602``):
``nan_to_num`` of ``outs_dec``, ``cls_branches`` / ``reg_branches`` (built as ``_init_layers`` :239-260 builds them: ONE module held ``num_pred`` times), the
reference-point add, sigmoid and the ``pc_range`` de-normalisation -- and ``get_bboxes`` (:1051-1071).  :class:`NMSFreeCoder` is the reference's coder of that
name (``core/bbox/coders/nms_free_coder.py:39-111`` over ``denormalize_bbox``, ``core/bbox/util.py:24-51``).  It sits between
:class:`toc3d_amd.PETRTemporalTransformer` (``outs_dec``) and :meth:`toc3d_amd.TemporalMemory.post_update_memory` (which reads ``all_cls_scores``,
``all_bbox_preds`` and ``outs_dec``).  Parameters live under the reference's names, so the ``pts_bbox_head.cls_branches.*`` / ``reg_branches.*`` keys of a
StreamPETR / ToC3D checkpoint load strictly.

Per frame (``csrc/head_outputs.hip``, ``include/toc3d.h``): ``toc3d_head_nan_to_num_rows`` -> ONE GEMM for the first layers of both towers (weights concatenated
along N) -> ``toc3d_head_ln_relu_rows`` -> the towers' second layers (two GEMMs) -> ``toc3d_head_outputs`` (last LayerNorm + ReLU / ReLU on load, the two
E -> 10 layers from LDS, reference points, sigmoid, pc_range).  The sequence is recorded once per shape into a launch plan and replayed with one C call per
frame.  Decoding is one launch, ``toc3d_nms_free_decode``.  No CPU path.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch
import torch.nn as nn

from . import lib
from .gemm import DEFAULT_PRECISION
from .staged import StagedModule, host_range, require_cuda

_NAME = "toc3d_amd.HeadOutputs"
DECODE_MAX_SLOTS, DECODE_MAX_NUM = 16384, 2048          # csrc/head_outputs.hip: num_query * num_classes keys in registers, max_num entries in LDS


def _no(what):
    raise NotImplementedError(f"{_NAME}: {what} is not implemented (supported: the inference-time branches of the shipped configs -- num_reg_fcs=2 "
                              "Linear + LayerNorm + ReLU class towers and Linear + ReLU box towers on a sigmoid classifier, precision 'bf16' or 'fp32x3')")


class NMSFreeCoder:
    """The reference's ``NMSFreeCoder`` (same constructor keywords) on ``toc3d_nms_free_decode``: top ``max_num`` of the ``num_query * num_classes`` sigmoid
    scores in descending order (ties: lowest flat index), ``denormalize_bbox``, the ``post_center_range`` / ``score_threshold`` mask.  No CPU path."""

    def __init__(self, pc_range, voxel_size=None, post_center_range=None, max_num=100, score_threshold=None, num_classes=10):
        self.pc_range, self.voxel_size, self.post_center_range = pc_range, voxel_size, post_center_range
        self.max_num, self.score_threshold, self.num_classes = max_num, score_threshold, num_classes

    def encode(self):
        pass

    def decode_fixed(self, cls_scores, bbox_preds, sub_half_height=False):
        """``cls_scores`` (B, Q, num_classes) logits, ``bbox_preds`` (B, Q, code_size) -> fixed-capacity device tensors ``(boxes (B, max_num, 9 or 7), scores
        (B, max_num), labels (B, max_num) int64, query_index (B, max_num) int64, counts (B,) int64)``: per sample the first ``counts[b]`` rows are the survivors in
        descending score order, the rest zeros (indices -1).  No host synchronisation; the inputs are not modified.  ``sub_half_height``: ``z -= h / 2`` of
        ``StreamPETRHead.get_bboxes`` (:1066)."""
        if self.post_center_range is None:
            raise NotImplementedError("Need to reorganize output as a batch, only support post_center_range is not None for now!")
        require_cuda("toc3d_amd.NMSFreeCoder", cls_scores, bbox_preds, on_device=False)
        if cls_scores.dim() != 3 or bbox_preds.dim() != 3 or cls_scores.shape[-1] != self.num_classes or bbox_preds.shape[:2] != cls_scores.shape[:2]:
            raise ValueError(f"toc3d_amd.NMSFreeCoder: cls_scores {tuple(cls_scores.shape)} / bbox_preds {tuple(bbox_preds.shape)} do not fit num_classes={self.num_classes}")
        require_cuda("toc3d_amd.NMSFreeCoder", cls_scores)
        B, Q, NC = cls_scores.shape
        CS = bbox_preds.shape[-1]
        dev = cls_scores.device
        K = int(self.max_num)
        with torch.cuda.device(dev):
            cls = cls_scores.detach().to(torch.float32).contiguous()
            box = bbox_preds.detach().to(device=dev, dtype=torch.float32).contiguous()
            ow = 9 if CS > 8 else 7
            boxes = torch.empty(B, K, ow, dtype=torch.float32, device=dev)
            scores = torch.empty(B, K, dtype=torch.float32, device=dev)
            labels, qidx = (torch.empty(B, K, dtype=torch.int64, device=dev) for _ in range(2))
            counts = torch.empty(B, dtype=torch.int64, device=dev)
            pcr = host_range(self.post_center_range)                  # (the C ABI reads it at call time)
            thr = self.score_threshold
            lib.call("toc3d_nms_free_decode", cls, NC, box, CS, B, Q, NC, CS, K, pcr, int(bool(thr)), float(thr) if thr else 0.0, int(bool(sub_half_height)),
                     boxes, scores, labels, qidx, counts, lib.stream_ptr())
        return boxes, scores, labels, qidx, counts

    def _listed(self, cls_scores, bbox_preds, sub_half_height=False):
        boxes, scores, labels, _, counts = self.decode_fixed(cls_scores, bbox_preds, sub_half_height)
        n = counts.tolist()                                            # the one host synchronisation
        return [dict(bboxes=boxes[b, :n[b]], scores=scores[b, :n[b]], labels=labels[b, :n[b]]) for b in range(len(n))]

    def decode_single(self, cls_scores, bbox_preds):
        """(num_query, num_classes), (num_query, code_size) -> ``{'bboxes', 'scores', 'labels'}`` (nms_free_coder.py:39-90)."""
        return self._listed(cls_scores[None], bbox_preds[None])[0]

    def decode(self, preds_dicts):
        """``preds_dicts['all_cls_scores'][-1]``, ``['all_bbox_preds'][-1]`` -> one ``{'bboxes', 'scores', 'labels'}`` per sample (:92-111)."""
        return self._listed(preds_dicts["all_cls_scores"][-1], preds_dicts["all_bbox_preds"][-1])


class HeadOutputs(StagedModule):
    _NAME, _RUNS, _SUPPORTED = _NAME, "the branches run", ("bf16", "fp32x3")

    def __init__(self, num_classes=10, embed_dims=256, num_reg_fcs=2, code_size=10, num_pred=6, normedlinear=False,
                 pc_range: Sequence[float] = (-51.2, -51.2, -5.0, 51.2, 51.2, 3.0), bbox_coder=None, precision=DEFAULT_PRECISION, launch_mode="plan",
                 levels="all"):
        super().__init__()
        if normedlinear:
            _no("normedlinear=True (NormedLinear)")
        if num_reg_fcs != 2:
            _no(f"num_reg_fcs={num_reg_fcs}")
        self._init_staged(precision, launch_mode)
        if levels not in ("all", "last"):
            _no(f"levels={levels!r} (use 'all' or 'last')")
        E = embed_dims
        if not isinstance(E, int) or E <= 0 or E % 64 or E > 1024 or (num_classes + code_size) * E * 4 > 64 * 1024:
            _no(f"embed_dims={E} with {num_classes} classes and code_size {code_size} (embed_dims a multiple of 64, <= 1024, both last layers within 64 KB of LDS)")
        if code_size != 8 and code_size < 10:
            _no(f"code_size={code_size} (8, or >= 10 with the velocity in columns 8, 9)")
        if num_classes < 1 or num_classes > 64 or code_size > 64 or num_pred < 1:
            _no(f"num_classes={num_classes} / code_size={code_size} / num_pred={num_pred}")
        self.num_classes, self.cls_out_channels, self.embed_dims, self.num_reg_fcs = num_classes, num_classes, E, num_reg_fcs
        self.code_size, self.num_pred, self.normedlinear = code_size, num_pred, False
        self.levels = levels
        # _init_layers :239-260 -- the SAME module num_pred times
        cls_branch, reg_branch = [], []
        for _ in range(num_reg_fcs):
            cls_branch += [nn.Linear(E, E), nn.LayerNorm(E), nn.ReLU(inplace=True)]
            reg_branch += [nn.Linear(E, E), nn.ReLU()]
        fc_cls = nn.Sequential(*cls_branch, nn.Linear(E, self.cls_out_channels))
        fc_reg = nn.Sequential(*reg_branch, nn.Linear(E, code_size))
        self.cls_branches = nn.ModuleList([fc_cls for _ in range(num_pred)])
        self.reg_branches = nn.ModuleList([fc_reg for _ in range(num_pred)])
        self._pc = host_range(pc_range)
        self.pc_range = [float(v) for v in pc_range]
        if isinstance(bbox_coder, dict):
            from .registry import build_bbox_coder
            bbox_coder = build_bbox_coder(bbox_coder)
        self.bbox_coder: Optional[NMSFreeCoder] = bbox_coder

    def init_weights(self):                    # :309-312
        for m in self.cls_branches:
            nn.init.constant_(m[-1].bias, -4.59511985013459)          # bias_init_with_prob(0.01)
        self._drop_derived()

    # ------------------------------------------------------------------------------------------------------------------------------
    def _pack(self, pk):
        dts, f32 = pk.dts, pk.f32                                  # (fp32x3: weights and the GEMMs' A rows as (hi, lo) planes)
        c, r = self.cls_branches[0], self.reg_branches[0]
        return dict(rows=dts.rows, tdt=dts.torch, planes=dts.x3p, l1=pk.linear(c[0], r[0]), l2c=pk.linear(c[3]), l2r=pk.linear(r[2]),
                    ln1=pk.layernorm(c[1]), ln2=pk.layernorm(c[4]), wc=f32(c[6].weight), bc=f32(c[6].bias), wr=f32(r[4].weight), br=f32(r[4].bias))

    def _alloc(self, key, dev):
        Lc, B, Q = key
        M, E, tdt, f = Lc * B * Q, self.embed_dims, self._packed["tdt"], torch.float32
        z = lambda r, c, d=f: torch.zeros(r, c, dtype=d, device=dev)
        return dict(x=z(M, E), clean=z(M, E), a0=z(M, E, tdt), h1=z(M, 2 * E), a1=z(M, 2 * E, tdt), h2=z(M, 2 * E), ref=z(B * Q, 3),
                    cls=z(M, self.cls_out_channels), box=z(M, self.code_size))

    def _frame(self, key, W):
        """The launch sequence of one frame on the staged inputs of workspace ``W`` (eager or being recorded)."""
        P, (Lc, B, Q) = self._packed, key
        M, E, NC, CS = Lc * B * Q, self.embed_dims, self.cls_out_channels, self.code_size
        s = lib.stream_ptr()

        def linear(a, wb, out, N, lda, ldo):               # f32 rows out (the LayerNorm statistics are taken on unrounded sums in both precisions)
            self._linear(a, wb, out, M, N, E, f32_out=True, lda=lda, ldo=ldo, a_planes=P["planes"])

        lib.call("toc3d_head_nan_to_num_rows", P["rows"], W["x"], E, W["clean"], E, W["a0"], E, M, E, s)
        linear(W["a0"], P["l1"], W["h1"], 2 * E, E, 2 * E)                                   # class tower | box tower, first layers
        g, b, eps = P["ln1"]
        lib.call("toc3d_head_ln_relu_rows", P["rows"], W["h1"], 2 * E, g, b, eps, W["a1"], 2 * E, M, E, E, s)
        half = lambda t: t.data_ptr() + E * t.element_size()                               # the box tower's E columns of a [M, 2E] buffer
        linear(W["a1"], P["l2c"], W["h2"], E, 2 * E, 2 * E)
        linear(half(W["a1"]), P["l2r"], half(W["h2"]), E, 2 * E, 2 * E)
        g, b, eps = P["ln2"]
        lib.call("toc3d_head_outputs", W["h2"], 2 * E, g, b, eps, P["wc"], P["bc"], P["wr"], P["br"], W["ref"], B * Q, self._pc,
                 W["cls"], NC, W["box"], CS, M, E, NC, CS, s)

    @torch.no_grad()
    def forward(self, outs_dec, reference_points):
        """``outs_dec`` (L, B, Q, E) f32 as :class:`PETRTemporalTransformer` returns it; ``reference_points`` (B, Q, 3) in [0, 1].  Returns ``(outs_dec,
        all_cls_scores, all_bbox_preds)``: the ``nan_to_num``-cleaned copy of ``outs_dec`` (L, B, Q, E), class logits (L, B, Q, num_classes) and boxes
        (L, B, Q, code_size) with centres in ``pc_range`` -- all three freshly allocated (none aliases a workspace).  With ``levels="last"`` only the last level
        is computed and returned (leading dimension 1): ``[-1]`` is all that ``post_update_memory``, ``decode`` and evaluation read."""
        require_cuda(_NAME, outs_dec, reference_points, on_device=False)
        if outs_dec.dim() != 4 or outs_dec.shape[-1] != self.embed_dims or tuple(reference_points.shape) != (*outs_dec.shape[1:3], 3):
            raise ValueError(f"{_NAME}: outs_dec {tuple(outs_dec.shape)} / reference_points {tuple(reference_points.shape)} do not fit embed_dims={self.embed_dims}")
        require_cuda(_NAME, outs_dec)
        L, B, Q, E = outs_dec.shape
        src = outs_dec if self.levels == "all" else outs_dec[-1:]
        Lc, dev = src.shape[0], outs_dec.device
        with torch.cuda.device(dev):
            key = (Lc, B, Q)
            W = self._workspace(key, dev)
            c = lambda t, w: t.detach().to(device=dev, dtype=torch.float32).reshape(-1, w).contiguous()
            lib.copy_segments([(W["x"], c(src, E)), (W["ref"], c(reference_points, 3))], lib.stream_ptr())
            self._run(key, lambda: self._frame(key, W))
            return (W["clean"].clone().view(Lc, B, Q, E), W["cls"].clone().view(Lc, B, Q, self.cls_out_channels),
                    W["box"].clone().view(Lc, B, Q, self.code_size))

    def get_bboxes(self, preds_dicts, img_metas=None, rescale=False):
        """``[[bboxes, scores, labels], ...]`` per sample from ``preds_dicts['all_cls_scores']`` / ``['all_bbox_preds']`` (:1051-1071): the coder's survivors in
        descending score order with ``z -= h / 2`` applied, sliced to each sample's count (one host synchronisation, for the ``[B]`` counts).  ``bboxes`` is a
        plain (n, 9) tensor, wrapped as ``img_metas[i]['box_type_3d'](bboxes, 9)`` when ``img_metas`` carries one.  Unlike the reference, which shifts ``z`` in
        the decoded tensor it was handed, this edits none of its inputs."""
        if self.bbox_coder is None:
            raise RuntimeError(f"{_NAME}.get_bboxes needs a bbox_coder (pass bbox_coder=dict(type='NMSFreeCoder', ...) to the constructor)")
        preds = self.bbox_coder._listed(preds_dicts["all_cls_scores"][-1], preds_dicts["all_bbox_preds"][-1], sub_half_height=True)
        ret = []
        for i, p in enumerate(preds):
            bboxes = p["bboxes"]
            if img_metas is not None and img_metas[i].get("box_type_3d") is not None:
                bboxes = img_metas[i]["box_type_3d"](bboxes, bboxes.size(-1))
            ret.append([bboxes, p["scores"], p["labels"]])
        return ret
