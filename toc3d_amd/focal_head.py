"""``FocalHead``, the 2-D auxiliary head (``img_roi_head`` of every shipped config), at eval on the GPU: the per-camera 2-D detections, the per-token sampling
weight and its ranking.

:class:`FocalHead` is the eval branch of the reference's ``FocalHead.forward`` (``dense_heads/focal_head.py:140-193``) over the layers of ``_init_layers``
(:119-134): two towers ``Conv2d 3x3 -> GroupNorm(32, .) -> ReLU`` on the neck's level-0 features, five 1x1 convs (``cls`` | ``centerness`` on the class tower,
``ltrb`` | ``center2d`` on the box tower), ``apply_ltrb`` / ``apply_center_offset`` (``models/utils/misc.py:26-56``) and
``sample_weight = sigmoid(max_c cls) * sigmoid(centerness)`` (:178-180), whose ``int(N*h*w * infer_ratio)`` best tokens per sample are ``topk_indexes`` -- the
list ``StreamPETRHead`` attends to instead of all image tokens.  Parameters live under the reference's sixteen names, so the ``img_roi_head.*`` keys of a
StreamPETR / ToC3D checkpoint load strictly.

Per frame (``csrc/focal_head.hip``, ``include/toc3d_focal.h``), four launches: ONE implicit-GEMM 3x3 conv for both towers (weights stacked along Cout, the
existing ``EPI_CONV3X3`` path) into f32 rows ``[M, 2 E]`` -> ``toc3d_focal_gn_stats`` -> ``toc3d_focal_heads`` -> ``toc3d_rank_desc`` on the sampling weight
(descending, ties to the lower index -- ``torch.topk`` leaves the tie order open; stable-descending is the rule of this package).  ``forward`` puts
``toc3d_nchw_to_rows`` in front; ``forward_rows`` starts from token rows.  ``select_rows`` / ``select`` are the selection-only frame a detector needs
(``Petr3D.simple_test_pts`` reads ``topk_indexes`` and nothing else, ``detectors/petr3d.py:524-525``, and the class tower alone decides it): the conv of
``shared_cls.0`` alone -> ``toc3d_focal_gn_stats`` on one tower -> ``toc3d_focal_sample_weight`` (``csrc/focal_select.hip``, ``include/toc3d_select.h``) ->
``toc3d_rank_desc``, with the bits of the full frame's ``topk_indexes`` and ``sample_weight``.  The sequence is recorded once per shape into a launch plan and replayed with one C
call per frame.  ``precision`` decides the conv's products (``"fp32x3"``: bf16 x 3 on f32 rows; ``"bf16"``); everything behind the conv is f32 in both.

Inference only: losses, assigner and sampler are accepted and nothing is built from them.  No CPU path.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import gemm, lib
from .gemm import DEFAULT_PRECISION
from .staged import StagedModule, require_cuda

_NAME = "toc3d_amd.FocalHead"
MAX_TOKENS = 16000             # toc3d_rank_desc (include/toc3d.h)
MAX_ROW_STATES = 4             # recorded plans of forward_rows name the caller's rows buffer: at most this many are kept


def _no(what):
    raise NotImplementedError(f"{_NAME}: {what} is not implemented (supported: the eval forward of the shipped configs -- in_channels and embed_dims multiples "
                              "of 64, precision 'bf16' or 'fp32x3')")


class FocalHead(StagedModule):
    _NAME, _RUNS, _SUPPORTED = _NAME, "the head runs", ("bf16", "fp32x3")

    def __init__(self, num_classes, in_channels=256, embed_dims=256, stride=16, use_hybrid_tokens=False, train_ratio=1.0, infer_ratio=1.0,
                 sync_cls_avg_factor=False, loss_cls2d=None, loss_centerness=None, loss_bbox2d=None, loss_iou2d=None, loss_centers2d=None, train_cfg=None,
                 test_cfg=None, init_cfg=None, precision=DEFAULT_PRECISION, launch_mode="plan", **kwargs):
        super().__init__()
        if use_hybrid_tokens:
            _no("use_hybrid_tokens=True (a random sampling ratio per training step)")
        for name, c in (("in_channels", in_channels), ("embed_dims", embed_dims)):
            if not isinstance(c, int) or c <= 0 or c % 64:
                _no(f"{name}={c} (a multiple of 64: the implicit-GEMM conv reads whole 64-channel K-tiles per tap)")
        if embed_dims % 32 or embed_dims > 1024:
            _no(f"embed_dims={embed_dims} (GroupNorm(32, .) on at most 1024 channels)")
        if not isinstance(num_classes, int) or num_classes < 1 or num_classes > 64 or (num_classes + 7) * embed_dims * 4 + 1024 > 64 * 1024:
            _no(f"num_classes={num_classes} with embed_dims={embed_dims} (1 .. 64 classes, the 1x1 convs' weights within 64 KB of LDS)")
        if not 0.0 <= float(infer_ratio) <= 1.0:
            raise ValueError(f"{_NAME}: infer_ratio={infer_ratio} is outside [0, 1]")
        self._init_staged(precision, launch_mode)
        self.num_classes, self.cls_out_channels, self.in_channels, self.embed_dims, self.stride = num_classes, num_classes, in_channels, embed_dims, stride
        self.use_hybrid_tokens, self.train_ratio, self.infer_ratio, self.sync_cls_avg_factor = False, train_ratio, infer_ratio, sync_cls_avg_factor
        self.train_cfg, self.test_cfg, self.fp16_enabled, self.bg_cls_weight = train_cfg, test_cfg, False, 0
        E = embed_dims
        # _init_layers :119-134
        self.cls = nn.Conv2d(E, num_classes, kernel_size=1)
        self.shared_reg = nn.Sequential(nn.Conv2d(in_channels, E, kernel_size=(3, 3), padding=1), nn.GroupNorm(32, num_channels=E), nn.ReLU())
        self.shared_cls = nn.Sequential(nn.Conv2d(in_channels, E, kernel_size=(3, 3), padding=1), nn.GroupNorm(32, num_channels=E), nn.ReLU())
        self.centerness = nn.Conv2d(E, 1, kernel_size=1)
        self.ltrb = nn.Conv2d(E, 4, kernel_size=1)
        self.center2d = nn.Conv2d(E, 2, kernel_size=1)
        self.init_weights()
        super().train(False)

    def init_weights(self):                    # :136-138
        for m in (self.cls, self.centerness):
            nn.init.constant_(m.bias, -4.59511985013459)              # bias_init_with_prob(0.01)
        self._drop_derived()

    def train(self, mode=True):
        if mode:
            raise NotImplementedError(f"{_NAME}: training mode is not implemented (inference only: losses, assigner and sampler are not built)")
        return super().train(False)

    # ------------------------------------------------------------------------------------------------------------------------------
    def _pack(self, pk):
        f32, E = pk.f32, self.embed_dims
        conv = lambda m: m.weight.detach().permute(0, 2, 3, 1).reshape(E, -1)          # (Cout, Cin, ky, kx) -> (Cout, ky, kx, Cin): the conv's column order
        cat = lambda *t: f32(torch.cat([x.detach().reshape(x.shape[0], -1) if x.dim() > 1 else x.detach() for x in t]))
        c, r = self.shared_cls, self.shared_reg
        return dict(dt=pk.dts.act, tdt=pk.dts.torch, conv=pk.wb(torch.cat([conv(c[0]), conv(r[0])]), torch.cat([c[0].bias.detach(), r[0].bias.detach()])),
                    gamma=cat(c[1].weight, r[1].weight), beta=cat(c[1].bias, r[1].bias), eps=float(c[1].eps),
                    wc=cat(self.cls.weight, self.centerness.weight), bc=cat(self.cls.bias, self.centerness.bias),
                    wr=cat(self.ltrb.weight, self.center2d.weight), br=cat(self.ltrb.bias, self.center2d.bias),
                    zeros=torch.zeros(256, dtype=torch.uint8, device=pk.dev))

    def _alloc(self, key, dev):
        B, N, h, w = key
        V, T, C, E, f = B * N, h * w, self.in_channels, self.embed_dims, torch.float32
        M = V * T
        z = lambda *s, d=f: torch.zeros(*s, dtype=d, device=dev)
        return dict(x=z(V, C, h, w), rows=z(M, C, d=self._packed["tdt"]), loc=z(M, 2), h=z(M, 2 * E), stats=z(V, 64, 2), cls=z(M, self.num_classes),
                    box=z(M, 4), ctr2d=z(M, 2), ctrness=z(M), weight=z(B, N * T), order=z(B, N * T, d=torch.int64))

    def _select_workspace(self, W, key, dev):
        """The selection-only frame's own buffers, beside the full frame's in ``W`` (built when the first selection of the shape runs)."""
        S = W.get("select")
        if S is None:
            B, N, h, w = key
            V, T, f = B * N, h * w, torch.float32
            z = lambda *s, d=f: torch.zeros(*s, dtype=d, device=dev)
            narrow = gemm.small_m_variant(V * T, 2 * self.embed_dims, 9 * self.in_channels, False) != 0          # (_select_launches: else the conv runs at full width into W["h"])
            S = W["select"] = dict(hc=z(V * T, self.embed_dims) if narrow else None, stats=z(V, 32, 2), weight=z(B, N * T), order=z(B, N * T, d=torch.int64))
        return S

    def _launches(self, key, W, rows, K):
        """``[(name, launch), ...]``: the four launches of one frame on the token rows ``rows`` [M, in_channels] (act dtype) and the staged ``location``
        (three when ``K == 0``: nothing is ranked)."""
        P, (B, N, h, w) = self._packed, key
        V, T, C, E = B * N, h * w, self.in_channels, self.embed_dims
        M = V * T
        s = lib.stream_ptr

        def conv():                                        # shared_cls.0 | shared_reg.0, f32 rows out in both precisions (the statistics are taken on unrounded sums)
            gemm.linear(self, lib.EPI_CONV3X3, rows, P["conv"][0], P["conv"][1], W["h"], M, 2 * E, 9 * C, lda=C, ldo=2 * E, conv=(P["zeros"], h, w),
                        variant=gemm.small_m_variant(M, 2 * E, 9 * C, False))
        stats = lambda: lib.call("toc3d_focal_gn_stats", lib.F32, W["h"], 2 * E, V, T, E, 2, P["eps"], W["stats"], s())
        heads = lambda: lib.call("toc3d_focal_heads", lib.F32, W["h"], 2 * E, W["stats"], P["gamma"], P["beta"], P["wc"], P["bc"], P["wr"], P["br"], W["loc"],
                                 V, T, E, self.num_classes, W["cls"], self.num_classes, W["box"], W["ctr2d"], W["ctrness"], W["weight"], s())
        rank = lambda: lib.call("toc3d_rank_desc", W["weight"], B, N * T, W["order"], s())
        return [("conv3x3", conv), ("gn_stats", stats), ("heads", heads)] + ([("rank_desc", rank)] if K > 0 else [])

    def _select_launches(self, key, W, rows, K):
        """``[(name, launch), ...]`` of the selection-only frame: the class tower's half of :meth:`_launches`, into the buffers of :meth:`_select_workspace`."""
        P, S, (B, N, h, w) = self._packed, W["select"], key
        V, T, C, E = B * N, h * w, self.in_channels, self.embed_dims
        M = V * T
        s = lib.stream_ptr
        # The tile of the FULL-width conv: all unsplit tiles accumulate K in one order, but a narrower N must not pick another tile family on its own.  Where the
        # full-width shape leaves the tile to the library's heuristic (0: M >= 16k rows), that heuristic may depend on N: the conv then runs at full width into
        # the full frame's buffer, and the two launches behind it read its first E columns (ldx = 2 E) -- the bits are the full frame's by construction.
        variant = gemm.small_m_variant(M, 2 * E, 9 * C, False)
        x, ldx, n = (S["hc"], E, E) if variant != 0 else (W["h"], 2 * E, 2 * E)

        def conv():                                        # shared_cls.0 alone: its rows come first in the packed stack
            gemm.linear(self, lib.EPI_CONV3X3, rows, P["conv"][0], P["conv"][1], x, M, n, 9 * C, lda=C, ldo=ldx, conv=(P["zeros"], h, w), variant=variant)
        stats = lambda: lib.call("toc3d_focal_gn_stats", lib.F32, x, ldx, V, T, E, 1, P["eps"], S["stats"], s())
        weight = lambda: lib.call("toc3d_focal_sample_weight", lib.F32, x, ldx, S["stats"], P["gamma"], P["beta"], P["wc"], P["bc"], V, T, E, self.num_classes,
                                  S["weight"], s())
        rank = lambda: lib.call("toc3d_rank_desc", S["weight"], B, N * T, S["order"], s())
        return [("conv3x3", conv), ("gn_stats", stats), ("sample_weight", weight)] + ([("rank_desc", rank)] if K > 0 else [])

    def _frame(self, key, W, rows, K, select=False):
        for _, launch in (self._select_launches if select else self._launches)(key, W, rows, K):
            launch()

    def _check(self, location, B, N, h, w):
        if self.training:
            raise NotImplementedError(f"{_NAME}: training mode is not implemented (call .eval(): the sampling ratio of a training step and the losses are out of scope)")
        if not (isinstance(location, torch.Tensor) and location.numel() == B * N * h * w * 2 and location.shape[-1] == 2):
            raise ValueError(f"{_NAME}: location {tuple(getattr(location, 'shape', ()))} is not (B*N, h, w, 2) for B, N, h, w = {B}, {N}, {h}, {w}")
        if min(B, N, h, w) < 1 or N * h * w > MAX_TOKENS:
            raise ValueError(f"{_NAME}: B, N, h, w = {B}, {N}, {h}, {w}: empty, or more than {MAX_TOKENS} tokens per sample (the ranking keeps a sample in LDS)")

    def _outputs(self, W, key, K):
        B, N, h, w = key
        V, T = B * N, h * w
        return dict(enc_cls_scores=W["cls"].clone().view(V, T, self.num_classes), enc_bbox_preds=W["box"].clone().view(V, T, 4),
                    pred_centers2d=W["ctr2d"].clone().view(V, T, 2), centerness=W["ctrness"].clone().view(V, T, 1),
                    topk_indexes=W["order"][:, :K].clone().view(B, K, 1) if K > 0 else torch.empty(B, 0, 1, dtype=torch.int64, device=W["order"].device),
                    sample_weight=W["weight"].clone().view(B, N * T, 1))

    def _select_outputs(self, W, key, K):
        B, N, h, w = key
        S = W["select"]
        return dict(topk_indexes=S["order"][:, :K].clone().view(B, K, 1) if K > 0 else torch.empty(B, 0, 1, dtype=torch.int64, device=S["order"].device),
                    sample_weight=S["weight"].clone().view(B, N * h * w, 1))

    @torch.no_grad()
    def forward(self, location, **data):
        """``data['img_feats']`` (B, N, C, h, w) f32 on the device (neck level 0), ``location`` (B*N, h, w, 2) normalised pixel centres
        (``Petr3D.prepare_location``).  Returns the reference's dict -- ``enc_cls_scores`` (B*N, h*w, num_classes) logits, ``enc_bbox_preds`` (B*N, h*w, 4)
        cxcywh in [0, 1], ``pred_centers2d`` (B*N, h*w, 2), ``centerness`` (B*N, h*w, 1) logits, ``topk_indexes`` (B, K, 1) int64 with
        ``K = int(N*h*w * infer_ratio)`` -- plus ``sample_weight`` (B, N*h*w, 1), the tensor that is ranked (:180; the reference computes it and does not return
        it).  All freshly allocated: none aliases a workspace."""
        return self._forward(location, data, False)

    @torch.no_grad()
    def select(self, location, **data):
        """:meth:`forward` for a caller that reads ``topk_indexes`` alone: ``dict(topk_indexes (B, K, 1) int64, sample_weight (B, N*h*w, 1))``, bit for bit
        :meth:`forward`'s, from the class tower only (module docstring).  Both freshly allocated."""
        return self._forward(location, data, True)

    def _forward(self, location, data, select):
        """:meth:`forward` (``select=False``) or :meth:`select`: one staging, one plan per kind."""
        src = data["img_feats"]
        require_cuda(_NAME, src, location, on_device=False)
        if src.dim() != 5 or src.shape[2] != self.in_channels:
            raise ValueError(f"{_NAME}: img_feats {tuple(src.shape)} is not (B, N, {self.in_channels}, h, w)")
        B, N, C, h, w = src.shape
        self._check(location, B, N, h, w)
        require_cuda(_NAME, src, location)
        K = int(N * h * w * self.infer_ratio)                                         # :155, the reference's expression
        dev, key = src.device, (B, N, h, w)
        with torch.cuda.device(dev):
            W = self._workspace(key, dev)
            c = lambda t: t.detach().to(device=dev, dtype=torch.float32).contiguous()
            lib.copy_segments([(W["x"], c(src))] + ([] if select else [(W["loc"], c(location))]), lib.stream_ptr())
            if select:
                self._select_workspace(W, key, dev)

            def launches():
                lib.call("toc3d_nchw_to_rows", self._packed["dt"], W["x"], W["rows"], C, B * N, C, h * w, lib.stream_ptr())
                self._frame(key, W, W["rows"], K, select)
            self._run(("select", key, K) if select else (key, K), launches)
            return self._select_outputs(W, key, K) if select else self._outputs(W, key, K)

    @torch.no_grad()
    def forward_rows(self, location, rows, ld, B, N, h, w):
        """:meth:`forward` on token rows: ``rows`` [B*N*h*w, ld] in the act dtype (bf16 on ``"bf16"``, plain f32 on ``"fp32x3"``: the conv gathers its taps
        from them, so ``ld == in_channels``), row (b, n, y, x) -- what ``toc3d_nchw_to_rows`` makes of ``img_feats``, and what the neck's conv leaves before its
        transpose.  No NCHW tensor is read; every other launch, and every bit, is :meth:`forward`'s.  A recorded plan names ``rows``: the buffer lives as long as
        the plan does."""
        return self._forward_rows(location, rows, ld, B, N, h, w, False)

    @torch.no_grad()
    def select_rows(self, location, rows, ld, B, N, h, w):
        """:meth:`select` on token rows, as :meth:`forward_rows` is :meth:`forward` on them: the same ``rows``, the same refusals, four launches (three when
        ``K == 0``), recorded under a plan key of its own within the same ``MAX_ROW_STATES``."""
        return self._forward_rows(location, rows, ld, B, N, h, w, True)

    def _forward_rows(self, location, rows, ld, B, N, h, w, select):
        """:meth:`forward_rows` (``select=False``) or :meth:`select_rows` (which stages no ``location``: the class tower does not read it)."""
        B, N, h, w, ld = (int(v) for v in (B, N, h, w, ld))
        require_cuda(_NAME, rows, location, on_device=False)
        self._check(location, B, N, h, w)
        require_cuda(_NAME, rows, location)
        dev, key = rows.device, (B, N, h, w)
        with torch.cuda.device(dev):
            W = self._workspace(key, dev)
            if rows.dim() != 2 or tuple(rows.shape) != (B * N * h * w, ld) or ld != self.in_channels or not rows.is_contiguous() or rows.dtype != self._packed["tdt"]:
                raise ValueError(f"{_NAME}: rows {tuple(rows.shape)} {rows.dtype} must be contiguous [{B * N * h * w}, {self.in_channels}] {self._packed['tdt']}")
            K = int(N * h * w * self.infer_ratio)
            if select:
                self._select_workspace(W, key, dev)
            else:
                lib.copy_segments([(W["loc"], location.detach().to(device=dev, dtype=torch.float32).contiguous())], lib.stream_ptr())
            skey = ("select_rows" if select else "rows", key, K, rows.data_ptr())
            self._run(skey, lambda: self._frame(key, W, rows, K, select), max_states=MAX_ROW_STATES)
            self._states[skey]["rows"] = rows
            return self._select_outputs(W, key, K) if select else self._outputs(W, key, K)
