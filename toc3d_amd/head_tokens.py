"""Token side of ``StreamPETRHead.forward`` on the GPU (second half): the consumers of the neck's
features right behind the backbone -- ``position_embeding`` (``dense_heads/streampetr_head.py:378-422``), ``memory_embed``,
``spatial_alignment`` (``MLN(8)``) and ``featurized_pe`` (``SELayer_Linear``), composed as ``forward`` :627-639 does.

Sub-module names equal the head's, so the ``pts_bbox_head.*`` keys of a reference checkpoint load unchanged
(``position_encoder.{0,2}``, ``memory_embed.{0,2}``, ``spatial_alignment.{reduce.0,gamma,beta}``, ``featurized_pe.{conv_reduce,
conv_expand}``).  Linear layers run on ``toc3d_linear``; geometry / LayerNorm / gates on ``toc3d_head_*`` kernels.  No CPU path.
``precision="fp32x3"`` (what an assembled :class:`toc3d_amd.StreamPETRHead` runs by default) goes through :func:`toc3d_amd.gemm.linear` instead: weights and the
row kernels' outputs as (hi, lo) planes, and the four ``nn.ReLU`` folded into their GEMMs (``EPI_BIAS_RELU``) -- nine GEMM launches and no ReLU launch.
``topk_indexes`` (what :class:`toc3d_amd.FocalHead` returns; the reference's ``topk_gather``, ``models/utils/misc.py:13-23``): the K listed tokens of every sample are
gathered BEFORE any arithmetic, as the reference does (:379-422, :627-639) -- the frustum kernel computes the listed tokens only
(``toc3d_head_frustum_inputs_sampled``), the feature rows are gathered from the full-token workspace (``toc3d_gather_token_rows``), and the nine GEMMs,
``toc3d_mln_apply`` and ``toc3d_se_gate`` run at ``M = B*K``.
``torch.linalg.inv`` of the (B*N) 4x4 ``lidar2img`` matrices is plumbing on the device (the reference hops to the CPU for it, :404).
"""
from __future__ import annotations

from typing import Sequence

import torch
import torch.nn as nn

from . import lib
from .gemm import round_up as _ru
from .staged import MLN, StagedModule, host_range, require_cuda


class _SE(nn.Module):                       # models/utils/misc.py:140-145
    def __init__(self, ch):
        super().__init__()
        self.conv_reduce, self.conv_expand = nn.Linear(ch, ch), nn.Linear(ch, ch)


class HeadTokenEmbedding(StagedModule):
    _NAME, _RUNS, _SUPPORTED = "toc3d_amd.HeadTokenEmbedding", "the token side runs", ("bf16", "fp32", "fp32x3")

    def __init__(self, in_channels=256, embed_dims=256, depth_num=64, depth_start=1.0, LID=True, stride=16,
                 position_range: Sequence[float] = (-61.2, -61.2, -10.0, 61.2, 61.2, 10.0), precision="fp32", **unused):
        super().__init__()
        self._init_staged(precision)                                        # (launched eagerly: the token side is not recorded into a plan)
        if embed_dims > 1024 or depth_num < 30:
            raise NotImplementedError(f"{self._NAME}: embed_dims={embed_dims} / depth_num={depth_num} is not implemented (embed_dims <= 1024, depth_num >= 30)")
        self.in_channels, self.embed_dims, self.depth_num, self.stride = in_channels, embed_dims, depth_num, stride
        E = embed_dims
        self.position_encoder = nn.Sequential(nn.Linear(depth_num * 3, 4 * E), nn.ReLU(), nn.Linear(4 * E, E))       # :262-266
        self.memory_embed = nn.Sequential(nn.Linear(in_channels, E), nn.ReLU(), nn.Linear(E, E))                      # :268-272
        self.spatial_alignment = MLN(8, E)                                                                            # :288
        self.featurized_pe = _SE(E)                                                                                   # :275
        self._pr = pr = host_range(position_range)
        index = torch.arange(0, depth_num, 1).float()                                                                 # :221-232
        if LID:
            cd = depth_start + (pr[3] - depth_start) / (depth_num * (1 + depth_num)) * index * (index + 1)
        else:
            cd = depth_start + (pr[3] - depth_start) / depth_num * index
        self.register_buffer("coords_d", cd, persistent=False)
        self.__dict__["_coords_d_owner"] = None                                         # bind_coords_d: an owner's Parameter that replaces the buffer

    def bind_coords_d(self, param):
        """Read the depth bins from ``param`` (a [depth_num] f32 Parameter of a module that owns this one, which moves and loads with its owner) instead of
        the buffer computed from the config: the reference keeps ``coords_d`` in its state dict (streampetr_head.py:231), so a checkpoint's values count."""
        assert tuple(param.shape) == (self.depth_num,)
        self.__dict__["_coords_d_owner"] = param            # (a plain attribute: the parameter stays its owner's, this module's state dict does not grow)

    def _pack(self, pk):
        dts, pack = pk.dts, pk.linear
        return dict(dts=dts, dt=dts.act, tdt=dts.torch, pe0=pack(self.position_encoder[0]), pe2=pack(self.position_encoder[2]), me0=pack(self.memory_embed[0]),
                    me2=pack(self.memory_embed[2]), red=pack(self.spatial_alignment.reduce[0]), gam=pack(self.spatial_alignment.gamma),
                    bet=pack(self.spatial_alignment.beta), se1=pack(self.featurized_pe.conv_reduce), se2=pack(self.featurized_pe.conv_expand))

    def _alloc(self, key, dev):
        # key: (B, N, h, w) -- every token -- or (B, N, h, w, K): K listed tokens per sample, whose "feat" holds the GATHERED rows (the full-token rows, which the
        # gather reads, stay in the (B, N, h, w) workspace: feat_workspace)
        (B, N, h, w), C, E, D, tdt, f = key[:4], self.in_channels, self.embed_dims, self.depth_num, self._packed["tdt"], torch.float32
        M = B * (N * h * w if len(key) == 4 else key[4])
        z = lambda r, c, d=tdt: torch.zeros(r, c, dtype=d, device=dev)
        return dict(pin=z(M, _ru(3 * D, 64)), cone_a=z(M, 64), cone=z(M, 8, f), h1=z(M, _ru(4 * E, 64)), feat=z(M, _ru(C, 64)), m1=z(M, _ru(E, 64)),
                    c1=z(M, _ru(E, 64)), mem_a=z(M, _ru(E, 64)), s1=z(M, _ru(E, 64)), pos=z(M, E, f), mem_raw=z(M, E, f), gam=z(M, E, f), bet=z(M, E, f), se=z(M, E, f))

    def feat_workspace(self, B, N, h, w, device):
        """``(rows, ld, dtype)``: this module's own token rows of the image features for a ``(B, N, h, w)`` -- the buffer ``toc3d_nchw_to_rows`` fills in
        :meth:`forward` --, its leading dimension and the C ABI's dtype of its rows.  A producer that holds the features as rows (the neck:
        :meth:`toc3d_amd.CPFPN.forward_fanout`) writes columns ``[0, in_channels)`` there; :meth:`forward_rows` then runs on them.  The buffer lives until
        ``load_state_dict`` / ``.to()``; the padding columns are zero and stay zero.  It is the full-token buffer whatever ``topk_indexes`` a frame brings: the
        sampled path gathers from it."""
        dev = torch.device(device)
        with torch.cuda.device(dev):
            W = self._workspace((B, N, h, w), dev)
        return W["feat"], W["feat"].shape[1], self._packed["dts"].rows

    @torch.no_grad()
    def forward_rows(self, shape, intrinsics: torch.Tensor, lidar2img: torch.Tensor, pad_shape, device, topk_indexes=None):
        """:meth:`forward` on token rows that already sit in :meth:`feat_workspace` of ``shape`` = (B, N, h, w): no NCHW tensor is read, copied or
        transposed (no ``toc3d_nchw_to_rows``); every other launch, and every bit, is :meth:`forward`'s."""
        B, N, h, w = (int(v) for v in shape)
        return self._forward(None, (B, N, h, w), torch.device(device), intrinsics, lidar2img, pad_shape, topk_indexes)

    def _index(self, topk_indexes, B, LEN):
        """``topk_indexes`` (B, K, 1) or (B, K) int64 on the device -> contiguous (B, K).  Values are not read here: the kernels clamp them into [0, LEN - 1]."""
        t = topk_indexes
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"{self._NAME}: topk_indexes must be a CUDA/HIP tensor -- the HIP extension is the only compute path (no CPU fallback)")
        if t.dim() == 3 and t.shape[2] == 1:
            t = t[:, :, 0]
        if t.dtype != torch.int64 or t.dim() != 2 or t.shape[0] != B:
            raise ValueError(f"{self._NAME}: topk_indexes {tuple(topk_indexes.shape)} {topk_indexes.dtype} is not int64 (B, K, 1) or (B, K) with B = {B}")
        if not 0 < t.shape[1] <= LEN:
            raise ValueError(f"{self._NAME}: topk_indexes lists K = {t.shape[1]} tokens per sample: 0 < K <= N*h*w = {LEN}")
        return t.contiguous()

    @torch.no_grad()
    def forward(self, img_feats: torch.Tensor, intrinsics: torch.Tensor, lidar2img: torch.Tensor, pad_shape, topk_indexes=None):
        """img_feats (B, N, C, h, w) f32 (neck level 0, ``data['img_feats']`` :626); intrinsics / lidar2img (B, N, 4, 4);
        pad_shape = (pad_h, pad_w[, 3]) of ``img_metas[0]['pad_shape'][0]``.  Returns (memory, pos_embed, cone): memory and pos_embed
        f32 (B, N*h*w, embed_dims), cone f32 (B, N*h*w, 8) (:419-421) -- all three freshly allocated, none aliases a workspace.
        ``topk_indexes`` (B, K, 1) or (B, K) int64 on the device, as ``FocalHead`` returns it: the three outputs hold the K listed tokens of every sample, in the
        list's order -- (B, K, embed_dims) and (B, K, 8); ``None``: every token, by today's launches."""
        require_cuda(self._NAME, img_feats)
        B, N, C, h, w = img_feats.shape
        if C != self.in_channels:
            raise ValueError(f"{self._NAME}: img_feats {tuple(img_feats.shape)} do not fit in_channels={self.in_channels}")
        return self._forward(img_feats, (B, N, h, w), img_feats.device, intrinsics, lidar2img, pad_shape, topk_indexes)

    def _forward(self, img_feats, shape, dev, intrinsics, lidar2img, pad_shape, topk_indexes=None):
        (B, N, h, w), C = shape, self.in_channels
        LEN = N * h * w
        index = None if topk_indexes is None else self._index(topk_indexes, B, LEN)
        Kt = LEN if index is None else index.shape[1]                    # token rows per sample
        with torch.cuda.device(dev):
            full = self._workspace((B, N, h, w), dev)                    # (its "feat": the full-token rows, sampled or not)
            W = full if index is None else self._workspace((B, N, h, w, Kt), dev)
            P = self._packed
            dt, rows = P["dt"], P["dts"].rows           # rows: the row kernels' output dtype -- the act dtype, or (hi, lo) planes on "fp32x3"
            E, D = self.embed_dims, self.depth_num
            M, s = B * Kt, lib.stream_ptr()
            memory = torch.empty(M, E, dtype=torch.float32, device=dev)
            pos_embed = torch.empty(M, E, dtype=torch.float32, device=dev)
            img2lidar = torch.linalg.inv(lidar2img.to(dev).float().reshape(B * N, 4, 4)).contiguous()
            intr = intrinsics.to(dev).float().reshape(B * N, 4, 4).contiguous()

            def linear(x, wb, out, n, k, f32_out=False, relu=False):
                wgt, b = wb
                if self.precision == "fp32x3":
                    # the GEMM family's own launcher: W in planes; A in planes for the four Linears a row kernel feeds -- the four with a ReLU behind them, which
                    # the epilogue applies --, plain f32 (the rows that epilogue left) for the Linear behind each.  Tiles by the query side's rule.
                    return self._linear(x, wb, out, M, n, wgt.shape[1], f32_out=f32_out, relu=relu, a_planes=relu)
                lib.call("toc3d_linear", dt, lib.EPI_RESIDUAL if f32_out else lib.EPI_BIAS, x, x.shape[1], wgt, wgt.shape[1], b, out, out.shape[1], None, 0, 0, None, None,
                         M, n, wgt.shape[1], 0, s)
                if relu:
                    lib.call("toc3d_relu_inplace", dt, out, out.numel(), s)

            # position_embeding :378-416
            coords_d = self.coords_d if self._coords_d_owner is None else self._coords_d_owner.detach().float().contiguous()
            if index is None:
                lib.call("toc3d_head_frustum_inputs", rows, img2lidar, intr, coords_d, self._pr, B, N, h, w, D, self.stride, int(pad_shape[0]),
                         int(pad_shape[1]), W["pin"], W["pin"].shape[1], W["cone_a"], 64, W["cone"], s)
            else:                                       # topk_gather of the geometry (:386-389): the listed tokens' frustum points, nothing else
                lib.call("toc3d_head_frustum_inputs_sampled", rows, img2lidar, intr, coords_d, self._pr, index, B, N, h, w, Kt, D, self.stride, int(pad_shape[0]),
                         int(pad_shape[1]), W["pin"], W["pin"].shape[1], W["cone_a"], 64, W["cone"], s)
            linear(W["pin"], P["pe0"], W["h1"], 4 * E, 3 * D, relu=True)
            linear(W["h1"], P["pe2"], W["pos"], E, 4 * E, f32_out=True)
            # memory_embed :635
            if img_feats is not None:                   # (forward_rows: the rows are in W["feat"] already)
                lib.call("toc3d_nchw_to_rows", rows, img_feats.float().contiguous(), full["feat"], full["feat"].shape[1], B * N, C, h * w, s)
            if index is not None:                       # topk_gather of the feature rows (:632): full-token workspace -> this K's rows
                lib.call("toc3d_gather_token_rows", rows, full["feat"], full["feat"].shape[1], index, B, LEN, Kt, C, W["feat"], W["feat"].shape[1], s)
            linear(W["feat"], P["me0"], W["m1"], E, C, relu=True)
            linear(W["m1"], P["me2"], W["mem_raw"], E, E, f32_out=True)
            # spatial_alignment :638
            linear(W["cone_a"], P["red"], W["c1"], E, 8, relu=True)
            linear(W["c1"], P["gam"], W["gam"], E, E, f32_out=True)
            linear(W["c1"], P["bet"], W["bet"], E, E, f32_out=True)
            lib.call("toc3d_mln_apply", rows, W["mem_raw"], W["gam"], W["bet"], M, E, memory, W["mem_a"], W["mem_a"].shape[1], s)
            # featurized_pe :639
            linear(W["mem_a"], P["se1"], W["s1"], E, E, relu=True)
            linear(W["s1"], P["se2"], W["se"], E, E, f32_out=True)
            lib.call("toc3d_se_gate", W["pos"], W["se"], pos_embed, M * E, s)
            cone = W["cone"].clone()
        return memory.view(B, Kt, E), pos_embed.view(B, Kt, E), cone.view(B, Kt, 8)
