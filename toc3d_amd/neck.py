"""Drop-in ``CPFPN`` neck (reference ``projects/mmdet3d_plugin/models/necks/cp_fpn.py:16-208``) on the HIP kernels.

Built for the configuration every shipped config uses (``ToC3D_faster.py:70-74``): one input level,
``num_outs=2``, no norm / activation, no extra convs: 1x1 lateral conv -> 3x3 conv (pad 1) -> stride-2
subsample as the extra level.  Both convs run as MFMA GEMMs on the NHWC buffer the backbone already holds
(no permute); the output is materialised as contiguous NCHW f32 because ``Petr3D.extract_img_feat`` calls
``.view(B, N, C, H, W)`` on it (``petr3d.py:239``).  State-dict names follow mmcv's ConvModule
(``lateral_convs.0.conv.weight`` ...).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import gemm, lib
from .plan import MODES, DerivedState, lru, run_frame


class _ConvModule(nn.Module):
    def __init__(self, cin, cout, k, padding=0):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, k, padding=padding)


class CPFPN(DerivedState, nn.Module):
    def __init__(self, in_channels, out_channels, num_outs, start_level=0, end_level=-1, add_extra_convs=False,
                 relu_before_extra_convs=False, no_norm_on_lateral=False, conv_cfg=None, norm_cfg=None, act_cfg=None,
                 upsample_cfg=dict(mode="nearest"), init_cfg=None, precision=None, **unused):
        super().__init__()
        assert isinstance(in_channels, list)
        if (len(in_channels) != 1 or start_level != 0 or end_level != -1 or add_extra_convs or norm_cfg is not None
                or act_cfg is not None or conv_cfg is not None or num_outs not in (1, 2)):
            raise NotImplementedError("CPFPN is built for the shipped single-level configuration (in_channels=[C], num_outs<=2)")
        if precision is None:
            precision = gemm.DEFAULT_PRECISION                         # the path that meets the reference's 1e-3 (gemm.py); bf16 is an explicit opt-in
        assert precision in ("bf16", "fp32", "fp32x3", "fp32x6")
        self.in_channels, self.out_channels, self.num_outs = in_channels, out_channels, num_outs
        self.precision = precision
        self.fp16_enabled = False
        self.lateral_convs = nn.ModuleList([_ConvModule(in_channels[0], out_channels, 1)])
        self.fpn_convs = nn.ModuleList([_ConvModule(out_channels, out_channels, 3, padding=1)])
        for m in self.modules():                                    # init_cfg Xavier uniform (cp_fpn.py:80-81)
            if isinstance(m, nn.Conv2d):
                nn.init.xavier_uniform_(m.weight)
                nn.init.zeros_(m.bias)
        self._drop_derived()
        self._tuned = {}                # (epilogue, M, N, K) -> GEMM tile variant (toc3d_amd.gemm.linear); bench.py shares the backbone's table
        self.autotune = True
        self.alias_outputs = False      # True: the returned level-0 tensor is the reused workspace (benchmarks, fused pipelines)
        self.launch_mode = unused.get("launch_mode", "plan")            # see toc3d_amd/plan.py
        assert self.launch_mode in MODES
        self._stream_pool = []

    # packed weights, workspaces and the recorded launch plans inside them are derived state (plan.DerivedState): weights that arrive through the
    # parent detector (mmcv load_checkpoint -> detector.load_state_dict) reach this module only in _load_from_state_dict, which drops them too
    _DERIVED = dict(_packed=None, _ws={}, _sk_ws={}, _sk_ws_old=[])
    _INSTANCE = dict(_stream_pool=[])

    def _pack(self, dev):
        dts = gemm.dtypes(self.precision)
        lw = self.lateral_convs[0].conv
        fw = self.fpn_convs[0].conv
        P = dict(dt=dts.act, tdt=dts.torch,
                 w_lat=gemm.pack_weight(lw.weight.reshape(self.out_channels, -1), dts, dev), b_lat=lw.bias.detach().float().contiguous(),
                 # (Cout, Cin, ky, kx) -> (Cout, ky, kx, Cin) to match toc3d_im2col_3x3's column order
                 w_fpn=gemm.pack_weight(fw.weight.permute(0, 2, 3, 1).reshape(self.out_channels, -1), dts, dev), b_fpn=fw.bias.detach().float().contiguous())
        torch.cuda.current_stream().synchronize()
        return P

    @torch.no_grad()
    def forward(self, inputs):
        return self._forward(inputs, None)

    @torch.no_grad()
    def forward_fanout(self, inputs, rows, ld_rows, dtype):
        """``forward`` with the conv rows fanned out (``toc3d_neck_rows_fanout`` in place of ``toc3d_nhwc_to_nchw``): the same NCHW outputs, bit for bit, and
        in the same launch the level-0 token rows ``rows`` [V*h*w, ld_rows] in the C ABI's ``dtype`` (``lib.BF16`` / ``F32`` / ``F32X3P``) -- what
        ``toc3d_nchw_to_rows`` would make of the NCHW tensor; columns from ``out_channels`` on are left as they are.  ``rows`` is the consumer's own buffer
        (:meth:`toc3d_amd.HeadTokenEmbedding.feat_workspace`): a recorded plan names it, like the input."""
        if not (isinstance(rows, torch.Tensor) and rows.is_cuda and rows.dim() == 2 and rows.is_contiguous() and rows.shape[1] == ld_rows):
            raise ValueError("toc3d_amd.CPFPN.forward_fanout: rows must be a contiguous 2-D device tensor whose row length is ld_rows")
        return self._forward(inputs, (rows, int(ld_rows), int(dtype)))

    def conv_rows(self, V, h, w):
        """``(rows, ld)``: the level-0 conv's own output rows [V*h*w, out_channels], plain f32 on every precision, of the last forward at this shape -- what the
        fan-out transposes.  A consumer that reads plain f32 token rows (``FocalHead`` on ``"fp32x3"``) takes them from here.  Valid until the next forward."""
        ws = self._ws.get((V, h, w))
        if ws is None:
            raise RuntimeError(f"toc3d_amd.CPFPN.conv_rows: no forward has run at V, h, w = {V}, {h}, {w}")
        return ws["o0"], ws["o0"].shape[1]

    def _forward(self, inputs, fan):
        assert len(inputs) == len(self.in_channels)
        feat = inputs[0]
        if not feat.is_cuda:
            raise RuntimeError("toc3d_amd.CPFPN: input must be a CUDA/HIP tensor (no CPU fallback)")
        V, Cin, h, w = feat.shape
        nhwc = feat.permute(0, 2, 3, 1)
        nhwc = nhwc if nhwc.is_contiguous() else nhwc.contiguous()      # zero-copy when fed by the toc3d_amd backbone
        nhwc = nhwc.float()
        dev = feat.device
        if self._packed is None:
            self._packed = self._pack(dev)
        P = self._packed
        dt, tdt = P["dt"], P["tdt"]
        M, Co = V * h * w, self.out_channels
        key = (V, h, w)
        if key not in self._ws:
            Kl, Kf = P["w_lat"].shape[1], P["w_fpn"].shape[1]
            implicit = Co % 64 == 0                      # the implicit-GEMM conv needs whole 64-channel K-tiles per tap; otherwise im2col + GEMM
            self._ws[key] = dict(a=torch.zeros(M, Kl, dtype=tdt, device=dev), implicit=implicit,
                                 lat=torch.empty(M, Co, dtype=tdt if implicit else torch.float32, device=dev),
                                 col=None if implicit else torch.zeros(M, Kf, dtype=tdt, device=dev),
                                 zeros=torch.zeros(256, dtype=torch.uint8, device=dev), o0=torch.empty(M, Co, dtype=torch.float32, device=dev),
                                 out0=torch.empty(V, Co, h, w, dtype=torch.float32, device=dev))
        ws = self._ws[key]
        Kl, Kf = ws["a"].shape[1], P["w_fpn"].shape[1]

        def frame(ex):
            s = lib.stream_ptr()
            if dt == lib.F32 and Kl == Cin:
                a = nhwc.reshape(M, Cin)
            else:
                a = ws["a"]
                lib.call("toc3d_pack_weight", dt, nhwc, M, Cin, a, M, Kl, s)           # f32 -> act conversion with K padding
            # 1x1 lateral conv: a GEMM whose output stays in the act dtype (the reference's f32 lateral is rounded once on its way into the 3x3
            # conv either way); 3x3 conv: an IMPLICIT GEMM (toc3d_conv3x3_nhwc) -- the operand loader gathers the nine neighbours of every pixel, the
            # [M, 9*C] im2col matrix (27 MB per frame, one launch) is gone.  Both with a per-shape autotuned tile (N = 256 leaves 94 tiles of
            # 128x128 for 256 CUs: the default tile is the wrong one).
            if ws["implicit"]:
                gemm.linear(self, lib.EPI_BIAS, a, P["w_lat"], P["b_lat"], ws["lat"], M, Co, Kl)
                gemm.linear(self, lib.EPI_CONV3X3, ws["lat"], P["w_fpn"], P["b_fpn"], ws["o0"], M, Co, Kf, conv=(ws["zeros"], h, w))
            else:                                        # channel counts that are not multiples of 64 (test configs): materialised im2col rows
                gemm.linear(self, lib.EPI_RESIDUAL, a, P["w_lat"], P["b_lat"], ws["lat"], M, Co, Kl)
                lib.call("toc3d_im2col_3x3", dt, ws["lat"], ws["col"], Kf, V, h, w, Co, s)
                gemm.linear(self, lib.EPI_RESIDUAL, ws["col"], P["w_fpn"], P["b_fpn"], ws["o0"], M, Co, Kf)
            if fan is None:
                lib.call("toc3d_nhwc_to_nchw", ws["o0"], ws["out0"], V, h * w, Co, s)
            else:
                lib.call("toc3d_neck_rows_fanout", fan[2], ws["o0"], Co, ws["out0"], fan[0], fan[1], V, h * w, Co, s)

        # The launch sequence names the input buffer: it can be recorded (and replayed with one C call) only for an input that sits
        # at a fixed address and is read in place -- the toc3d_amd backbone's own output buffer.  Anything else launches eagerly.
        in_place = nhwc.data_ptr() == feat.data_ptr() and feat.dtype == torch.float32
        if fan is not None and fan[0].shape[0] != M:
            raise ValueError(f"toc3d_amd.CPFPN.forward_fanout: rows has {fan[0].shape[0]} rows, the frame has {M} tokens")
        if in_place:
            skey = nhwc.data_ptr() if fan is None else (nhwc.data_ptr(), fan[0].data_ptr(), fan[1], fan[2])       # the fanned-out frame names the rows buffer too
            state = lru(ws.setdefault("launch", {}), skey, dict, 4)
            if fan is not None:
                state["rows"] = fan[0]                  # a recorded plan points into it: it lives as long as the plan does, whatever its owner does
            run_frame(state, self.launch_mode, 1, frame, self._stream_pool)
        else:
            run_frame({}, "eager", 1, frame, self._stream_pool)
        out0 = ws["out0"] if self.alias_outputs else ws["out0"].clone()
        outs = [out0]
        if self.num_outs > 1:
            outs.append(out0[:, :, ::2, ::2])          # F.max_pool2d(k=1, stride=2) == strided subsample (cp_fpn.py:187)
        return tuple(outs)
