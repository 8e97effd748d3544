"""How the host drives the library's GEMM family (``toc3d_linear_fused``, ``toc3d_linear_fused_ws``, ``toc3d_linear_qkv_rope``; ``include/toc3d.h``): the one
place that maps a precision to the ABI's dtype codes, packs a weight the way the GEMMs read it, picks a tile variant per shape and lays the arguments out in
header order.  Backbone, neck, decoder and the head-token module import from here; ``lib.call`` stays the only gate to the library.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import lib

# What a reference config dropped in UNCHANGED gets (no `precision` key): the fastest path that meets the reference's own tolerance -- north_star's
# 1e-3 relative on the fp32 feature maps (tools/test.py:204-206 runs the reference in fp32): "fp32x3" (f32 buffers, every contraction as three bf16 MFMAs on (hi, lo)
# operand splits: 3e-5 rel. max on the full-size goldens, ~0.5x the bf16 path's frames/s).  "bf16" -- BASELINE.json configs[1], the benchmarked headline: rel. L2
# 1.3e-2 with the reference's token selection forced, like a torch-bf16 run of the reference -- is an explicit opt-in (`precision="bf16"` in the config dict);
# "fp32" = exact-f32 MFMA (5e-6), "fp32x6" = f32-grade products from six bf16 MFMAs.  INTEGRATION.md, "Precision".
DEFAULT_PRECISION = "fp32x3"


def round_up(a: int, b: int) -> int:
    return (a + b - 1) // b * b


# ------------------------------------------------------------------------------------------------
# precision -> dtype codes
# ------------------------------------------------------------------------------------------------
class Dtypes(NamedTuple):
    act: int                # lib dtype of the activation / packed-weight buffers: BF16, or F32 on every f32-buffer precision
    torch: torch.dtype      # ... and its torch twin
    gemm: int               # arithmetic of the linear layers: "fp32x3" keeps every buffer in f32 and forms the GEMM products as three bf16 MFMAs on the operands'
                            # (hi, lo) splits (include/toc3d.h TOC3D_DTYPE_F32X3; F32X3W with the weights stored as planes) -- the parity-grade path at a third of
                            # the bf16 MFMA rate instead of a sixteenth
    rows: int               # dtype handed to the row kernels that produce a GEMM's A operand (LayerNorm / gather / rebase, the f32 attention): f32 arithmetic
                            # either way, the output rows as (hi, lo) planes when x3p (TOC3D_DTYPE_F32X3P)
    attn: int               # dtype of the f32-buffer window attention: exact f32 products or, with x3_attention, bf16 x 3 products; output rows plain or as planes
    x3p: bool               # fp32x3 with its GEMM operands as (hi, lo) planes (schedule switch x3_planes)


def attn_dtype(precision, x3_attention, planes_out):
    """dtype of an attention launch on ``precision``: on fp32x3, (bf16 x 3 products?, output rows as planes?) -> F32 / F32X3WO / F32X3 / F32X3P."""
    if precision != "fp32x3":
        return lib.BF16 if precision == "bf16" else lib.F32
    return {(False, False): lib.F32, (False, True): lib.F32X3WO, (True, False): lib.F32X3, (True, True): lib.F32X3P}[(bool(x3_attention), bool(planes_out))]


def dtypes(precision, x3_planes=True, x3_attention=True) -> Dtypes:
    """Every dtype code a module on ``precision`` hands to the library.  ``x3_planes`` / ``x3_attention``: the backbones' schedule switches of the same names
    (they only matter on "fp32x3"; a module without them runs with planes)."""
    act = lib.BF16 if precision == "bf16" else lib.F32
    x3p = precision == "fp32x3" and bool(x3_planes)
    gemm = {"fp32x3": lib.F32X3W if x3p else lib.F32X3, "fp32x6": lib.F32X6}.get(precision, act)
    return Dtypes(act, torch.bfloat16 if precision == "bf16" else torch.float32, gemm, lib.F32X3P if x3p else act, attn_dtype(precision, x3_attention, x3p), x3p)


def dtypes_of(owner) -> Dtypes:
    return dtypes(owner.precision, getattr(owner, "x3_planes", True), getattr(owner, "x3_attention", True))


def launch_dtype(gemm, a_planes, o_planes, rope=False):
    """The dtype of one GEMM launch.  fp32x3 on (hi, lo) planes (gemm == F32X3W): W always; A when its producer wrote planes; the SwiGLU hidden units / out_act
    when the consuming GEMM reads planes.  EPI_QKV_ROPE: the rotated rows always leave as planes (toc3d_window_attention_rot stages them by DMA)."""
    if gemm != lib.F32X3W:
        return gemm
    return {(False, False): lib.F32X3W, (True, False): lib.F32X3WA, (False, True): lib.F32X3WO, (True, True): lib.F32X3P}[(bool(a_planes), bool(o_planes) or rope)]


# ------------------------------------------------------------------------------------------------
# weight packing
# ------------------------------------------------------------------------------------------------
def planes(w, dts: Dtypes):
    """fp32x3 with x3_planes: a packed f32 weight -> (hi, lo) bf16 planes, in place (include/toc3d.h, TOC3D_DTYPE_F32X3W): the GEMM then DMAs the planes
    instead of splitting the W tile in LDS in every workgroup of every launch."""
    if dts.x3p:
        lib.call("toc3d_x3_planes", w, w.shape[1], w, w.shape[1], w.shape[0], w.shape[1], lib.stream_ptr())
    return w


def pack_weight(w: torch.Tensor, dts: Dtypes, device=None):
    """f32 [N, K] -> act [ceil128(N), ceil64(K)] via the C ABI, on ``device`` (default: where ``w`` lives); as planes when ``dts.x3p``."""
    w = w.detach().float().contiguous()
    if device is not None:
        w = w.to(device)
    N, K = w.shape
    out = torch.empty(round_up(N, 128), round_up(K, 64), dtype=dts.torch, device=w.device)
    lib.call("toc3d_pack_weight", dts.act, w, N, K, out, out.shape[0], out.shape[1], lib.stream_ptr())
    return planes(out, dts)


class Packer:
    """What a module's ``_pack`` turns parameters into device operands with, for one precision (``dts``) and device."""

    def __init__(self, dts: Dtypes, dev):
        self.dts, self.dev = dts, dev

    def f32(self, t):
        return t.detach().float().contiguous().to(self.dev)

    def wb(self, w, b):
        """f32 [N, K] weight and [N] bias -> (packed weight, f32 bias)."""
        return pack_weight(w, self.dts, self.dev), self.f32(b)

    def linear(self, *layers):
        """``nn.Linear`` layers of one K, concatenated along N -> (packed weight, f32 bias)."""
        return self.wb(torch.cat([l.weight.detach() for l in layers]), torch.cat([l.bias.detach() for l in layers]))

    def layernorm(self, m):
        return self.f32(m.weight), self.f32(m.bias), float(m.eps)


# ------------------------------------------------------------------------------------------------
# the launcher
SPLITK_VARIANT = 4014     # four K slices on 64x64 tiles, added in slice order (include/toc3d.h, the fused GEMM's split-K entry point)


def small_m_variant(M, N, K, residual):
    """GEMM tile variant (include/toc3d.h, toc3d_linear_ex) for a query-side GEMM (the decoder's, the head branches').  These have M = 900 .. 5400 rows: the
    library's default 128x128 tile makes 16 workgroups of the M = 900, N = 256 ones on a 256-CU chip.  Measured at M = 900 (profiles/decoder_gemm_small_m.txt):
    64x64 tiles (variant 14) win every shape of fewer than 256 default tiles in fp32x3 and tie in bf16; the FFN's second layer (K = 2048 into N = 256) wants the K
    dimension cut as well -- 62 -> 18 us (fp32x3), 22 -> 11 us (bf16) with the deterministic four-way split-K.  0 = the library's heuristic (the M = 6000 key /
    value projections)."""
    if ((M + 127) // 128) * ((N + 127) // 128) >= 256:
        return 0
    if residual and K >= 1024 and K % 512 == 0:
        return SPLITK_VARIANT
    return 14


# ------------------------------------------------------------------------------------------------
_flush = None                  # 256 MB scratch shared by all models: evicts L2 + Infinity Cache between tuning launches

# + 100: 8 row bands per XCD.  The 2-D XCD partitions (+ 200 / + 300, round 3) win 6-20 % on isolated cold w1|w2 / w3 launches and nothing inside the frame
# (profiles/r03_xcd_order_sweep.txt): they stay available through the C ABI but are not tuning candidates.
_VARIANTS = {lib.BF16: (1, 8, 9, 10, 13, 14, 15, 16, 17, 19, 22, 24, 26, 27, 28, 29, 30, 33, 45, 47, 49, 51, 52, 53, 54, 55, 56, 57, 58, 59, 60, 61, 62, 63, 110, 114, 116, 117, 126, 145, 147, 149, 151, 152,
                        154, 155, 156, 158, 159, 160, 161, 163),
             lib.F32: (1, 8, 9, 10, 13, 14, 16, 17, 22, 26, 28, 33, 110, 126),
             lib.F32X3: (1, 8, 9, 10, 14, 16, 17, 19, 22, 26, 28, 29, 33, 45, 47, 49, 52, 53, 110, 114, 116, 117, 122, 126, 129, 145, 147, 149, 152)}
# the phased big tiles on planes (round 6) need BOTH operands in planes: candidates of TOC3D_DTYPE_F32X3P only
_VARIANTS_X3P = _VARIANTS[lib.F32X3] + (54, 55, 56, 57, 58, 59, 60, 61, 62, 63, 154, 155, 156, 158, 159, 160, 161, 162, 163)      # (54-59: the 96- / 160-row tiles, planes only too)
_VARIANTS[lib.F32X6] = _VARIANTS[lib.F32X3W] = _VARIANTS[lib.F32X3WO] = _VARIANTS[lib.F32X3WA] = _VARIANTS[lib.F32X3]
_VARIANTS[lib.F32X3P] = _VARIANTS_X3P


def _tune(dtg, epi, call, out, ldo, rep_out, M):
    """The fastest tile / pipeline variant for this launch, measured on its real operands; ``call(variant, out, rep_out)`` issues it."""
    global _flush
    o = out
    if epi in (lib.EPI_RESIDUAL, lib.EPI_RESIDUAL_LN, lib.EPI_RESIDUAL_STATS):   # in-place residual add: tune into scratch
        o = torch.empty(M, ldo, dtype=torch.float32, device=out.device)
    rep_s = torch.empty_like(rep_out) if rep_out is not None else None
    cands = _VARIANTS[dtg]
    # what launch_cfg (csrc/gemm_kernels.h) refuses, read off the tile's geometry
    bn, wn = (lambda v: lib.TILES[v % 100][1]), (lambda v: lib.TILES[v % 100][3])
    if epi in (lib.EPI_SWIGLU, lib.EPI_SWIGLU_STATS, lib.EPI_SWIGLU_STATS_LN):
        cands = [v for v in cands if (bn(v) // wn(v)) % 32 == 0]     # a wavefront owns whole (w1, w2) 32-column groups
    if epi in (lib.EPI_SWIGLU_STATS, lib.EPI_SWIGLU_STATS_LN):
        cands = [v for v in cands if bn(v) % 128 == 0]               # statistics slots are 128 packed columns
    # Inside the block sequence every GEMM starts on cold operands (the previous kernels streamed tens of MB through
    # L2 / Infinity Cache): time single launches behind a cache-sized memset, not a warm back-to-back loop, or the
    # tuner prefers shallow pipelines that lose in place (tools/ubench/n1024_all_variants.py).
    if _flush is None or _flush.device != out.device:
        _flush = torch.empty(64 * 1024 * 1024, dtype=torch.float32, device=out.device)

    def cold_time(v, reps):
        try:
            call(v, o, rep_s)
        except RuntimeError:                             # a tile variant that cannot serve this epilogue
            return float("inf")
        ts = []
        for _ in range(reps):
            _flush.zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call(v, o, rep_s)
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return min(ts)
    # two passes: a quick one over every candidate, then the four best again with more samples (single cold launches
    # are noisy, and a wrong pick costs 10-20 % on that shape for the lifetime of the model)
    short = sorted((cold_time(v, 3), v) for v in cands)[:4]
    return min((cold_time(v, 9), v) for _, v in short)[1]


def _splitk_workspace(owner, need, device, stream):
    """One zeroed split-K workspace (arrival tickets + partial tiles; the launches re-arm the tickets) per owner and stream: launches on one lane share it."""
    pool = owner.__dict__.setdefault("_sk_ws", {})
    key = (device.index, stream)                      # (the default stream's handle is 0 on every device: ADVICE r05)
    ws = pool.get(key)
    if ws is None or ws.numel() * 4 < need:
        if ws is not None:
            owner.__dict__.setdefault("_sk_ws_old", []).append(ws)      # recorded plans may still name it
        ws = pool[key] = torch.zeros((need + 3) // 4, dtype=torch.int32, device=device)
    return ws


def linear(owner, epi, A, W, bias, out, M, N, K, *, lda=None, ldw=None, ldo=None, residual=None, ldr=0, residual_row_mod=0, rep_out=None, rep_index=None,
           n_valid=0, stats_out=(None, 0), stats_in=(None, 0, 0), col_sums=None, ln_n=0, ln_eps=0.0, out_act=None, ld_act=0, residual_index=None,
           conv=None, rope=None, a_planes=False, o_planes=False, variant=None):
    """One GEMM of the fused family, arguments named as in include/toc3d.h (leading dimensions default to the tensors' row lengths).  Grouped where the ABI packs
    them: ``stats_out=(buf, cap)``; ``stats_in=(buf, cap, slots_per_row)``; ``conv=(zero_line, h, w)`` of EPI_CONV3X3; ``rope=(rope_rc, rope_tab, rope_side,
    q_scale)`` of EPI_QKV_ROPE (toc3d_linear_qkv_rope).  ``a_planes`` / ``o_planes``: the A rows arrive / the act-dtype output leaves as (hi, lo) planes (fp32x3).
    ``EPI_BIAS_RELU`` takes what ``EPI_BIAS`` takes (its ``out`` is plain in the act dtype on every precision: a ReLU output that a planes GEMM multiplies
    goes in as plain f32, ``a_planes=False``).

    The tile / pipeline variant is ``variant`` when the caller decides it, else the fastest one for this (epilogue, M, N, K), measured once on the real operands
    the first time the shape is seen (never while a launch plan is being recorded: shapes are warmed up eagerly).  ``owner`` = the owner of that table and of the
    split-K workspaces: anything with ``_tuned`` (dict), ``autotune`` (bool) and ``precision`` (the backbones, the neck; the decoder passes ``variant``).
    All unsplit variants accumulate K in the same order, so the choice does not change results."""
    dtg = launch_dtype(dtypes_of(owner).gemm, a_planes, o_planes, rope=epi == lib.EPI_QKV_ROPE)
    lda, ldw, ldo = (A.shape[1] if lda is None else lda), (W.shape[1] if ldw is None else ldw), (out.shape[1] if ldo is None else ldo)
    s = lib.stream_ptr()
    var = owner._tuned.get((epi, M, N, K)) if variant is None else variant
    if epi == lib.EPI_QKV_ROPE:
        # the rotating epilogue costs what the bias epilogue costs: it shares that epilogue's tile table (no second tuning sweep)
        if var is None:
            var = owner._tuned.get((lib.EPI_BIAS, M, N, K), 0)
        lib.call("toc3d_linear_qkv_rope", dtg, var, A, lda, W, ldw, bias, out, ldo, M, N, K, *rope, s)
        return
    if conv is not None:
        out_act, ld_act = conv[0], (conv[1] << 32) | conv[2]

    def args(v, o, rep):
        return (dtg, epi, v, A, lda, W, ldw, bias, o, ldo, residual, ldr, residual_row_mod, rep, rep_index, M, N, K, n_valid,
                stats_out[0], stats_out[1], stats_in[0], stats_in[1] | stats_in[2] << 32, col_sums, ln_n, ln_eps, out_act, ld_act, residual_index)
    if var is None:
        var = 0
        if lib.recording():
            # a shape first seen while recording (the eager warm-up forward normally tunes every shape): heuristic tile, no timing
            lib.call("toc3d_linear_fused", *args(0, out, rep_out), s)
            return
        if owner.autotune and not torch.cuda.is_current_stream_capturing():
            var = _tune(dtg, epi, lambda v, o, rep: lib.call("toc3d_linear_fused", *args(v, o, rep), s), out, ldo, rep_out, M)
        owner._tuned[(epi, M, N, K)] = var
    if var >= 1000:
        # a deterministic split-K pick (include/toc3d.h, toc3d_linear_fused_ws; only a table or the caller can name one: the tuner's candidates are the unsplit
        # variants -- measured slower on every launch of the backbone's frame, profiles/r05_splitk.txt)
        ws = _splitk_workspace(owner, int(lib.load().toc3d_linear_splitk_workspace_bytes(var, M, N)), out.device, s)
        lib.call("toc3d_linear_fused_ws", *args(var, out, rep_out), ws, ws.numel() * 4, s)
        return
    lib.call("toc3d_linear_fused", *args(var, out, rep_out), s)
