"""Drop-in ``ToC3DEVAViT`` / ``EVA_ViT`` backbones whose forward runs on the gfx950 HIP kernels.

Host-side mirror of the reference's backbone interface (same class names, constructor kwargs, forward
signature, return type and state-dict names):

* ``ToC3DEVAViT``  <- ``projects/mmdet3d_plugin/models/backbones/toc3d_eva_vit.py:25-326``
* ``EVA_ViT``      <- ``projects/mmdet3d_plugin/models/backbones/eva_vit.py:270-428``
* ``ToC3DViTReturnType`` <- ``.../backbones/toc3d_utils.py:10-25``

The modules only *hold* parameters (so a reference ``.pth`` loads unchanged) and sequence calls into the
C ABI (``include/toc3d.h``); no torch op touches activations on the hot path.  PyTorch is used for device
memory, streams and parameter bookkeeping only.  There is no CPU fallback: a non-CUDA input raises.

Extra (non-reference) constructor kwarg: ``precision`` = ``"bf16"`` (bf16 MFMA operands, f32 accumulate,
f32 residual stream), ``"fp32"`` (exact-f32 MFMA, the strict-parity path) or ``"fp32x3"`` (f32 buffers everywhere, the linear
layers' products as three bf16 MFMAs on (hi, lo) operand splits: parity-grade at several times the fp32 path's speed).
``schedule`` = dict of overrides of the launch-schedule attributes of ``schedule_defaults`` (A/B runs, tests); the defaults are the shipped schedule.
Extra forward kwarg: ``gumbel_noise`` (list of 3 tensors (B*Nv, T, 2)) to make the stochastic soft mask
(``toc3d_utils.py:147``) reproducible; when omitted the noise is drawn on the device like the reference does.
"""
from __future__ import annotations

import math
from functools import partial
from types import SimpleNamespace
from typing import Dict, NamedTuple, Optional

import torch
import torch.nn as nn

from . import gemm, lib
from .gemm import DEFAULT_PRECISION, round_up              # (DEFAULT_PRECISION: re-exported, the configs and tests read it from here)
from .plan import MODES, DerivedState, EagerExec, lru, run_frame
from .staged import MLN, dim_t
from .synth import MOTION_DIM, QUERY_DIM, rope_tables


class ToC3DViTReturnType:
    """Same fields as the reference's return type (``toc3d_utils.py:10-25``)."""

    def __init__(self, img_feats=None, token_masks=None, attn_scores=None, keep_idx=None, drop_idx=None,
                 aux_outputs: list = None) -> None:
        self.img_feats = img_feats
        self.token_masks = token_masks
        self.attn_scores = attn_scores
        self.keep_idx = keep_idx
        self.drop_idx = drop_idx
        self.aux_outputs = aux_outputs


def _return_type():
    """The class forward() returns.  ``Petr3D.extract_img_feat`` tests ``isinstance(out, ToC3DViTReturnType)`` against the class it
    imported from the reference plugin (``detectors/petr3d.py:17,159``): when that plugin module has been imported in this process
    (the detector did), its class is used, so the drop-in needs no manual re-binding; otherwise the local twin above."""
    import sys
    ref = sys.modules.get("projects.mmdet3d_plugin.models.backbones.toc3d_utils")
    cls = getattr(ref, "ToC3DViTReturnType", None) if ref is not None else None
    return cls if isinstance(cls, type) else ToC3DViTReturnType


# ------------------------------------------------------------------------------------------------
# parameter containers (reference state-dict naming; forward is never called on them)
# ------------------------------------------------------------------------------------------------
class _Rope(nn.Module):
    def __init__(self, side: int, half_head_dim: int, pt_seq_len: int):
        super().__init__()
        cos, sin = rope_tables(side, half_head_dim, pt_seq_len)
        self.register_buffer("freqs_cos", cos)
        self.register_buffer("freqs_sin", sin)


class _PatchEmbed(nn.Module):
    def __init__(self, in_chans, embed_dim, patch):
        super().__init__()
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=patch, stride=patch)


class _Attention(nn.Module):
    def __init__(self, dim, qkv_bias, rope):
        super().__init__()
        self.q_proj = nn.Linear(dim, dim, bias=False)
        self.k_proj = nn.Linear(dim, dim, bias=False)
        self.v_proj = nn.Linear(dim, dim, bias=False)
        if qkv_bias:
            self.q_bias = nn.Parameter(torch.zeros(dim))
            self.v_bias = nn.Parameter(torch.zeros(dim))
        else:
            self.q_bias = self.v_bias = None
        self.rope = rope
        self.proj = nn.Linear(dim, dim)


class _SwiGLU(nn.Module):
    def __init__(self, dim, hidden, norm_layer):
        super().__init__()
        self.w1 = nn.Linear(dim, hidden)
        self.w2 = nn.Linear(dim, hidden)
        self.ffn_ln = norm_layer(hidden)
        self.w3 = nn.Linear(hidden, dim)


class _Block(nn.Module):
    def __init__(self, dim, mlp_ratio, qkv_bias, norm_layer, rope):
        super().__init__()
        self.norm1 = norm_layer(dim)
        self.attn = _Attention(dim, qkv_bias, rope)
        self.norm2 = norm_layer(dim)
        self.mlp = _SwiGLU(dim, int(dim * mlp_ratio), norm_layer)


class _Scorer(nn.Module):
    """MotionAwareQueryGuidedTokenSelector parameters (toc3d_utils.py:99-112,216-224,321-332)."""

    def __init__(self, embed_dim, num_queries, ratio, pc_range):
        super().__init__()
        self.ratio = ratio
        q = QUERY_DIM
        self.in_conv = nn.Sequential(nn.LayerNorm(embed_dim), nn.Linear(embed_dim, embed_dim), nn.GELU())
        self.out_conv = nn.Sequential(nn.Linear(embed_dim, embed_dim // 2), nn.GELU(),
                                      nn.Linear(embed_dim // 2, embed_dim // 4), nn.GELU(),
                                      nn.Linear(embed_dim // 4, 2), nn.LogSoftmax(dim=-1))
        self.input_proj = nn.Sequential(nn.Linear(embed_dim, q))
        self.aggregate = nn.Sequential(nn.Linear(num_queries, 2), nn.LogSoftmax(dim=-1))
        self.pc_range = nn.Parameter(torch.tensor(pc_range, dtype=torch.float32), requires_grad=False)
        self.query_embedding = nn.Sequential(nn.Linear(q * 3 // 2, q), nn.ReLU(), nn.Linear(q, q))
        self.ego_pose_pe = MLN(MOTION_DIM, q, reset_parameters=True)
        self.ego_pose_queries = MLN(MOTION_DIM, q, reset_parameters=True)
        self.time_embedding = nn.Sequential(nn.Linear(q, q), nn.LayerNorm(q))


def _init_weights(m):
    """toc3d_eva_vit.py:219-228 / eva_vit.py:400-407."""
    if isinstance(m, nn.Linear):
        nn.init.trunc_normal_(m.weight, std=0.02)
        if m.bias is not None:
            nn.init.constant_(m.bias, 0)
    elif isinstance(m, nn.LayerNorm):
        nn.init.constant_(m.bias, 0)
        nn.init.constant_(m.weight, 1.0)


# ------------------------------------------------------------------------------------------------
# shared engine: weight packing + per-shape plan + the launch sequence
# ------------------------------------------------------------------------------------------------
class Windows(NamedTuple):
    """One window list as the attention launches take it (include/toc3d.h, toc3d_window_attention*), built once where its buffers are allocated: the static dense
    map of a window type (``plan["dense"][L]["win"]``: ``npad``, no ``count_k``) or a scorer stage's selection (``plan["sel"][(st, L)]["win"]``: ``count_k``, pads
    in the block's pad rows).  ``rc``: RoPE position of every row (the pre-rotated path); ``stride``: slots per window.  The dicts keep the same tensors."""
    rc: Optional[torch.Tensor]
    rows: torch.Tensor
    slots: torch.Tensor
    count_q: torch.Tensor
    count_k: Optional[torch.Tensor]
    npad: Optional[torch.Tensor]
    stride: int
    nwin: int
    max_count: int


def schedule_defaults(precision):
    """The launch-schedule switches of the backbones and their shipped defaults per precision.  Plain attributes (``model.fold_norm2 = False`` before the
    first forward, or ``schedule=dict(...)`` at construction); every one is pinned by a test (tests/test_gpu_e2e.py, tests/test_cpu_abi.py).  The
    experiments of rounds 2-3 that lost (LayerNorm statistics in the consuming K loop, scatter folded into the next gather, prefetch across the frame
    boundary, lighter event fences) are gone from the tree since round 6: LABNOTES.md keeps their measurements, the git history their kernels."""
    bf16 = precision == "bf16"
    fast = precision in ("bf16", "fp32x3")
    return dict(
        x3_attention=precision == "fp32x3",  # fp32x3: the attention's two contractions as bf16 x 3 products too (f32 RoPE / softmax / accumulation; TOC3D_DTYPE_F32X3 of toc3d_window_attention)
        x3_planes=precision == "fp32x3",   # fp32x3: packed weights, the GEMMs' A operands and the GEMM-to-GEMM activations as (hi, lo) bf16 planes (TOC3D_DTYPE_F32X3W / F32X3P)
        carry_compact=fast,          # consecutive accelerated blocks of one window type continue on the same compact rows (_accel_block)
        fold_ffn_ln=fast,            # SwiGLU.ffn_ln folded across the w1|w2 -> w3 GEMM boundary (include/toc3d.h, the fused GEMM's LayerNorm epilogues)
        fold_norm2=fast,             # norm2 folded across the attention-projection -> w1|w2 boundary the same way
        gathered_residual=True,      # the gather skips the f32 copy of the kept rows; the projection GEMM reads their residual from x through crow_tok
        prefetch_weights=192 if bf16 else 0,   # workgroups of each attention launch that pull the next GEMMs' weights towards the chip (0 = off)
        attn_rot=fast,               # RoPE + q scale in the q|k|v GEMM epilogue, attention on the pre-rotated buffer with K / V staged by DMA (fp32x3, round 6: on (hi, lo)
                                     # planes -- needs x3_planes; both contractions as bf16 x 3 products, f32 softmax statistics and accumulation)
        gather_split=False,          # True / 2 / 8 / 16: every window's merge_tokens cut over 4 / 2 / 8 / 16 workgroups (toc3d_gather_merge_ln_split, same bits as the
                                     # single-workgroup form).  Round 4, built on the theory that one CU's load path bounds the merge -- measured: the launch is a chain
                                     # of dependent round trips, not bandwidth (12-17 us either way, profiles/r04_gather_split.txt), +-0.5 % in the frame: off
        side_lanes=True,             # scorer query prep and rankings on lanes beside the block chain (False: on the chain's own lane)
        big_windows_first=True,      # dense attention windows ordered biggest-first in the static window lists
        launch_mode="plan",          # "plan" (recorded launch plan replayed from C), "graph" (explicit hipGraph), "eager"
    )


class _BackboneBase(DerivedState, nn.Module):
    LN_EPS = 1e-6            # norm_layer=partial(nn.LayerNorm, eps=1e-6), toc3d_eva_vit.py:38
    SCORER_LN_EPS = 1e-5     # nn.LayerNorm default inside the scorers

    def _setup_common(self, img_size, patch_size, in_chans, embed_dim, depth, num_heads, mlp_ratio, qkv_bias,
                      use_abs_pos, pt_hw_seq_len, window_size, global_window_size, global_attn_indexes,
                      pretrain_img_size, pretrain_use_cls_token, out_feature, precision, img_norm_cfg=None, pad_size_divisor=32, schedule=None):
        assert precision in ("bf16", "fp32", "fp32x3", "fp32x6"), precision
        # uint8 boundary: with img_norm_cfg (the config's dict(mean, std, to_rgb), ToC3D_faster.py:13-14)
        # forward() also accepts raw uint8 HWC camera images and applies NormalizeMultiviewImage + PadMultiViewImage
        # (datasets/pipelines/transform_3d.py:87-100,38-50) inside the patch-embedding im2col
        self.img_norm_cfg = None
        if img_norm_cfg is not None:
            self.img_norm_cfg = dict(mean=torch.tensor(list(img_norm_cfg["mean"]), dtype=torch.float32),
                                     std=torch.tensor(list(img_norm_cfg["std"]), dtype=torch.float32),
                                     to_rgb=bool(img_norm_cfg.get("to_rgb", True)))
            assert self.img_norm_cfg["mean"].numel() == 3 and self.img_norm_cfg["std"].numel() == 3
        self.pad_size_divisor = int(pad_size_divisor)
        assert self.pad_size_divisor % patch_size == 0, "PadMultiViewImage divisor must be a multiple of the patch size"
        if embed_dim // num_heads != 64 or embed_dim % num_heads:
            raise NotImplementedError("the HIP attention kernel is built for head_dim 64 (EVA-02 L/B/tiny test config)")
        if embed_dim % 64 or embed_dim > 1024:
            raise NotImplementedError("embed_dim must be a multiple of 64 and <= 1024")
        self.precision = precision
        self.embed_dim, self.depth, self.num_heads = embed_dim, depth, num_heads
        self.patch_size, self.in_chans = patch_size, in_chans
        self.window_size, self.global_window_size = window_size, global_window_size
        self.global_attn_indexes = tuple(global_attn_indexes)
        self.pretrain_use_cls_token = pretrain_use_cls_token
        self.hidden_dim = int(embed_dim * mlp_ratio)
        self.patch_embed = _PatchEmbed(in_chans, embed_dim, patch_size)
        if use_abs_pos:
            npatch = (pretrain_img_size // patch_size) ** 2
            self.pos_embed = nn.Parameter(torch.zeros(1, npatch + (1 if pretrain_use_cls_token else 0), embed_dim))
        else:
            self.pos_embed = None
        half = embed_dim // num_heads // 2
        self.rope_win = _Rope(window_size, half, pt_hw_seq_len)
        self.rope_glb = _Rope(img_size // patch_size, half, pt_hw_seq_len)
        if img_size // patch_size != global_window_size:
            raise NotImplementedError("global RoPE table side (img_size/patch) must equal global_window_size")
        self._out_features = [out_feature]
        self._out_feature_channels = {out_feature: embed_dim}
        self._out_feature_strides = {out_feature: patch_size}
        self._drop_derived()
        self._tuned: Dict[tuple, int] = {}
        self.autotune = True            # pick the GEMM tile variant per shape by measurement (first eager forward)
        self.alias_outputs = False      # True: returned tensors alias the reused workspace (benchmarks)
        self.view_groups = 1            # > 1: split the views into groups that run concurrently on separate lanes (HIP streams)
        # launch-schedule switches (schedule_defaults above): shipped defaults per precision, overridable per model -- no environment variables
        sched = schedule_defaults(precision)
        unknown = set(schedule or {}) - set(sched)
        if unknown:
            raise TypeError(f"unknown schedule switches {sorted(unknown)}; known: {sorted(sched)}")
        sched.update(schedule or {})
        for k_, v_ in sched.items():
            setattr(self, k_, v_)
        assert self.launch_mode in MODES, self.launch_mode
        self._stream_pool = []

    # -- derived state (plan.DerivedState): new weights or a device move drop the packed weights, the recorded launch plans that point into them and
    # the split-K workspaces of the dropped plans' device (the Gumbel frame counter survives: plans on the same device keep naming it, _rng_state
    # carries its value to a new one); copies / pickles start without them and without this instance's streams -----------------------------------
    _DERIVED = dict(_packed=None, _plans={}, _sk_ws={}, _sk_ws_old=[])
    _INSTANCE = dict(_stream_pool=[])

    def __getstate__(self):
        d = super().__getstate__()
        if d.get("_gumbel_rng") is not None:
            # A copy CONTINUES the noise stream where this model stands (same key, the counter's value carried as a host tensor that _rng_state moves to
            # the copy's device) instead of replaying it from frame 0: original and replica then draw the same noise for the frames that follow -- replicas
            # of a model that has run share their noise; assign a different gumbel_seed to a replica that needs its own stream.
            d["_gumbel_rng"] = d["_gumbel_rng"].detach().to("cpu").clone()
        return d

    def __setstate__(self, d):
        # pickles written before `gumbel_seed` became a property carry the plain attribute
        if "gumbel_seed" in d and "_gumbel_seed" not in d:
            d = dict(d)
            d["_gumbel_seed"] = d.pop("gumbel_seed")
        super().__setstate__(d)           # (nn.Module back-fills the hook dictionaries that pickles of older torch versions lack)

    # -- helpers ---------------------------------------------------------------------------------------
    def _accelerated(self, i):
        return False                                      # dense backbone: every block is Block.forward (ToC3DEVAViT overrides)

    # -- dtype codes of this precision and schedule (gemm.dtypes has the table) -------------------------------
    @property
    def _dts(self):
        return gemm.dtypes(self.precision, self.x3_planes, self.x3_attention)

    _dt = property(lambda self: self._dts.act)
    _tdt = property(lambda self: self._dts.torch)
    _dt_gemm = property(lambda self: self._dts.gemm)
    _dt_rows = property(lambda self: self._dts.rows)
    _dt_attn = property(lambda self: self._dts.attn)
    _x3p = property(lambda self: self._dts.x3p)

    def _block_side(self, i):
        return self.global_window_size if i in self.global_attn_indexes else self.window_size

    def _pack_blocks(self, dev):
        C, Hd = self.embed_dim, self.hidden_dim
        Hp = round_up(Hd, 64)
        pk = gemm.Packer(self._dts, dev)
        f = pk.f32
        blocks = []
        for blk in self.blocks:
            a, m = blk.attn, blk.mlp
            p = {}
            zb = torch.zeros(C, device=dev)
            qb = a.q_bias if a.q_bias is not None else zb
            vb = a.v_bias if a.v_bias is not None else zb
            p["wqkv"], p["bqkv"] = pk.wb(torch.cat([a.q_proj.weight, a.k_proj.weight, a.v_proj.weight], 0), torch.cat([qb, zb, vb]))
            p["v_bias"] = f(vb)
            p["wproj"], p["bproj"] = pk.wb(a.proj.weight, a.proj.bias)
            w12 = torch.empty(2 * Hp, C, dtype=self._tdt, device=dev)
            b12 = torch.empty(2 * Hp, dtype=torch.float32, device=dev)
            lib.call("toc3d_pack_swiglu", self._dt, f(m.w1.weight), f(m.w2.weight), f(m.w1.bias), f(m.w2.bias), Hd, C, w12, b12, Hp, C, lib.stream_ptr())
            p["w12"], p["b12"] = w12, b12                         # (-> planes below, after the lnfold pack may have rewritten it)
            if self.fold_norm2:                                   # gamma2-scaled interleaved weights + (c1, c2) in packed column order; replaces w12 / b12
                p["c1_12"], p["c2_12"] = torch.empty(2 * Hp, device=dev), torch.empty(2 * Hp, device=dev)
                lib.call("toc3d_pack_swiglu_lnfold", self._dt, f(m.w1.weight), f(m.w2.weight), f(m.w1.bias), f(m.w2.bias),
                         f(blk.norm2.weight), f(blk.norm2.bias), Hd, C, w12, p["c1_12"], p["c2_12"], Hp, C, lib.stream_ptr())
            if self.fold_ffn_ln:
                N3, K3 = m.w3.weight.shape
                w3f = torch.empty(round_up(N3, 128), Hp, dtype=self._tdt, device=dev)
                p["c1"], p["c2"] = torch.empty(N3, device=dev), torch.empty(N3, device=dev)
                lib.call("toc3d_pack_weight_lnfold", self._dt, f(m.w3.weight), f(m.ffn_ln.weight), f(m.ffn_ln.bias),
                         f(m.w3.bias), N3, K3, w3f, w3f.shape[0], Hp, p["c1"], p["c2"], lib.stream_ptr())
                p["w3"] = gemm.planes(w3f, self._dts)                       # gamma-scaled; c1 / c2 carry the mean and beta / bias terms
            else:
                p["w3"], p["b3"] = pk.wb(m.w3.weight, m.w3.bias)
            gemm.planes(w12, self._dts)
            for n, mod in (("ln1", blk.norm1), ("ln2", blk.norm2), ("lnf", m.ffn_ln)):
                p[n + "_w"], p[n + "_b"] = f(mod.weight), f(mod.bias)
            p["cos"], p["sin"] = f(a.rope.freqs_cos), f(a.rope.freqs_sin)
            p["rope_side"] = self._check_axial_rope(p["cos"], p["sin"])
            if self.attn_rot:                                     # compact axial tables [2, L, 16]: one entry per frequency pair (the q|k|v GEMM's rotating epilogue)
                L = p["rope_side"]
                tabs = []
                for nm in ("cos", "sin"):
                    t = p[nm].view(L, L, 64)
                    tabs.append(torch.stack([t[:, 0, 0:32:2], t[0, :, 32:64:2]]))
                p["rope_tab"] = torch.stack(tabs).contiguous()       # [cos | sin][2, L, 16]
            blocks.append(p)
        torch.cuda.current_stream().synchronize()      # the f32 temporaries above must outlive the pack kernels
        return blocks

    @staticmethod
    def _check_axial_rope(cos, sin):
        """The attention kernel keeps a [2, L, 16] extract of the RoPE buffers in LDS, which is exact iff the buffers have
        VisionRotaryEmbeddingFast's axial structure (eva_utils.py:362-371).  Verified here, on the loaded buffers."""
        L = int(math.isqrt(cos.shape[0]))
        if L * L != cos.shape[0] or cos.shape[1] != 64:
            raise NotImplementedError("RoPE buffers must be [L*L, 64]")
        for t in (cos, sin):
            g = t.view(L, L, 64)
            ok = (torch.equal(g[:, :, :32], g[:, :1, :32].expand(L, L, 32)) and torch.equal(g[:, :, 32:], g[:1, :, 32:].expand(L, L, 32))
                  and torch.equal(t[:, 0::2], t[:, 1::2]))
            if not ok:
                raise NotImplementedError("RoPE buffers do not have the axial (row | column, pair-repeated) structure of "
                                          "VisionRotaryEmbeddingFast; the HIP attention kernel only supports that form")
        return L

    def _pack_common(self):
        dev = self.patch_embed.proj.weight.device
        if dev.type != "cuda":
            raise RuntimeError("toc3d_amd backbones run on an AMD GPU through libtoc3d_gfx950.so; there is no CPU path "
                               "(move the module to cuda)")
        lib.load()
        P = {"dev": dev}
        pk = gemm.Packer(self._dts, dev)
        P["w_patch"], P["b_patch"] = pk.wb(self.patch_embed.proj.weight.reshape(self.embed_dim, -1), self.patch_embed.proj.bias)
        P["blocks"] = self._pack_blocks(dev)
        P["pos"] = {}                                   # (h, w) -> bicubic-resized abs-pos, built on first use
        if self.pos_embed is not None:                  # source grid (cls row dropped, eva_utils.py:240-243)
            P["pos_embed"] = pk.f32(self.pos_embed[0, 1:] if self.pretrain_use_cls_token else self.pos_embed[0]).clone()
        return P

    _pack = _pack_common                                # what forward() packs on first use (ToC3DEVAViT adds the scorers and the pad rows)

    def _pos_for(self, h, w, dev):
        C = self.embed_dim
        pe = self._packed.get("pos_embed") if self._packed is not None else None
        if pe is None:
            return None
        S = int(math.isqrt(pe.shape[0]))
        assert S * S == pe.shape[0]
        out = torch.empty(h * w, C, dtype=torch.float32, device=dev)
        lib.call("toc3d_abs_pos_bicubic", pe, S, C, out, h, w, lib.stream_ptr())
        torch.cuda.current_stream().synchronize()
        return out

    def _dense_map(self, V, h, w, L, dev):
        nW = V * (-(-h // L)) * (-(-w // L))
        N = L * L
        d = {"rows": torch.empty(nW, N, dtype=torch.int32, device=dev), "slots": torch.empty(nW, N, dtype=torch.int32, device=dev),
             "count": torch.empty(nW, dtype=torch.int32, device=dev), "npad": torch.empty(nW, dtype=torch.int32, device=dev),
             "nW": nW, "N": N, "max_count": min(N, min(L, h) * min(L, w))}
        lib.call("toc3d_window_map_dense", V, h, w, L, d["rows"], d["slots"], d["count"], d["npad"], lib.stream_ptr())
        if self.big_windows_first:
            # Windows are independent, so their order in the lists is free: biggest first.  The attention grid is dispatched in list order and the
            # edge windows of a 20 x 50 token grid are a fraction of the full ones (16 x 16 windows: 256 / 64 / 32 / 8 keys; 20 x 20: 400 / 200); with
            # the full windows spread over the dispatch rounds the launch ends on a round of stragglers (profiles/r03_attn_timeline.txt: dense
            # 20 x 20, 288 workgroups at one per CU: span 36 us for 23 us workgroups).  Done once per plan, on the static maps.
            perm = torch.argsort(d["count"], descending=True, stable=True)
            for k in ("rows", "slots", "count", "npad"):
                d[k] = d[k][perm].contiguous()
        return d

    def _base_plan(self, V, H, W, x, B, max_rows=0):
        """The work plan of one view group of ``B`` frames: ``x`` its rows of the master's residual stream, the activation buffers (``max_rows``: of the compact
        rows too) and the static dense window lists."""
        C, Hp = self.embed_dim, round_up(self.hidden_dim, 64)
        p = self.patch_size
        h, w = H // p, W // p
        T, M = h * w, V * h * w
        R = max(M, max_rows)
        tdt, dev = self._tdt, x.device
        Kc = self.in_chans * p * p
        plan = dict(V=V, h=h, w=w, T=T, M=M, B=B, x=x,
                    a=torch.empty(R, C, dtype=tdt, device=dev),
                    qkv=torch.empty(R, 3 * C, dtype=tdt, device=dev),
                    att=torch.empty(R, C, dtype=tdt, device=dev),
                    hid=torch.zeros(R, Hp, dtype=tdt, device=dev),
                    hln=torch.zeros(R, Hp, dtype=tdt, device=dev),
                    col=torch.zeros(M, round_up(Kc, 64), dtype=tdt, device=dev),
                    Kc=Kc)
        if self.fold_ffn_ln:                                      # per-row partial (sum, sum^2) slots of the hidden units: header + [R, cap, 2]
            plan["stats_cap"] = round_up(-(-2 * Hp // 128), 2)
            plan["stats"] = torch.zeros(4 + R * plan["stats_cap"] * 2, dtype=torch.float32, device=dev)
            plan["stats2_cap"] = C // 64                          # norm2 fold: one slot per 64 residual-stream columns
            plan["stats2"] = torch.zeros(4 + R * plan["stats2_cap"] * 2, dtype=torch.float32, device=dev)
        plan["dense"] = {L: self._dense_map(V, h, w, L, dev) for L in {self.window_size, self.global_window_size}}
        if self.attn_rot:                                         # RoPE position of every token row per window type: (r % L) << 16 | (c % L)
            r = torch.arange(h, device=dev, dtype=torch.int32).view(1, h, 1).expand(V, h, w)
            c = torch.arange(w, device=dev, dtype=torch.int32).view(1, 1, w).expand(V, h, w)
            for L, d in plan["dense"].items():
                d["rc"] = (((r % L) << 16) | (c % L)).reshape(-1).contiguous()
        for d in plan["dense"].values():
            d["win"] = Windows(d.get("rc"), d["rows"], d["slots"], d["count"], None, d["npad"], d["N"], d["nW"], d["max_count"])
        return plan

    _plan = _base_plan                                  # what _master_plan asks for per view group (ToC3DEVAViT adds the selections and the scorer's buffers)

    def _master_plan(self, V, H, W, B, dev):
        """The plan of one input shape: the residual stream ``x`` of all views, and per view group (_group_layout) a work plan on its row slice (whole 128-byte
        lines: C * 4 bytes per token) with its first view / frame and their counts."""
        h, w = H // self.patch_size, W // self.patch_size
        T = h * w
        m = dict(V=V, h=h, w=w, T=T, M=V * T, x=torch.empty(V * T, self.embed_dim, dtype=torch.float32, device=dev), groups=[])
        for (v0, nv, f0, nf) in self._group_layout(V, B):
            gp = self._plan(nv, H, W, m["x"][v0 * T:(v0 + nv) * T], nf)
            gp["v0"], gp["nv"], gp["frame0"] = v0, nv, f0
            m["groups"].append(gp)
        return m

    def _linear(self, epi, A, W, bias, out, M, N, K, **kw):
        """One linear layer with a per-shape autotuned tile variant (gemm.linear; this model owns the table)."""
        gemm.linear(self, epi, A, W, bias, out, M, N, K, **kw)

    def save_packed(self, path):
        """Write the packed device weights (what the kernels consume) to a safetensors file; see ``packed_io``."""
        from .packed_io import save_packed
        save_packed(self, path)

    def load_packed(self, path):
        """Restore weights from ``save_packed`` (module already on the GPU); replaces load_state_dict + packing."""
        from .packed_io import load_packed
        load_packed(self, path)

    def save_tuning(self, path):
        """Persist the autotuned (epilogue, M, N, K) -> variant table (JSON), e.g. to profile without tuning launches."""
        import json
        with open(path, "w") as f:
            json.dump({"precision": self.precision, "table": [[list(k), v] for k, v in self._tuned.items()]}, f)

    def load_tuning(self, path):
        import json
        with open(path) as f:
            d = json.load(f)
        if d.get("precision") == self.precision:
            tab = {tuple(k): int(v) for k, v in d["table"]}
            if self.precision == "fp32x3" and not self._x3p:
                # the shipped fp32x3 tables were tuned with the operands in planes and name tiles that only exist on planes (csrc/gemm_kernels.h launch_epi_x: the
                # 96- / 160-row tiles and the phased ones): with x3_planes off those launches would be refused -- such shapes fall back to first-use tuning / the heuristic
                tab = {k: v for k, v in tab.items() if v % 1000 % 100 not in lib.X3_PLANES_ONLY_VARIANTS}
            self._tuned.update(tab)

    # -- launch sequences -----------------------------------------------------------------------------
    def _stem_im2col(self, plan, img):
        """The one kernel that reads the caller's image tensor (a new pointer every frame): always launched directly, in front of
        the recorded part of the frame, on the caller's stream."""
        s = lib.stream_ptr()
        V = plan["V"]
        H, W = plan["h"] * self.patch_size, plan["w"] * self.patch_size
        Kp = plan["col"].shape[1]
        if img.dtype == torch.uint8:
            n = self.img_norm_cfg
            lib.call("toc3d_im2col_patches_u8", self._dt, img, V, img.shape[1], img.shape[2], n["mean"], n["std"], int(n["to_rgb"]),
                     plan["col"], Kp, H, W, self.patch_size, s)
        else:
            lib.call("toc3d_im2col_patches", self._dt, img, plan["col"], Kp, V, self.in_chans, H, W, self.patch_size, s)

    def _stem_gemm(self, plan, P):
        """PatchEmbed GEMM + abs-pos add (toc3d_eva_vit.py:243-247) -> residual stream x f32 [V*T, C]."""
        C = self.embed_dim
        pos = P["pos"][(plan["h"], plan["w"])]
        self._linear(lib.EPI_RESIDUAL, plan["col"], P["w_patch"], P["b_patch"], plan["x"], plan["M"], C, plan["col"].shape[1],
                     residual=pos, ldr=C, residual_row_mod=plan["T"] if pos is not None else 0)

    def _ensure_pos(self, P, h, w, dev):
        if (h, w) not in P["pos"]:
            P["pos"][(h, w)] = self._pos_for(h, w, dev)

    def _run_frame(self, master, n_lanes, frame_fn, variant=None):
        """One frame in the configured launch mode (toc3d_amd/plan.py: eager / recorded plan / explicit hipGraph)."""
        run_frame(master.setdefault("launch", {}).setdefault(variant, {}), self.launch_mode, n_lanes, frame_fn, self._stream_pool)

    def _prefetch_args(self, P, i):
        """(n_prefetch, prefetch_ptrs, prefetch_bytes, prefetch_workgroups) of block i's attention launch: the weights of the GEMMs that follow it."""
        bp = P["blocks"][i]
        ts = [bp["wproj"], bp["w12"], bp["w3"]] + ([P["blocks"][i + 1]["wqkv"]] if i + 1 < self.depth else [])
        if not self.prefetch_weights:
            ts = []
        return (len(ts), *lib.ptr_arrays(ts, min_len=1), self.prefetch_weights)

    def _qkv_attention(self, P, i, plan, M, win: Windows):
        """q|k|v projection + windowed attention of block i on plan["a"] [M, C] -> plan["att"] (eva_vit.py:97-113, toc3d_eva_vit.py:495-512), on the window list
        ``win``: a dense map (pads folded analytically: ``npad`` and the block's v bias) or a selection (pads read from the block's pad rows)."""
        bp = P["blocks"][i]
        C = self.embed_dim
        rot = self._rot_ok(win.stride)                  # decided once: the rotating GEMM epilogue, the rotated pad rows and the pre-rotated attention go together
        v_bias = None if win.npad is None else bp["v_bias"]
        pad = None if win.count_k is None else bp["pad_rot" if rot else "pad_qkv"]
        args = (plan["qkv"], 3 * C, plan["att"], C, win.rows, win.slots, win.count_q, win.count_k, win.npad, pad, win.stride, win.nwin, win.max_count, self.num_heads)
        if rot:
            self._linear(lib.EPI_QKV_ROPE, plan["a"], bp["wqkv"], bp["bqkv"], plan["qkv"], M, 3 * C, C,
                         rope=(win.rc, bp["rope_tab"], bp["rope_side"], lib.ATTN_ROT_Q_SCALE), a_planes=self._x3p, o_planes=self._x3p)
            if self._x3p:       # planes in, planes out; no weight prefetch riding on this form
                lib.call("toc3d_window_attention_rot", lib.F32X3P, *args, v_bias, 0, None, None, 0, lib.stream_ptr())
            else:
                lib.call("toc3d_window_attention_rot", self._dt, *args, v_bias, *self._prefetch_args(P, i), lib.stream_ptr())
            return
        self._linear(lib.EPI_BIAS, plan["a"], bp["wqkv"], bp["bqkv"], plan["qkv"], M, 3 * C, C, a_planes=self._x3p)
        args = (self._dt_attn, *args, bp["cos"], bp["sin"], bp["rope_side"], v_bias, 64 ** -0.5)
        if self.prefetch_weights:   # the launch also pulls the weights of the GEMMs that follow it (this block's proj / w1|w2 / w3, the next block's q|k|v) towards the chip
            lib.call("toc3d_window_attention_pf", *args, *self._prefetch_args(P, i), lib.stream_ptr())
        else:
            lib.call("toc3d_window_attention", *args, lib.stream_ptr())

    def _rot_ok(self, stride):
        """The pre-rotated attention path serves this window size: bf16 up to 416 keys (K and V of a head whole in LDS); fp32x3 on planes any size of the model
        (windows over 288 keys in super-tiles) -- needs the GEMM operands in planes (x3_planes)."""
        if not self.attn_rot:
            return False
        if self.precision == "bf16":
            return stride <= 416
        return self._x3p and stride <= 1024

    def _proj(self, bp, plan, rows, out, rep_out, rep_index, res=None, res_index=None):
        """attn.proj + residual add (eva_vit.py:115,262 / toc3d_eva_vit.py:514,379) into ``out`` f32 [rows, C]: in place by default, or with the
        residual of row m read from row ``res_index[m]`` of ``res`` (the token-major stream; compact rows that were never copied).  With
        norm2 folded the epilogue also leaves the updated rows in bf16 (plan["a"]) and their statistics (plan["stats2"]) for the w1|w2 GEMM."""
        C = self.embed_dim
        res = out if res is None else res
        kw = dict(residual=res, ldr=C, rep_out=rep_out, rep_index=rep_index, residual_index=res_index, a_planes=self._x3p)
        if self.fold_norm2:
            self._linear(lib.EPI_RESIDUAL_STATS, plan["att"], bp["wproj"], bp["bproj"], out, rows, C, C, stats_out=(plan["stats2"], plan["stats2_cap"]),
                         out_act=plan["a"], ld_act=C, o_planes=self._x3p, **kw)     # the f32 copy leaves as planes: the w1|w2 GEMM's A operand
        else:
            self._linear(lib.EPI_RESIDUAL, plan["att"], bp["wproj"], bp["bproj"], out, rows, C, C, **kw)

    def _mlp(self, bp, plan, rows, res, rep_out, rep_index):
        """norm2 -> SwiGLU (w1|w2, ffn_ln, w3) -> + residual (eva_vit.py:263, toc3d_eva_vit.py:381-384); res is f32 [rows, C]."""
        s = lib.stream_ptr()
        C, Hd = self.embed_dim, self.hidden_dim
        Hp = plan["hid"].shape[1]
        dt = self._dt
        if self.fold_ffn_ln:
            # ffn_ln folded: the SwiGLU GEMM leaves per-row (sum, sum^2) slots, the w3 GEMM (gamma-scaled weights) normalises in its epilogue;
            # norm2 folded the same way: plan["a"] / plan["stats2"] were left by the projection GEMM (_proj), no LayerNorm launch here
            st, cap = plan["stats"], plan["stats_cap"]
            if self.fold_norm2:
                self._linear(lib.EPI_SWIGLU_STATS_LN, plan["a"], bp["w12"], bp["c2_12"], plan["hid"], rows, 2 * Hp, C, n_valid=Hd, stats_out=(st, cap),
                             stats_in=(plan["stats2"], plan["stats2_cap"], C // 64), col_sums=bp["c1_12"], ln_n=C, ln_eps=self.LN_EPS,
                             a_planes=self._x3p, o_planes=self._x3p)       # A = the projection's copy (planes), hidden units as planes for w3
            else:
                lib.call("toc3d_layernorm_rows", dt, res, C, None, None, bp["ln2_w"], bp["ln2_b"], self.LN_EPS, plan["a"], C, rows, C, s)
                self._linear(lib.EPI_SWIGLU_STATS, plan["a"], bp["w12"], bp["b12"], plan["hid"], rows, 2 * Hp, C, n_valid=Hd, stats_out=(st, cap), o_planes=self._x3p)
            self._linear(lib.EPI_RESIDUAL_LN, plan["hid"], bp["w3"], bp["c2"], res, rows, C, Hp, residual=res, ldr=C, rep_out=rep_out, rep_index=rep_index,
                         stats_in=(st, cap, -(-2 * Hp // 128)), col_sums=bp["c1"], ln_n=Hd, ln_eps=self.LN_EPS, a_planes=self._x3p)
            return
        lib.call("toc3d_layernorm_rows", dt, res, C, None, None, bp["ln2_w"], bp["ln2_b"], self.LN_EPS, plan["a"], C, rows, C, s)
        self._linear(lib.EPI_SWIGLU, plan["a"], bp["w12"], bp["b12"], plan["hid"], rows, 2 * Hp, C, n_valid=Hd)
        lib.call("toc3d_layernorm_act", dt, plan["hid"], Hp, bp["lnf_w"], bp["lnf_b"], self.LN_EPS, plan["hln"], Hp, rows, Hd, s)
        self._linear(lib.EPI_RESIDUAL, plan["hln"], bp["w3"], bp["b3"], res, rows, C, Hp, residual=res, ldr=C, rep_out=rep_out, rep_index=rep_index)

    def _dense_block(self, i, plan, P):
        """Block.forward (eva_vit.py:247-268): LN -> window attention (pads folded analytically) -> +res; MLP -> +res."""
        s = lib.stream_ptr()
        bp = P["blocks"][i]
        C, M = self.embed_dim, plan["M"]
        x = plan["x"]
        lib.call("toc3d_layernorm_rows", self._dt_rows, x, C, None, None, bp["ln1_w"], bp["ln1_b"], self.LN_EPS, plan["a"], C, M, C, s)
        self._qkv_attention(P, i, plan, M, plan["dense"][self._block_side(i)]["win"])
        self._proj(bp, plan, M, x, None, None)
        self._mlp(bp, plan, M, x, None, None)

    # -- view groups: independent views processed concurrently on separate HIP streams ----------
    def _group_layout(self, V, B):
        """[(view0, n_views, frame0, n_frames)] per group; falls back to one group when the split is not frame-aligned."""
        G = max(1, int(self.view_groups))
        vpf = V // B
        if G > 1 and V % G == 0:
            Vg = V // G
            if Vg % vpf == 0:
                return [(g * Vg, Vg, g * (Vg // vpf), Vg // vpf) for g in range(G)]
            if vpf % Vg == 0:
                return [(g * Vg, Vg, (g * Vg) // vpf, 1) for g in range(G)]
        return [(0, V, 0, B)]

    def _check_input(self, x):
        """-> (tensor, H, W): f32 NCHW (B*Nv, 3, H, W) as the reference's detector passes it (petr3d.py:139-141), or uint8 HWC
        (B*Nv, H0, W0, 3) raw camera images when the backbone was built with ``img_norm_cfg``; H, W are the padded sizes."""
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise RuntimeError("toc3d_amd: input must be a CUDA/HIP tensor -- the HIP extension is the only compute path "
                               "(no CPU fallback)")
        if x.dtype == torch.uint8:
            if self.img_norm_cfg is None:
                raise ValueError("uint8 images need the backbone to be built with img_norm_cfg=dict(mean=..., std=..., to_rgb=...)")
            if x.dim() != 4 or x.shape[3] != 3 or self.in_chans != 3:
                raise ValueError(f"expected uint8 HWC images (B*Nv, H, W, 3), got {tuple(x.shape)}")
            d = self.pad_size_divisor
            return x.contiguous(), -(-x.shape[1] // d) * d, -(-x.shape[2] // d) * d
        if x.dim() != 4 or x.shape[1] != self.in_chans or x.shape[2] % self.patch_size or x.shape[3] % self.patch_size:
            raise ValueError(f"expected (B*Nv, {self.in_chans}, H, W) with H, W multiples of {self.patch_size}, got {tuple(x.shape)}")
        return x.float().contiguous(), x.shape[2], x.shape[3]

    # -- the frame driver: what both forwards do around their block loops ------------------------------------------------------------
    def _master(self, x, frames=None):
        """-> (checked input, its master plan): the weights packed on first use, the plan looked up under the input's shape, dtype, ``frames`` (the ToC3D
        backbone's; the dense one has none: every view stands alone) and ``view_groups``.  Each plan holds ~1 GB of workspaces at full size: the 8 most recently
        used are kept."""
        x, H, W = self._check_input(x)
        if self._packed is None:
            self._packed = self._pack()
            self._plans = {}
        V = x.shape[0]
        B = V if frames is None else frames
        assert V % B == 0
        key = (tuple(x.shape), x.dtype) + (() if frames is None else (frames,)) + (self.view_groups,)
        return x, lru(self._plans, key, lambda: self._master_plan(V, H, W, B, x.device), 8)

    def _drive(self, master, x, n_lanes, blocks, ahead=None, variant=None):
        """One frame on ``n_lanes`` lanes, lanes 0..G-1 the view groups': the stem's im2col per group on the caller's stream, in front of the frame (it reads the
        caller's tensor); then, in the configured launch mode, ``ahead(ex)`` (what has to be issued before the groups fork), the entry waits, the stem GEMM per
        group, ``blocks(ex)`` and the joins into lane 0.  ``variant``: which of the master's recordings this launch sequence is."""
        P, groups = self._packed, master["groups"]
        self._ensure_pos(P, master["h"], master["w"], x.device)
        for gp in groups:
            self._stem_im2col(gp, x[gp["v0"]:gp["v0"] + gp["nv"]])

        def frame(ex):
            if ahead is not None:
                ahead(ex)
            for g in range(1, len(groups)):
                ex.wait(g, 0)
            for g, gp in enumerate(groups):
                with ex.lane(g):
                    self._stem_gemm(gp, P)
            blocks(ex)
            for l in range(1, n_lanes):
                ex.wait(0, l)
        self._run_frame(master, n_lanes, frame, variant)

    def _feature_view(self, plan):
        x = plan["x"] if self.alias_outputs else plan["x"].clone()
        return x.view(plan["V"], plan["h"], plan["w"], self.embed_dim).permute(0, 3, 1, 2)   # NCHW view of NHWC (:294)

    def output_shape(self):
        return {n: dict(channels=self._out_feature_channels[n], stride=self._out_feature_strides[n]) for n in self._out_features}


class EVA_ViT(_BackboneBase):
    """Dense EVA-02 ViT (StreamPETR baseline backbone), reference ``eva_vit.py:270-428``."""

    def __init__(self, img_size=1024, patch_size=16, in_chans=3, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4 * 2 / 3,
                 qkv_bias=True, drop_path_rate=0.0, norm_layer=partial(nn.LayerNorm, eps=1e-6), act_layer=nn.GELU,
                 use_abs_pos=True, use_rel_pos=False, rope=True, pt_hw_seq_len=16, intp_freq=True, window_size=0,
                 global_window_size=20, use_checkpoint=True, global_attn_indexes=(), residual_block_indexes=(),
                 use_act_checkpoint=False, pretrain_img_size=224, pretrain_use_cls_token=True, return_intermediate=False,
                 out_feature="last_feat", xattn=True, precision=DEFAULT_PRECISION, **unused):
        super().__init__()
        if use_rel_pos or len(residual_block_indexes) or return_intermediate or not rope or not intp_freq or window_size <= 0:
            raise NotImplementedError("use_rel_pos / residual blocks / return_intermediate / rope=False / window_size=0 "
                                      "are dead code for the shipped configs and not built")
        self._setup_common(img_size, patch_size, in_chans, embed_dim, depth, num_heads, mlp_ratio, qkv_bias, use_abs_pos,
                           pt_hw_seq_len, window_size, global_window_size, global_attn_indexes, pretrain_img_size,
                           pretrain_use_cls_token, out_feature, precision, unused.get("img_norm_cfg"), unused.get("pad_size_divisor", 32), unused.get("schedule"))
        self.blocks = nn.ModuleList([
            _Block(embed_dim, mlp_ratio, qkv_bias, partial(nn.LayerNorm, eps=1e-6),
                   self.rope_glb if i in self.global_attn_indexes else self.rope_win) for i in range(depth)])
        if self.pos_embed is not None:
            nn.init.trunc_normal_(self.pos_embed, std=0.02)
        self.apply(_init_weights)

    @torch.no_grad()
    def forward(self, x, *args, **kwargs):
        x, master = self._master(x)
        groups = master["groups"]

        def blocks(ex):
            for i in range(self.depth):
                for g, gp in enumerate(groups):
                    with ex.lane(g):
                        self._dense_block(i, gp, self._packed)
        self._drive(master, x, len(groups), blocks)
        return {self._out_features[0]: self._feature_view(master)}


class ToC3DEVAViT(_BackboneBase):
    """EVA-02 ViT with ToC3D motion-query-guided token compression, reference ``toc3d_eva_vit.py:25-326``."""
    _gumbel_seed = None              # (class defaults: an instance restored from an old pickle finds them)
    _gumbel_rng = None

    def __init__(self, img_size=1024, patch_size=16, in_chans=3, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4 * 2 / 3,
                 qkv_bias=True, drop_path_rate=0.0, norm_layer=partial(nn.LayerNorm, eps=1e-6), act_layer=nn.GELU,
                 use_abs_pos=True, use_rel_pos=False, rope=True, rope_acc=False, pt_hw_seq_len=16, intp_freq=True,
                 window_size=0, global_window_size=20, use_checkpoint=True, global_attn_indexes=(), residual_block_indexes=(),
                 use_act_checkpoint=False, pretrain_img_size=224, pretrain_use_cls_token=True, out_feature="last_feat",
                 return_intermediate=False, xattn=True, pruning_loc=None, pruning_score_type="attention", score_mask=True,
                 pruning_attn_scale=True, pruning_num_queries=256, accelerate_global=True, token_ratio=None,
                 use_represent_tokens=True, pc_range=None, token_selection_loss=None, precision=DEFAULT_PRECISION, **unused):
        super().__init__()
        if (use_rel_pos or len(residual_block_indexes) or return_intermediate or not rope or not rope_acc or not intp_freq
                or pruning_score_type != "attention" or not score_mask or not use_represent_tokens or window_size <= 0):
            raise NotImplementedError("only the shipped ToC3D configuration family is built: rope + rope_acc, "
                                      "pruning_score_type='attention', score_mask, use_represent_tokens")
        pruning_loc = list(pruning_loc or [])
        assert token_ratio is not None and len(token_ratio) == len(pruning_loc)
        assert len(set(pruning_loc) & set(global_attn_indexes)) == 0, \
            "The pruning score calculation layer cannot be the global attention layer"          # toc3d_eva_vit.py:141-142
        assert pc_range is not None
        if any(not (0.0 < r < 1.0) for r in token_ratio):
            raise NotImplementedError("token_ratio must be in (0, 1): ratio 1.0 makes the reference return permuted tokens "
                                      "(toc3d_eva_vit.py:463); use EVA_ViT for the dense baseline")
        self._setup_common(img_size, patch_size, in_chans, embed_dim, depth, num_heads, mlp_ratio, qkv_bias, use_abs_pos,
                           pt_hw_seq_len, window_size, global_window_size, global_attn_indexes, pretrain_img_size,
                           pretrain_use_cls_token, out_feature, precision, unused.get("img_norm_cfg"), unused.get("pad_size_divisor", 32), unused.get("schedule"))
        self.pruning_loc = pruning_loc
        self.pruning_num_queries = pruning_num_queries
        self.pruning_attn_scale = pruning_attn_scale
        self.accelerate_global = accelerate_global
        self.token_ratio = list(token_ratio)
        self.use_represent_tokens = use_represent_tokens
        self.token_selection_loss = None                 # training-only (TokenSelectionLoss); inference build
        # Device-side Gumbel draw (toc3d_gumbel_noise) when no noise is injected: Philox key = gumbel_seed (None: torch.initial_seed() at the first
        # forward, so torch.manual_seed() before inference is honoured like by the reference's generator), counter = ONE frame counter per model
        # (_gumbel_rng, device memory), shared by every launch plan -- a second input shape, or a plan rebuilt after eviction, continues the stream
        # instead of replaying it from frame 0.
        self._gumbel_seed = None
        self._gumbel_rng = None
        half = embed_dim // num_heads // 2
        self.score_predictor = nn.ModuleList([_Scorer(embed_dim, pruning_num_queries, token_ratio[i], pc_range)
                                              for i in range(len(pruning_loc))])
        self.rope_win_acc = _Rope(window_size, half, pt_hw_seq_len)
        self.rope_glb_acc = _Rope(img_size // patch_size, half, pt_hw_seq_len)
        self.blocks = nn.ModuleList()
        for i in range(depth):
            glb = i in self.global_attn_indexes
            if self._accelerated(i):
                r = self.rope_glb_acc if glb else self.rope_win_acc
            else:
                r = self.rope_glb if glb else self.rope_win
            self.blocks.append(_Block(embed_dim, mlp_ratio, qkv_bias, partial(nn.LayerNorm, eps=1e-6), r))
        if self.pos_embed is not None:
            nn.init.trunc_normal_(self.pos_embed, std=0.02)
        self.apply(_init_weights)                        # like the reference (:217) this also re-inits the MLN gamma/beta Linears

    def _accelerated(self, i):                           # toc3d_eva_vit.py:178-180
        return len(self.pruning_loc) > 0 and i >= self.pruning_loc[0] and (self.accelerate_global or i not in self.global_attn_indexes)

    def loss(self, *a, **k):
        raise NotImplementedError("training-only: TokenSelectionLoss is outside the inference hot path")

    # -- packing -------------------------------------------------------------------------------------
    def _pack(self):
        P = self._pack_common()
        dev = P["dev"]
        s = lib.stream_ptr()
        # kept padded slots of an accelerated block are the row LN1(0) = beta1 (toc3d_eva_vit.py:414,372): its q|k|v
        # projection is a per-block constant, produced here by the same LayerNorm + GEMM kernels as a real row
        C = self.embed_dim
        minus1 = torch.full((1,), -1, dtype=torch.int32, device=dev)
        keep = []                                          # temporaries of the pack launches, dropped after the last synchronize below
        for i, bp in enumerate(P["blocks"]):
            if not self._accelerated(i):
                continue
            a_row = torch.empty(1, C, dtype=self._tdt, device=dev)
            bp["pad_qkv"] = torch.empty(1, 3 * C, dtype=self._tdt, device=dev)
            lib.call("toc3d_layernorm_rows", self._dt, bp["ln1_w"], C, minus1, None, bp["ln1_w"], bp["ln1_b"], self.LN_EPS, a_row, C, 1, C, s)
            lib.call("toc3d_linear", self._dt_gemm, lib.EPI_BIAS, a_row, C, bp["wqkv"], C, bp["bqkv"], bp["pad_qkv"], 3 * C, None, 0, 0, None, None,
                     1, 3 * C, C, 0, s)
            if self.attn_rot and (self.precision == "bf16" or self._x3p):
                # ... and, for the pre-rotated attention, that row rotated for EVERY window slot by the same GEMM epilogue that rotates real rows
                # (bit-identical to an explicit pad row at that slot): pad_rot [L*L, 3C], row = window slot
                L = bp["rope_side"]
                sl = torch.arange(L * L, device=dev, dtype=torch.int32)
                rc = (((sl // L) << 16) | (sl % L)).to(torch.int32).contiguous()
                a_rep = a_row.expand(L * L, C).contiguous()
                bp["pad_rot"] = torch.empty(L * L, 3 * C, dtype=self._tdt, device=dev)
                self._linear(lib.EPI_QKV_ROPE, a_rep, bp["wqkv"], bp["bqkv"], bp["pad_rot"], L * L, 3 * C, C, rope=(rc, bp["rope_tab"], L, lib.ATTN_ROT_Q_SCALE),
                             variant=0)                               # (fp32x3: A = the plain f32 LayerNorm row, W in planes, the rotated rows as planes)
                keep += [a_rep, rc]
        torch.cuda.current_stream().synchronize()
        nfl = lib.load().toc3d_motion_weights_floats()
        # positional_encoding.py:18,32 -- same torch expression as the reference, evaluated on the host
        d3, d1 = dim_t(128).to(dev), dim_t(256).to(dev)
        pk = gemm.Packer(self._dts, dev)
        f = pk.f32
        P["scorers"] = []
        P["motion_all"] = torch.empty(len(self.score_predictor), nfl, dtype=torch.float32, device=dev)
        P["motion_stride"] = nfl
        for si, sp in enumerate(self.score_predictor):
            q = {}
            mw = P["motion_all"][si]
            srcs = [f(sp.query_embedding[0].weight), f(sp.query_embedding[0].bias), f(sp.query_embedding[2].weight), f(sp.query_embedding[2].bias)]
            for mln in (sp.ego_pose_pe, sp.ego_pose_queries):
                srcs += [f(mln.reduce[0].weight), f(mln.reduce[0].bias), f(mln.gamma.weight), f(mln.gamma.bias), f(mln.beta.weight), f(mln.beta.bias)]
            srcs += [f(sp.time_embedding[0].weight), f(sp.time_embedding[0].bias), f(sp.time_embedding[1].weight), f(sp.time_embedding[1].bias),
                     f(sp.pc_range), d3, d1]
            keep.append(srcs)
            lib.call("toc3d_pack_motion_weights", *srcs, mw, s)
            q["motion"] = mw
            q["w_in"], q["b_in"] = f(sp.input_proj[0].weight), f(sp.input_proj[0].bias)
            q["w_agg"], q["b_agg"] = f(sp.aggregate[0].weight), f(sp.aggregate[0].bias)
            q["scale"] = QUERY_DIM ** -0.5 if self.pruning_attn_scale else 1.0
            # first-frame scorer (ScoreBasedTokenSelector.score)
            q["ln_w"], q["ln_b"] = f(sp.in_conv[0].weight), f(sp.in_conv[0].bias)
            q["w_ic"], q["b_ic"] = pk.wb(sp.in_conv[1].weight, sp.in_conv[1].bias)
            q["w_o0"], q["b_o0"] = pk.wb(sp.out_conv[0].weight, sp.out_conv[0].bias)
            q["w_o2"], q["b_o2"] = pk.wb(sp.out_conv[2].weight, sp.out_conv[2].bias)
            q["w_o4"], q["b_o4"] = f(sp.out_conv[4].weight), f(sp.out_conv[4].bias)
            P["scorers"].append(q)
        torch.cuda.current_stream().synchronize()
        return P

    def _plan(self, V, H, W, x, B):
        C, dev = self.embed_dim, x.device
        p = self.patch_size
        h, w = H // p, W // p
        sel_geo = {}
        max_rows, max_nw = 0, 0
        rows_fn = lib.load().toc3d_window_topk_rows
        for L in {self.window_size, self.global_window_size}:
            nW = V * (-(-h // L)) * (-(-w // L))
            max_nw = max(max_nw, nW)
            for st, r in enumerate(self.token_ratio):
                k = int(L * L * r)                        # toc3d_utils.py:138
                ms = int(rows_fn(V, h, w, L, k))          # compact rows: kept real tokens + one representative per window
                sel_geo[(st, L)] = (nW, L * L, k, ms)
                max_rows = max(max_rows, ms)
        plan = self._base_plan(V, H, W, x, B, max_rows)
        T, M = plan["T"], plan["M"]
        i32 = dict(dtype=torch.int32, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        plan["slow"] = torch.empty(max_rows, C, **f32)
        plan["rep1"] = torch.empty(max_nw, C, **f32)
        plan["rep2"] = torch.empty(max_nw, C, **f32)
        plan["rep3"] = torch.empty(max_nw, C, **f32)          # second block of a carried pair (carry_compact)
        plan["rep4"] = torch.empty(max_nw, C, **f32)
        # arrival counters + partial sums of the split merge (zeroed once: the kernel re-arms its counters)
        plan["gm_scratch"] = torch.zeros(int(lib.load().toc3d_gather_merge_ln_scratch_bytes(max_nw, C)) // 4, **f32)
        plan["sel"] = {}
        for key, (nW, N, k, ms) in sel_geo.items():
            L = key[1]
            plan["sel"][key] = dict(nW=nW, N=N, k=k, rows=ms, max_q=min(k, min(L, h) * min(L, w)) + 1,
                                    order=torch.empty(nW, N, **i32), tok=torch.empty(nW, N, **i32), wgt=torch.empty(nW, N, **f32),
                                    prow=torch.empty(nW, N, **i32), crow_tok=torch.empty(ms, **i32), rep_index=torch.empty(ms, **i32),
                                    rep_row=torch.empty(nW, **i32), arows=torch.empty(nW, k + 1, **i32),
                                    aslots=torch.empty(nW, k + 1, **i32), acount_q=torch.empty(nW, **i32), acount_k=torch.empty(nW, **i32),
                                    crow_rc=torch.zeros(ms, **i32))
            s = plan["sel"][key]
            s["win"] = Windows(s["crow_rc"], s["arows"], s["aslots"], s["acount_q"], s["acount_k"], None, k + 1, nW, s["max_q"])
        ns = len(self.pruning_loc)
        plan["pred"] = [torch.empty(M, 2, **f32) for _ in range(ns)]
        plan["u1"] = plan["u2"] = None                    # first-frame scorer scratch, allocated on demand
        return plan

    def _master_plan(self, V, H, W, B, dev):
        """The base's (x + one work plan per view group) + the shared outputs (masks, scores, image-level order), the query-side buffers and the staging buffers."""
        C, Q, ns = self.embed_dim, self.pruning_num_queries, len(self.pruning_loc)
        m = super()._master_plan(V, H, W, B, dev)
        T = m["T"]
        f32 = dict(dtype=torch.float32, device=dev)
        m.update(score=[torch.empty(V * T, **f32) for _ in range(ns)], mask=[torch.empty(V * T, **f32) for _ in range(ns)],
                 order=[torch.empty(V, T, dtype=torch.int64, device=dev) for _ in range(ns)],
                 prep=dict(mq=torch.empty(ns, B, Q, QUERY_DIM, **f32), wc=torch.empty(ns, B, C, 2, **f32), bc=torch.empty(ns, B, 2, **f32)))
        # Inputs that change pointer every frame are copied into fixed staging buffers in front of the frame (a few KB; the images
        # are read in place by the im2col kernel, which is launched directly), so the launch sequence itself only ever names
        # buffers of this plan and can be recorded once (toc3d_amd/plan.py).  Timestamps keep their dtype (f64 in the streaming
        # loop): both staging buffers exist, the plan key carries which one a recording used.
        m["stage"] = dict(tq=torch.empty(B, Q, QUERY_DIM, **f32), rp=torch.empty(B, Q, 3, **f32), vel=torch.empty(B, Q, 2, **f32),
                          ts32=torch.empty(B, Q, 1, **f32), ts64=torch.empty(B, Q, 1, dtype=torch.float64, device=dev),
                          pose=torch.empty(B, Q, 4, 4, **f32), inv=torch.empty(B, 4, 4, **f32), new=torch.zeros(B, **f32),
                          gumbel_all=torch.empty(ns, V * T, 2, **f32), rng=self._rng_state(dev))
        m["stage"]["gumbel"] = [m["stage"]["gumbel_all"][s_] for s_ in range(ns)]      # one buffer: the device-side draw fills all stages in one launch
        for gp in m["groups"]:
            gp["prep"], nv = m["prep"], gp["nv"]
            if len(m["groups"]) == 1:
                gp["score"], gp["mask"], gp["order"] = m["score"], m["mask"], m["order"]
            else:
                # Groups run on different streams, i.e. on different XCDs whose L2s are not coherent with each other: two
                # groups must never write into the same 128-byte line.  A slice boundary at T floats (4000 B at 800x320)
                # falls inside a line, so every group gets private, separately allocated score / mask / order buffers and
                # forward() copies them into the contiguous outputs after the streams have joined.
                gp["score"] = [torch.empty(nv * T, **f32) for _ in range(ns)]
                gp["mask"] = [torch.empty(nv * T, **f32) for _ in range(ns)]
                gp["order"] = [torch.empty(nv, T, dtype=torch.int64, device=dev) for _ in range(ns)]
        return m

    @property
    def gumbel_seed(self):
        return self._gumbel_seed

    @gumbel_seed.setter
    def gumbel_seed(self, seed):
        # the key is an argument of the recorded toc3d_gumbel_noise launch: plans recorded with the old key must not be replayed
        if seed != self._gumbel_seed:
            self._plans = {}
        self._gumbel_seed = seed

    def _rng_state(self, dev):
        """The model's Gumbel frame counter (uint64 [2]: counter, ticket) on ``dev`` -- created once, named by every recorded plan.  A model that
        moves to another device (or a copy restored from __getstate__) takes the counter's VALUE along: the stream continues, it is not replayed."""
        if self._gumbel_rng is None:
            self._gumbel_rng = torch.zeros(2, dtype=torch.int64, device=dev)
        elif self._gumbel_rng.device != dev:
            self._gumbel_rng = self._gumbel_rng.to(dev)
        if self._gumbel_seed is None:
            self._gumbel_seed = int(torch.initial_seed()) & 0x7fffffffffffffff
        return self._gumbel_rng

    # -- scorer stage (toc3d_eva_vit.py:264-285) -------------------------------------------------------
    # -- extension points of the test-only subclass (toc3d_amd/testing.py); the product forward carries no test switches -----------------
    _instrumented = False            # True: every frame launches eagerly (the subclass reads intermediate buffers between launches)

    def _stage_override(self, st, plan, score, mask):
        """After scorer stage ``st`` of one view group wrote its image-level scores / soft mask.  No-op here."""

    def _block_done(self, i, plan, carried):
        """After block ``i`` of one view group was issued (``carried``: its update of x is still pending in the compact rows).  No-op here."""

    def _run_frame(self, master, n_lanes, frame_fn, variant=None):
        if self._instrumented:
            frame_fn(EagerExec(n_lanes, self._stream_pool))
        else:
            super()._run_frame(master, n_lanes, frame_fn, variant)

    def _score_stage(self, ex, lane, side, prep_lane, st, plan, P, prev_exists, gumbel, frame_new=None):
        """One scorer stage of one view group (toc3d_eva_vit.py:264-285) on ``lane``; work that does not gate the block chain
        (image-level ranking, the selection of the window type the next block does not use) goes to the group's side lane (``side``: its lane / pending / L record of forward()).
        ``frame_new`` (a mixed step: f32 flags of this group's frames, device memory): the query path scores every row, then the
        static chain runs on every row and its last launch overwrites the rows of the flagged frames only."""
        s = lib.stream_ptr()
        q = P["scorers"][st]
        C, dt = self.embed_dim, self._dt
        V, T, M, B = plan["V"], plan["T"], plan["M"], plan["B"]
        x = plan["x"]
        mask_prev = plan["mask"][st - 1] if st > 0 else None        # masks start as ones (:251), replaced per stage (:266)
        g = gumbel[st]
        pred, score, mask = plan["pred"][st], plan["score"][st], plan["mask"][st]
        if prev_exists:
            if st == 0:
                ex.wait(lane, prep_lane)                            # query-side prep (all stages) ran on its own lane
            f0 = plan["frame0"]
            lib.call("toc3d_score_tokens", x, C, mask_prev, plan["prep"]["wc"][st][f0:f0 + B], plan["prep"]["bc"][st][f0:f0 + B], g, V, T, V // B,
                     pred, score, mask, s)
        if not prev_exists or frame_new is not None:
            # ScoreBasedTokenSelector.score (toc3d_utils.py:114-129); the reference also evaluates the motion-aware
            # queries here and discards them (:376-385) -- skipped, no observable effect
            t_act, u1, u2 = plan["att"], plan["u1"], plan["u2"]
            lib.call("toc3d_layernorm_rows", dt, x, C, None, mask_prev, q["ln_w"], q["ln_b"], self.SCORER_LN_EPS, plan["a"], C, M, C, s)
            self._linear(lib.EPI_GELU, plan["a"], q["w_ic"], q["b_ic"], t_act, M, C, C)
            lib.call("toc3d_global_mean_half", dt, t_act, C, V, T, C, s)
            self._linear(lib.EPI_GELU, t_act, q["w_o0"], q["b_o0"], u1, M, C // 2, C)
            self._linear(lib.EPI_GELU, u1, q["w_o2"], q["b_o2"], u2, M, C // 4, q["w_o2"].shape[1])
            if frame_new is None:
                lib.call("toc3d_score_head", dt, u2, u2.shape[1], C // 4, q["w_o4"], q["b_o4"], g, M, pred, score, mask, s)
            else:                                                   # a group holds B whole frames, or (B = 1) part of one: M // B rows per flag
                lib.call("toc3d_score_head_frames", dt, u2, u2.shape[1], C // 4, q["w_o4"], q["b_o4"], g, frame_new, M // B, M, pred, score, mask, s)
        self._stage_override(st, plan, score, mask)

        def topk(L):
            sel = plan["sel"][(st, L)]
            lib.call("toc3d_window_topk", score, V, plan["h"], plan["w"], L, sel["k"], sel["order"], sel["tok"], sel["wgt"], sel["prow"],
                     sel["crow_tok"], sel["rep_index"], sel["rep_row"], sel["arows"], sel["aslots"], sel["acount_q"], sel["acount_k"], sel["crow_rc"], lib.stream_ptr())
        # image-level keep/drop lists are only returned to the caller (vis / loss): rank them beside the blocks
        # ... and so is the selection for the window type the next block does not use (first needed two blocks later)
        first = self._block_side(self.pruning_loc[st])
        ex.wait(side.lane, lane)
        side.pending, side.L = True, None
        with ex.lane(side.lane):
            lib.call("toc3d_rank_desc", score, V, T, plan["order"][st], lib.stream_ptr())
            for L in {self.window_size, self.global_window_size} - {first}:
                topk(L)
                side.L = L
        topk(first)

    @staticmethod
    def _join_side(ex, lane, side):
        if side.pending:
            ex.wait(lane, side.lane)
            side.pending = False

    def _query_prep(self, ex, prep_lane, master, P, ts_key):
        """get_motion_aware_queries + the collapse of input_proj/einsum/aggregate for all stages and frames (identical
        inputs, per-stage weights; toc3d_utils.py:376-385), on its own lane beside the first six blocks."""
        prep, sg = master["prep"], master["stage"]
        ts = sg[ts_key]
        B, Q, C = sg["tq"].shape[0], sg["tq"].shape[1], self.embed_dim
        ns = len(self.pruning_loc)
        ex.wait(prep_lane, 0)
        with ex.lane(prep_lane):
            s = lib.stream_ptr()
            lib.call("toc3d_motion_queries", P["motion_all"], ns, P["motion_stride"], sg["tq"], sg["rp"], sg["vel"], ts, 1 if ts.dtype == torch.float64 else 0,
                     sg["pose"], sg["inv"], B, Q, prep["mq"], s)
            for st in range(ns):
                q = P["scorers"][st]
                lib.call("toc3d_collapse_query_scorer", prep["mq"][st], q["w_in"], q["b_in"], q["w_agg"], q["b_agg"], B, Q, C, float(q["scale"]),
                         prep["wc"][st], prep["bc"][st], s)

    def _accel_block(self, ex, lane, side, i, st, plan, P, carry_in=False, carry_out=False):
        """ToC3DEVAViTBlock.forward (toc3d_eva_vit.py:395-477).
        carry_out / carry_in (bf16 path, ``carry_compact``): two consecutive blocks of one window type and stage select the same
        tokens, so the second one continues on the first one's compact rows -- no scatter + gather in between.  Exact for the kept
        rows; the representative row it would re-merge from the updated dropped tokens, sum_j w_j (x_j + delta) = rep_in + W*delta,
        is rebuilt from the first block's updated row (toc3d_rebase_layernorm_rows; W != 1 in ragged windows, whose -1e6 pad scores enter the
        weight normalisation).  The dropped tokens receive all four updates at the end."""
        s = lib.stream_ptr()
        bp = P["blocks"][i]
        C = self.embed_dim
        if side.L == self._block_side(i):                 # this window type's selection was computed on the side lane
            self._join_side(ex, lane, side)
            side.L = None
        sel = plan["sel"][(st, self._block_side(i))]
        nW, N, k, rows = sel["nW"], sel["N"], sel["k"], sel["rows"]
        slow = plan["slow"]
        if carry_in:
            lib.call("toc3d_rebase_layernorm_rows", self._dt_rows, slow, C, sel["rep_index"], sel["tok"], sel["wgt"], N, k, plan["rep1"], plan["rep2"],
                     bp["ln1_w"], bp["ln1_b"], self.LN_EPS, plan["a"], C, rows, s)
        elif self.gather_split:
            lib.call("toc3d_gather_merge_ln_split", self._dt_rows, plan["x"], C, sel["tok"], sel["wgt"], sel["crow_tok"], sel["rep_row"], nW, N, k, rows,
                     bp["ln1_w"], bp["ln1_b"], self.LN_EPS, slow, plan["a"], C, 0 if self.gathered_residual else 1,
                     plan["gm_scratch"], plan["gm_scratch"].numel() * 4, int(self.gather_split) if self.gather_split is not True else 0, s)
        else:
            lib.call("toc3d_gather_merge_ln_ex", self._dt_rows, plan["x"], C, sel["tok"], sel["wgt"], sel["crow_tok"], sel["rep_row"], nW, N, k, rows,
                     bp["ln1_w"], bp["ln1_b"], self.LN_EPS, slow, plan["a"], C, 0 if self.gathered_residual else 1, s)
        self._qkv_attention(P, i, plan, rows, sel["win"])
        ra, rb = (plan["rep3"], plan["rep4"]) if carry_in else (plan["rep1"], plan["rep2"])
        via_x = self.gathered_residual and not carry_in  # kept rows were not copied: their residual comes from x through crow_tok
        self._proj(bp, plan, rows, slow, ra, sel["rep_index"], res=plan["x"] if via_x else None, res_index=sel["crow_tok"] if via_x else None)
        self._mlp(bp, plan, rows, slow, rb, sel["rep_index"])
        if not carry_out:
            lib.call("toc3d_scatter_update", plan["x"], C, sel["tok"], sel["prow"], nW, N, k, slow, plan["rep1"], plan["rep2"],
                     plan["rep3"] if carry_in else None, plan["rep4"] if carry_in else None, s)

    def _carries(self, i):
        """Block i may hand its compact rows to block i + 1 (same stage, same window type, both accelerated)."""
        return (self.carry_compact and i + 1 < self.depth and self._accelerated(i) and self._accelerated(i + 1)
                and (i + 1) not in self.pruning_loc and self._block_side(i) == self._block_side(i + 1))

    @torch.no_grad()
    def forward(self, x, temp_queries=None, prev_exists=None, temp_ref_points=None, temp_vel=None, temp_timestamp=None,
                temp_ego_pose=None, ego_pose_inv=None, *args, gumbel_noise=None, **kwargs):
        if "forced_scores" in kwargs:
            raise TypeError("forced_scores is a test instrument: wrap the model with toc3d_amd.testing.instrument(model)")
        # the reference's detector passes a Python bool (petr3d.py:122,155); a tensor costs one host sync per frame
        B = temp_queries.shape[0] if temp_queries is not None else 1
        mixed = None                                             # a list / tuple of B Python bools: one per frame (B camera streams stepped together)
        if isinstance(prev_exists, (list, tuple)):
            flags = tuple(bool(p) for p in prev_exists)
            if temp_queries is None:
                B = len(flags)
            if len(flags) != B:
                raise ValueError(f"prev_exists has {len(flags)} entries for {B} frames")
            prev = any(flags)                                    # all True / all False: the two paths of the single bool, launch for launch
            if prev and not all(flags):
                mixed = flags                                    # some frames start a scene, the others continue: the third recorded mode
        else:
            prev = bool(prev_exists.bool().flatten()[0].item()) if isinstance(prev_exists, torch.Tensor) else bool(prev_exists)
        x, plan = self._master(x, B)
        P, dev, V, ns = self._packed, x.device, x.shape[0], len(self.pruning_loc)
        groups, sg = plan["groups"], plan["stage"]
        G, T = len(groups), plan["T"]
        s0 = lib.stream_ptr()

        # ---- per-frame inputs -> the plan's staging buffers (tiny copies on the caller's stream, in front of the frame) -----------
        ts_key = "ts32"
        staged = []                                              # (dst, src) pairs, staged with ONE launch (every launch has a ~5 us floor)
        if prev and ns:
            assert temp_queries is not None and ego_pose_inv is not None, "prev_exists=True needs the memory-bank tensors"

            def put(dst, t, dtype=torch.float32):
                t = t.to(device=dev, dtype=dtype).contiguous()
                assert t.numel() == dst.numel(), (tuple(t.shape), tuple(dst.shape))
                staged.append((dst, t))                          # t stays referenced until the copy is enqueued (same stream: safe to free)
            put(sg["tq"], temp_queries), put(sg["rp"], temp_ref_points), put(sg["vel"], temp_vel)
            put(sg["pose"], temp_ego_pose), put(sg["inv"], ego_pose_inv)
            if temp_timestamp.dtype == torch.float64:            # the memory bank's f64 epoch timestamps
                ts_key = "ts64"
                put(sg["ts64"], temp_timestamp, torch.float64)
            else:
                put(sg["ts32"], temp_timestamp)
            if mixed is not None:
                # which frames are new, as f32 in device memory: the recorded mixed frame serves every pattern.  One small tensor per pattern seen,
                # made once (at most 2^B - 2 of them), so a step costs no host-to-device copy of its own
                pats = plan.setdefault("new_patterns", {})
                if mixed not in pats:
                    pats[mixed] = torch.tensor([0.0 if p else 1.0 for p in mixed], dtype=torch.float32, device=dev)
                staged.append((sg["new"], pats[mixed]))
        draw = gumbel_noise is None and ns > 0               # F.gumbel_softmax's own sampling (toc3d_utils.py:147), drawn inside the frame: toc3d_gumbel_noise
        for st in range(ns):
            if not draw:
                staged.append((sg["gumbel"][st], gumbel_noise[st].to(device=dev, dtype=torch.float32).reshape(V * T, 2).contiguous()))
        lib.copy_segments(staged, s0)
        if not prev or mixed is not None:
            for gp in groups:                                    # first-frame scorer scratch
                if gp["u1"] is None:
                    gp["u1"], gp["u2"] = (torch.zeros(gp["M"], max(64, self.embed_dim // d), dtype=self._tdt, device=dev) for d in (2, 4))

        # ---- the frame: lanes 0..G-1 = view groups, G..2G-1 = their side lanes, 2G = query-side scorer prep -----------------------
        # side_lanes=False (A/B switch): the scorer's query preparation and the rankings run on the block chain's own lane instead of beside it
        serial = not self.side_lanes
        prep_lane = 0 if serial else 2 * G

        def ahead(ex):
            if draw:
                # part of the recorded frame: the frame counter lives in device memory, so every replay draws fresh noise (one launch for all stages)
                lib.call("toc3d_gumbel_noise", sg["gumbel_all"], sg["gumbel_all"].numel(), self.gumbel_seed, sg["rng"], lib.stream_ptr())
            if prev and ns:
                self._query_prep(ex, prep_lane, plan, P, ts_key)

        def blocks(ex):
            # side-lane work of each group that is outstanding while the frame is issued: its lane, something was put there since the last join, the window
            # type whose selection runs there -- scheduler state of this pass, not of the plan
            sides = [SimpleNamespace(lane=g if serial else G + g, pending=False, L=None) for g in range(G)]
            st, pending = -1, False
            for i in range(self.depth):
                if i in self.pruning_loc:
                    st += 1
                # carried compact sets come in pairs (the scatter takes four updates): a block either receives one or may hand one on
                cin = pending
                cout = self._accelerated(i) and self._carries(i) and not cin
                pending = cout
                for g, gp in enumerate(groups):
                    with ex.lane(g):
                        if i in self.pruning_loc:
                            r0, r1 = gp["v0"] * T, (gp["v0"] + gp["nv"]) * T
                            new = None if mixed is None else sg["new"][gp["frame0"]:gp["frame0"] + gp["B"]]
                            self._score_stage(ex, g, sides[g], prep_lane, st, gp, P, prev, [gm[r0:r1] for gm in sg["gumbel"]], new)
                        if self._accelerated(i):
                            self._accel_block(ex, g, sides[g], i, st, gp, P, carry_in=cin, carry_out=cout)
                        else:
                            self._dense_block(i, gp, P)
                        self._block_done(i, gp, cout)
            for g, gp in enumerate(groups):
                with ex.lane(g):
                    self._join_side(ex, g, sides[g])
                    if G > 1:
                        # private per-group buffers -> the contiguous outputs, on the group's own lane (write-only, disjoint
                        # bytes; nothing reads the shared buffers before the join below)
                        v0, nv = gp["v0"], gp["nv"]
                        for st_ in range(ns):
                            lib.call("toc3d_copy_bytes", plan["mask"][st_][v0 * T:(v0 + nv) * T], gp["mask"][st_], nv * T * 4, lib.stream_ptr())
                            lib.call("toc3d_copy_bytes", plan["order"][st_][v0:v0 + nv], gp["order"][st_], nv * T * 8, lib.stream_ptr())
        self._drive(plan, x, 2 * G + 1, blocks, ahead, variant=("mixed" if mixed is not None else prev, ts_key, draw))
        h, w = plan["h"], plan["w"]
        cl = (lambda t: t) if self.alias_outputs else (lambda t: t.clone())
        masks = [cl(plan["mask"][s]).view(V, h, w, 1) for s in range(ns)]
        keep, drop = [], []
        for s in range(ns):
            kimg = int(T * self.token_ratio[s])
            order = cl(plan["order"][s])
            keep.append(order[:, :kimg])
            drop.append(order[:, kimg:])
        return _return_type()({self._out_features[0]: self._feature_view(plan)}, masks or None, None,
                              keep_idx=keep or None, drop_idx=drop or None, aux_outputs=None)
