"""StreamPETR's temporal decoder on the GPU: the reference's ``PETRTemporalTransformer`` (``models/utils/petr_transformer.py:431-517``, called at
``dense_heads/streampetr_head.py:580``) at eval time -- ``num_layers`` post-norm layers of ``self_attn, norm, cross_attn, norm, ffn, norm``
(``PETRTemporalDecoderLayer._forward`` :714-760) and the decoder's shared ``post_norm`` on every layer's output (:413-425).

It sits between :class:`toc3d_amd.HeadTokenEmbedding` (which hands out ``memory`` and ``pos_embed``) and
:meth:`toc3d_amd.TemporalMemory.post_update_memory` (which consumes ``outs_dec``).  Parameters live under the reference's state-dict names, so the
``pts_bbox_head.transformer.*`` slice of a StreamPETR / ToC3D checkpoint loads strictly.

Per frame (``csrc/mha.hip``, ``include/toc3d.h``): the projections and the FFN run on ``toc3d_linear``; ``nn.MultiheadAttention.in_proj_weight`` is split into
its q, k, v thirds at pack time (q is projected from ``query + query_pos``, k from ``key + key_pos``, v from ``value``, :311-314).  The keys / values that do not
change over the layers -- ``memory (+ pos_embed)`` of the cross-attention and the ``temp_memory (+ temp_pos)`` rows of the self-attention -- are projected ONCE,
with the layers' weights concatenated along N (four GEMMs outside the layer loop instead of 24 inside).  Attention = ``toc3d_mha_attention_ex`` (keys streamed,
online softmax); every ``norm`` = ``toc3d_add_layernorm_pos``, which also writes the next projections' inputs and, after the FFN, the layer's slice of
``outs_dec``.  The layer loop is recorded once per shape into a launch plan and replayed with one C call per frame.  No CPU path.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import gemm, lib
from .gemm import DEFAULT_PRECISION
from .staged import StagedModule, require_cuda

_ORDER = ("self_attn", "norm", "cross_attn", "norm", "ffn", "norm")


class _Attention(nn.Module):                # parameter container: PETRMultiheadAttention / mmcv MultiheadAttention keep an nn.MultiheadAttention under `.attn`
    def __init__(self, embed_dims, num_heads):
        super().__init__()
        self.embed_dims, self.num_heads = embed_dims, num_heads
        self.attn = nn.MultiheadAttention(embed_dims, num_heads)


class _FFN(nn.Module):                      # mmcv FFN, num_fcs = 2: layers.0.0 = Linear(E, F), layers.1 = Linear(F, E)
    def __init__(self, embed_dims, feedforward_channels):
        super().__init__()
        self.layers = nn.Sequential(nn.Sequential(nn.Linear(embed_dims, feedforward_channels), nn.ReLU(inplace=True), nn.Dropout(0.0)),
                                    nn.Linear(feedforward_channels, embed_dims), nn.Dropout(0.0))


class _Layer(nn.Module):
    def __init__(self, embed_dims, num_heads, feedforward_channels):
        super().__init__()
        self.attentions = nn.ModuleList([_Attention(embed_dims, num_heads) for _ in range(2)])
        self.ffns = nn.ModuleList([_FFN(embed_dims, feedforward_channels)])
        self.norms = nn.ModuleList([nn.LayerNorm(embed_dims) for _ in range(3)])


class _Decoder(nn.Module):
    def __init__(self, num_layers, embed_dims, num_heads, feedforward_channels):
        super().__init__()
        self.layers = nn.ModuleList([_Layer(embed_dims, num_heads, feedforward_channels) for _ in range(num_layers)])
        self.post_norm = nn.LayerNorm(embed_dims)
        self.embed_dims = embed_dims


SPLITK_VARIANT, _tile_variant = gemm.SPLITK_VARIANT, gemm.small_m_variant      # re-exported: tests read the query-side tile rule from here


def _parse(encoder, decoder):
    """The config family of the shipped files (projects/configs/ToC3D/ToC3D_faster.py:114-139) -> (num_layers, embed_dims, num_heads, feedforward_channels)."""
    def no(what):
        raise NotImplementedError(f"toc3d_amd.PETRTemporalTransformer: {what} is not implemented (supported: the post-norm PETRTransformerDecoder of the "
                                  "shipped configs -- PETRTemporalDecoderLayer with MultiheadAttention + PETRMultiheadAttention, head_dim 32, return_intermediate=True)")
    if encoder is not None:
        no("an encoder")
    if not isinstance(decoder, dict):
        no("a decoder that is not a config dict")
    d = dict(decoder)
    if d.pop("type", "PETRTransformerDecoder") != "PETRTransformerDecoder":
        no(f"decoder type {decoder.get('type')!r}")
    if not d.pop("return_intermediate", False):
        no("return_intermediate=False")
    if d.pop("post_norm_cfg", dict(type="LN")) != dict(type="LN"):
        no("a post_norm_cfg other than dict(type='LN')")
    num_layers = d.pop("num_layers", None)
    lay = d.pop("transformerlayers", None)
    d.pop("init_cfg", None)
    if d or not isinstance(lay, dict) or not isinstance(num_layers, int) or num_layers < 1:
        no(f"this decoder config (unknown keys {sorted(d)})")
    lay = dict(lay)
    if lay.pop("type", None) != "PETRTemporalDecoderLayer":
        no("a transformer layer other than PETRTemporalDecoderLayer")
    if tuple(lay.pop("operation_order", ())) != _ORDER:
        no(f"operation_order other than {_ORDER} (pre-norm or otherwise)")
    if lay.pop("norm_cfg", dict(type="LN")) != dict(type="LN"):
        no("a norm_cfg other than dict(type='LN')")
    if lay.pop("batch_first", False):
        no("batch_first layers")
    attn = lay.pop("attn_cfgs", None)
    if isinstance(attn, dict):
        attn = [attn, attn]
    if not isinstance(attn, (list, tuple)) or len(attn) != 2:
        no("attn_cfgs that are not two attention configs")
    dims = set()
    for a, allowed in zip(attn, (("MultiheadAttention", "PETRMultiheadAttention"), ("PETRMultiheadAttention",))):
        a = dict(a)
        if a.get("type") not in allowed:
            no(f"attention type {a.get('type')!r}")
        extra = set(a) - {"type", "embed_dims", "num_heads", "dropout", "attn_drop", "proj_drop", "dropout_layer", "fp16", "init_cfg", "batch_first"}
        if extra or a.get("batch_first", False):
            no(f"attention options {sorted(extra)}")
        dims.add((a.get("embed_dims"), a.get("num_heads")))
    if len(dims) != 1:
        no("attentions of different widths")
    E, H = dims.pop()
    if not (isinstance(E, int) and isinstance(H, int) and H > 0 and E == 32 * H):
        no(f"embed_dims / num_heads = {E} / {H} != 32")
    ffn = lay.pop("ffn_cfgs", None)
    F = lay.pop("feedforward_channels", None)
    for k in ("ffn_dropout", "with_cp", "init_cfg"):          # dropout values are accepted and ignored (eval); checkpointing is a training device
        lay.pop(k, None)
    if ffn is not None:
        ffn = dict(ffn)
        if ffn.get("type", "FFN") != "FFN" or ffn.get("num_fcs", 2) != 2 or ffn.get("embed_dims", E) != E or not ffn.get("add_identity", True) \
                or ffn.get("act_cfg", dict(type="ReLU")).get("type") != "ReLU":
            no("an FFN other than mmcv's two-layer ReLU FFN with identity")
        F = ffn.get("feedforward_channels", F)
    elif E != 256:
        no("embed_dims != 256 without ffn_cfgs (the reference's default ffn_cfgs pins 256)")
    if F is None:
        F = 1024                                               # the layer's default ffn_cfgs (petr_transformer.py:559-566)
    if lay:
        no(f"layer options {sorted(lay)}")
    if E % 64 or F % 64:
        no("embed_dims or feedforward_channels that are not multiples of 64")
    return num_layers, E, H, F


class PETRTemporalTransformer(StagedModule):
    _NAME, _RUNS, _SUPPORTED = "toc3d_amd.PETRTemporalTransformer", "the decoder runs", ("bf16", "fp32x3")
    _INSTANCE = dict(StagedModule._INSTANCE, capture=None)

    def __init__(self, encoder=None, decoder=None, init_cfg=None, cross=False, precision=DEFAULT_PRECISION, launch_mode="plan"):
        super().__init__()
        L, E, H, F = _parse(encoder, decoder)
        self._init_staged(precision, launch_mode)
        self.encoder = None
        self.decoder = _Decoder(L, E, H, F)
        self.embed_dims, self.num_heads, self.feedforward_channels, self.num_layers, self.cross = E, H, F, L, cross
        self.capture = None                    # test instrument: a dict here receives clones of every norm's output (eager launches only)

    def init_weights(self):                    # petr_transformer.py:461-466
        for m in self.modules():
            if hasattr(m, "weight") and isinstance(m.weight, torch.Tensor) and m.weight.dim() > 1:
                nn.init.xavier_uniform_(m.weight)
        self._drop_derived()

    # ------------------------------------------------------------------------------------------------------------------------------
    def _pack(self, pk):
        dts, pack = pk.dts, pk.wb                                  # (fp32x3: weights as (hi, lo) planes)
        layers = []
        thirds = lambda a: (a.attn.in_proj_weight.detach().chunk(3), a.attn.in_proj_bias.detach().chunk(3))
        ck, cv, tk, tv = [], [], [], []
        for lay in self.decoder.layers:
            (sq, sk, sv), (sbq, sbk, sbv) = thirds(lay.attentions[0])
            (cq, ckw, cvw), (cbq, cbk, cbv) = thirds(lay.attentions[1])
            ck.append((ckw, cbk)); cv.append((cvw, cbv)); tk.append((sk, sbk)); tv.append((sv, sbv))
            f0, f1 = lay.ffns[0].layers[0][0], lay.ffns[0].layers[1]
            layers.append(dict(s_qk=pack(torch.cat([sq, sk]), torch.cat([sbq, sbk])), s_v=pack(sv, sbv),
                               s_o=pk.linear(lay.attentions[0].attn.out_proj), c_q=pack(cq, cbq), c_o=pk.linear(lay.attentions[1].attn.out_proj),
                               f0=pk.linear(f0), f1=pk.linear(f1), norms=[pk.layernorm(n) for n in lay.norms]))
        cat = lambda ps: pack(torch.cat([w for w, _ in ps]), torch.cat([b for _, b in ps]))
        # (the attention reads and writes plain rows: bf16 x 3 products on fp32x3, no planes)
        return dict(dt=dts.act, tdt=dts.torch, dta=gemm.attn_dtype(self.precision, x3_attention=True, planes_out=False), layers=layers,
                    ck=cat(ck), cv=cat(cv), tk=cat(tk), tv=cat(tv), post=pk.layernorm(self.decoder.post_norm)[:2])

    def _alloc(self, key, dev):
        B, Nq, Nk, Nm = key
        E, F, L, tdt = self.embed_dims, self.feedforward_channels, self.num_layers, self._packed["tdt"]
        z = lambda r, c, d=tdt: torch.zeros(r, c, dtype=d, device=dev)
        f = torch.float32
        W = dict(memory=z(B * Nk, E, f), pos=z(B * Nk, E, f), tgt=z(B * Nq, E, f), qpos=z(B * Nq, E, f),
                 mem_a=z(B * Nk, E), mem_pa=z(B * Nk, E), ck=z(B * Nk, L * E), cv=z(B * Nk, L * E),
                 x=[z(B * Nq, E, f) for _ in range(3)], y=z(B * Nq, E, f), xa=z(B * Nq, E), xpa=z(B * Nq, E), qk=z(B * Nq, 2 * E), v=z(B * Nq, E),
                 att=z(B * Nq, E), qc=z(B * Nq, E), h=z(B * Nq, F), outs=torch.zeros(L, B * Nq, E, dtype=f, device=dev))
        if Nm:
            W.update(tmem=z(B * Nm, E, f), tpos=z(B * Nm, E, f), tm_a=z(B * Nm, E), tm_pa=z(B * Nm, E), tk=z(B * Nm, L * E), tv=z(B * Nm, L * E))
        return W

    def _frame(self, key, W):
        """The launch sequence of one frame on the staged inputs of workspace ``W`` (eager or being recorded)."""
        P, (B, Nq, Nk, Nm) = self._packed, key
        E, F, L, H = self.embed_dims, self.feedforward_channels, self.num_layers, self.num_heads
        dt, dta = P["dt"], P["dta"]
        Mq = B * Nq
        cap = None if lib.recording() else self.capture
        s, linear = lib.stream_ptr(), self._linear

        def norm(nrm, x_out, act=None, act_pos=None, post=None, out2=None):
            g, b, eps = nrm
            lib.call("toc3d_add_layernorm_pos", dt, W["y"], E, g, b, eps, W["qpos"], E, x_out, E, act, E, act_pos, E,
                     None if post is None else post[0], None if post is None else post[1], out2, E, Mq, E, s)

        def attention(q, ldq, k, ldk, v, ldv, nk, k2=None, v2=None, ld2=0, nk2=0):
            lib.call("toc3d_mha_attention_ex", dta, q, ldq, k, ldk, v, ldv, k2, ld2, v2, ld2, W["att"], E, B, Nq, nk, nk2, H, E // H,
                     float(E // H) ** -0.5, s)

        off = lambda t, l: t.data_ptr() + l * E * t.element_size()       # layer l's E columns of a [rows, L * E] buffer
        # once per frame: the inputs in the form the projections read, and the layer-independent keys / values of all layers
        lib.call("toc3d_add_pos_rows", dt, W["memory"], E, W["pos"], E, W["mem_a"], E, W["mem_pa"], E, B * Nk, E, s)
        linear(W["mem_pa"], P["ck"], W["ck"], B * Nk, L * E, E)
        linear(W["mem_a"], P["cv"], W["cv"], B * Nk, L * E, E)
        if Nm:
            lib.call("toc3d_add_pos_rows", dt, W["tmem"], E, W["tpos"], E, W["tm_a"], E, W["tm_pa"], E, B * Nm, E, s)
            linear(W["tm_pa"], P["tk"], W["tk"], B * Nm, L * E, E)
            linear(W["tm_a"], P["tv"], W["tv"], B * Nm, L * E, E)
        lib.call("toc3d_add_pos_rows", dt, W["tgt"], E, W["qpos"], E, W["xa"], E, W["xpa"], E, Mq, E, s)
        x = W["tgt"]
        x1, x2, x3 = W["x"]
        for l, lp in enumerate(P["layers"]):
            # self_attn (:715-734): q, k from query + query_pos, v from query; keys = [query; temp_memory]
            linear(W["xpa"], lp["s_qk"], W["qk"], Mq, 2 * E, E)
            linear(W["xa"], lp["s_v"], W["v"], Mq, E, E)
            k_self = W["qk"].data_ptr() + E * W["qk"].element_size()          # the k half of the fused q | k rows
            if Nm:
                attention(W["qk"], 2 * E, k_self, 2 * E, W["v"], E, Nq, off(W["tk"], l), off(W["tv"], l), L * E, Nm)
            else:
                attention(W["qk"], 2 * E, k_self, 2 * E, W["v"], E, Nq)
            linear(W["att"], lp["s_o"], W["y"], Mq, E, E, residual=x)
            norm(lp["norms"][0], x1, act_pos=W["xpa"])
            # cross_attn (:741-754)
            linear(W["xpa"], lp["c_q"], W["qc"], Mq, E, E)
            attention(W["qc"], E, off(W["ck"], l), L * E, off(W["cv"], l), L * E, Nk)
            linear(W["att"], lp["c_o"], W["y"], Mq, E, E, residual=x1)
            norm(lp["norms"][1], x2, act=W["xa"])
            # ffn (:756-759)
            linear(W["xa"], lp["f0"], W["h"], Mq, F, E)
            lib.call("toc3d_relu_inplace", dt, W["h"], W["h"].numel(), s)
            linear(W["h"], lp["f1"], W["y"], Mq, E, F, residual=x2)
            last = l == L - 1
            norm(lp["norms"][2], x3, act=None if last else W["xa"], act_pos=None if last else W["xpa"], post=P["post"], out2=W["outs"][l])
            x = x3
            if cap is not None:
                for n, t in enumerate((x1, x2, x3)):
                    cap[f"l{l}_norm{n}"] = t.clone().view(B, Nq, E)

    @torch.no_grad()
    def forward(self, memory, tgt, query_pos, pos_embed, attn_masks, temp_memory=None, temp_pos=None, mask=None, reg_branch=None):
        """Batch-first shapes as the reference (:467-517): ``memory``, ``pos_embed`` (B, Nk, E) -- exactly what ``HeadTokenEmbedding.forward`` returns;
        ``tgt`` (``None`` = zeros), ``query_pos`` (B, Nq, E); ``temp_memory``, ``temp_pos`` (B, Nm, E) or both ``None`` (self-attention keys = the queries alone).
        ``attn_masks``: ``None`` or a bool tensor without a ``True`` (the eval-time mask, streampetr_head.py:643-647); ``mask`` must be ``None``.

        Returns ``(outs_dec (L, B, Nq, E) f32, memory, None)``.  The reference's third element is the stack of head-averaged cross-attention maps; at
        eval nothing but ``TokenSelectionLoss`` reads them, so an inference library returns ``None`` there.  ``outs_dec`` is freshly allocated (it aliases no
        workspace); ``memory`` is the caller's tensor."""
        require_cuda(self._NAME, memory)
        if mask is not None:
            raise NotImplementedError("toc3d_amd.PETRTemporalTransformer: key_padding_mask is not implemented (the head passes None)")
        if attn_masks is not None and bool(torch.as_tensor(attn_masks).any()):
            raise NotImplementedError("toc3d_amd.PETRTemporalTransformer: attn_masks with masked entries -- training-time denoising queries are out of scope")
        if (temp_memory is None) != (temp_pos is None):
            raise ValueError("temp_memory and temp_pos come together or not at all")
        dev = memory.device
        B, Nk, E = memory.shape
        Nq = query_pos.shape[1]
        Nm = 0 if temp_memory is None else temp_memory.shape[1]
        assert E == self.embed_dims and query_pos.shape == (B, Nq, E) and pos_embed.shape == (B, Nk, E) and (tgt is None or tgt.shape == (B, Nq, E))
        assert Nm == 0 or (temp_memory.shape == (B, Nm, E) and temp_pos.shape == (B, Nm, E))
        with torch.cuda.device(dev):
            key = (B, Nq, Nk, Nm)
            W = self._workspace(key, dev)
            # inputs -> the fixed buffers the (recorded) launches read
            c = lambda t: t.detach().to(device=dev, dtype=torch.float32).reshape(-1, E).contiguous()
            pairs = [(W["memory"], c(memory)), (W["pos"], c(pos_embed)), (W["qpos"], c(query_pos))]
            if tgt is None:
                W["tgt"].zero_()
            else:
                pairs.append((W["tgt"], c(tgt)))
            if Nm:
                pairs += [(W["tmem"], c(temp_memory)), (W["tpos"], c(temp_pos))]
            lib.copy_segments(pairs, lib.stream_ptr())
            self._run(key, lambda: self._frame(key, W), mode="eager" if self.capture is not None else None)
            outs = W["outs"].clone().view(self.num_layers, B, Nq, E)
        return outs, memory, None
