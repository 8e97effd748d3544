"""``StreamPETRHead``: the assembled head -- every step of the reference's ``StreamPETRHead.forward`` (``dense_heads/streampetr_head.py:604-680``) at inference
time, under ONE ``pts_bbox_head.*`` state dict and the reference's type name.

The head owns the five modules of this package that each run one step and composes them exactly as the hand-written chain did::

    memory, pos_embed, cone = tokens(img_feats, intrinsics, lidar2img, pad_shape)          # HeadTokenEmbedding      :627-639
    bank.pre_update_memory(data)                                                           # TemporalMemory          :625
    tgt, query_pos, reference_points, temp_memory, temp_pos, rec_ego_pose = queries.forward_from(bank)    # HeadQueries :641-652
    outs_dec, _, _ = transformer(memory, tgt, query_pos, pos_embed, None, temp_memory, temp_pos)          # PETRTemporalTransformer :654
    outs_dec, all_cls_scores, all_bbox_preds = outputs(outs_dec, reference_points)         # HeadOutputs             :582-602
    bank.post_update_memory(data, rec_ego_pose, all_cls_scores, all_bbox_preds, outs_dec)  #                         :659

One set of tensors: the sub-modules are built first and the head registers THEIR parameter containers under the reference's names (``position_encoder``,
``memory_embed``, ``featurized_pe``, ``spatial_alignment``; ``reference_points``, ``query_embedding``, ``time_embedding``, ``ego_pose_pe``, ``ego_pose_memory``;
``cls_branches``, ``reg_branches``; ``transformer``), adds ``pseudo_reference_points`` and the reference's five frozen parameters (``code_weights``, ``match_costs``,
``pc_range``, ``position_range``, ``coords_d``, :207-231).  The token, query and output modules themselves are plain attributes, not registered children, so every
key appears once.  Packed weights, workspaces, recorded plans and the :class:`toc3d_amd.TemporalMemory` (built on first use on the module's device from
``pseudo_reference_points.weight``) are derived state: ``load_state_dict``, ``.to()`` and copies drop them; ``reset_memory()`` drops the bank.

Differences to the reference, by design:
* ``memory_center`` is accepted and NOT modified: the reference scales it by the padded image size in place (:392-393); the token kernel computes the pixel
  centres itself (``toc3d_head_frustum_inputs``) and never reads it;
* ``rec_ego_pose`` handed to ``post_update_memory`` holds ``num_query + num_propagated`` identities, not the reference's ``num_query + 2 * num_propagated``
  (:447-449), of which it can only index the former (see :class:`toc3d_amd.HeadQueries`);
* ``topk_indexes`` (``img_roi_head``) raises unless the head is built with ``token_sampling=True`` -- a keyword of this package: the list then goes to the token
  side (:class:`toc3d_amd.HeadTokenEmbedding`) and the decoder's cross-attention runs on its K keys per sample; training (``prepare_for_dn``, losses) and
  ``self.training`` raise; ``precision`` is ``"fp32x3"`` (default) or ``"bf16"``;
* ``coords_d`` is read from the parameter (a checkpoint's values win, as in the reference); ``pc_range`` / ``position_range`` reach the kernels as host copies
  of the config's values; as an extension to the reference, a checkpoint whose ranges differ from the config's by more than 1 % (more than a half / bf16
  rounding of the same numbers) is refused at load instead of being silently ignored.
No CPU path.
"""
from __future__ import annotations

from typing import Sequence

import torch
import torch.nn as nn

from . import gemm, registry
from . import plan as _plan
from .head_outputs import HeadOutputs
from .head_queries import HeadQueries
from .head_tokens import HeadTokenEmbedding
from .memory import TemporalMemory

_NAME = "toc3d_amd.StreamPETRHead"
_SUPPORTED = ("fp32x3", "bf16")
_DEFAULT_CODE_WEIGHTS = [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2]        # :122
_RENAMED = {".self_attn.": ".attentions.0.", ".multihead_attn.": ".attentions.1.", ".decoder.norm.": ".decoder.post_norm."}      # :550-555
_BANK = ("memory_embedding", "memory_reference_point", "memory_timestamp", "memory_egopose", "memory_velo")


def _bank_attr(name):
    return property(lambda self: None if self._bank is None else getattr(self._bank, name))


class StreamPETRHead(_plan.DerivedState, nn.Module):
    _version = 2                                # :63 -- state dicts saved without it (or with version < 2) get the key renames of :547-562

    def __init__(self, num_classes, in_channels=256, stride=16, embed_dims=256, num_query=100, num_reg_fcs=2, memory_len=1024, topk_proposals=256,
                 num_propagated=256, with_dn=True, with_ego_pos=True, match_with_velo=True, match_costs=None, transformer=None, sync_cls_avg_factor=False,
                 code_weights=None, bbox_coder=None, loss_cls=None, loss_bbox=None, loss_iou=None, train_cfg=None, test_cfg=dict(max_per_img=100),
                 depth_step=0.8, depth_num=64, LID=False, depth_start=1, position_range: Sequence[float] = (-65, -65, -8.0, 65, 65, 8.0), scalar=5,
                 noise_scale=0.4, noise_trans=0.0, dn_weight=1.0, split=0.5, init_cfg=None, normedlinear=False, precision=gemm.DEFAULT_PRECISION,
                 launch_mode="plan", levels="all", token_sampling=False, **kwargs):
        """Every keyword of the reference's ``__init__`` (:65-111); the ``pts_bbox_head=dict(...)`` block of the shipped configs builds it unchanged.  The loss,
        assigner, denoising (``with_dn``, ``scalar``, ``noise_*``, ``dn_weight``, ``split``), ``train_cfg`` and unknown keys (``with_position``) are accepted and
        ignored -- only ``loss_cls['use_sigmoid']`` is read (the reference sizes the class branch from it, :200-203; a missing ``loss_cls`` means the
        reference's default, a softmax classifier, and is refused like one).  Extra: ``precision``, ``launch_mode``, ``levels`` of :class:`toc3d_amd.HeadOutputs`, and
        ``token_sampling``: accept ``forward(..., topk_indexes=...)`` (off by default: the call raises as it always did)."""
        super().__init__()
        if precision not in _SUPPORTED:
            raise NotImplementedError(f"{_NAME}: precision {precision!r} is not implemented: the decoder and the class / box branches run in "
                                      f"{' or '.join(repr(p) for p in _SUPPORTED)} only")
        if not isinstance(transformer, dict) or not isinstance(bbox_coder, dict):
            raise ValueError(f"{_NAME}: needs transformer=dict(type='PETRTemporalTransformer', ...) and bbox_coder=dict(type='NMSFreeCoder', ...) (pc_range comes "
                             "from the coder, :215)")
        if loss_cls is None or not loss_cls.get("use_sigmoid", False):
            raise NotImplementedError(f"{_NAME}: a softmax classifier is not implemented: the reference sizes the class branch from loss_cls['use_sigmoid'] (:200-203) "
                                      "and its default loss_cls has none (num_classes + 1 outputs); pass loss_cls=dict(..., use_sigmoid=True) as the shipped configs do")
        self.code_size = int(kwargs.pop("code_size", 10))                                                  # :115-118
        cw = list(_DEFAULT_CODE_WEIGHTS if code_weights is None else code_weights)[:self.code_size]       # :119-124
        mc = cw if match_costs is None else list(match_costs)                                              # :126-129
        self.num_query, self.num_classes, self.cls_out_channels, self.in_channels = num_query, num_classes, num_classes, in_channels
        self.memory_len, self.topk_proposals, self.num_propagated = memory_len, topk_proposals, num_propagated
        self.with_dn, self.with_ego_pos, self.match_with_velo, self.num_reg_fcs = with_dn, with_ego_pos, match_with_velo, num_reg_fcs
        self.train_cfg, self.test_cfg, self.fp16_enabled, self.embed_dims = None, test_cfg, False, embed_dims
        self.depth_step, self.depth_num, self.position_dim, self.LID, self.depth_start, self.stride = depth_step, depth_num, depth_num * 3, LID, depth_start, stride
        self.num_pred, self.normedlinear, self.bg_cls_weight, self.sync_cls_avg_factor = 6, normedlinear, 0, sync_cls_avg_factor     # :192 -- six, whatever the decoder's depth
        self.precision, self.launch_mode, self.levels, self.token_sampling = precision, launch_mode, levels, bool(token_sampling)

        self.transformer = registry.build_transformer(transformer, precision=precision, launch_mode=launch_mode)                        # :205
        self.bbox_coder = registry.build_bbox_coder(bbox_coder)                                                                          # :213
        pc_range = [float(v) for v in self.bbox_coder.pc_range]
        # the modules that run the steps: plain attributes (their parameters are registered below, once, under the head's names)
        parts = self.__dict__
        parts["_tokens"] = HeadTokenEmbedding(in_channels=in_channels, embed_dims=embed_dims, depth_num=depth_num, depth_start=depth_start, LID=LID, stride=stride,
                                              position_range=position_range, precision=precision)
        parts["_queries"] = HeadQueries(num_query=num_query, memory_len=memory_len, num_propagated=num_propagated, embed_dims=embed_dims, with_ego_pos=with_ego_pos,
                                        pc_range=pc_range, precision=precision, launch_mode=launch_mode)
        parts["_outputs"] = HeadOutputs(num_classes=num_classes, embed_dims=embed_dims, num_reg_fcs=num_reg_fcs, code_size=self.code_size, num_pred=self.num_pred,
                                        normedlinear=normedlinear, pc_range=pc_range, bbox_coder=self.bbox_coder, precision=precision, launch_mode=launch_mode,
                                        levels=levels)
        if getattr(self.transformer, "embed_dims", embed_dims) != embed_dims:
            raise ValueError(f"{_NAME}: the transformer's embed_dims {self.transformer.embed_dims} != embed_dims {embed_dims}")
        t, q, o = self._tokens, self._queries, self._outputs
        self.cls_branches, self.reg_branches = o.cls_branches, o.reg_branches                                                           # :257-260
        self.position_encoder, self.memory_embed, self.featurized_pe = t.position_encoder, t.memory_embed, t.featurized_pe               # :262-275
        self.reference_points = q.reference_points                                                                                       # :277
        if num_propagated > 0:
            self.pseudo_reference_points = nn.Embedding(num_propagated, 3)                                                               # :279
        self.query_embedding, self.spatial_alignment, self.time_embedding = q.query_embedding, t.spatial_alignment, q.time_embedding     # :282-293
        if with_ego_pos:
            self.ego_pose_pe, self.ego_pose_memory = q.ego_pose_pe, q.ego_pose_memory                                                    # :296-298
        frozen = lambda v: nn.Parameter(torch.as_tensor(v, dtype=torch.float32).clone(), requires_grad=False)
        self.code_weights, self.match_costs = frozen(cw), frozen(mc)                                                                     # :207-211
        self.pc_range, self.position_range = frozen(pc_range), frozen([float(v) for v in position_range])                               # :215-219
        self.coords_d = frozen(t.coords_d)                                                                                               # :221-231 (the token module's expression is the reference's)
        t.bind_coords_d(self.coords_d)                              # the parameter IS the token kernel's depth bins: it moves and loads with the head
        self._drop_derived()

    # ---- derived state -------------------------------------------------------------------------------------------------------------------------
    _DERIVED = dict(_bank=None)

    def _drop_derived(self):
        super()._drop_derived()
        for part in ("_tokens", "_queries", "_outputs"):
            if part in self.__dict__:
                self.__dict__[part]._drop_derived()

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        version = local_metadata.get("version", None)                                                      # :547-562
        if version is None or version < 2:
            for k in list(state_dict.keys()):
                for old, new in _RENAMED.items():
                    if old in k:
                        state_dict[k.replace(old, new)] = state_dict.pop(k)
                        break
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)
        for name, host in (("pc_range", self._queries._pc), ("position_range", self._tokens._pr)):
            if not torch.allclose(getattr(self, name).detach().float().cpu(), host, rtol=1e-2, atol=0.0):       # (1 %: a checkpoint kept in half / bf16 is the same geometry)
                error_msgs.append(f"{_NAME}: {prefix}{name} = {getattr(self, name).tolist()} differs from the config's {host.tolist()}: the kernels take the "
                                  "ranges from the config (build the head from the config the checkpoint was trained with)")

    def _memory(self, device=None) -> TemporalMemory:
        if self._bank is None:
            dev = self.pc_range.device if device is None else torch.device(device)
            pseudo = self.pseudo_reference_points.weight if self.num_propagated > 0 else None
            self._bank = TemporalMemory(self.memory_len, self.topk_proposals, self.num_propagated, self.embed_dims, self._queries.pc_range, pseudo, device=dev)
        return self._bank

    def init_weights(self):                                                                                # :300-312
        self._queries.init_weights()
        if self.num_propagated > 0:
            nn.init.uniform_(self.pseudo_reference_points.weight.data, 0, 1)
            self.pseudo_reference_points.weight.requires_grad = False
        self.transformer.init_weights()
        self._outputs.init_weights()
        self._drop_derived()

    # ---- the memory bank: the reference's methods and attributes (:315-377; detectors/petr3d.py:115-136) --------------------------------------
    def reset_memory(self):
        self._bank = None

    def pre_update_memory(self, data):
        self._memory(data["prev_exists"].device if isinstance(data.get("prev_exists"), torch.Tensor) else None).pre_update_memory(data)

    def post_update_memory(self, data, rec_ego_pose, all_cls_scores, all_bbox_preds, outs_dec, mask_dict=None):
        self._memory().post_update_memory(data, rec_ego_pose, all_cls_scores, all_bbox_preds, outs_dec, mask_dict)

    def backbone_queries(self, num_proposals, prev_exists, batch_size=1):
        """What ``Petr3D.extract_img_feat`` hands to the backbone (``detectors/petr3d.py:115-134``): :meth:`toc3d_amd.TemporalMemory.backbone_queries`."""
        return self._memory().backbone_queries(num_proposals, prev_exists, batch_size)

    memory_embedding, memory_reference_point, memory_timestamp, memory_egopose, memory_velo = map(_bank_attr, _BANK)

    # ---- forward ---------------------------------------------------------------------------------------------------------------------------------
    def img_feats_rows_buffer(self, B, N, h, w, device=None):
        """``(rows, ld, dtype)`` of :meth:`toc3d_amd.HeadTokenEmbedding.feat_workspace`: where a producer of token rows (``CPFPN.forward_fanout``) puts them for
        ``forward(..., img_feats_rows=True)``."""
        return self._tokens.feat_workspace(B, N, h, w, self.pc_range.device if device is None else device)

    @torch.no_grad()
    def forward(self, memory_center, img_metas, topk_indexes=None, img_feats_rows=False, **data):
        """``data``: ``img_feats`` (B, N, C, h, w), ``intrinsics`` / ``lidar2img`` (B, N, 4, 4), ``prev_exists`` (B,), ``timestamp`` (B,) f64, ``ego_pose`` /
        ``ego_pose_inv`` (B, 4, 4) -- what ``Petr3D.forward_pts_train`` / ``simple_test_pts`` pass (``petr3d.py:319-320``); ``img_metas[0]['pad_shape'][0]`` =
        (pad_h, pad_w[, 3]).  ``memory_center`` is accepted and left as it is (module docstring).  Returns ``dict(all_cls_scores (L, B, Q, num_classes),
        all_bbox_preds (L, B, Q, code_size), dn_mask_dict=None)`` with Q = num_query + num_propagated and L = the decoder's layers (1 with ``levels="last"``).
        ``img_feats_rows=True``: the token rows of ``img_feats`` already sit in :meth:`img_feats_rows_buffer` of its shape (a detector's neck put them there); the
        tensor gives the shape and the device and is not read.
        ``topk_indexes`` (B, K, 1) or (B, K) int64 on the device (``FocalHead``'s), with ``token_sampling=True`` only: the token side and the decoder's
        cross-attention run on the K listed tokens of every sample; queries, outputs and both memory updates are what they are without it."""
        if self.training:
            raise RuntimeError(f"{_NAME}: training mode is not implemented (call .eval(): denoising queries and the losses are out of scope)")
        if topk_indexes is not None and not self.token_sampling:
            raise NotImplementedError(f"{_NAME}: topk_indexes (token selection by img_roi_head) is not implemented on a head built without token_sampling=True; "
                                      "the shipped configs pass None at eval")
        x = data["img_feats"]
        if img_feats_rows:
            (B, N, C, h, w) = x.shape
            if C != self.in_channels or not x.is_cuda:
                raise ValueError(f"{_NAME}: img_feats {tuple(x.shape)} on {x.device} do not fit in_channels={self.in_channels} on the GPU")
            memory, pos_embed, _ = self._tokens.forward_rows((B, N, h, w), data["intrinsics"], data["lidar2img"], img_metas[0]["pad_shape"][0], x.device,
                                                             topk_indexes=topk_indexes)
        else:
            memory, pos_embed, _ = self._tokens(x, data["intrinsics"], data["lidar2img"], img_metas[0]["pad_shape"][0], topk_indexes=topk_indexes)
        bank = self._memory(x.device)
        bank.pre_update_memory(data)
        tgt, query_pos, reference_points, temp_memory, temp_pos, rec_ego_pose = self._queries.forward_from(bank)
        outs_dec, _, _ = self.transformer(memory, tgt, query_pos, pos_embed, None, temp_memory, temp_pos)
        outs_dec, all_cls_scores, all_bbox_preds = self._outputs(outs_dec, reference_points)
        bank.post_update_memory(data, rec_ego_pose, all_cls_scores, all_bbox_preds, outs_dec)
        return dict(all_cls_scores=all_cls_scores, all_bbox_preds=all_bbox_preds, dn_mask_dict=None)

    def get_bboxes(self, preds_dicts, img_metas, rescale=False):
        """``[[bboxes, scores, labels], ...]`` per sample (:1051-1071): :meth:`toc3d_amd.HeadOutputs.get_bboxes`."""
        return self._outputs.get_bboxes(preds_dicts, img_metas, rescale)
