"""``Petr3D``: the assembled detector -- the reference's top-level class (``detectors/petr3d.py``) at inference time, under the reference's type name, built
from this package's backbone (``ToC3DEVAViT`` / ``EVA_ViT``), neck (``CPFPN``) and head (``StreamPETRHead``).

``simple_test`` is one frame: ``extract_img_feat`` (backbone, neck; :84-243) and ``simple_test_pts`` (head, box decoding; :521-541), with the two places where the
ToC3D loop closes -- the head's memory bank supplies the backbone's motion queries of the NEXT frame (:115-157), and the scene token decides ``prev_exists`` and
``reset_memory()`` (:527-532, :546-549).  The ``model=dict(type='Petr3D', ...)`` block of a shipped config builds it unchanged.

One thing a detector that owns both modules does that the hand-written chain cannot: the neck's last launch fans its conv rows out
(``toc3d_neck_rows_fanout``, :meth:`toc3d_amd.CPFPN.forward_fanout`) -- to the NCHW tensor the reference ``.view()``s (:239; ``data['img_feats']``, the bits of a
separate ``CPFPN.forward``) and, in the same pass, to the token rows the head's ``memory_embed`` reads (``streampetr_head.py:629``), in the head's own workspace.
The head then runs on those rows (``forward(..., img_feats_rows=True)``): the transpose back, and the copy in front of it, are gone; every other launch and every
bit of the frame are the chain's.

Differences to the reference, by design:
* inference only: training mode, ``forward_train`` and ``forward(return_loss=True)`` raise ``NotImplementedError``;
  ``use_grid_mask`` is accepted (GridMask is the identity outside training, ``grid_mask.py:85``); ``test_time_print`` is accepted and ignored;
* ``token_select_vis=True`` (:562-579) is still refused BY THE CONSTRUCTOR, which the tests of the earlier surface pin; the step itself is there and is switched on
  after construction (:meth:`Petr3D.enable_token_vis`) or by :func:`build_vis_detector`, which takes the shipped ``token_vis_ToC3D`` blocks unchanged.  The
  overlays are rendered on the device (:class:`toc3d_amd.TokenVis`); every detection result and every piece of derived state keeps its bits.  The same holds
  for :meth:`Petr3D.enable_box_vis`, which draws the decoded boxes onto the camera views and a top-down panel (:class:`toc3d_amd.BoxVis`; the reference does that
  outside the detector, ``tools/visualize.py``);
* with ``aux_2d_only=True`` (the default) ``img_roi_head=dict(type='FocalHead', ...)`` is accepted and nothing is built from it: the reference returns
  ``topk_indexes=None`` at eval without calling it (:319-320).  A checkpoint's ``img_roi_head.*`` keys are then dropped from the unexpected keys of
  ``load_state_dict``; nothing else is forgiven;
* with ``aux_2d_only=False`` the block builds ``self.img_roi_head`` (:class:`toc3d_amd.FocalHead`, its sixteen tensors in the state dict and loaded strictly) and
  the head with ``token_sampling=True``: every frame FocalHead ranks the tokens and the head's token side and cross-attention run on the
  ``int(N*h*w * infer_ratio)`` best of each sample (:521-541).  ``simple_test_pts`` reads ``topk_indexes`` alone (:524-525), so it takes FocalHead's
  selection-only frame (``select_rows`` on the neck's rows, ``select`` on a foreign tensor): the class tower only, the bits of the full forward's list.
  ``forward_roi_head`` stays the reference's method and returns the full dict.  ``location`` (:311-316) is built once per shape and kept as derived state;
* the ``pts_*`` parts and ``img_rpn_head`` are accepted as ``None`` only; backbones and necks other than this package's are refused at construction;
* ``prev_exists`` reaches the backbone as the Python bool the scene-token comparison already is: no host synchronisation;
* ``extract_img_feat(img)`` does not squeeze the caller's ``img`` in place (:102 does);
* extra keywords: ``precision`` (handed to the three parts), ``gumbel_noise=`` on ``simple_test`` / ``extract_img_feat`` (handed to the backbone);
* extra methods: ``simple_test_streams`` / ``reset_streams`` -- B independent camera streams per step, scene changes per stream (``extract_img_feat`` then takes
  ``prev_exists`` as a list of B bools).
Derived state (packed weights, workspaces, plans, the bank) belongs to the parts; ``load_state_dict``, ``.to()`` and ``init_weights()`` drop it, and
``prev_scene_token`` with it.  No CPU path.
"""
from __future__ import annotations

import json
import os

import torch
import torch.nn as nn

from . import plan as _plan
from . import registry
from .backbone import EVA_ViT, ToC3DEVAViT
from .focal_head import FocalHead
from .head import StreamPETRHead
from .neck import CPFPN
from .token_vis import TokenVis
from .box_vis import BoxVis
from .nusc_results import POSE_KEYS, NuScenesResults
from .tracking import TRACKING_META, HungarianPubTracker, PubTracker, build_tracker

_NAME = "toc3d_amd.Petr3D"
_ABSENT = ("pts_voxel_layer", "pts_voxel_encoder", "pts_middle_encoder", "pts_fusion_layer", "pts_backbone", "pts_neck", "img_rpn_head")


def bbox3d2result(bboxes, scores, labels, attrs=None):
    """mmdet3d's ``bbox3d2result`` (``mmdet3d/core/bbox/transforms.py``) when mmdet3d is importable; otherwise the dict that function builds, on the CPU."""
    try:  # pragma: no cover - mmdet3d is not installed in the build image
        from mmdet3d.core import bbox3d2result as _impl
        return _impl(bboxes, scores, labels, attrs)
    except ImportError:
        pass
    result = dict(boxes_3d=bboxes.to("cpu"), scores_3d=scores.cpu(), labels_3d=labels.cpu())
    if attrs is not None:
        result["attrs_3d"] = attrs.cpu()
    return result


class Petr3D(_plan.DerivedState, nn.Module):
    def __init__(self, use_grid_mask=False, pts_voxel_layer=None, pts_voxel_encoder=None, pts_middle_encoder=None, pts_fusion_layer=None, img_backbone=None,
                 pts_backbone=None, img_neck=None, pts_neck=None, pts_bbox_head=None, img_roi_head=None, img_rpn_head=None, train_cfg=None, test_cfg=None,
                 num_frame_head_grads=2, num_frame_backbone_grads=2, num_frame_losses=2, stride=16, position_level=0, aux_2d_only=True, single_test=False,
                 pretrained=None, token_select_vis=False, vis_num_sample=20, vis_start_id=0, vis_out_path="./token_vis", test_time_print=False, precision=None):
        """Every keyword of the reference's ``__init__`` (:27-55), plus ``precision``."""
        super().__init__()
        given = dict(pts_voxel_layer=pts_voxel_layer, pts_voxel_encoder=pts_voxel_encoder, pts_middle_encoder=pts_middle_encoder, pts_fusion_layer=pts_fusion_layer,
                     pts_backbone=pts_backbone, pts_neck=pts_neck, img_rpn_head=img_rpn_head)
        present = [k for k in _ABSENT if given[k] is not None]
        if present:
            raise NotImplementedError(f"{_NAME}: {', '.join(present)} not implemented: the camera-only detector of the shipped configs passes None")
        if token_select_vis:
            raise NotImplementedError(f"{_NAME}: token_select_vis=True (petr3d.py:562-579) is not implemented as a constructor keyword: call enable_token_vis() on the "
                                      "built detector, or build it with toc3d_amd.build_vis_detector(cfg)")
        if position_level != 0:
            raise NotImplementedError(f"{_NAME}: position_level={position_level} is not implemented: the head reads neck level 0 (the shipped configs' default)")
        if not all(isinstance(c, dict) for c in (img_backbone, img_neck, pts_bbox_head)):
            raise ValueError(f"{_NAME}: needs img_backbone=dict(...), img_neck=dict(...) and pts_bbox_head=dict(...)")
        if img_roi_head is not None and not (isinstance(img_roi_head, dict) and img_roi_head.get("type") == "FocalHead"):
            raise NotImplementedError(f"{_NAME}: img_roi_head is accepted as dict(type='FocalHead', ...) or None only")
        kw = {} if precision is None else dict(precision=precision)
        # aux_2d_only=False: FocalHead selects the head's tokens at eval (:319-323).  Built first: what it refuses about its own config is the first thing said
        # (with aux_2d_only=True, or without the config block, nothing is built and the reference calls nothing: :319)
        roi = registry.build_head(img_roi_head, **kw) if not aux_2d_only and img_roi_head is not None else None
        if roi is not None and not isinstance(roi, FocalHead):
            raise NotImplementedError(f"{_NAME}: img_roi_head builds this package's FocalHead only, got {type(roi).__name__}")
        head_cfg = dict(pts_bbox_head)                                      # MVXTwoStageDetector.__init__: the head gets the pts slice of train_cfg / test_cfg
        head_cfg.update(train_cfg=train_cfg.get("pts") if train_cfg else None, test_cfg=test_cfg.get("pts") if test_cfg else None)
        if roi is not None:
            head_cfg["token_sampling"] = True                              # the head takes the roi head's topk_indexes
        self.img_backbone = registry.build_backbone(img_backbone, **kw)
        self.img_neck = registry.build_neck(img_neck, **kw)
        self.pts_bbox_head = registry.build_head(head_cfg, **kw)
        if not isinstance(self.img_backbone, (EVA_ViT, ToC3DEVAViT)) or not isinstance(self.img_neck, CPFPN) or not isinstance(self.pts_bbox_head, StreamPETRHead):
            raise NotImplementedError(f"{_NAME}: built from this package's EVA_ViT / ToC3DEVAViT, CPFPN and StreamPETRHead only, got "
                                      f"{type(self.img_backbone).__name__}, {type(self.img_neck).__name__}, {type(self.pts_bbox_head).__name__}")
        if self.img_neck.out_channels != self.pts_bbox_head.in_channels:
            raise ValueError(f"{_NAME}: the neck's out_channels {self.img_neck.out_channels} != the head's in_channels {self.pts_bbox_head.in_channels}")
        if roi is not None:
            if roi.in_channels != self.img_neck.out_channels:
                raise ValueError(f"{_NAME}: the neck's out_channels {self.img_neck.out_channels} != img_roi_head's in_channels {roi.in_channels}")
            self.img_roi_head = roi
        self.precision = precision
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.use_grid_mask = use_grid_mask
        self.num_frame_head_grads, self.num_frame_backbone_grads, self.num_frame_losses = num_frame_head_grads, num_frame_backbone_grads, num_frame_losses
        self.single_test, self.stride, self.position_level, self.aux_2d_only = single_test, stride, position_level, aux_2d_only
        self.query_backbone_selection = getattr(self.img_backbone, "pruning_loc", None) is not None                                     # :73-74
        self.token_select_vis, self.vis_num_sample, self.vis_out_path, self.vis_start_id, self.cur_id = False, vis_num_sample, vis_out_path, vis_start_id, 0
        self.test_time_print = test_time_print
        self._token_vis = None                                              # a TokenVis, made by enable_token_vis()
        self.box_vis, self.box_vis_num_sample, self.box_vis_start_id, self.box_vis_out_path, self.box_vis_cur_id = False, 0, 0, "./box_vis", 0
        self._box_vis = None                                                # a BoxVis, made by enable_box_vis()
        self.format_nusc_results, self.nusc_results = False, None           # a NuScenesResults, made by enable_nusc_results()
        self.track_results, self.tracker, self.tracking_score_threshold, self.tracking_results = False, None, 0.25, {}     # a PubTracker, made by enable_tracking()
        self._drop_derived()
        self.eval()

    with_img_neck, with_pts_bbox = True, True

    @property
    def with_img_roi_head(self):
        return getattr(self, "img_roi_head", None) is not None

    # ---- derived state: the parts keep their own; the detector's is the scene it is in, the tensor whose rows sit in the head's workspace and the roi head's
    # location (key, tensor) ------------------------------------------------------------------------------------------------------------------------------
    _DERIVED = dict(prev_scene_token=None, prev_scene_tokens=None, _fanned=None, last_frame=None, _location=None)

    def train(self, mode=True):
        if mode:
            raise NotImplementedError(f"{_NAME}: training mode is not implemented (inference only)")
        return super().train(False)

    def init_weights(self):
        if hasattr(self.img_backbone, "init_weights"):
            self.img_backbone.init_weights()
        self.pts_bbox_head.init_weights()
        for part in (self.img_backbone, self.img_neck):
            part._drop_derived()
        if self.with_img_roi_head:
            self.img_roi_head.init_weights()
        self._drop_derived()

    def load_state_dict(self, state_dict, strict=True, **kw):
        """Without an ``img_roi_head`` module (``aux_2d_only=True``) ``strict=True`` forgives exactly the ``img_roi_head.*`` keys of a shipped checkpoint: nothing
        at eval reads them (module docstring).  With one they load like every other key: a checkpoint without them is a "Missing key" error."""
        if self.with_img_roi_head:
            return super().load_state_dict(state_dict, strict=strict, **kw)
        kept = type(state_dict)((k, v) for k, v in state_dict.items() if not k.startswith("img_roi_head."))
        if hasattr(state_dict, "_metadata"):
            kept._metadata = state_dict._metadata
        return super().load_state_dict(kept, strict=strict, **kw)

    # ---- token selection overlays (:562-579) -----------------------------------------------------------------------------------------------------------------
    def enable_token_vis(self, vis_num_sample=20, vis_start_id=0, vis_out_path="./token_vis"):
        """What ``token_select_vis=True`` with these three keywords sets up in the reference (:48-55): from the next frame on, while ``vis_num_sample > 0``, every
        frame whose number ``cur_id`` (counted from this call) is at least ``vis_start_id`` is rendered into ``./{vis_out_path}/{cur_id}/``.  A dense backbone has
        no token masks: ``ValueError``."""
        if not self.query_backbone_selection:
            raise ValueError(f"{_NAME}: enable_token_vis needs a token-selecting backbone (ToC3DEVAViT with pruning_loc): a dense backbone has no masks")
        self.token_select_vis, self.vis_num_sample, self.vis_start_id, self.vis_out_path, self.cur_id = True, int(vis_num_sample), int(vis_start_id), vis_out_path, 0
        if self._token_vis is None:
            self._token_vis = TokenVis(patch_size=getattr(self.img_backbone, "patch_size", 16))
        return self

    def disable_token_vis(self):
        self.token_select_vis = False
        return self

    def _vis_norm_cfg(self, meta, img):
        """``img_metas[0]['img_norm_cfg']`` (:575); the uint8 image form, whose pipeline has no normalisation step to record one, takes the backbone's."""
        cfg = meta.get("img_norm_cfg") if isinstance(meta, dict) else None
        if cfg is None and img.dtype == torch.uint8:
            cfg = getattr(self.img_backbone, "img_norm_cfg", None)
        return cfg

    def _vis_step(self, img_metas, img, token_masks, keep_idxes, drop_idxes, streams=None):
        """:562-579, in the reference's place: after ``extract_img_feat``, before the head.  ``streams``: B, for a step of several camera streams -- counted once,
        stream b written under ``{cur_id}/stream{b}/``."""
        if not (self.token_select_vis and self.vis_num_sample > 0):
            return
        if self.cur_id >= self.vis_start_id:
            out = f"./{self.vis_out_path}/{self.cur_id}/"
            vis = self._token_vis
            rendered = vis.render(img, token_masks, keep_idxes, drop_idxes, self._vis_norm_cfg(img_metas[0], img))
            if streams is None:
                vis.write(rendered, out)
            else:
                n = rendered["ori"].shape[0] // streams
                for b in range(streams):
                    vis.write(rendered, f"{out}stream{b}/", views=range(b * n, (b + 1) * n))
            self.vis_num_sample -= 1
        self.cur_id += 1

    # ---- predicted boxes on the camera views and a top-down panel (no counterpart in the reference's detector: tools/visualize.py draws from a result JSON) ----
    def enable_box_vis(self, num_sample=20, start_id=0, out_path="./box_vis", **box_vis_kwargs):
        """From the next frame on, while ``num_sample > 0``, every frame whose number (counted from this call, with a counter of its own: ``box_vis_cur_id``) is at
        least ``start_id`` has its detections drawn into ``./{out_path}/{cur_id}/`` (``view{v}_pred.png``, ``bev_pred.png``); a step of several camera streams
        writes stream b under ``{cur_id}/stream{b}/``.  ``box_vis_kwargs`` go to :class:`toc3d_amd.BoxVis`.  Every result and every piece of derived state keeps
        its bits; the token overlays (:meth:`enable_token_vis`) may be on as well."""
        self._box_vis = BoxVis(**box_vis_kwargs)
        self.box_vis, self.box_vis_num_sample, self.box_vis_start_id, self.box_vis_out_path, self.box_vis_cur_id = True, int(num_sample), int(start_id), out_path, 0
        return self

    def disable_box_vis(self):
        self.box_vis = False
        return self

    def _box_vis_step(self, img_metas, data, bbox_list, streams=None):
        """In :meth:`_pts_results`: from the device tensors ``get_bboxes`` returned, before ``bbox3d2result`` moves them to the host.  Counts as
        :meth:`_vis_step` does."""
        if not (self.box_vis and self.box_vis_num_sample > 0):
            return
        if data.get("lidar2img") is None:
            raise ValueError(f"{_NAME}: box visualisation is enabled but the frame carries no lidar2img (data['lidar2img'], (B, N, 4, 4)): the boxes cannot be "
                             "projected into the views")
        if self.box_vis_cur_id >= self.box_vis_start_id:
            out = f"./{self.box_vis_out_path}/{self.box_vis_cur_id}/"
            vis, img, l2i = self._box_vis, data["img"], data["lidar2img"]
            for b, (bboxes, scores, labels) in enumerate(bbox_list):
                cfg = self._vis_norm_cfg(img_metas[b if streams is not None else 0], img)
                rendered = vis.render(img[b], bboxes, scores, labels, l2i[b], cfg)
                vis.write(rendered, out if streams is None else f"{out}stream{b}/")
            self.box_vis_num_sample -= 1
        self.box_vis_cur_id += 1

    # ---- submission records (the reference makes them after the run, on the host: mmdet3d/datasets/nuscenes_dataset.py:301-368, :576-657) ----------------------
    def enable_nusc_results(self, **nusc_results_kwargs):
        """From the next frame on every sample's detections are turned into nuScenes submission records on the device (:class:`toc3d_amd.NuScenesResults`, to
        which ``nusc_results_kwargs`` go) and added to ``self.nusc_results`` under ``img_metas[b]['sample_idx']``; ``self.nusc_results.dump(prefix)`` writes the
        file.  The poses are read from ``img_metas[b]``: ``lidar2ego_rotation``, ``lidar2ego_translation``, ``ego2global_rotation``, ``ego2global_translation``,
        the keys of a nuScenes info record.  Every result and every piece of derived state keeps its bits; both visualisations may be on as well."""
        self.nusc_results = NuScenesResults(**nusc_results_kwargs)
        self.format_nusc_results = True
        return self

    def disable_nusc_results(self):
        """Stops the formatting; ``self.nusc_results`` keeps what it has gathered."""
        self.format_nusc_results = False
        return self

    # ---- tracking ids (the reference tracks after the run, on the host, from results_nusc.json: nusc_tracking/pub_test.py:77-153) ------------------------------
    def enable_tracking(self, max_age=3, score_threshold=0.25, hungarian=False, **tracker_kwargs):
        """From the next frame on the submission records of every sample are tracked on the device (:func:`toc3d_amd.build_tracker`, to which ``hungarian`` and
        ``max_age`` -- ``pub_test.py``'s defaults are False and 3 -- and ``tracker_kwargs`` go: a :class:`toc3d_amd.PubTracker`, or with ``hungarian=True`` a
        :class:`toc3d_amd.HungarianPubTracker`, at most 512 records a sample), one tracker per camera stream, and the frame's tracking records (``pub_test.py:115-128``) are
        kept in ``self.tracking_results`` under ``img_metas[b]['sample_idx']``; :meth:`dump_tracking` writes the file.  Needs :meth:`enable_nusc_results`, whose
        records it steps on.  A stream's tracker starts afresh where the scene-token comparison of :meth:`simple_test` / :meth:`simple_test_streams` starts a
        scene.  THE TIMESTAMP is ``data['timestamp']``, the float64 ``(B,)`` tensor the frame carries: the frame's own time, where ``pub_test.py`` uses the sample's
        ``timestamp * 1e-6`` from the devkit (:54) -- the two differ where a dataset pipeline rebases or replaces the frame time, and then so do the time lags
        and with them the predicted positions; :meth:`PubTracker.track_file` on the dumped records is the route that is exact to the reference's script.  Every
        detection result, the records of ``nusc_results`` and every piece of derived state keep their bits."""
        if not self.format_nusc_results or self.nusc_results is None:
            raise ValueError(f"{_NAME}: enable_tracking needs the submission records it tracks: call enable_nusc_results() first")
        self._tracker_kwargs = dict(tracker_kwargs, max_age=max_age, class_names=self.nusc_results.class_names)
        self._tracker_hungarian = bool(hungarian)
        self.tracker = self._build_tracker()
        self.track_results, self.tracking_score_threshold = True, float(score_threshold)
        return self

    def _build_tracker(self, **more):
        return build_tracker(hungarian=self._tracker_hungarian, classes=(PubTracker, HungarianPubTracker), **dict(self._tracker_kwargs, **more))

    def disable_tracking(self):
        """Stops the tracking; ``self.tracking_results`` keeps what it has gathered."""
        self.track_results = False
        return self

    def dump_tracking(self, jsonfile_prefix):
        """``{jsonfile_prefix}/tracking_result.json`` (created with its directory) as ``pub_test.py:89-152`` writes it -> the path."""
        os.makedirs(jsonfile_prefix, exist_ok=True)
        path = os.path.join(jsonfile_prefix, "tracking_result.json")
        with open(path, "w") as fh:
            json.dump(dict(results=self.tracking_results, meta=dict(TRACKING_META)), fh)
        return path

    def _tracking_step(self, tokens, fixed, data, first):
        """The trackers' step on the records still on the device: one launch for all streams."""
        B = len(tokens)
        if fixed is None or B == 0:
            return
        if not self.format_nusc_results:
            raise ValueError(f"{_NAME}: tracking is enabled but the submission records are not (disable_tracking() before disable_nusc_results())")
        ts = data.get("timestamp")
        if not isinstance(ts, torch.Tensor) or ts.numel() != B:
            raise ValueError(f"{_NAME}: tracking is enabled but the frame carries no timestamp (data['timestamp'], float64 ({B},))")
        if self.tracker.num_streams != B:                                   # another number of streams: every stream starts afresh, as the head's bank does
            self.tracker = self._build_tracker(num_streams=B)
        dev = fixed["rec"].device
        out = self.tracker.step_fixed(fixed["rec"], fixed["score"], fixed["name"], fixed["kept"], ts.to(device=dev, dtype=torch.float64).reshape(B),
                                      [True] * B if first is None else first, self.tracking_score_threshold)
        host = {k: v.cpu().numpy() for k, v in dict(out, rec=fixed["rec"], score=fixed["score"], name=fixed["name"]).items()}
        annos = self.tracker.records_to_annos(host["rec"], host["score"], host["name"], host["track_id"], host["order"], host["num_out"], tokens)
        for token, a in zip(tokens, annos):
            self.tracking_results[token] = a

    def _nusc_results_step(self, img_metas, bbox_list, data=None, first=None):
        """In :meth:`_pts_results`: from the device tensors ``get_bboxes`` returned, before ``bbox3d2result`` moves them to the host; one launch for all samples
        (and one more for the trackers, after :meth:`enable_tracking`; ``first``: per sample, whether it starts a scene)."""
        if not self.format_nusc_results:
            if self.track_results:
                raise ValueError(f"{_NAME}: tracking is enabled but the submission records are not (disable_tracking() before disable_nusc_results())")
            return
        for b, meta in enumerate(img_metas[:len(bbox_list)]):
            for key in POSE_KEYS + ("sample_idx",):
                if key not in meta:
                    raise ValueError(f"{_NAME}: nuScenes results are enabled but img_metas[{b}] has no {key!r} (needed: sample_idx, {', '.join(POSE_KEYS)})")
        metas = img_metas[:len(bbox_list)]
        tokens = [m["sample_idx"] for m in metas]
        if self.track_results:                                              # the device half as well: the trackers step on it
            fixed, formatted = self.nusc_results.format_device(bbox_list, metas, tokens)
        else:
            fixed, formatted = None, self.nusc_results.format(bbox_list, metas, tokens)
        for token, annos in zip(tokens, formatted):
            self.nusc_results.add(token, annos)
        if self.track_results:
            self._tracking_step(tokens, fixed, data or {}, first)

    # ---- the reference's methods -------------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def extract_img_feat(self, img, len_queue=1, training_mode=False, gt_bboxes=None, centers2d=None, depths=None, prev_exists=None, ego_pose_inv=None,
                         gumbel_noise=None):
        """:84-243 at eval: ``(img_feats (B, N, C, h, w), token_masks, attn_scores, keep_idxes, drop_idxes)``.  ``prev_exists``: the Python bool of the scene-token
        comparison (a tensor costs one host synchronisation)."""
        if img is None:
            return None, None, None, None, None
        if training_mode or len_queue != 1:
            raise NotImplementedError(f"{_NAME}: extract_img_feat with training_mode / len_queue != 1 is not implemented (inference only)")
        B = img.size(0)
        if img.dim() == 6:
            img = img.flatten(1, 2)
        if img.dim() == 5:
            img = img.flatten(0, 1)                                                                                                     # :101-105
        if ego_pose_inv is not None and ego_pose_inv.dim() == 4:
            ego_pose_inv = ego_pose_inv.flatten(0, 1)
        head, backbone = self.pts_bbox_head, self.img_backbone
        if self.query_backbone_selection:
            assert prev_exists is not None                                                                                               # :121
            q = head.backbone_queries(backbone.pruning_num_queries, prev_exists, B)                                                     # :122-136
            extra = {} if gumbel_noise is None else dict(gumbel_noise=gumbel_noise)
            out = backbone(x=img, temp_queries=q["temp_queries"], temp_ref_points=q["temp_ref_points"], temp_vel=q["temp_vel"],
                           temp_timestamp=q["temp_timestamp"], temp_ego_pose=q["temp_ego_pose"], prev_exists=q["prev_exists"], ego_pose_inv=ego_pose_inv, **extra)
            token_masks, attn_scores, keep_idxes, drop_idxes, feats = out.token_masks, out.attn_scores, out.keep_idx, out.drop_idx, out.img_feats
        else:
            token_masks = attn_scores = keep_idxes = drop_idxes = None
            feats = backbone(img)
        feats = list(feats.values()) if isinstance(feats, dict) else list(feats)
        V, _, h, w = feats[0].shape
        rows, ld, dtype = head.img_feats_rows_buffer(B, V // B, h, w, feats[0].device)
        outs = self.img_neck.forward_fanout(feats, rows, ld, dtype)                                                                     # :189-190, and the head's :629
        BN, C, H, W = outs[self.position_level].size()
        img_feats = outs[self.position_level].view(B, BN // B, C, H, W)                                                                  # :239
        self._fanned = (img_feats, rows)
        return img_feats, token_masks, attn_scores, keep_idxes, drop_idxes

    def extract_feat(self, img, T, training_mode=False, gt_bboxes=None, centers2d=None, depths=None, prev_exists=None, ego_pose_inv=None):
        return self.extract_img_feat(img, T, training_mode, gt_bboxes, centers2d, depths, prev_exists, ego_pose_inv)                   # :246-260

    @torch.no_grad()
    def prepare_location(self, img_metas, **data):
        """:311-316 with ``misc.locations`` (:59-84): the normalised pixel centres, (B*N, h, w, 2).  (The head takes them and does not read them.)"""
        pad_h, pad_w = img_metas[0]["pad_shape"][0][:2]
        bs, n = data["img_feats"].shape[:2]
        h, w = data["img_feats"].shape[-2:]
        dev, s = data["img_feats"].device, self.stride
        shifts_x = (torch.arange(0, s * w, step=s, dtype=torch.float32, device=dev) + s // 2) / pad_w
        shifts_y = (torch.arange(0, h * s, step=s, dtype=torch.float32, device=dev) + s // 2) / pad_h
        shift_y, shift_x = torch.meshgrid(shifts_y, shifts_x, indexing="ij")
        location = torch.stack((shift_x.reshape(-1), shift_y.reshape(-1)), dim=1).reshape(h, w, 2)
        return location[None].repeat(bs * n, 1, 1, 1)

    @torch.no_grad()
    def forward_roi_head(self, location, **data):
        """:318-323: ``{'topk_indexes': None}`` with ``aux_2d_only`` or without an ``img_roi_head``; otherwise FocalHead's full dict -- from the neck's rows
        (``forward_rows``) when ``data['img_feats']`` is the tensor :meth:`extract_img_feat` returned last, from the tensor (``forward``) otherwise.
        (:meth:`simple_test_pts` does not call this: it reads ``topk_indexes`` alone and takes FocalHead's selection-only path.)"""
        if self.aux_2d_only or not self.with_img_roi_head:
            return {"topk_indexes": None}                                                                                                # :319-320
        x = data["img_feats"]
        rows = self._roi_rows(x) if self._is_fanned(x) else None
        if rows is None:
            return self.img_roi_head(location, **data)
        return self.img_roi_head.forward_rows(location, rows[0], rows[1], x.shape[0], x.shape[1], x.shape[3], x.shape[4])

    # ---- token selection (aux_2d_only=False) ---------------------------------------------------------------------------------------------------------------
    def _is_fanned(self, x):
        """``x`` is the tensor :meth:`extract_img_feat` returned last, and its rows are still the head's (new weights or a move of the head alone give it a
        new workspace)."""
        fanned = self._fanned
        return bool(fanned is not None and x is fanned[0]
                    and self.pts_bbox_head.img_feats_rows_buffer(x.shape[0], x.shape[1], x.shape[3], x.shape[4], x.device)[0] is fanned[1])

    def _roi_rows(self, x):
        """``(rows, ld)`` of the fanned frame as FocalHead's conv reads them: on ``"bf16"`` the bf16 rows the fan-out wrote into the head's workspace, otherwise
        the neck's own plain-f32 conv rows (the head's f32 rows may be (hi, lo) planes).  None where neither fits (``ld != in_channels``)."""
        B, N, _, h, w = x.shape
        roi = self.img_roi_head
        if roi.precision == "bf16":
            rows, ld = self._fanned[1], self._fanned[1].shape[1]
        else:
            rows, ld = self.img_neck.conv_rows(B * N, h, w)
        return (rows, ld) if ld == roi.in_channels and rows.dtype == (torch.bfloat16 if roi.precision == "bf16" else torch.float32) else None

    def _roi_location(self, img_metas, x):
        """:meth:`prepare_location`, once per (pad_shape, B, N, h, w, device): derived state, not rebuilt every frame."""
        key = (tuple(img_metas[0]["pad_shape"][0][:2]), x.shape[0], x.shape[1], x.shape[3], x.shape[4], x.device)
        if self._location is None or self._location[0] != key:
            self._location = (key, self.prepare_location(img_metas, img_feats=x))
        return self._location[1]

    def _check_keeps_tokens(self, img):
        """The ``ValueError`` of a selection that keeps no token, from the image's shape: before the frame's first launch.  (The uint8 form, whose padded size
        the backbone decides, is caught by :meth:`_select_tokens`, in front of the roi head's launches.)"""
        if self.aux_2d_only or not self.with_img_roi_head or not isinstance(img, torch.Tensor) or img.dim() < 5 or img.dtype == torch.uint8:
            return
        n = img.shape[-4] * (img.shape[-2] // self.stride) * (img.shape[-1] // self.stride)
        if int(n * self.img_roi_head.infer_ratio) == 0:
            raise ValueError(f"{_NAME}: img_roi_head keeps int({n} tokens * infer_ratio {self.img_roi_head.infer_ratio}) = 0 tokens: the head cannot attend to none")

    def _select_tokens(self, img_metas, data):
        """``(location, topk_indexes)`` for the head: ``(None, None)`` on the ``aux_2d_only`` path (:319-320); otherwise FocalHead's ``topk_indexes`` (B, K, 1)
        through its selection-only frame -- ``select_rows`` on the neck's rows of the fanned frame, ``select`` on any other tensor."""
        if self.aux_2d_only or not self.with_img_roi_head:
            return None, None
        x, roi = data["img_feats"], self.img_roi_head
        B, N, _, h, w = x.shape
        if int(N * h * w * roi.infer_ratio) == 0:
            raise ValueError(f"{_NAME}: img_roi_head keeps int({N * h * w} tokens * infer_ratio {roi.infer_ratio}) = 0 tokens: the head cannot attend to none")
        location = self._roi_location(img_metas, x)
        rows = self._roi_rows(x) if self._is_fanned(x) else None
        if rows is None:
            out = roi.select(location, img_feats=x)
        else:
            out = roi.select_rows(location, rows[0], rows[1], B, N, h, w)
        return location, out["topk_indexes"]

    @torch.no_grad()
    def simple_test_pts(self, img_metas, **data):
        """:521-541.  The head runs on the rows the neck left in its workspace when ``data['img_feats']`` is the tensor :meth:`extract_img_feat` returned last;
        any other tensor goes through the head's own transpose."""
        location, topk_indexes = self._select_tokens(img_metas, data)      # (aux_2d_only: None, None -- the location is what the head ignores, never built)
        if img_metas[0]["scene_token"] != self.prev_scene_token:
            self.prev_scene_token = img_metas[0]["scene_token"]
            data["prev_exists"] = data["img"].new_zeros(1)
            self.pts_bbox_head.reset_memory()
            first = [True]
        else:
            data["prev_exists"] = data["img"].new_ones(1)
            first = [False]
        return self._pts_results(img_metas, location, topk_indexes, data, first=first)

    def _pts_results(self, img_metas, location, topk_indexes, data, streams=None, first=None):
        """The head on ``data`` (``prev_exists`` decided by the caller) and the decoded lists, one per sample; after :meth:`enable_box_vis` the lists are drawn
        while they are still on the device (``streams``: B, for a step of several camera streams)."""
        fanned = self._is_fanned(data["img_feats"])
        self._fanned = None
        outs = self.pts_bbox_head(location, img_metas, topk_indexes, img_feats_rows=fanned, **data)
        bbox_list = self.pts_bbox_head.get_bboxes(outs, img_metas)
        self._box_vis_step(img_metas, data, bbox_list, streams)
        self._nusc_results_step(img_metas, bbox_list, data, first)
        return [bbox3d2result(bboxes, scores, labels) for bboxes, scores, labels in bbox_list]

    @torch.no_grad()
    def simple_test(self, img_metas, gt_bboxes=None, centers2d=None, depths=None, gumbel_noise=None, **data):
        """:543-594: ``[dict(pts_bbox=dict(boxes_3d, scores_3d, labels_3d))]``.  What :meth:`extract_img_feat` returned for the frame -- the reference hands it to
        ``token_selection_vis`` (:562-579) -- stays readable as ``self.last_frame`` until the next one; after :meth:`enable_token_vis` it is rendered there too."""
        self._check_keeps_tokens(data["img"])
        prev_exists = img_metas[0]["scene_token"] == self.prev_scene_token                                                               # :546-549, as the bool it is
        img_feats, token_masks, _, keep_idxes, drop_idxes = self.extract_img_feat(data["img"], 1, gt_bboxes=gt_bboxes, centers2d=centers2d, depths=depths,
                                                                                  prev_exists=prev_exists, ego_pose_inv=data["ego_pose_inv"], gumbel_noise=gumbel_noise)
        data["img_feats"] = img_feats
        self.last_frame = dict(img_feats=img_feats, token_masks=token_masks, keep_idxes=keep_idxes, drop_idxes=drop_idxes)
        self._vis_step(img_metas, data["img"], token_masks, keep_idxes, drop_idxes)                                                     # :562-579
        bbox_list = [dict() for _ in range(len(img_metas))]
        for result_dict, pts_bbox in zip(bbox_list, self.simple_test_pts(img_metas, **data)):
            result_dict["pts_bbox"] = pts_bbox
        return bbox_list

    # ---- several camera streams per step (no counterpart in the reference, whose simple_test compares ONE scene token) ---------------------------------------
    @torch.no_grad()
    def simple_test_streams(self, img_metas, gumbel_noise=None, **data):
        """One step of B independent camera streams (several vehicles, or several scenes of an offline evaluation) in one forward of every part.
        ``img_metas``: a list of B dicts, stream b's at index b; ``data['img']`` (B, N, 3, H, W) -- or the uint8 form the backbone takes, (B, N, H0, W0, 3) --
        and every other key with a leading B (``intrinsics`` / ``lidar2img`` (B, N, 4, 4), ``timestamp`` (B,), ``ego_pose`` / ``ego_pose_inv`` (B, 4, 4)).
        Returns a list of B ``dict(pts_bbox=dict(boxes_3d, scores_3d, labels_3d))``; ``self.last_frame`` as after :meth:`simple_test`, with a leading B.

        Each stream's scene token is compared with that stream's previous one (``self.prev_scene_tokens``, derived state like ``prev_scene_token``): the
        backbone gets the list of B Python bools (a step in which some streams start a scene and others continue is ONE forward), the head the (B,) tensor,
        whose zeros make ``pre_update_memory`` clear exactly those samples of the bank.  ``reset_memory()`` is called only when every stream is new -- and
        when B differs from the previous step's: a change of B restarts EVERY stream (the bank is allocated per batch size; stream b of the new step is not
        known to be stream b of the old one).  Stream b is what a B = 1 detector stepped through :meth:`simple_test` computes for it."""
        self._check_keeps_tokens(data["img"])
        B = len(img_metas)
        tokens = [m["scene_token"] for m in img_metas]
        before = self.prev_scene_tokens
        if before is None or len(before) != B:
            before = [None] * B
        prev = [p is not None and t == p for t, p in zip(tokens, before)]
        self.prev_scene_tokens = tokens
        self.prev_scene_token = None                    # (a later simple_test starts a scene: the two forms are not meant to be interleaved on one detector)
        if not any(prev):
            self.pts_bbox_head.reset_memory()
        img_feats, token_masks, _, keep_idxes, drop_idxes = self.extract_img_feat(data["img"], 1, prev_exists=prev, ego_pose_inv=data["ego_pose_inv"],
                                                                                  gumbel_noise=gumbel_noise)
        data["img_feats"] = img_feats
        self.last_frame = dict(img_feats=img_feats, token_masks=token_masks, keep_idxes=keep_idxes, drop_idxes=drop_idxes)
        self._vis_step(img_metas, data["img"], token_masks, keep_idxes, drop_idxes, streams=B)
        data["prev_exists"] = torch.tensor([1.0 if p else 0.0 for p in prev], dtype=torch.float32, device=data["img"].device)
        location, topk_indexes = self._select_tokens(img_metas, data)
        return [dict(pts_bbox=r) for r in self._pts_results(img_metas, location, topk_indexes, data, streams=B, first=[not p for p in prev])]

    def reset_streams(self, indices=None):
        """Forget the scene tokens of the streams ``indices`` (default: all): their next step starts a scene whatever token it carries."""
        if self.prev_scene_tokens is None:
            return
        for b in range(len(self.prev_scene_tokens)) if indices is None else indices:
            self.prev_scene_tokens[b] = None

    def forward_test(self, img_metas, rescale=None, gt_bboxes=None, centers2d=None, depths=None, gumbel_noise=None, **data):
        if not isinstance(img_metas, list):
            raise TypeError("{} must be a list, but got {}".format("img_metas", type(img_metas)))                                       # :510-513
        for key in data:                                                                                                                 # :514-518
            data[key] = data[key][0][0].unsqueeze(0) if key != "img" else data[key][0]
        return self.simple_test(img_metas[0], gt_bboxes, centers2d, depths, gumbel_noise=gumbel_noise, **data)

    def forward_train(self, *args, **kwargs):
        raise NotImplementedError(f"{_NAME}: forward_train is not implemented (inference only)")

    def forward(self, return_loss=True, **data):
        if return_loss:
            raise NotImplementedError(f"{_NAME}: forward(return_loss=True) is not implemented (inference only); call forward(return_loss=False, ...)")
        for key in ("gt_bboxes", "centers2d", "depths"):                                                                                 # :415-417
            if key in data:
                data[key] = list(zip(*data[key]))
        return self.forward_test(**data)


def build_vis_detector(cfg, **kw):
    """A ``model=dict(type='Petr3D', token_select_vis=True, vis_num_sample=..., vis_start_id=..., ...)`` block of the shipped ``token_vis_ToC3D`` configs, unchanged:
    the four visualisation keywords are taken out, the rest builds through ``build_detector``, and the visualisation is enabled when the flag was set (the
    constructor itself keeps refusing the flag: module docstring)."""
    cfg = dict(cfg)
    flag = cfg.pop("token_select_vis", False)
    vis = {k: cfg.pop(k) for k in ("vis_num_sample", "vis_start_id", "vis_out_path") if k in cfg}
    if not flag:
        cfg.update(vis)                                                     # kept as the attributes the constructor makes of them
    det = registry.build_detector(cfg, **kw)
    if flag:
        det.enable_token_vis(**vis)
    return det
