"""Detections as nuScenes submission records in the global frame, made on the device (``toc3d_boxes_to_global``, include/toc3d_results.h).

The reference turns ``boxes_3d / scores_3d / labels_3d`` into what ``--eval`` and a submission read in the vendored mmdet3d:
``mmdet3d/datasets/nuscenes_dataset.py:301-368`` (``_format_bbox``), ``:576-619`` (``output_to_nusc_box``), ``:622-657`` (``lidar_nusc_box_to_global``), with the
class ranges clamped by ``projects/mmdet3d_plugin/datasets/nuscenes_dataset.py:56-58``: a Python loop that builds a ``pyquaternion`` object and a ``NuScenesBox``
per detection, after a host copy.  Here :meth:`NuScenesResults.format_fixed` does the geometry, the range filter and the attribute choice for every sample of a
step in one launch, from the tensors ``NMSFreeCoder.decode_fixed`` leaves on the device; :meth:`NuScenesResults.records_to_annos` names the classes and
attributes on the host, and :meth:`NuScenesResults.dump` writes ``results_nusc.json`` with the standard library.  Neither mmdet3d nor pyquaternion nor the
nuScenes devkit is needed.

Differences to the reference, by design (include/toc3d_results.h states the arithmetic):
* the float64 rounding order: the rotation matrix comes from the standard quaternion formula, each operation rounded once, where pyquaternion normalises the pose
  again and multiplies two 4 x 4 matrices -- the records agree to a few units in the last place of their terms;
* a box with a label outside the class list or a value that is not finite is dropped, where the reference would raise or write NaN into the JSON;
* the yaw is promoted to float64 before it is halved, as pyquaternion does under the NumPy 1.x promotion mmdet3d 1.0.0rc6 runs on.
No CPU path for the records.
"""
from __future__ import annotations

import json
import math
import os

import numpy as np
import torch

from . import lib

__all__ = ["NuScenesResults", "CLASS_NAMES", "CLASS_RANGE", "ATTRIBUTES", "POSE_KEYS"]
_NAME = "toc3d_amd.NuScenesResults"

# the class order of the shipped configs (projects/configs/*: class_names)
CLASS_NAMES = ("car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle", "pedestrian", "traffic_cone")
# eval_version -> class_range of the devkit's configs (nuscenes/eval/detection/configs/detection_cvpr_2019.json), in metres
CLASS_RANGE = {
    "detection_cvpr_2019": dict(car=50, truck=50, bus=50, trailer=50, construction_vehicle=50, pedestrian=40, motorcycle=40, bicycle=40, traffic_cone=30, barrier=30),
}
# AttrMapping_rev (mmdet3d/datasets/nuscenes_dataset.py:94-103): the index is what the kernel writes, -1 the empty attribute
ATTRIBUTES = ("cycle.with_rider", "cycle.without_rider", "pedestrian.moving", "pedestrian.standing", "pedestrian.sitting_lying_down", "vehicle.moving",
              "vehicle.parked", "vehicle.stopped")
# DefaultAttribute (:72-83)
_DEFAULT_ATTRIBUTE = dict(car="vehicle.parked", pedestrian="pedestrian.moving", trailer="vehicle.parked", truck="vehicle.parked", bus="vehicle.moving",
                          motorcycle="cycle.without_rider", construction_vehicle="vehicle.parked", bicycle="cycle.without_rider", barrier="", traffic_cone="")
# the branch at :327-346: above the speed threshold / at or below it; every other class takes its default
_MOVING = dict(car="vehicle.moving", construction_vehicle="vehicle.moving", bus="vehicle.moving", truck="vehicle.moving", trailer="vehicle.moving",
               bicycle="cycle.with_rider", motorcycle="cycle.with_rider")
_STILL = dict(pedestrian="pedestrian.standing", bus="vehicle.stopped")
SPEED_THR = 0.2                          # :327
POSE_KEYS = ("lidar2ego_rotation", "lidar2ego_translation", "ego2global_rotation", "ego2global_translation")       # of a nuScenes info record
ANNO_KEYS = ("sample_token", "translation", "size", "rotation", "velocity", "detection_name", "detection_score", "attribute_name")      # :348-356, in order


def attribute_index(name: str) -> int:
    return ATTRIBUTES.index(name) if name else -1


def _unit_quaternion(q, what):
    q = np.asarray(q, dtype=np.float64).reshape(-1)
    if q.shape != (4,) or not np.isfinite(q).all():
        raise ValueError(f"{_NAME}: {what} must be four finite numbers (w, x, y, z), got {q.tolist()}")
    norm = math.sqrt(float((q * q).sum()))
    if norm == 0.0 or abs(norm - 1.0) > 1e-6:
        raise ValueError(f"{_NAME}: {what} is no unit quaternion: its norm {norm!r} is off 1 by more than 1e-6 (was the wrong field passed?)")
    return q / norm


def _translation(t, what):
    t = np.asarray(t, dtype=np.float64).reshape(-1)
    if t.shape != (3,) or not np.isfinite(t).all():
        raise ValueError(f"{_NAME}: {what} must be three finite numbers, got {t.tolist()}")
    return t


def pose_array(poses) -> np.ndarray:
    """Pose records (dicts with :data:`POSE_KEYS`) -> float64 ``(B, 2, 7)``: per sample lidar -> ego, then ego -> global, each ``(w, x, y, z, tx, ty, tz)`` with
    the quaternion normalised in float64 (``q / |q|``).  A missing key, a non-finite or zero quaternion and one whose norm is off 1 by more than 1e-6 are
    ``ValueError``."""
    out = np.empty((len(poses), 2, 7), dtype=np.float64)
    for b, p in enumerate(poses):
        for key in POSE_KEYS:
            if key not in p:
                raise ValueError(f"{_NAME}: pose record {b} has no {key!r} (needed: {', '.join(POSE_KEYS)})")
        for k, pre in enumerate(("lidar2ego", "ego2global")):
            out[b, k, :4] = _unit_quaternion(p[pre + "_rotation"], f"{pre}_rotation of pose record {b}")
            out[b, k, 4:] = _translation(p[pre + "_translation"], f"{pre}_translation of pose record {b}")
    return out


class NuScenesResults:
    """``boxes_3d / scores_3d / labels_3d`` -> the records of a nuScenes detection submission.

    >>> res = toc3d_amd.NuScenesResults()
    >>> bbox_list = head.get_bboxes(outs, img_metas)
    >>> for token, annos in zip(tokens, res.format(bbox_list, infos, tokens)):
    ...     res.add(token, annos)
    >>> res.dump("./work_dirs/pts_bbox")
    """

    def __init__(self, class_names=CLASS_NAMES, eval_version="detection_cvpr_2019", max_depth=60, with_velocity=True, class_range=None, modality=None):
        names = tuple(class_names)
        if not 1 <= len(names) <= lib.RESULTS_MAX_CLASSES:
            raise ValueError(f"{_NAME}: 1 to {lib.RESULTS_MAX_CLASSES} class names, got {len(names)}")
        for n in names:
            if n not in _DEFAULT_ATTRIBUTE:
                raise ValueError(f"{_NAME}: unknown class name {n!r} (the nuScenes detection classes are {', '.join(CLASS_NAMES)})")
        if class_range is None:
            if eval_version not in CLASS_RANGE:
                raise ValueError(f"{_NAME}: unknown eval_version {eval_version!r} (known: {', '.join(CLASS_RANGE)}); pass class_range=dict(name=metres, ...)")
            class_range = CLASS_RANGE[eval_version]
        missing = [n for n in names if n not in class_range]
        if missing:
            raise ValueError(f"{_NAME}: class_range has no entry for {missing}")
        # projects/mmdet3d_plugin/datasets/nuscenes_dataset.py:56-58
        self.class_range = {n: min(class_range[n], max_depth) for n in names}
        if not all(np.isfinite(float(v)) for v in self.class_range.values()):
            raise ValueError(f"{_NAME}: class ranges must be finite, got {self.class_range}")
        self.class_names, self.eval_version, self.max_depth, self.with_velocity = names, eval_version, max_depth, bool(with_velocity)
        self.modality = modality
        self.attr_moving = tuple(_MOVING.get(n, _DEFAULT_ATTRIBUTE[n]) for n in names)
        self.attr_still = tuple(_STILL.get(n, _DEFAULT_ATTRIBUTE[n]) for n in names)
        self.speed_thr = SPEED_THR
        self.results = {}                                                   # sample_token -> annos, filled by add()
        self._tables = {}                                                   # device -> (class_range f64, attr_moving i32, attr_still i32)

    def _tables_on(self, dev):
        key = str(dev)
        if key not in self._tables:
            rng = torch.tensor([float(self.class_range[n]) for n in self.class_names], dtype=torch.float64)
            mov = torch.tensor([attribute_index(a) for a in self.attr_moving], dtype=torch.int32)
            still = torch.tensor([attribute_index(a) for a in self.attr_still], dtype=torch.int32)
            self._tables[key] = tuple(t.to(dev) for t in (rng, mov, still))
        return self._tables[key]

    # ---- the device half ---------------------------------------------------------------------------------------------------------------------------------
    def format_fixed(self, boxes, scores, labels, counts, poses):
        """``boxes`` f32 ``(B, K, >= 7)`` (``>= 9`` with the velocity), ``scores`` f32 ``(B, K)``, ``labels`` int64 ``(B, K)``, ``counts`` int64 ``(B,)``: what
        ``NMSFreeCoder.decode_fixed(..., sub_half_height=True)`` returns, on the device.  ``poses``: B pose records (:func:`pose_array`), or the float64
        ``(B, 2, 7)`` array / tensor made of them.  -> ``dict(rec (B, K, 12) f64, score (B, K) f32, name, attr, src (B, K) int32, kept (B,) int64)`` on the
        device: per sample the first ``kept[b]`` rows are the boxes inside their class range, in input order; the rest zeros (indices -1).  One launch, no
        host synchronisation."""
        for t, what in ((boxes, "boxes"), (scores, "scores"), (labels, "labels"), (counts, "counts")):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise RuntimeError(f"{_NAME}: {what} must be a CUDA/HIP tensor -- the HIP extension is the only compute path")
        width = 9 if self.with_velocity else 7
        if boxes.dim() != 3 or boxes.shape[2] < width:
            raise ValueError(f"{_NAME}: boxes must be (B, K, >= {width}){' with the velocity in columns 7, 8' if self.with_velocity else ''}, got {tuple(boxes.shape)}")
        B, K = boxes.shape[:2]
        if tuple(scores.shape) != (B, K) or tuple(labels.shape) != (B, K) or tuple(counts.shape) != (B,) or labels.dtype != torch.int64 or counts.dtype != torch.int64:
            raise ValueError(f"{_NAME}: scores ({B}, {K}), int64 labels ({B}, {K}) and int64 counts ({B},) expected, got {tuple(scores.shape)}, "
                             f"{labels.dtype} {tuple(labels.shape)}, {counts.dtype} {tuple(counts.shape)}")
        if K > lib.RESULTS_MAX_BOXES:
            raise ValueError(f"{_NAME}: {K} boxes a sample exceed {lib.RESULTS_MAX_BOXES} (TOC3D_RESULTS_MAX_BOXES, the decoder's own cap)")
        dev = boxes.device
        if isinstance(poses, torch.Tensor):
            pose = poses.to(device=dev, dtype=torch.float64).contiguous()
        else:
            host = np.ascontiguousarray(poses, dtype=np.float64) if isinstance(poses, np.ndarray) else pose_array(poses)
            pose = torch.from_numpy(host).pin_memory().to(dev, non_blocking=True)       # (a pageable copy would wait for the stream)
        if tuple(pose.shape) != (B, 2, 7):
            raise ValueError(f"{_NAME}: {B} samples need {B} pose records ((B, 2, 7)), got {tuple(pose.shape)}")
        with torch.cuda.device(dev):
            boxes = boxes.float()
            if B and K and not (boxes.stride(2) == 1 and boxes.stride(1) >= width and boxes.stride(0) >= K * boxes.stride(1)):
                boxes = boxes.contiguous()
            scores, labels, counts = scores.float().contiguous(), labels.contiguous(), counts.contiguous()
            rng, mov, still = self._tables_on(dev)
            out = dict(rec=torch.empty(B, K, lib.RESULTS_REC, dtype=torch.float64, device=dev), score=torch.empty(B, K, dtype=torch.float32, device=dev),
                       name=torch.empty(B, K, dtype=torch.int32, device=dev), attr=torch.empty(B, K, dtype=torch.int32, device=dev),
                       src=torch.empty(B, K, dtype=torch.int32, device=dev))
            if B and K:
                out["kept"] = torch.empty(B, dtype=torch.int64, device=dev)
                lib.call("toc3d_boxes_to_global", boxes, boxes.stride(1), boxes.stride(0), scores, labels, counts, B, K, int(self.with_velocity), pose, rng, mov, still,
                         len(self.class_names), self.speed_thr, out["rec"], out["score"], out["name"], out["attr"], out["src"], out["kept"], lib.stream_ptr())
            else:
                out["kept"] = torch.zeros(B, dtype=torch.int64, device=dev)  # (nothing is launched for no boxes)
        return out

    def format(self, bbox_list, poses, sample_tokens=None):
        """``bbox_list``: the ``[[bboxes, scores, labels], ...]`` lists ``get_bboxes`` returns, on the device (``bboxes`` a ``(n, >= 7)`` tensor or an object with
        ``.tensor``); ``poses``: a pose record per sample.  Packs the lists, formats them in one launch, copies the records to the host once and returns, per
        sample, the list of dicts the reference appends (:348-356): ``sample_token`` (when ``sample_tokens`` is given), ``translation``, ``size``, ``rotation``,
        ``velocity``, ``detection_name``, ``detection_score``, ``attribute_name``; numbers are Python floats."""
        return self.format_device(bbox_list, poses, sample_tokens)[1]

    def format_device(self, bbox_list, poses, sample_tokens=None):
        """What :meth:`format` is built on -> ``(fixed, annos)``: the :meth:`format_fixed` dict of the packed lists, still on the device (``None`` for no samples;
        what :class:`toc3d_amd.PubTracker` steps on), and what :meth:`format` returns."""
        B = len(bbox_list)
        if len(poses) != B or (sample_tokens is not None and len(sample_tokens) != B):
            raise ValueError(f"{_NAME}: {B} samples need {B} pose records{'' if sample_tokens is None else ' and sample tokens'}")
        pose = pose_array(poses)                                            # the refusals come before any device work
        if B == 0:
            return None, []
        width = 9 if self.with_velocity else 7
        tensors = [getattr(bb, "tensor", bb) for bb, _, _ in bbox_list]
        for t in tensors:
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dim() == 2 and t.shape[1] >= width):
                raise ValueError(f"{_NAME}: bboxes must be (n, >= {width}) tensors on the device (or objects whose .tensor is one)")
        dev = tensors[0].device
        ns = [int(t.shape[0]) for t in tensors]
        K = max(ns)
        boxes = torch.zeros(B, K, width, dtype=torch.float32, device=dev)
        scores = torch.zeros(B, K, dtype=torch.float32, device=dev)
        labels = torch.zeros(B, K, dtype=torch.int64, device=dev)
        for b, (t, (_, sc, lb)) in enumerate(zip(tensors, bbox_list)):
            if ns[b]:
                boxes[b, :ns[b]] = t[:, :width]
                scores[b, :ns[b]] = sc
                labels[b, :ns[b]] = lb
        counts = torch.tensor(ns, dtype=torch.int64).pin_memory().to(dev, non_blocking=True)
        out = self.format_fixed(boxes, scores, labels, counts, pose)
        host = {k: out[k].cpu().numpy() for k in ("rec", "score", "name", "attr", "kept")}
        return out, self.records_to_annos(host["rec"], host["score"], host["name"], host["attr"], host["kept"], sample_tokens)

    # ---- the host half -----------------------------------------------------------------------------------------------------------------------------------
    def records_to_annos(self, rec, score, name, attr, kept, tokens=None):
        """numpy in, dicts out: ``rec (B, K, 12)``, ``score / name / attr (B, K)``, ``kept (B,)`` as :meth:`format_fixed` makes them -> per sample the list of
        ``kept[b]`` annotation dicts with the reference's keys in its order (``sample_token`` only with ``tokens``)."""
        rec, score, name, attr, kept = (np.asarray(a) for a in (rec, score, name, attr, kept))
        B = rec.shape[0]
        if rec.ndim != 3 or rec.shape[2] != lib.RESULTS_REC or score.shape != rec.shape[:2] or name.shape != rec.shape[:2] or attr.shape != rec.shape[:2] or kept.shape != (B,):
            raise ValueError(f"{_NAME}: rec (B, K, 12), score / name / attr (B, K) and kept (B,) expected, got {rec.shape}, {score.shape}, {name.shape}, {attr.shape}, {kept.shape}")
        if tokens is not None and len(tokens) != B:
            raise ValueError(f"{_NAME}: {B} samples need {B} sample tokens, got {len(tokens)}")
        out = []
        for b in range(B):
            annos = []
            for i in range(int(kept[b])):
                r = rec[b, i].tolist()
                anno = dict(sample_token=tokens[b]) if tokens is not None else {}
                anno.update(translation=r[0:3], size=r[3:6], rotation=r[6:10], velocity=r[10:12], detection_name=self.class_names[int(name[b, i])],
                            detection_score=float(score[b, i]), attribute_name=ATTRIBUTES[int(attr[b, i])] if attr[b, i] >= 0 else "")
                annos.append(anno)
            out.append(annos)
        return out

    def add(self, sample_token, annos):
        """``nusc_annos[sample_token] = annos`` (:358): a later call for the same token replaces the earlier one."""
        self.results[sample_token] = annos
        return self

    def dump(self, jsonfile_prefix):
        """``{jsonfile_prefix}/results_nusc.json`` (created with its directory) as ``{'meta': modality, 'results': {...}}`` (:359-368) -> the path."""
        os.makedirs(jsonfile_prefix, exist_ok=True)
        path = os.path.join(jsonfile_prefix, "results_nusc.json")
        with open(path, "w") as fh:
            json.dump(dict(meta=self.modality, results=self.results), fh)
        return path
