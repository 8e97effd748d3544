"""Predicted 3-D boxes drawn on the camera views and on a top-down (BEV) panel, with the pixels made on the device (``toc3d_box_segments``,
``toc3d_box_segments_bev``, ``toc3d_segments_render``, include/toc3d_boxes.h).

The reference shows its detections through ``tools/visualize.py`` -> ``tools/visual_nuscenes.py::render_sample`` (six camera panels and a top-down one, from a
result JSON, with the nuScenes devkit and matplotlib), the vendored mmdet3d through ``core/visualizer/image_vis.py:61-126`` (``draw_lidar_bbox3d_on_img``,
``cv2.line``).  Here :meth:`BoxVis.render` draws from the tensors ``get_bboxes`` holds on the device and the frame's ``lidar2img`` onto the images the frame
holds, in two launches (four with the BEV panel), and :meth:`BoxVis.write` copies the finished bytes to the host once and encodes them with the PNG writer of
:mod:`toc3d_amd.token_vis`.

Differences to mmdet3d's routine, by design:
* an edge that crosses the camera's near plane is clipped there, in 3-D, and one wholly behind it is dropped (``image_vis.py:119`` clamps the depth to 1e-5,
  which smears a box behind a camera across that camera's image);
* lines are the integer coverage rule of include/toc3d_boxes.h (a stroke of width ``thickness`` with round caps, not anti-aliased), not ``cv2.line``'s;
* boxes are coloured by class and box 0 -- the highest score -- ends on top; boxes below ``score_thr`` (``tools/visualize.py:15``: 0.25) are not drawn;
* the arrays and the files are red first whatever ``to_rgb`` says.  No CPU path for the pixels.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import lib
from .token_vis import _image_arg, write_png

__all__ = ["BoxVis", "DEFAULT_PALETTE"]
_NAME = "toc3d_amd.BoxVis"

# RGB per class, in the class order of the shipped configs: car, truck, construction_vehicle, bus, trailer, barrier, motorcycle, bicycle, pedestrian, traffic_cone
DEFAULT_PALETTE = ((255, 158, 0), (255, 158, 0), (255, 158, 0), (255, 158, 0), (255, 158, 0), (112, 128, 144), (255, 61, 99), (255, 61, 99), (0, 0, 230), (47, 79, 79))
GUARD = lib.BOXES_MAX_GUARD              # the band around the image that segments are clipped to: the widest, which every thickness allows


class BoxVis:
    """Detections as pictures in two steps: :meth:`render` (device) and :meth:`write` (host).

    >>> vis = toc3d_amd.BoxVis()
    >>> boxes, scores, labels = head.get_bboxes(outs, img_metas)[0]
    >>> r = vis.render(data["img"], boxes, scores, labels, data["lidar2img"], img_norm_cfg)
    >>> vis.write(r, "./box_vis/0/")
    """

    def __init__(self, score_thr: float = 0.25, thickness: int = 2, near: float = 0.1, palette=None, bev_size: int = 640, bev_range: float = 51.2,
                 bev_background=(255, 255, 255)):
        if int(thickness) != thickness or not 1 <= thickness <= lib.BOXES_MAX_THICKNESS:
            raise ValueError(f"{_NAME}: thickness must be an integer in [1, {lib.BOXES_MAX_THICKNESS}], got {thickness!r}")
        if int(bev_size) != bev_size or not 1 <= bev_size <= lib.BOXES_MAX_SIDE:
            raise ValueError(f"{_NAME}: bev_size must be an integer in [1, {lib.BOXES_MAX_SIDE}], got {bev_size!r}")
        if not (float(bev_range) > 0 and np.isfinite(float(bev_range))):
            raise ValueError(f"{_NAME}: bev_range must be a positive number of metres, got {bev_range!r}")
        pal = np.asarray(DEFAULT_PALETTE if palette is None else palette)
        if pal.ndim != 2 or pal.shape[1] != 3 or not 1 <= pal.shape[0] <= 254 or (pal < 0).any() or (pal > 255).any() or (pal != np.rint(pal)).any():
            raise ValueError(f"{_NAME}: palette must be 1 to 254 RGB byte triples, got an array of shape {pal.shape}")
        bg = tuple(int(c) for c in bev_background)
        if len(bg) != 3 or any(not 0 <= c <= 255 for c in bg):
            raise ValueError(f"{_NAME}: bev_background must be three bytes, got {bev_background!r}")
        self.score_thr, self.thickness, self.near = float(score_thr), int(thickness), float(near)
        self.bev_size, self.bev_range, self.bev_background = int(bev_size), float(bev_range), bg
        self.palette = pal.astype(np.uint8)
        self._palette_dev = {}                                              # device -> the palette there
        self._ws = {}

    def _palette_on(self, dev):
        key = str(dev)
        if key not in self._palette_dev:
            self._palette_dev[key] = torch.from_numpy(self.palette).to(dev).contiguous()
        return self._palette_dev[key]

    def render(self, imgs, boxes, scores, labels, lidar2img, img_norm_cfg=None, bev: bool = True):
        """``imgs``: f32 ``(V, 3, H, W)`` normalised images (leading dimensions are flattened) or uint8 ``(V, H, W, 3)`` raw frames (``img_norm_cfg`` is then
        required), as :meth:`TokenVis.render` takes them.  ``boxes``: f32 ``(n, >= 7)`` rows ``(x, y, z_bottom, dx, dy, dz, yaw, ...)`` or an object with
        ``.tensor``; ``scores`` f32 ``(n,)``; ``labels`` int64 ``(n,)``: what ``get_bboxes`` returns for one sample, on the device.  ``lidar2img``: ``(V, 4, 4)``
        or ``(1, V, 4, 4)``, any float dtype, host or device.
        -> ``dict(views (V, H, W, 3), bev (S, S, 3) or None, ...)``: device uint8 tensors, red first, in a per-shape workspace of this object, valid until the next
        call; also the segment tables the pixels were made from (``segf``, ``segi``, ``cidx`` ``(V, n, 12, ...)`` and ``bev_segf``, ``bev_segi``, ``bev_cidx``
        ``(n, 5, ...)``).  Two launches, four with ``bev`` (one and two when ``n == 0``)."""
        img, u8, V, H, W, stride, mean, std, to_rgb = _image_arg(imgs, img_norm_cfg, _NAME)
        dev, kind = imgs.device, int(u8)
        if H > lib.BOXES_MAX_SIDE or W > lib.BOXES_MAX_SIDE:
            raise ValueError(f"{_NAME}: images {H} x {W} exceed {lib.BOXES_MAX_SIDE} (TOC3D_BOXES_MAX_SIDE)")
        box = getattr(boxes, "tensor", boxes)
        if not (isinstance(box, torch.Tensor) and box.is_cuda and box.dim() == 2 and box.shape[1] >= 7):
            raise ValueError(f"{_NAME}: boxes must be a (n, >= 7) tensor on the device (or an object whose .tensor is one)")
        n = box.shape[0]
        box = box.float()
        if n and box.stride(1) != 1:
            box = box.contiguous()
        if not (isinstance(scores, torch.Tensor) and scores.is_cuda and tuple(scores.shape) == (n,)):
            raise ValueError(f"{_NAME}: scores must be a ({n},) tensor on the device")
        if not (isinstance(labels, torch.Tensor) and labels.is_cuda and tuple(labels.shape) == (n,) and labels.dtype == torch.int64):
            raise ValueError(f"{_NAME}: labels must be an int64 ({n},) tensor on the device")
        scores, labels = scores.float().contiguous(), labels.contiguous()
        proj = torch.as_tensor(lidar2img) if not isinstance(lidar2img, torch.Tensor) else lidar2img
        if not proj.is_floating_point():
            raise ValueError(f"{_NAME}: lidar2img must hold floats, got {proj.dtype}")
        if proj.dim() == 4 and proj.shape[0] == 1:
            proj = proj[0]
        if tuple(proj.shape) != (V, 4, 4):
            raise ValueError(f"{_NAME}: lidar2img must be ({V}, 4, 4) or (1, {V}, 4, 4) for {V} views, got {tuple(proj.shape)}")
        proj = proj.to(device=dev, dtype=torch.float32).contiguous()
        S = self.bev_size
        key = (V, H, W, str(dev))
        if key not in self._ws:
            self._ws = {key: dict(views=torch.empty((V, H, W, 3), dtype=torch.uint8, device=dev), bev=torch.empty((S, S, 3), dtype=torch.uint8, device=dev), cap=-1)}
        ws = self._ws[key]
        if n > ws["cap"]:                                                   # the tables grow with the largest n seen
            EC, EB = lib.BOXES_CAMERA_EDGES, lib.BOXES_BEV_EDGES
            m = max(n, 1)
            ws.update(cap=n, segf=torch.empty(V * m * EC * 4, dtype=torch.float32, device=dev), segi=torch.empty(V * m * EC * 4, dtype=torch.int32, device=dev),
                      cidx=torch.empty(V * m * EC, dtype=torch.uint8, device=dev), bsegf=torch.empty(m * EB * 4, dtype=torch.float32, device=dev),
                      bsegi=torch.empty(m * EB * 4, dtype=torch.int32, device=dev), bcidx=torch.empty(m * EB, dtype=torch.uint8, device=dev))
        pal, ncol, t = self._palette_on(dev), self.palette.shape[0], self.thickness
        s = lib.stream_ptr()
        lib.call("toc3d_box_segments", box if n else None, box.stride(0) if n else 7, scores if n else None, labels if n else None, n, self.score_thr, ncol,
                 proj, V, self.near, H, W, GUARD, t, ws["segf"], ws["segi"], ws["cidx"], s)
        lib.call("toc3d_segments_render", img, kind, stride, V, H, W, *mean, *std, int(to_rgb), 0, 0, 0, ws["segi"], ws["cidx"], n * lib.BOXES_CAMERA_EDGES,
                 pal, ncol, t, GUARD, ws["views"], s)
        EC, EB = lib.BOXES_CAMERA_EDGES, lib.BOXES_BEV_EDGES
        out = dict(views=ws["views"], bev=None, to_rgb=to_rgb, segf=ws["segf"][:V * n * EC * 4].view(V, n, EC, 4), segi=ws["segi"][:V * n * EC * 4].view(V, n, EC, 4),
                   cidx=ws["cidx"][:V * n * EC].view(V, n, EC), bev_segf=None, bev_segi=None, bev_cidx=None)
        if bev:
            lib.call("toc3d_box_segments_bev", box if n else None, box.stride(0) if n else 7, scores if n else None, labels if n else None, n, self.score_thr, ncol,
                     S, self.bev_range, GUARD, t, ws["bsegf"], ws["bsegi"], ws["bcidx"], s)
            lib.call("toc3d_segments_render", None, 2, 0, 1, S, S, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 0, *self.bev_background, ws["bsegi"], ws["bcidx"], n * EB,
                     pal, ncol, t, GUARD, ws["bev"], s)
            out.update(bev=ws["bev"], bev_segf=ws["bsegf"][:n * EB * 4].view(n, EB, 4), bev_segi=ws["bsegi"][:n * EB * 4].view(n, EB, 4),
                       bev_cidx=ws["bcidx"][:n * EB].view(n, EB))
        return out

    def write(self, rendered, output_path, views=None):
        """``view{v}_pred.png`` per view and, when rendered, ``bev_pred.png`` under ``output_path`` (created), in true colours (the arrays are red first and are
        stored in array order).  One copy to the host, then the encoder.  ``views``: a range of the rendered views to write, numbered from 0 in the file names
        (default: all).  -> the list of file names."""
        os.makedirs(output_path, exist_ok=True)
        pics = rendered["views"].cpu().numpy()
        names = []
        for k, v in enumerate(range(pics.shape[0]) if views is None else views):
            names.append(os.path.join(output_path, f"view{k}_pred.png"))
            write_png(names[-1], pics[v], blue_first=False)
        if rendered.get("bev") is not None:
            names.append(os.path.join(output_path, "bev_pred.png"))
            write_png(names[-1], rendered["bev"].cpu().numpy(), blue_first=False)
        return names
