"""Image side of the patch embedding on the GPU.

The reference normalises, pads and transposes every camera image on the host and ships float32 NCHW to the GPU
(``NormalizeMultiviewImage`` / ``PadMultiViewImage``, ``datasets/pipelines/transform_3d.py:87-100,38-50``;
``DefaultFormatBundle``, ``mmdet3d/datasets/pipelines/formating.py:42-47``).  The pixels are integer valued at that point
(``LoadMultiViewImageFromFiles(to_float32=True)`` + PIL resize/crop of uint8 data), so the same tensor can be produced on
the device from the uint8 HWC images: a quarter of the host-to-device bytes (4.6 MB instead of 18.4 MB per 6-view frame).

``prepare_images`` materialises that float tensor (drop-in for the three pipeline steps); a backbone built with
``img_norm_cfg=...`` skips even that and reads the uint8 images straight in its patch-embedding im2col
(``toc3d_im2col_patches_u8``), with bit-identical results.

``ResizeCropFlipRotImage`` is the step in front of those: the reference's eval-time ``Image.resize`` + ``Image.crop`` of the raw camera frames
(``datasets/pipelines/transform_3d.py:108-172,247-298``), on the device, with Pillow's bytes (``toc3d_resize_crop_u8``, include/toc3d_ingest.h).
"""
from __future__ import annotations

import math
from typing import Sequence

import numpy as np
import torch

from . import lib


def prepare_images(img_u8: torch.Tensor, mean: Sequence[float], std: Sequence[float], to_rgb: bool = True,
                   size_divisor: int = 32) -> torch.Tensor:
    """uint8 HWC (V, H, W, 3) on the GPU -> float32 NCHW (V, 3, Hp, Wp), Hp / Wp = H / W rounded up to ``size_divisor``."""
    if not isinstance(img_u8, torch.Tensor) or not img_u8.is_cuda:
        raise RuntimeError("toc3d_amd.preprocess: images must be CUDA/HIP tensors -- the HIP extension is the only compute path")
    if img_u8.dtype != torch.uint8 or img_u8.dim() != 4 or img_u8.shape[3] != 3:
        raise ValueError(f"expected uint8 HWC images (V, H, W, 3), got {img_u8.dtype} {tuple(img_u8.shape)}")
    if size_divisor % 4:
        raise ValueError("size_divisor must be a multiple of 4")
    img_u8 = img_u8.contiguous()
    V, H, W, _ = img_u8.shape
    Hp, Wp = -(-H // size_divisor) * size_divisor, -(-W // size_divisor) * size_divisor
    out = torch.empty(V, 3, Hp, Wp, dtype=torch.float32, device=img_u8.device)
    m = torch.tensor(list(mean), dtype=torch.float32)
    s = torch.tensor(list(std), dtype=torch.float32)
    lib.call("toc3d_normalize_images", img_u8, V, H, W, m, s, int(bool(to_rgb)), out, Hp, Wp, lib.stream_ptr())
    return out


# ---- camera ingest: Pillow's resize and crop ---------------------------------------------------------------------------------------------------------------------
PRECISION_BITS = 32 - 8 - 2              # Pillow's fixed point for 8-bit data (src/libImaging/Resample.c): coefficients times 2^22, accumulator int32


def _bicubic(t: float) -> float:
    a = -0.5
    if t < 0.0:
        t = -t
    if t < 1.0:
        return ((a + 2.0) * t - (a + 3.0)) * t * t + 1
    if t < 2.0:
        return (((t - 5) * t + 8) * t - 4) * a
    return 0.0


def resample_tables(in_size: int, out_size: int, first: int = 0, count: int = None):
    """Pillow's ``precompute_coeffs`` + ``normalize_coeffs_8bpc`` for the BICUBIC filter (what ``Image.resize(size)`` uses), for outputs
    [first, first + count) of an axis resized from ``in_size`` to ``out_size``: (coef int32 [count, ksize], bounds int32 [count, 2] = (first source index, tap
    count), ksize).  Python floats (IEEE double) in Pillow's operation order, so the integers are Pillow's."""
    count = out_size - first if count is None else count
    if in_size <= 0 or out_size <= 0 or first < 0 or count <= 0 or first + count > out_size:
        raise ValueError(f"bad axis: in_size {in_size}, out_size {out_size}, outputs [{first}, {first} + {count})")
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    coef = np.zeros((count, ksize), dtype=np.int32)
    bounds = np.zeros((count, 2), dtype=np.int32)
    for i in range(count):
        xx = first + i
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        k = [int(0.5 + v * (1 << PRECISION_BITS)) if v >= 0 else int(-0.5 + v * (1 << PRECISION_BITS)) for v in w]
        assert 255 * sum(abs(v) for v in k) + (1 << (PRECISION_BITS - 1)) < 2 ** 31, "the row overflows Pillow's int32 accumulator"
        assert all(abs(v) < 1 << 23 for v in k), "a coefficient beyond signed 24 bits: the kernel multiplies on the 24-bit multiplier"
        coef[i, :xmax] = k
        bounds[i] = (xmin, xmax)
    return coef, bounds, ksize


def _identity_tables(first: int, count: int):
    """An axis Pillow does not resample (equal sizes): one tap of 1.0, which gives the byte back ((2^21 + p 2^22) >> 22 = p)."""
    coef = np.full((count, 1), 1 << PRECISION_BITS, dtype=np.int32)
    bounds = np.stack([np.arange(first, first + count, dtype=np.int32), np.ones(count, dtype=np.int32)], axis=1)
    return coef, bounds, 1


def tile_span(bounds_v: np.ndarray, tile_h: int = lib.INGEST_TILE_H) -> int:
    """The most source rows the vertical taps of ``tile_h`` consecutive output rows span (``max_span`` of toc3d_resize_crop_u8)."""
    return max(int((bounds_v[y0:y0 + tile_h, 0] + bounds_v[y0:y0 + tile_h, 1]).max() - bounds_v[y0, 0]) for y0 in range(0, len(bounds_v), tile_h))


class ResizeCropFlipRotImage:
    """The reference's ``ResizeCropFlipRotImage(data_aug_conf, training=False)`` (datasets/pipelines/transform_3d.py:108-172) on the device: ``Image.resize`` to
    ``resize_dims`` and ``Image.crop`` of every raw uint8 camera frame, with Pillow's bytes, in one launch; and the matching update of the intrinsics.
    Eval branch only: ``training=True``, a non-zero ``rot_lim`` and anything but 3-channel uint8 frames raise.  The coefficient tables are made once per
    (size, crop) and kept on the device.

    >>> ingest = toc3d_amd.ResizeCropFlipRotImage(ida_aug_conf, training=False)
    >>> img = ingest(raw_u8)                                    # (B, N, 900, 1600, 3) uint8 on the device -> (B, N, fH, fW, 3)
    >>> intrinsics, lidar2img = ingest.update_cameras(intrinsics, extrinsics)
    """

    def __init__(self, data_aug_conf=None, with_2d=True, filter_invisible=True, training=True):
        if training:
            raise NotImplementedError("toc3d_amd.ResizeCropFlipRotImage: the eval branch only (training=False); training augmentation stays on the host")
        if data_aug_conf is None or tuple(data_aug_conf.get("rot_lim", (0.0, 0.0))) != (0.0, 0.0):
            raise NotImplementedError("toc3d_amd.ResizeCropFlipRotImage: needs a data_aug_conf with rot_lim (0.0, 0.0): rotation is not supported (nor by the reference)")
        self.data_aug_conf = dict(data_aug_conf)
        self.training, self.with_2d, self.filter_invisible = False, with_2d, filter_invisible
        resize, (newW, newH), crop = self.geometry()
        if not (0 <= crop[0] and 0 <= crop[1] and crop[2] <= newW and crop[3] <= newH and crop[0] < crop[2] and crop[1] < crop[3]):
            raise ValueError(f"the crop {crop} leaves the resized image {newW} x {newH}: Pillow would fill with zeros, which this path does not do")
        self._tables, self._ws = {}, {}

    def geometry(self):
        """(resize, resize_dims, crop): ``_sample_augmentation`` of the eval branch (:290-297), in the reference's Python arithmetic."""
        H, W = self.data_aug_conf["H"], self.data_aug_conf["W"]
        fH, fW = self.data_aug_conf["final_dim"]
        resize = max(fH / H, fW / W)
        resize_dims = (int(W * resize), int(H * resize))
        newW, newH = resize_dims
        crop_h = int((1 - np.mean(self.data_aug_conf["bot_pct_lim"])) * newH) - fH
        crop_w = int(max(0, newW - fW) / 2)
        return resize, resize_dims, (crop_w, crop_h, crop_w + fW, crop_h + fH)

    def ida_mat(self) -> torch.Tensor:
        """The 3 x 3 float32 matrix of ``_img_transform`` (:247-273) without flip and rotation: scale by ``resize``, shift by minus the crop's corner."""
        resize, _, crop = self.geometry()
        m = torch.eye(3)
        m[:2, :2] *= resize
        m[:2, 2] -= torch.Tensor(crop[:2])
        return m

    def host_tables(self):
        """{'h': (coef, bounds, ksize), 'v': ...} as numpy arrays, restricted to the crop; an axis of unchanged size gets the one-tap identity."""
        H, W = self.data_aug_conf["H"], self.data_aug_conf["W"]
        _, (newW, newH), crop = self.geometry()
        fH, fW = crop[3] - crop[1], crop[2] - crop[0]
        return dict(h=_identity_tables(crop[0], fW) if newW == W else resample_tables(W, newW, crop[0], fW),
                    v=_identity_tables(crop[1], fH) if newH == H else resample_tables(H, newH, crop[1], fH))

    def _device_tables(self, device):
        key = str(device)
        if key not in self._tables:
            t = self.host_tables()
            (ch, bh, kh), (cv, bv, kv) = t["h"], t["v"]
            span = tile_span(bv)
            if max(kh, kv) > lib.INGEST_MAX_KSIZE or span > lib.INGEST_LDS_ROWS:
                raise ValueError(f"resize too strong for the kernel's LDS budget: ksize ({kh}, {kv}) > {lib.INGEST_MAX_KSIZE} or a tile spans {span} > {lib.INGEST_LDS_ROWS} rows")
            dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
            self._tables[key] = (dv(ch), dv(bh), kh, dv(cv), dv(bv), kv, span)
        return self._tables[key]

    def __call__(self, img_u8: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
        """uint8 HWC (V, H0, W0, 3) or (B, N, H0, W0, 3) on the device -> the same rank at (fH, fW), Pillow's bytes.  ``out=`` (contiguous, same shape) receives
        the result; without it the result is a per-shape workspace of this object that stays valid until the next call with that shape: clone it to keep it."""
        if not isinstance(img_u8, torch.Tensor) or not img_u8.is_cuda:
            raise RuntimeError("toc3d_amd.ResizeCropFlipRotImage: images must be CUDA/HIP tensors -- the HIP extension is the only compute path")
        H, W = self.data_aug_conf["H"], self.data_aug_conf["W"]
        fH, fW = self.data_aug_conf["final_dim"]
        if img_u8.dtype != torch.uint8 or img_u8.dim() not in (4, 5) or tuple(img_u8.shape[-3:]) != (H, W, 3):
            raise ValueError(f"expected uint8 HWC frames (V, {H}, {W}, 3) or (B, N, {H}, {W}, 3), got {img_u8.dtype} {tuple(img_u8.shape)}")
        img_u8 = img_u8.contiguous()
        shape = tuple(img_u8.shape[:-3]) + (fH, fW, 3)
        if out is None:
            key = (shape, str(img_u8.device))
            if key not in self._ws:
                self._ws[key] = torch.empty(shape, dtype=torch.uint8, device=img_u8.device)
            out = self._ws[key]
        elif not (isinstance(out, torch.Tensor) and out.dtype == torch.uint8 and tuple(out.shape) == shape and out.device == img_u8.device and out.is_contiguous()):
            raise ValueError(f"out= must be a contiguous uint8 tensor {shape} on {img_u8.device}")
        ch, bh, kh, cv, bv, kv, span = self._device_tables(img_u8.device)
        V = img_u8.numel() // (H * W * 3)
        lib.call("toc3d_resize_crop_u8", img_u8, W * 3, V, H, W, out, fW * 3, fH, fW, ch, bh, kh, cv, bv, kv, span, lib.stream_ptr())
        return out

    def update_cameras(self, intrinsics, extrinsics):
        """(intrinsics, lidar2img) as :164 and :170 compute them, per camera: ``K[:3, :3] = ida_mat @ K[:3, :3]`` (the float32 matrix times K in K's own
        dtype's promotion, stored back in K's dtype) and ``lidar2img = K @ E``.  Numpy arrays (or lists of them, as the dataset holds them) in, lists of new
        arrays out: the inputs are not changed."""
        ida = self.ida_mat().numpy()
        new_k, l2i = [], []
        for k, e in zip(intrinsics, extrinsics):
            k = np.array(k, copy=True)
            k[:3, :3] = ida @ k[:3, :3]
            new_k.append(k)
            l2i.append(k @ np.asarray(e))
        return new_k, l2i
