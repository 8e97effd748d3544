"""Token selection overlays: the reference's ``token_selection_vis`` (``models/utils/token_select_vis.py:27-80``; ``Petr3D.simple_test`` calls it at
``detectors/petr3d.py:562-579`` when ``token_select_vis=True``) with the pixels made on the device (``toc3d_token_alpha``, ``toc3d_token_vis_render``,
include/toc3d_vis.h).

The reference copies the images, masks and index lists to the host, denormalises with OpenCV, repeats every ``(hp, wp)`` mask up to the image with two
``np.repeat`` per stage, concatenates an alpha plane and writes ``V x stages x 3`` PNGs.  Here :meth:`TokenVis.render` makes the uint8 arrays ``cv2.imwrite``
would store (float32 arithmetic, round half to even, clip) in ``L + 1`` launches, and :meth:`TokenVis.write` copies the finished bytes to the host once and
encodes the reference's file names with a small PNG writer on the standard library.

Differences to the reference, by design:
* the images may also be the raw uint8 HWC frames the backbone takes when built with ``img_norm_cfg``: the image bytes are then the frame's own (channels
  swapped when ``to_rgb``), and the padding up to the token grid is ``rint(mean)``, which is what the reference gets from a zero-padded normalised image;
* an index outside ``[0, hp*wp)`` is ignored (the reference asserts; a negative one wraps there), and a stage that kept nothing (``K == 0``) renders every
  token as dropped (the reference's ``keep_idx.max()`` raises);
* ``img_norm_cfg=None`` writes the float image's own values rounded and clipped (the reference hands the float array to ``cv2.imwrite``, which does that);
* ``write(..., fix_colors=True)`` stores true colours; the default follows ``cv2.imwrite`` (below).  No CPU path for the pixels.
"""
from __future__ import annotations

import os
import struct
import zlib

import numpy as np
import torch

from . import lib

__all__ = ["TokenVis", "token_selection_vis", "encode_png", "write_png"]
_NAME = "toc3d_amd.TokenVis"


# ---- PNG: 8-bit RGB / RGBA, filter 0 on every row, zlib level 1 ---------------------------------------------------------------------------------------------------
def _chunk(tag: bytes, body: bytes) -> bytes:
    return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) & 0xFFFFFFFF)


def encode_png(rgb: np.ndarray) -> bytes:
    """uint8 (H, W, 3) or (H, W, 4), channels in PNG order (red first; alpha last) -> the bytes of a PNG file."""
    rgb = np.asarray(rgb)
    if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] not in (3, 4) or rgb.shape[0] < 1 or rgb.shape[1] < 1:
        raise ValueError(f"encode_png: expected uint8 (H, W, 3) or (H, W, 4), got {rgb.dtype} {rgb.shape}")
    H, W, C = rgb.shape
    rows = np.empty((H, 1 + W * C), dtype=np.uint8)
    rows[:, 0] = 0                                                          # filter type 0 (None)
    rows[:, 1:] = rgb.reshape(H, W * C)
    ihdr = struct.pack(">IIBBBBB", W, H, 8, 2 if C == 3 else 6, 0, 0, 0)
    return b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(rows.tobytes(), 1)) + _chunk(b"IEND", b"")


def write_png(path: str, arr: np.ndarray, blue_first: bool = True):
    """``cv2.imwrite(path, arr)`` for a uint8 (H, W, 3 | 4) array: with ``blue_first`` array channel 0 is stored as blue (OpenCV's convention), channel 2 as
    red, a fourth channel as alpha; without it the channels are stored in array order."""
    arr = np.asarray(arr)
    if blue_first:
        arr = np.concatenate([arr[..., 2::-1], arr[..., 3:]], axis=-1)
    with open(path, "wb") as f:
        f.write(encode_png(arr))


def _three(v, what, name):
    """mean / std of an img_norm_cfg -- a list, a numpy array or a tensor -- as three Python floats (the entry point takes them as float32)."""
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().numpy()
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    if v.size != 3:
        raise ValueError(f"{name}: img_norm_cfg['{what}'] must have 3 entries, got {v.size}")
    return [float(x) for x in v]


def _image_arg(imgs, img_norm_cfg, name):
    """The image argument of ``TokenVis.render`` and ``BoxVis.render`` (``name``: the caller, for the messages): f32 NCHW images or uint8 HWC frames on the
    device, leading dimensions flattened.  -> ``(img, u8, V, H0, W0, stride, mean, std, to_rgb)``: the tensor the entry point reads (f32 contiguous; uint8 as it
    came where its rows are dense pixels at one stride, else contiguous), the source size, the row stride in bytes (0 for f32) and what ``img_norm_cfg`` says
    (None: the image's own values, channels as they are)."""
    if not isinstance(imgs, torch.Tensor) or not imgs.is_cuda:
        raise RuntimeError(f"{name}: images must be CUDA/HIP tensors -- the HIP extension is the only compute path")
    u8 = imgs.dtype == torch.uint8
    img = imgs.reshape(-1, *imgs.shape[-3:]) if imgs.dim() != 4 else imgs
    if u8:
        if img_norm_cfg is None:
            raise ValueError(f"{name}: uint8 frames need img_norm_cfg=dict(mean=..., std=..., to_rgb=...)")
        if img.shape[3] != 3:
            raise ValueError(f"{name}: expected uint8 HWC frames (V, H, W, 3), got {tuple(imgs.shape)}")
        V, H0, W0 = img.shape[:3]
        if not (img.stride(3) == 1 and img.stride(2) == 3 and img.stride(1) >= 3 * W0 and img.stride(0) == H0 * img.stride(1)):
            img = img.contiguous()
        stride = img.stride(1)
    else:
        if img.dim() != 4 or img.shape[1] != 3:
            raise ValueError(f"{name}: expected f32 NCHW images (V, 3, H, W), got {tuple(imgs.shape)}")
        img = img.float().contiguous()
        V, H0, W0 = img.shape[0], img.shape[2], img.shape[3]
        stride = 0
    cfg = img_norm_cfg if img_norm_cfg is not None else dict(mean=[0.0, 0.0, 0.0], std=[1.0, 1.0, 1.0], to_rgb=False)
    mean, std = _three(cfg["mean"], "mean", name), _three(cfg["std"], "std", name)
    to_rgb = bool(cfg.get("to_rgb", True)) if img_norm_cfg is not None else False
    return img, u8, V, H0, W0, stride, mean, std, to_rgb


class TokenVis:
    """``token_selection_vis`` in two steps: :meth:`render` (device) and :meth:`write` (host).

    >>> vis = toc3d_amd.TokenVis(patch_size=16)
    >>> out = backbone(img, ...)                                            # ToC3DViTReturnType
    >>> r = vis.render(img, out.token_masks, out.keep_idx, out.drop_idx, img_norm_cfg)
    >>> vis.write(r, "./token_vis/0/")
    """

    def __init__(self, patch_size: int = 16, min_alpha: float = 0.3, max_alpha: float = 1.0):
        if int(patch_size) != patch_size or patch_size < 1:
            raise ValueError(f"{_NAME}: patch_size must be a positive integer, got {patch_size!r}")
        self.patch_size, self.min_alpha, self.max_alpha = int(patch_size), float(min_alpha), float(max_alpha)
        self._ws = {}

    def render(self, input_imgs, masks, keep_idxes=None, drop_idxes=None, img_norm_cfg=None):
        """``input_imgs``: f32 ``(V, 3, H, W)`` normalised images (leading dimensions are flattened), or uint8 ``(V, H0, W0, 3)`` raw frames (``img_norm_cfg`` is
        then required: its ``to_rgb`` and ``mean`` are used).  ``masks``: the backbone's list of L ``(V, hp, wp, 1)`` f32 token masks; ``keep_idxes`` /
        ``drop_idxes``: its lists of ``(V, K_s)`` int64 indices (``drop_idxes`` is only asked whether it is there, as in the reference).
        -> ``dict(ori (V, H, W, 3), masks (L, V, H, W, 4), keepidx (L, V, H, W, 4) or None, to_rgb)``: device uint8 tensors in a per-shape workspace of this
        object, valid until the next call; channel order as the reference's arrays (what ``imdenormalize(to_bgr=False)`` leaves).  ``L + 1`` launches."""
        img, u8, V, H0, W0, stride, mean, std, to_rgb = _image_arg(input_imgs, img_norm_cfg, _NAME)
        masks = list(masks)
        L, p = len(masks), self.patch_size
        if L == 0:
            raise ValueError(f"{_NAME}: no masks (a dense backbone has none)")
        with_keep = keep_idxes is not None and drop_idxes is not None        # :29, :61
        keeps = list(keep_idxes) if with_keep else []
        if with_keep and len(keeps) != L:
            raise ValueError(f"{_NAME}: {len(keeps)} keep lists for {L} masks")
        m0 = masks[0]
        if m0.dim() != 4 or m0.shape[0] != V or m0.shape[3] != 1:
            raise ValueError(f"{_NAME}: expected masks (V={V}, hp, wp, 1), got {tuple(m0.shape)}")
        hp, wp = m0.shape[1], m0.shape[2]
        H, W, T = hp * p, wp * p, hp * wp
        if u8 and not (H0 <= H and W0 <= W):
            raise ValueError(f"{_NAME}: frames {H0} x {W0} do not fit the {hp} x {wp} token grid at patch {p}")
        if not u8 and (H0 != H or W0 != W):                                 # :47-48
            raise ValueError(f"{_NAME}: images {H0} x {W0} are not the {hp} x {wp} token grid at patch {p}")
        if T > lib.VIS_MAX_TOKENS:
            raise ValueError(f"{_NAME}: {T} tokens a view > {lib.VIS_MAX_TOKENS} (TOC3D_VIS_MAX_TOKENS)")
        A, dev = (2 * L if with_keep else L), img.device
        key = (V, H, W, A, str(dev))
        if key not in self._ws:
            e = lambda *s: torch.empty(s, dtype=torch.uint8, device=dev)
            self._ws = {key: dict(alpha=e(A, V, T), ori=e(V, H, W, 3), rgba=e(A, V, H, W, 4))}          # one shape at a time: a frame's planes are tens of MB
        ws = self._ws[key]
        s = lib.stream_ptr()
        for l, m in enumerate(masks):
            if tuple(m.shape) != (V, hp, wp, 1) or not m.is_cuda:
                raise ValueError(f"{_NAME}: mask {l} is {tuple(m.shape)}, expected {(V, hp, wp, 1)} on the device")
            m = m.float().contiguous()
            k = None
            if with_keep:
                k = keeps[l]
                if k.dim() != 2 or k.shape[0] != V or k.dtype != torch.int64 or not k.is_cuda:
                    raise ValueError(f"{_NAME}: keep list {l} must be int64 (V={V}, K) on the device, got {k.dtype} {tuple(k.shape)}")
                if k.shape[1] > 1 and k.stride(1) != 1:
                    k = k.contiguous()
            K = k.shape[1] if with_keep else 0
            lib.call("toc3d_token_alpha", m, k if K else None, (max(k.stride(0), K) if K else 0), K, V, T, self.min_alpha, self.max_alpha,
                     ws["alpha"][l], ws["alpha"][L + l] if with_keep else None, s)
        lib.call("toc3d_token_vis_render", img, int(u8), stride, V, H0, W0, H, W, p, ws["alpha"], A, *mean, *std, int(to_rgb), ws["ori"], ws["rgba"], s)
        return dict(ori=ws["ori"], masks=ws["rgba"][:L], keepidx=ws["rgba"][L:] if with_keep else None, to_rgb=to_rgb)

    def write(self, rendered, output_path, fix_colors: bool = False, views=None):
        """The reference's files under ``output_path`` (created): per view and stage ``view{v}_layer{l}.png`` (RGBA), ``view{v}_layer{l}_ori.png`` (RGB; the
        same image once per stage, as the reference writes it) and, when rendered, ``view{v}_layer{l}_keepidx.png``.  One copy to the host, then the encoder.
        The files follow ``cv2.imwrite``: array channel 0 is stored as blue -- so with a ``to_rgb=True`` config they come out red/blue-swapped, exactly as the
        reference's do; ``fix_colors=True`` stores true colours whatever ``to_rgb`` is.  ``views``: a range of the rendered views to write, numbered from 0 in
        the file names (default: all).  -> the list of file names, in the reference's order."""
        os.makedirs(output_path, exist_ok=True)
        ori = rendered["ori"].cpu().numpy()
        masks = rendered["masks"].cpu().numpy()
        keep = None if rendered["keepidx"] is None else rendered["keepidx"].cpu().numpy()
        blue_first = not (fix_colors and rendered.get("to_rgb", False))     # a to_rgb image holds red first: stored in array order when colours are fixed
        names = []
        views = range(ori.shape[0]) if views is None else views
        for n, v in enumerate(views):
            for l in range(masks.shape[0]):
                for tag, arr in ((f"view{n}_layer{l}.png", masks[l, v]), (f"view{n}_layer{l}_ori.png", ori[v])):
                    names.append(os.path.join(output_path, tag))
                    write_png(names[-1], arr, blue_first)
            if keep is not None:
                for l in range(keep.shape[0]):
                    names.append(os.path.join(output_path, f"view{n}_layer{l}_keepidx.png"))
                    write_png(names[-1], keep[l, v], blue_first)
        return names


def token_selection_vis(input_imgs, masks, keep_idxes, drop_idxes, img_norm_cfg, output_path, patch_size: int = 16, min_alpha: float = 0.3,
                        max_alpha: float = 1.0):
    """The reference's function, under its signature: render and write."""
    vis = TokenVis(patch_size, min_alpha, max_alpha)
    return vis.write(vis.render(input_imgs, masks, keep_idxes, drop_idxes, img_norm_cfg), output_path)
