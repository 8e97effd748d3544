"""Camera ingest (toc3d_amd.ResizeCropFlipRotImage, include/toc3d_ingest.h): the cases of tests/golden/ingest_cases.npz, their seeded inputs, and the numpy
restatement of Pillow's 8-bit resampler that the CPU and GPU tests compare with.  The restatement works in int64 and reproduces Pillow's int32 accumulator
because ``resample_tables`` asserts that no row of coefficients can overflow it.  Importing this module needs no GPU."""
import os

import numpy as np

from support import DEV  # noqa: F401  (the device the GPU tests use)
from toc3d_amd import preprocess as P

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "ingest_cases.npz")
FIXTURE_META = os.path.join(GOLDEN, "ingest_cases.json")

# case -> (source H, W), final_dim (fH, fW), and what the geometry must come to: resize_dims (newW, newH), crop, ksize per axis (h, v)
CASES = {
    "a": dict(H=90, W=160, final_dim=(32, 80), resize_dims=(80, 45), crop=(0, 13, 80, 45), ksize=(9, 9)),          # scale 0.5, 9 taps, crop_h 13
    "b": dict(H=53, W=97, final_dim=(29, 40), resize_dims=(53, 29), crop=(6, 0, 46, 29), ksize=(9, 9)),            # non-integer scale, crop_w 6, odd widths
    "c": dict(H=90, W=160, final_dim=(80, 160), resize_dims=(160, 90), crop=(0, 10, 160, 90), ksize=(1, 1)),       # identity resize, crop only
    "d": dict(H=48, W=64, final_dim=(70, 100), resize_dims=(100, 75), crop=(0, 5, 100, 75), ksize=(5, 5)),         # upscale, 5 taps, crop_h 5
}
# further resize strengths, against the restatement (and Pillow, on the CPU): (H, W), final_dim, ksize -- 7 and 11 have a 4-byte source form of their own, 13 has none
SCALES = {"k7": ((48, 64), (36, 48), 7), "k11": ((48, 64), (21, 28), 11), "k13": ((48, 64), (18, 24), 13), "k9_wide": ((70, 200), (35, 100), 9)}
FORMS = ("random", "stripes")            # V = 1 random bytes; V = 3: random, alternating 0 / 255 columns, alternating 0 / 255 rows
BIG = {"320x800": (320, 800), "800x1600": (800, 1600)}      # 6 x 900 x 1600 -> final_dim


def conf(H, W, final_dim):
    """A data_aug_conf with the shipped configs' keys (projects/configs/token_vis_ToC3D/ToC3D_faster.py, ida_aug_conf)."""
    return dict(resize_lim=(0.38, 0.55), final_dim=tuple(final_dim), bot_pct_lim=(0.0, 0.0), rot_lim=(0.0, 0.0), H=H, W=W, rand_flip=True)


def case_conf(case):
    c = CASES[case]
    return conf(c["H"], c["W"], c["final_dim"])


def case_seed(case, form):
    return 1000 * (1 + sorted(CASES).index(case)) + FORMS.index(form)


def frames(case, form):
    """uint8 (V, H, W, 3): the seeded input of a fixture case."""
    c = CASES[case]
    H, W = c["H"], c["W"]
    rng = np.random.default_rng(case_seed(case, form))
    if form == "random":
        return rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8)
    img = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
    img[1] = ((np.arange(W) % 2) * 255).astype(np.uint8)[None, :, None]          # over- and undershoot of the bicubic taps: the clamp at both ends
    img[2] = ((np.arange(H) % 2) * 255).astype(np.uint8)[:, None, None]
    return img


def cameras(case, form, V):
    """float64 intrinsics and extrinsics (V, 4, 4) as the dataset holds them (lists of 4 x 4 arrays)."""
    rng = np.random.default_rng(case_seed(case, form) + 500)
    K = np.tile(np.eye(4), (V, 1, 1))
    K[:, 0, 0] = K[:, 1, 1] = 1200.0 + rng.uniform(-50, 50, V)
    K[:, 0, 2], K[:, 1, 2] = 800.0 + rng.uniform(-20, 20, V), 450.0 + rng.uniform(-20, 20, V)
    E = np.tile(np.eye(4), (V, 1, 1))
    E[:, :3, :] = rng.standard_normal((V, 3, 4))
    return K, E


def big_frames(seed=7):
    """uint8 (6, 900, 1600, 3): smooth gradients plus noise, alternating lines (views 1, 2) and a 5 x 3 checkerboard (view 3), from a seeded generator."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:900, 0:1600]
    img = np.empty((6, 900, 1600, 3), dtype=np.uint8)
    for v in range(6):
        base = (x * (v + 1) // 7 + y * (6 - v) // 5)[..., None] + np.array([0, 85, 170])
        img[v] = (base + rng.integers(0, 64, (900, 1600, 3))).astype(np.uint8)
    img[1, :, ::2] = 0
    img[1, :, 1::2] = 255
    img[2, ::2] = 255
    img[2, 1::2] = 0
    img[3] = np.where(((x // 5 + y // 3) % 2)[..., None] == 0, 0, 255)       # edges wide enough to over- and undershoot at scale 0.5: the clamp at both ends
    return img


def pass_1d(src, coef, bounds, axis):
    """One pass of ImagingResample for 8-bit data along ``axis`` (0: rows, 1: columns) of src uint8 (R, C, 3): 2^21 + sum pixel * k, >> 22, clipped."""
    s = src.astype(np.int64)
    n = len(bounds)
    out = np.empty((n,) + src.shape[1:] if axis == 0 else (src.shape[0], n, 3), dtype=np.uint8)
    for i in range(n):
        lo, cnt = int(bounds[i, 0]), int(bounds[i, 1])
        k = coef[i, :cnt].astype(np.int64)
        if axis == 0:
            acc = (1 << 21) + np.tensordot(k, s[lo:lo + cnt], axes=(0, 0))
            out[i] = np.clip(acc >> 22, 0, 255)
        else:
            acc = (1 << 21) + np.tensordot(s[:, lo:lo + cnt], k, axes=(1, 0))
            out[:, i] = np.clip(acc >> 22, 0, 255)
    return out


def restated(img, tables):
    """uint8 (V, H0, W0, 3) -> (V, fH, fW, 3): the horizontal pass over the source rows the vertical taps need, rounded to uint8, then the vertical pass."""
    (ch, bh, _), (cv, bv, _) = tables["h"], tables["v"]
    r0, r1 = int(bv[0, 0]), int((bv[:, 0] + bv[:, 1]).max())
    bv0 = bv.copy()
    bv0[:, 0] -= r0
    return np.stack([pass_1d(pass_1d(f[r0:r1], ch, bh, 1), cv, bv0, 0) for f in img])


def restated_case(conf_, img):
    return restated(img, P.ResizeCropFlipRotImage(conf_, training=False).host_tables())
