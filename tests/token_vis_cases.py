"""Token selection overlays (toc3d_amd.TokenVis, include/toc3d_vis.h): the cases of tests/golden/token_vis_cases.npz, their seeded inputs, the numpy
restatement of the reference's ``token_selection_vis`` (float32 arrays as it hands them to ``mmcv.imwrite``, and the bytes ``cv2.imwrite`` makes of them: round
half to even, clip) that the CPU and GPU tests compare with, and the set of pixel values on which two roundings and a fused multiply-add differ after rounding.
Importing this module needs no GPU."""
import os
import struct
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "token_vis_cases.npz")
FIXTURE_META = os.path.join(GOLDEN, "token_vis_cases.json")

SHIPPED_NORM = dict(mean=[103.530, 116.280, 123.675], std=[57.375, 57.120, 58.395], to_rgb=False)     # token_vis_ToC3D/ToC3D_faster.py:13-14
RGB_NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)              # the other convention mmdet configs use

# case -> V views, raw frames (H0, W0) padded to the token grid (hp, wp) at `patch`, K kept tokens per stage (None: no index lists), mask values, img_norm_cfg
CASES = {
    "one": dict(V=1, raw=(16, 16), grid=(1, 1), patch=16, K=(1,), soft=False, norm=SHIPPED_NORM),                  # one patch
    "two": dict(V=2, raw=(30, 44), grid=(2, 3), patch=16, K=(4, 2), soft=True, norm=RGB_NORM),                     # padded frames, to_rgb, soft masks
    "p8": dict(V=2, raw=(24, 40), grid=(3, 5), patch=8, K=(6, 3, 1), soft=False, norm=SHIPPED_NORM),               # three stages, another patch size
    "plain": dict(V=1, raw=(16, 32), grid=(1, 2), patch=16, K=None, soft=True, norm=SHIPPED_NORM),                 # no index lists: no keepidx files
}
# further shapes, against the restatement on the GPU: V, (H0, W0), (hp, wp), patch, K per stage, to_rgb
SHAPES = {
    "1x16x16": dict(V=1, raw=(16, 16), grid=(1, 1), patch=16, K=(1,), soft=False, norm=SHIPPED_NORM),
    "2x32x48": dict(V=2, raw=(32, 48), grid=(2, 3), patch=16, K=(3, 1), soft=True, norm=SHIPPED_NORM),
    "3x48x208": dict(V=3, raw=(48, 208), grid=(3, 13), patch=16, K=(20, 7, 0), soft=False, norm=SHIPPED_NORM),     # 13 patches wide; a stage that kept nothing
    "u8_30x44_rgb": dict(V=2, raw=(30, 44), grid=(2, 3), patch=16, K=(4, 2), soft=False, norm=RGB_NORM),
    "u8_30x44_bgr": dict(V=2, raw=(30, 44), grid=(2, 3), patch=16, K=(4, 2), soft=False, norm=SHIPPED_NORM),
    "w_odd": dict(V=2, raw=(9, 15), grid=(3, 5), patch=3, K=(5, 2), soft=True, norm=SHIPPED_NORM),                 # W % 4 != 0: the one-pixel form
}
BIG = dict(V=6, raw=(320, 800), grid=(20, 50), patch=16, K=(500, 400, 300), soft=False, norm=SHIPPED_NORM)         # the shipped size, three stages


def f32(v):
    return np.asarray(v, dtype=np.float32)


def to_bytes(arr):
    """cv2.imwrite's conversion of a float array: saturate_cast<uchar> = round half to even, clip."""
    return np.clip(np.rint(arr), 0, 255).astype(np.uint8)


def imnormalize(raw, mean, std, to_rgb):
    """mmcv.imnormalize restated: uint8 HWC -> float32 HWC, channels swapped when to_rgb, (x - mean) * (1 / std) with the reciprocal formed in float64."""
    x = raw.astype(np.float32)
    if to_rgb:
        x = x[..., ::-1]
    x = x - np.asarray(mean, dtype=np.float64).reshape(1, -1).astype(np.float32)
    return (x * (1 / np.asarray(std, dtype=np.float64).reshape(1, -1)).astype(np.float32)).astype(np.float32)


def imdenormalize(img, mean, std, to_bgr=True):
    """mmcv.imdenormalize restated in numpy float32: img * std, then + mean -- two roundings.  (OpenCV's own last-bit behaviour for float input is not run.)"""
    assert not to_bgr, "token_selection_vis passes to_bgr=False"
    return (img.astype(np.float32) * f32(std).reshape(1, -1)).astype(np.float32) + f32(mean).reshape(1, -1)


def inputs(c, seed):
    """The seeded inputs of a case: raw uint8 frames (V, H0, W0, 3); the float32 NCHW images the reference's pipeline makes of them (normalised, zero-padded to
    the token grid); per stage a mask (V, hp, wp, 1) float32, and keep / drop index lists (V, K) / (V, T - K) int64 -- or None."""
    rng = np.random.default_rng(seed)
    V, (H0, W0), (hp, wp), p = c["V"], c["raw"], c["grid"], c["patch"]
    H, W, T = hp * p, wp * p, hp * wp
    raw = rng.integers(0, 256, (V, H0, W0, 3), dtype=np.uint8)
    raw[0, 0, :4] = [[0, 0, 0], [255, 255, 255], [0, 255, 128], [255, 0, 1]][:min(4, W0)]
    n = c["norm"]
    img = np.zeros((V, 3, H, W), dtype=np.float32)
    for v in range(V):
        img[v, :, :H0, :W0] = imnormalize(raw[v], n["mean"], n["std"], n["to_rgb"]).transpose(2, 0, 1)
    L = len(c["K"]) if c["K"] is not None else 2
    masks, keeps, drops = [], [], []
    for l in range(L):
        order = np.stack([rng.permutation(T) for _ in range(V)]).astype(np.int64)
        K = c["K"][l] if c["K"] is not None else max(1, T // 2)
        m = np.zeros((V, T), dtype=np.float32)
        np.put_along_axis(m, order[:, :K], 1.0, axis=1)
        if c["soft"]:
            m = np.where(m > 0, m, rng.choice(f32([0.0, 0.25, 0.5]), size=(V, T))).astype(np.float32)
        masks.append(m.reshape(V, hp, wp, 1))
        keeps.append(order[:, :K])
        drops.append(order[:, K:])
    if c["K"] is None:
        keeps = drops = None
    return dict(raw=raw, img=img, masks=masks, keeps=keeps, drops=drops)


def case_seed(name):
    return 7000 + sorted(list(CASES) + list(SHAPES) + ["big"]).index(name)


def token_alpha(m, min_alpha=0.3, max_alpha=1.0):
    """float32 tokens -> the float32 alpha values the reference concatenates: 255 * (m * (max - min) + min), the difference a Python float, every op float32."""
    m = f32(m)
    return f32(255) * (m * np.float32(max_alpha - min_alpha) + np.float32(min_alpha))


def restated(img, masks, keeps, drops, norm, patch=16, min_alpha=0.3, max_alpha=1.0, prefix=""):
    """-> [(file name, float32 array (H, W, 3 | 4))] in the order the reference writes them.  ``img`` float32 (V, 3, H, W).  An empty keep row is every token
    dropped and an index outside [0, T) is ignored (the reference asserts or wraps there; the device code does this)."""
    out = []
    V, _, H, W = img.shape
    hp, wp = H // patch, W // patch
    up = lambda t: np.repeat(np.repeat(t.reshape(hp, wp, 1), patch, axis=0), patch, axis=1)
    for v in range(V):
        pic = np.ascontiguousarray(img[v].transpose(1, 2, 0))
        if norm is not None:
            pic = imdenormalize(pic, norm["mean"], norm["std"], to_bgr=False)
        for l, m in enumerate(masks):
            assert m.shape[1:] == (hp, wp, 1)
            out.append((f"{prefix}view{v}_layer{l}.png", np.concatenate([pic, up(token_alpha(m[v], min_alpha, max_alpha))], axis=-1)))
            out.append((f"{prefix}view{v}_layer{l}_ori.png", pic))
        if keeps is not None and drops is not None:
            for l, k in enumerate(keeps):
                member = np.zeros(hp * wp, dtype=np.float32)
                idx = np.asarray(k[v]).reshape(-1)
                member[idx[(idx >= 0) & (idx < hp * wp)]] = 1
                out.append((f"{prefix}view{v}_layer{l}_keepidx.png", np.concatenate([pic, up(token_alpha(member, min_alpha, max_alpha))], axis=-1)))
    return out


def restated_u8(raw, masks, keeps, drops, norm, patch=16, min_alpha=0.3, max_alpha=1.0, prefix=""):
    """The same for raw uint8 frames (V, H0, W0, 3): the frame's own bytes (channels swapped when to_rgb), rint(mean) in the padding."""
    V, H0, W0, _ = raw.shape
    hp, wp = masks[0].shape[1:3]
    pic = np.empty((V, hp * patch, wp * patch, 3), dtype=np.float32)
    pic[:] = np.rint(f32(norm["mean"]))
    pic[:, :H0, :W0] = raw[..., ::-1] if norm["to_rgb"] else raw
    return restated(pic.transpose(0, 3, 1, 2), masks, keeps, drops, None, patch, min_alpha, max_alpha, prefix)


def planes(files, V, L, with_keep):
    """The list of :func:`restated` as the arrays TokenVis.render returns: uint8 ori (V, H, W, 3), masks (L, V, H, W, 4), keepidx (L, V, H, W, 4) or None."""
    by = {os.path.basename(n): to_bytes(a) for n, a in files}
    ori = np.stack([by[f"view{v}_layer0_ori.png"] for v in range(V)])
    masks = np.stack([np.stack([by[f"view{v}_layer{l}.png"] for v in range(V)]) for l in range(L)])
    keep = np.stack([np.stack([by[f"view{v}_layer{l}_keepidx.png"] for v in range(V)]) for l in range(L)]) if with_keep else None
    return ori, masks, keep


# ---- two roundings against a fused multiply-add -----------------------------------------------------------------------------------------------------------------
def two_roundings(x, sd, mu):
    return (f32(x) * f32(sd)).astype(np.float32) + f32(mu)


def fused(x, sd, mu):
    """fma(x, sd, mu) rounded to float32: the product is exact in float64; -> (value, safe) where safe says that the float64 sum lies so far from a float32 tie
    that its own rounding cannot have changed the float32 result."""
    s = np.asarray(x, dtype=np.float64) * np.float64(f32(sd)) + np.float64(f32(mu))
    r = s.astype(np.float32)
    safe = (np.nextafter(s, np.inf).astype(np.float32) == r) & (np.nextafter(s, -np.inf).astype(np.float32) == r)
    return r, safe


def fma_sensitive(norm=SHIPPED_NORM, seed=11, per_byte=48):
    """(x float32 [n], c int [n]): normalised pixel values of channel c whose denormalised byte differs between two roundings and a fused multiply-add.  Such
    values sit within a float32 step of a half (a random search finds about one in 10^6), so the search draws, with a fixed seed, ``per_byte`` neighbours of
    the preimage of every k + 0.5."""
    rng = np.random.default_rng(seed)
    xs, cs = [], []
    for c in range(3):
        sd, mu = np.float32(norm["std"][c]), np.float32(norm["mean"][c])
        x0 = ((np.arange(255, dtype=np.float64) + 0.5 - np.float64(mu)) / np.float64(sd)).astype(np.float32)
        x = (x0.view(np.int32)[:, None] + rng.integers(-24, 25, (255, per_byte), dtype=np.int32)).astype(np.int32).view(np.float32).reshape(-1)
        x = np.unique(x)
        fu, safe = fused(x, sd, mu)
        hit = safe & (to_bytes(two_roundings(x, sd, mu)) != to_bytes(fu))
        xs.append(x[hit])
        cs.append(np.full(int(hit.sum()), c))
    return np.concatenate(xs), np.concatenate(cs)


# ---- a PNG decoder, to read back what toc3d_amd.token_vis writes ---------------------------------------------------------------------------------------------------
def decode_png(data):
    """A decoder for what the writer makes (8-bit RGB / RGBA, no interlace, any row filter the standard defines) -> uint8 (H, W, C) in file order."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF, "chunk CRC"
        chunks.append((tag, body))
        pos += 12 + n
    assert [t for t, _ in chunks][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    W, H, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, comp, filt, lace) == (8, 0, 0, 0) and ctype in (2, 6)
    C = 3 if ctype == 2 else 4
    raw = zlib.decompress(b"".join(b for t, b in chunks if t == b"IDAT"))
    rows = np.frombuffer(raw, dtype=np.uint8).reshape(H, 1 + W * C)
    assert (rows[:, 0] == 0).all(), "filter 0 on every row"
    return rows[:, 1:].reshape(H, W, C).copy()
