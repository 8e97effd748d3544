"""Cases and restated references of the kernels that only move, pad, interleave or transpose data (shared by test_gpu_layout_kernels.py, test_cpu_layout_cases.py and
test_cpu_layout_abi.py; no GPU needed here, and no reference calls the library):

  toc3d_copy_bytes, toc3d_copy_segments, toc3d_nhwc_to_nchw                                   csrc/tokens.hip
  toc3d_im2col_patches, toc3d_im2col_patches_u8, toc3d_normalize_images, toc3d_pack_weight, toc3d_pack_swiglu, toc3d_conv3x3_nhwc      csrc/gemm.hip
  toc3d_im2col_3x3                                                                            csrc/scorer.hip

Every result is a permutation, a zero pad, a round-to-nearest-even conversion or two single-rounded f32 operations, so the comparison is ``bits_equal``; only the
implicit 3x3 conv is also held to an f64 reference (``conv_ok``).  Every reference and input builder takes the device as an argument: the CPU tests evaluate them
on the host, the GPU tests on the device (large inputs never cross the bus).

PLANTED holds, per reference, the results a plausible kernel bug would give; tests/test_cpu_layout_cases.py shows that the comparison the GPU test applies tells
each of them from the truth on every case where the bug can act (a variant returns None where it cannot: no padding, one channel, one image ...)."""
import torch
import torch.nn.functional as F

from epilogue_cases import TOL_F32

# ---- first-pass capacities of the capped grid-stride loops: lanes = workgroup cap x 256 ------------------------------------------------------------------------
COPY_BYTES_LANES = 2048 * 256      # csrc/tokens.hip, toc3d_copy_bytes: `(work + 255) / 256 < 2048 ? ... : 2048` workgroups of 256
COPY_SEGS_LANES = 64 * 256         # csrc/tokens.hip, toc3d_copy_segments: `bx = per < 1 ? 1 : (per > 64 ? 64 : per)` workgroups of 256 per segment
IMG_LANES = 8192 * 256             # csrc/gemm.hip, toc3d_im2col_patches / toc3d_im2col_patches_u8 / toc3d_normalize_images: `... < 8192 ? ... : 8192`
PACK_LANES = 4096 * 256            # csrc/gemm.hip, toc3d_pack_weight / toc3d_pack_swiglu: `... < 4096 ? ... : 4096`
CAPS = dict(copy_bytes=COPY_BYTES_LANES, copy_segments=COPY_SEGS_LANES, im2col_patches=IMG_LANES, im2col_patches_u8=IMG_LANES, normalize_images=IMG_LANES,
            pack_weight=PACK_LANES, pack_swiglu=PACK_LANES)


def first_pass_items(kernel, shape):
    """The work-item count the entry point of ``kernel`` computes for ``shape`` (one item = one trip of one lane through the grid-stride loop):
      copy_bytes        (nbytes, dst offset, src offset)  16-byte units when both pointers are 16-byte aligned and there is one, else bytes
      copy_segments     (nbytes, dst offset, src offset)  16-byte units of ONE segment (aligned), else 0: only the byte loop runs
      im2col_patches    (V, Cin, H, W, p)                 four px per item
      im2col_patches_u8 (V, Hp, Wp, p)                    four px, all three channels, per item
      normalize_images  (V, Hp, Wp)                       four px, all three channels, per item
      pack_weight       (Np, Kp)                          one packed element per item
      pack_swiglu       (Hp, Kp)                          one packed element per item, 2 * Hp rows"""
    if kernel == "copy_bytes":
        n, do, so = shape
        n16 = n // 16 if do % 16 == 0 and so % 16 == 0 else 0
        return n16 if n16 > 0 else n
    if kernel == "copy_segments":
        n, do, so = shape
        return n // 16 if do % 16 == 0 and so % 16 == 0 else 0
    if kernel == "im2col_patches":
        V, Cin, H, W, p = shape
        return V * (H // p) * (W // p) * Cin * p * p // 4
    if kernel == "im2col_patches_u8":
        V, Hp, Wp, p = shape
        return V * (Hp // p) * (Wp // p) * p * (p // 4)
    if kernel == "normalize_images":
        V, Hp, Wp = shape
        return V * Hp * (Wp // 4)
    if kernel == "pack_weight":
        Np, Kp = shape
        return Np * Kp
    if kernel == "pack_swiglu":
        Hp, Kp = shape
        return 2 * Hp * Kp
    raise KeyError(kernel)


def ru(a, b):
    return (a + b - 1) // b * b


# ---- the comparisons -----------------------------------------------------------------------------------------------------------------------------------------
def bits(t):
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def bits_equal(a, b):
    """Zero differing bits, on whichever device the operands live (NaN sentinels and signed zeros compare as bit patterns)."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def conv_ratio(got, ref):
    """max|got - ref| over TOL_F32 * max|ref| (<= 1.0 required): the project's bar for f32-accumulated outputs."""
    return ((got.double() - ref).abs().max() / (TOL_F32 * ref.abs().max())).item()


def conv_ok(got, ref):
    return conv_ratio(got, ref) <= 1.0


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------------------------
PREFILL = 0x5A                     # what a copy's destination holds before the call; rand_bytes never produces it, so a byte that was not copied shows


def _gen(seed, device):
    return torch.Generator(device=device).manual_seed(seed)


def rand_bytes(n, seed, device="cpu"):
    """n bytes, none equal to PREFILL."""
    t = torch.randint(0, 255, (n,), generator=_gen(seed, device), device=device, dtype=torch.int16)
    return (t + (t >= PREFILL).to(torch.int16)).to(torch.uint8)


def rand_f32(shape, seed, device="cpu", scale=1.0):
    return torch.randn(*shape, generator=_gen(seed, device), device=device) * scale


def rand_u8(shape, seed, device="cpu"):
    return torch.randint(0, 256, shape, generator=_gen(seed, device), device=device, dtype=torch.int16).to(torch.uint8)


IMG_NORM = dict(mean=[103.530, 116.280, 123.675], std=[57.375, 57.120, 58.395])       # projects/configs/ToC3D/ToC3D_faster.py:13-14


# ---- case tables -----------------------------------------------------------------------------------------------------------------------------------------------
MIB = 1 << 20
# (nbytes, dst byte offset, src byte offset, wraps)
COPY_BYTES = [(0, 0, 0, False), (1, 0, 0, False), (15, 0, 0, False), (16, 0, 0, False), (17, 0, 0, False), (4101, 0, 0, False),
              (8 * MIB + 4096 + 5, 0, 0, True),                                   # n16 = 524 544: a second trip of the 16-byte loop, then a 5-byte tail
              (4101, 1, 0, False), (4101, 0, 3, False), (4101, 3, 3, False),
              (COPY_BYTES_LANES + 300, 1, 1, True)]                              # the byte loop takes a second trip
SEG_BODY = 3 * COPY_SEGS_LANES * 16                                              # the largest aligned segment whose lanes all miss the four-deep body
# one launch of 16 segments: (nbytes, dst offset, src offset)
COPY_SEGMENTS_MIXED = [(0, 0, 0), (1, 0, 0), (15, 0, 0), (17, 0, 0), (SEG_BODY, 0, 0), (SEG_BODY + 16, 0, 0), (MIB + 48 + 7, 0, 0),
                       (300001, 1, 0), (300001, 0, 3), (300001, 5, 5), (4096, 0, 0), (100, 0, 0), (33, 2, 0), (64, 0, 0), (16, 0, 0), (4097, 0, 16)]
COPY_SEGMENTS_SMALL = [(0, 0, 0), (1, 0, 0), (15, 0, 0), (16, 0, 0), (17, 0, 0), (255, 1, 0), (256, 0, 0), (1000, 0, 7), (4095, 3, 3), (4080, 0, 0)]
COPY_SEGMENTS_17 = [(37 + 16 * i + (i % 3), i % 2, (i % 4) * (i % 3 == 0)) for i in range(17)]

NHWC = [(1, 1, 1), (2, 31, 33), (3, 33, 31), (2, 37, 1), (1, 64, 256), (2, 1000, 48)]                           # (V, T, C)
IM2COL = [(1, 3, 16, 16, 16, False), (2, 1, 8, 12, 4, False), (3, 3, 32, 48, 8, False), (2, 3, 48, 32, 16, False),
          (12, 3, 320, 800, 16, True)]                                          # (V, Cin, H, W, p, wraps); the last: two streams of six cameras at the small shipped size
NORMALIZE = [(3, 33, 47, 64, 64, False), (12, 609, 1099, 640, 1120, True)]      # (V, H, W, Hp, Wp, wraps)
PACK_WEIGHT = [(1, 1, 128, 64, False), (130, 70, 256, 128, False), (200, 128, 256, 128, False), (1100, 950, 1152, 960, True)]      # (N, K, Np, Kp, wraps)
PACK_SWIGLU = [(Hd, K, 64 if Hd <= 17 else 384, Kp, False) for Hd in (1, 16, 17, 341) for K, Kp in ((64, 64), (70, 128))] + [(600, 890, 640, 896, True)]   # (Hd, K, Hp, Kp, wraps)
CONV = [(1, 1, 1, 64, 128, 128), (3, 1, 7, 64, 128, 128), (3, 5, 1, 64, 128, 128), (2, 3, 5, 128, 256, 256), (5, 2, 2, 64, 64, 68), (2, 9, 17, 192, 130, 130)]   # (V, h, w, C, Cout, ldo)
# the tile variants of test_conv3x3_implicit_gemm_equals_im2col_gemm (tests/test_gpu_ops.py)
CONV_VARIANTS = (1, 8, 9, 10, 13, 14, 16, 17, 19, 22, 26, 28, 33, 45, 49, 51, 110, 114, 126)
CONV_VARIANTS_BF16 = (24, 27, 30)


def wrap_checks():
    """[(kernel, shape, wraps)] of every case of a capped grid-stride kernel: a wrap case must exceed the first pass, a tail case must stay below it."""
    out = [("copy_bytes", (n, do, so), wr) for n, do, so, wr in COPY_BYTES]
    out += [("im2col_patches", (V, Cin, H, W, p), wr) for V, Cin, H, W, p, wr in IM2COL]
    out += [("normalize_images", (V, Hp, Wp), wr) for V, H, W, Hp, Wp, wr in NORMALIZE]
    out += [("im2col_patches_u8", (V, Hp, Wp, 16), wr) for V, H, W, Hp, Wp, wr in NORMALIZE]
    out += [("pack_weight", (Np, Kp), wr) for N, K, Np, Kp, wr in PACK_WEIGHT]
    out += [("pack_swiglu", (Hp, Kp), wr) for Hd, K, Hp, Kp, wr in PACK_SWIGLU]
    return out


# ---- references ------------------------------------------------------------------------------------------------------------------------------------------------
def ref_copy(dst_before, src):
    """A copy of len(src) bytes into a destination of the same length."""
    return src.clone()


def ref_nhwc_to_nchw(x):
    """[V, T, C] -> [V, C, T]."""
    return x.permute(0, 2, 1).clone(memory_format=torch.contiguous_format)      # (always new memory: .contiguous() hands x itself back when C == 1)


def ref_im2col(img, p):
    """NCHW [V, C, H, W] -> rows (v, pr, pc), columns (ch, py, px)."""
    V, C, H, W = img.shape
    h, w = H // p, W // p
    return img.reshape(V, C, h, p, w, p).permute(0, 2, 4, 1, 3, 5).reshape(V * h * w, C * p * p)


def norm_consts(mean, std, device):
    """(mean, 1 / std) as the entry points form them: f32 mean, fl32(1 / f64(fl32(std)))."""
    m = torch.tensor(mean, dtype=torch.float32)
    s = (1.0 / torch.tensor(std, dtype=torch.float32).double()).float()
    return m.to(device), s.to(device)


def ref_normalize(u8, mean, std, to_rgb, Hp, Wp, pad_value=None):
    """uint8 HWC [V, H, W, 3] -> f32 NCHW [V, 3, Hp, Wp]: channel flip if to_rgb, fl32(fl32(x - mean) * fl32(1 / f64(std))) -- two separate f32 operations, each
    rounded once --, zeros below and right of the image.  (pad_value: what a planted variant puts there instead.)"""
    V, H, W, _ = u8.shape
    m, s = norm_consts(mean, std, u8.device)
    x = u8.float()
    if to_rgb:
        x = x.flip(-1)
    d = x - m
    y = d * s
    out = torch.zeros(V, 3, Hp, Wp, device=u8.device)
    if pad_value is not None:
        out += pad_value.view(1, 3, 1, 1)
    out[:, :, :H, :W] = y.permute(0, 3, 1, 2)
    return out


def ref_pack_weight(w, Np, Kp, tdt):
    N, K = w.shape
    out = torch.zeros(Np, Kp, device=w.device)
    out[:N, :K] = w
    return out.to(tdt)


def _interleave(a, b, group):
    """Rows of a and b [Hp, ...] interleaved in groups of ``group``: a's rows g*group .., then b's rows g*group .., per group g."""
    Hp = a.shape[0]
    return torch.stack([a.reshape(Hp // group, group, *a.shape[1:]), b.reshape(Hp // group, group, *b.shape[1:])], 1).reshape(2 * Hp, *a.shape[1:])


def ref_pack_swiglu(w1, w2, b1, b2, Hp, Kp, tdt, group=16, pad_bias=False):
    """-> (W [2 Hp, Kp] in tdt, bias f32 [2 Hp]): packed row 32 b + i is w1 row 16 b + i, row 32 b + 16 + i is w2 row 16 b + i, the bias goes the same way; units
    from Hd on and columns from K on are zero.  (group, pad_bias: the planted variants.)"""
    Hd, K = w1.shape
    pw = lambda w: F.pad(w, (0, Kp - K, 0, Hp - Hd))
    pb = (lambda b: torch.cat([b, b[Hd - 1:Hd].expand(Hp - Hd)])) if pad_bias else (lambda b: F.pad(b, (0, Hp - Hd)))
    return _interleave(pw(w1), pw(w2), group).to(tdt), _interleave(pb(b1), pb(b2), group)


def _taps_3x3(x, check_cols=True, check_rows=True):
    """The nine neighbours of every pixel of NHWC x [V, h, w, C] -> [V*h*w, 9, C], by explicit index arithmetic.  check_cols / check_rows False: the planted
    variants that leave out one of the two border checks and only keep the tap inside the whole tensor."""
    V, h, w, C = x.shape
    M = V * h * w
    m = torch.arange(M, device=x.device)
    xx, yy, vv = m % w, (m // w) % h, m // (w * h)
    flat = x.reshape(M, C)
    out = []
    for ky in range(3):
        for kx in range(3):
            dy, dx = ky - 1, kx - 1
            ok = torch.ones(M, dtype=torch.bool, device=x.device)
            if check_rows:
                ok &= (yy + dy >= 0) & (yy + dy < h)
            if check_cols:
                ok &= (xx + dx >= 0) & (xx + dx < w)
            src = m + dy * w + dx
            ok &= (src >= 0) & (src < M)
            out.append(torch.where(ok[:, None], flat[src.clamp(0, M - 1)], torch.zeros((), device=x.device, dtype=x.dtype)))
    return torch.stack(out, 1)


def ref_im2col_3x3(x):
    """NHWC [V, h, w, C] -> rows (v, y, x), columns (ky, kx, c), pad 1."""
    V, h, w, C = x.shape
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    return torch.cat([xp[:, ky:ky + h, kx:kx + w, :] for ky in range(3) for kx in range(3)], -1).reshape(V * h * w, 9 * C)


def ref_conv3x3_f64(x, Wc, b):
    """F.conv2d (pad 1) in f64 on the operands as the dtype rounded them: x NHWC [V, h, w, C], Wc [Cout, C, 3, 3], b [Cout] -> [V*h*w, Cout] in f64."""
    V, h, w, C = x.shape
    return F.conv2d(x.double().permute(0, 3, 1, 2), Wc.double(), b.double(), padding=1).permute(0, 2, 3, 1).reshape(V * h * w, Wc.shape[0])


def conv_weight_rows(Wc):
    """[Cout, C, 3, 3] -> [Cout, 9 C] in toc3d_im2col_3x3's column order (ky, kx, c)."""
    return Wc.permute(0, 2, 3, 1).reshape(Wc.shape[0], -1)


def conv_from_cols(cols, Wc, b):
    """The conv as a matmul over im2col rows, in f64."""
    return cols.double() @ conv_weight_rows(Wc).double().T + b.double()


# ---- planted wrong variants ------------------------------------------------------------------------------------------------------------------------------------
def _im2col_swapped(img, p):
    V, C, H, W = img.shape
    h, w = H // p, W // p
    return img.reshape(V, C, h, p, w, p).permute(0, 2, 4, 1, 5, 3).reshape(V * h * w, C * p * p)


def _im2col_channel_minor(img, p):
    V, C, H, W = img.shape
    if C == 1:
        return None
    h, w = H // p, W // p
    return img.reshape(V, C, h, p, w, p).permute(0, 2, 4, 3, 5, 1).reshape(V * h * w, C * p * p)


def _normalize_no_flip(u8, mean, std, to_rgb, Hp, Wp):
    return ref_normalize(u8, mean, std, not to_rgb, Hp, Wp)


def _normalize_pad_not_zero(u8, mean, std, to_rgb, Hp, Wp):
    if (Hp, Wp) == tuple(u8.shape[1:3]):
        return None
    m, s = norm_consts(mean, std, u8.device)
    return ref_normalize(u8, mean, std, to_rgb, Hp, Wp, pad_value=(0.0 - m) * s)


def _swiglu_groups_of_32(w1, w2, b1, b2, Hp, Kp, tdt):
    return ref_pack_swiglu(w1, w2, b1, b2, Hp, Kp, tdt, group=32)


def _swiglu_pad_bias(w1, w2, b1, b2, Hp, Kp, tdt):
    return None if Hp == w1.shape[0] else ref_pack_swiglu(w1, w2, b1, b2, Hp, Kp, tdt, pad_bias=True)


def _pack_weight_no_column_pad(w, Np, Kp, tdt):
    """Columns from K on read on into the next row instead of holding zero."""
    N, K = w.shape
    if Kp == K:
        return None
    n, k = torch.arange(N, device=w.device)[:, None], torch.arange(Kp, device=w.device)[None, :]
    out = torch.zeros(Np, Kp, device=w.device)
    out[:N] = w.reshape(-1)[(n * K + k) % (N * K)]
    return out.to(tdt)


def _transpose_drops_channel_tail(x, before):
    """before: what the output buffer [V, C, T] held."""
    V, T, C = x.shape
    if C % 32 == 0:
        return None
    out = ref_nhwc_to_nchw(x)
    out[:, C - C % 32:, :] = before[:, C - C % 32:, :]
    return out


def _transpose_drops_token_tail(x, before):
    V, T, C = x.shape
    if T % 32 == 0:
        return None
    out = ref_nhwc_to_nchw(x)
    out[:, :, T - T % 32:] = before[:, :, T - T % 32:]
    return out


def _copy_stops_at_16(dst_before, src):
    n = len(src)
    if n % 16 == 0:
        return None
    out = src.clone()
    out[n - n % 16:] = dst_before[n - n % 16:]
    return out


def copy_skips_a_stripe(dst_before, src, lanes):
    """The second of the four loads in flight is never stored: 16-byte units [lanes, 2 lanes) of the first trip (aligned copies longer than 3 * lanes units)."""
    n16 = len(src) // 16
    if n16 <= 3 * lanes:
        return None
    out = src.clone()
    out[lanes * 16:2 * lanes * 16] = dst_before[lanes * 16:2 * lanes * 16]
    return out


def _gather_flat_image(x):
    """The image treated as flat: x - 1 at x = 0 reads the previous row's last pixel (the column check is missing)."""
    return _taps_3x3(x, check_cols=False).reshape(-1, 9 * x.shape[3])


def _gather_across_images(x):
    """y - 1 at y = 0 reads the last row of the previous image (the row check is missing)."""
    return _taps_3x3(x, check_rows=False).reshape(-1, 9 * x.shape[3])


def gather_fault_applies(name, V, h, w):
    """Where the two border faults must show: the flat image wherever a row has a neighbour to run into (w > 1, and a pixel before it), across images when
    there is more than one."""
    return (w > 1 and V * h > 1) if name == "flat_image" else V > 1


PLANTED = {
    "im2col": {"px_py_exchanged": _im2col_swapped, "channel_minor": _im2col_channel_minor},
    "normalize": {"no_channel_flip": _normalize_no_flip, "pad_is_normalized_zero": _normalize_pad_not_zero},
    "pack_swiglu": {"groups_of_32": _swiglu_groups_of_32, "pad_units_get_a_bias": _swiglu_pad_bias},
    "pack_weight": {"no_column_pad": _pack_weight_no_column_pad},
    "nhwc_to_nchw": {"drops_channel_tail": _transpose_drops_channel_tail, "drops_token_tail": _transpose_drops_token_tail},
    "copy": {"stops_at_whole_16_bytes": _copy_stops_at_16},
    "copy_segments": {"stops_at_whole_16_bytes": _copy_stops_at_16, "skips_a_stripe": lambda before, src: copy_skips_a_stripe(before, src, COPY_SEGS_LANES)},
    "im2col_3x3": {"flat_image": _gather_flat_image, "across_images": _gather_across_images},
}
