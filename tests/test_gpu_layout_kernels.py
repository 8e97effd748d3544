"""GPU: the kernels that only move, pad, interleave or transpose data (toc3d_copy_bytes, toc3d_copy_segments, toc3d_nhwc_to_nchw, toc3d_im2col_patches,
toc3d_im2col_patches_u8, toc3d_normalize_images, toc3d_pack_weight, toc3d_pack_swiglu, toc3d_im2col_3x3) bit for bit against the plain-indexing references of
tests/layout_cases.py, and the implicit 3x3 conv (toc3d_conv3x3_nhwc) at maps smaller than one tile -- past the first trip of every capped grid-stride loop,
through the four-loads-in-flight body of the segment copy and its hand-over to the plain loop and the byte tail, at the channel and token tails of the 32 x 32
transpose tile.

Common to every case: the output lies between 256 guard bytes of 0xA5 that must be unchanged; padding columns and rows hold the NaN sentinel (support.sent's
pattern) and are compared bit for bit with the rest; inputs are unchanged after the call.  Large inputs are made on the device with a seeded generator and
compared there.  tests/test_cpu_layout_cases.py shows that these comparisons reject every planted wrong variant and that every wrap case wraps.  Each test prints
what it asserted on (-s); profiles/layout_kernels_parity.txt is one such run."""
import numpy as np
import pytest
import torch

import layout_cases as L
from support import DEV, S, SENT16, is_sent, pack, worst_report
from toc3d_amd import lib

pytestmark = pytest.mark.gpu

DTYPES = [("fp32", lib.F32, torch.float32), ("bf16", lib.BF16, torch.bfloat16)]          # as tests/test_gpu_ops.py
GUARD, GUARD_BYTE = 256, 0xA5
note, _report = worst_report("layout kernels", 24, bound="bound TOL_F32 * max|ref|")


class Guarded:
    """[256 guard bytes | `off` more guard bytes | payload of nbytes | 256 guard bytes]: the payload starts `off` bytes past a 16-byte boundary."""
    def __init__(self, nbytes, off=0, fill16=SENT16, fill8=None):
        self.lo, self.n = GUARD + off, nbytes
        self.raw = torch.full((self.lo + nbytes + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
        assert self.raw.data_ptr() % 16 == 0
        if fill8 is not None:
            self.payload.fill_(fill8)
        else:
            self.payload.view(torch.int16).fill_(fill16)

    @property
    def payload(self):
        return self.raw[self.lo:self.lo + self.n]

    def typed(self, tdt, rows, ld):
        return self.payload.view(tdt).view(rows, ld)

    def guards_ok(self):
        return bool((self.raw[:self.lo] == GUARD_BYTE).all()) and bool((self.raw[self.lo + self.n:] == GUARD_BYTE).all())


def _esz(tdt):
    return 2 if tdt == torch.bfloat16 else 4


def _expect(buf, ref, rows, cols):
    """What a [R, ld] output that held the sentinel must hold afterwards: ref in [:rows, :cols], the sentinel everywhere else."""
    exp = buf.clone()
    exp[:rows, :cols] = ref
    return exp


def _wraps(kernel, shape, wraps):
    items, cap = L.first_pass_items(kernel, shape), L.CAPS[kernel]
    assert items > cap if wraps else items < cap, (kernel, shape, items, cap)
    return f"{items} items / first pass {cap}" + (" (wraps)" if wraps else "")


# ---- toc3d_copy_bytes / toc3d_copy_segments ----------------------------------------------------------------------------------------------------------------------
def _copy_pair(n, do, so, seed):
    sraw = L.rand_bytes(so + n + 16, seed, DEV)
    assert sraw.data_ptr() % 16 == 0
    return Guarded(n, off=do, fill8=L.PREFILL), sraw, sraw[so:so + n]


def _check_copy(tag, g, sraw, src, sraw0):
    whole = torch.full_like(g.raw, GUARD_BYTE)
    whole[g.lo:g.lo + g.n] = src
    assert torch.equal(g.raw, whole), f"{tag}: {int((g.raw != whole).sum())} bytes of payload + guards differ, first at {int((g.raw != whole).nonzero()[0]) - g.lo} of {g.n}"
    assert torch.equal(sraw, sraw0), f"{tag}: the source changed"


@pytest.mark.parametrize("n,do,so,wraps", L.COPY_BYTES)
def test_copy_bytes(n, do, so, wraps):
    how = _wraps("copy_bytes", (n, do, so), wraps)
    g, sraw, src = _copy_pair(n, do, so, seed=n % 1000)
    sraw0 = sraw.clone()
    lib.call("toc3d_copy_bytes", g.payload, src, n, S())
    torch.cuda.synchronize()
    _check_copy(f"copy_bytes {n} [{do}/{so}]", g, sraw, src, sraw0)
    print(f"[layout] toc3d_copy_bytes {n} bytes [dst +{do} / src +{so}], {'16-byte' if do % 16 == 0 and so % 16 == 0 and n >= 16 else 'byte'} path, {how}: "
          f"payload and both guards equal bit for bit, source unchanged")


@pytest.mark.parametrize("table", ["COPY_SEGMENTS_MIXED", "COPY_SEGMENTS_SMALL", "COPY_SEGMENTS_17"])
def test_copy_segments(table):
    """MIXED: one launch of 16 segments, 64 workgroups each: the four-deep body for no lane / one lane / every lane, the plain loop after it, byte tails, unaligned
    segments on the byte loop.  SMALL: one workgroup per segment.  17: lib.copy_segments splits into two launches."""
    segs = getattr(L, table)
    made = [_copy_pair(n, do, so, seed=100 + i) for i, (n, do, so) in enumerate(segs)]
    before = [sraw.clone() for _, sraw, _ in made]
    lib.copy_segments([(g.payload, src) for g, _, src in made], S())
    torch.cuda.synchronize()
    lanes = L.COPY_SEGS_LANES
    for (n, do, so), (g, sraw, src), s0 in zip(segs, made, before):
        _check_copy(f"{table} segment {n} [{do}/{so}]", g, sraw, src, s0)
        n16 = L.first_pass_items("copy_segments", (n, do, so))
        body = 0 if table != "COPY_SEGMENTS_MIXED" or n16 <= 3 * lanes else min(lanes, n16 - 3 * lanes)
        print(f"[layout] toc3d_copy_segments {table[14:].lower()}: {n} bytes [dst +{do} / src +{so}]: {n16} 16-byte units, four-deep body in {body} lanes, "
              f"{n - 16 * n16} bytes on the byte loop: payload and guards equal bit for bit")
    if table == "COPY_SEGMENTS_MIXED":
        assert max(n for n, _, _ in segs) // 16 > 64 * 256                    # the launch has its 64 workgroups per segment: stride == COPY_SEGS_LANES


def test_copy_segments_empty_launch():
    lib.call("toc3d_copy_segments", 0, None, None, None, S())
    g, sraw, src = _copy_pair(0, 0, 0, seed=1)
    lib.copy_segments([(g.payload, src)], S())                                   # one segment of no bytes: returns before the launch
    torch.cuda.synchronize()
    assert g.guards_ok()
    print("[layout] toc3d_copy_segments n = 0 and one empty segment: TOC3D_OK, nothing written")


# ---- toc3d_nhwc_to_nchw ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,T,C", L.NHWC)
def test_nhwc_to_nchw(V, T, C):
    x = L.rand_f32((V, T, C), seed=4, device=DEV)
    x0 = x.clone()
    g = Guarded(V * C * T * 4)
    out = g.typed(torch.float32, V * C, T)
    lib.call("toc3d_nhwc_to_nchw", x, out, V, T, C, S())
    torch.cuda.synchronize()
    assert L.bits_equal(out.view(V, C, T), L.ref_nhwc_to_nchw(x0)) and g.guards_ok() and torch.equal(x, x0)
    print(f"[layout] toc3d_nhwc_to_nchw V={V} T={T} (T % 32 = {T % 32}) C={C} (C % 32 = {C % 32}): {V * C * T} elements equal bit for bit, guards and input unchanged")


# ---- toc3d_im2col_patches ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [0, 32])
@pytest.mark.parametrize("name,dt,tdt", DTYPES)
@pytest.mark.parametrize("V,Cin,H,W,p,wraps", L.IM2COL)
def test_im2col_patches(V, Cin, H, W, p, wraps, name, dt, tdt, pad):
    how = _wraps("im2col_patches", (V, Cin, H, W, p), wraps)
    img = L.rand_f32((V, Cin, H, W), seed=1, device=DEV)
    img0 = img.clone()
    M, Kc = V * (H // p) * (W // p), Cin * p * p
    ldo = Kc + pad
    g = Guarded(M * ldo * _esz(tdt))
    out = g.typed(tdt, M, ldo)
    exp = _expect(out, L.ref_im2col(img0, p).to(tdt), M, Kc)
    lib.call("toc3d_im2col_patches", dt, img, out, ldo, V, Cin, H, W, p, S())
    torch.cuda.synchronize()
    assert L.bits_equal(out, exp), f"{int((L.bits(out) != L.bits(exp)).sum())} of {out.numel()} elements differ (sentinel columns included)"
    assert g.guards_ok() and torch.equal(img, img0)
    print(f"[layout] toc3d_im2col_patches {name} V={V} Cin={Cin} {H}x{W} p={p} ldo={ldo}, {how}: {M} x {Kc} equal bit for bit, "
          f"{pad} sentinel columns per row, guards and input unchanged")


# ---- toc3d_normalize_images / toc3d_im2col_patches_u8 -----------------------------------------------------------------------------------------------------------------
MEAN, STD = L.IMG_NORM["mean"], L.IMG_NORM["std"]
_IMG = {}


def _image(case, to_rgb):
    """(u8 on the device, its untouched copy, ref_normalize evaluated on the device): made once per case, shared by the tests below and never written.  The device
    evaluation of the reference is tied to oracle/image_oracle.py on the small case whenever a new entry is made."""
    V, H, W, Hp, Wp, _ = case
    if (case, to_rgb) not in _IMG:
        from oracle import image_oracle as I
        sV, sH, sW, sHp, sWp, _ = L.NORMALIZE[0]
        small = L.rand_u8((sV, sH, sW, 3), seed=2, device=DEV)
        on_dev = L.ref_normalize(small, MEAN, STD, to_rgb, sHp, sWp).cpu()
        oracle = torch.from_numpy(I.prepare_images(small.cpu().numpy(), MEAN, STD, to_rgb, 32))
        assert L.bits_equal(on_dev, oracle), "ref_normalize evaluated on the device differs from oracle/image_oracle.py"
        u8 = L.rand_u8((V, H, W, 3), seed=2, device=DEV)
        _IMG.clear()                                                          # one large image set at a time
        _IMG[(case, to_rgb)] = (u8, u8.clone(), L.ref_normalize(u8, MEAN, STD, to_rgb, Hp, Wp))
    return _IMG[(case, to_rgb)]


@pytest.mark.parametrize("to_rgb", [False, True])
@pytest.mark.parametrize("case", L.NORMALIZE, ids=lambda c: "x".join(map(str, c[:5])))
def test_normalize_images(case, to_rgb):
    V, H, W, Hp, Wp, wraps = case
    how = _wraps("normalize_images", (V, Hp, Wp), wraps)
    u8, u80, ref = _image(case, to_rgb)
    g = Guarded(V * 3 * Hp * Wp * 4)
    out = g.typed(torch.float32, V * 3 * Hp, Wp)
    lib.call("toc3d_normalize_images", u8, V, H, W, torch.tensor(MEAN), torch.tensor(STD), int(to_rgb), out, Hp, Wp, S())
    torch.cuda.synchronize()
    assert L.bits_equal(out.view(V, 3, Hp, Wp), ref), f"{int((L.bits(out.view(V, 3, Hp, Wp)) != L.bits(ref)).sum())} of {ref.numel()} elements differ"
    assert g.guards_ok() and torch.equal(u8, u80)
    print(f"[layout] toc3d_normalize_images V={V} {H}x{W} -> {Hp}x{Wp} to_rgb={int(to_rgb)}, {how}: {ref.numel()} elements equal bit for bit "
          f"({Hp - H} padded rows, {Wp - W} padded columns exactly 0, W % 4 = {W % 4}), guards and input unchanged; device reference == image_oracle on the small case")


@pytest.mark.parametrize("pad", [0, 64])
@pytest.mark.parametrize("name,dt,tdt", DTYPES)
@pytest.mark.parametrize("to_rgb", [False, True])
@pytest.mark.parametrize("case", L.NORMALIZE, ids=lambda c: "x".join(map(str, c[:5])))
def test_im2col_patches_u8(case, to_rgb, name, dt, tdt, pad):
    """Against ref_im2col(ref_normalize(...)) -- never against the other kernel."""
    V, H, W, Hp, Wp, wraps = case
    p = 16
    how = _wraps("im2col_patches_u8", (V, Hp, Wp, p), wraps)
    u8, u80, ref = _image(case, to_rgb)
    M, Kc = V * (Hp // p) * (Wp // p), 3 * p * p
    ldo = Kc + pad
    g = Guarded(M * ldo * _esz(tdt))
    out = g.typed(tdt, M, ldo)
    exp = _expect(out, L.ref_im2col(ref, p).to(tdt), M, Kc)
    lib.call("toc3d_im2col_patches_u8", dt, u8, V, H, W, torch.tensor(MEAN), torch.tensor(STD), int(to_rgb), out, ldo, Hp, Wp, p, S())
    torch.cuda.synchronize()
    assert L.bits_equal(out, exp), f"{int((L.bits(out) != L.bits(exp)).sum())} of {out.numel()} elements differ (sentinel columns included)"
    assert g.guards_ok() and torch.equal(u8, u80)
    print(f"[layout] toc3d_im2col_patches_u8 {name} V={V} {H}x{W} -> {Hp}x{Wp} to_rgb={int(to_rgb)} ldo={ldo}, {how}: {M} x {Kc} equal bit for bit, "
          f"{pad} sentinel columns per row, guards and input unchanged")


# ---- toc3d_pack_weight / toc3d_pack_swiglu ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dt,tdt", DTYPES)
@pytest.mark.parametrize("N,K,Np,Kp,wraps", L.PACK_WEIGHT)
def test_pack_weight(N, K, Np, Kp, wraps, name, dt, tdt):
    how = _wraps("pack_weight", (Np, Kp), wraps)
    w = L.rand_f32((N, K), seed=3, device=DEV)
    w0 = w.clone()
    g = Guarded(Np * Kp * _esz(tdt))
    out = g.typed(tdt, Np, Kp)
    lib.call("toc3d_pack_weight", dt, w, N, K, out, Np, Kp, S())
    torch.cuda.synchronize()
    ref = L.ref_pack_weight(w0, Np, Kp, tdt)
    assert L.bits_equal(out, ref), f"{int((L.bits(out) != L.bits(ref)).sum())} of {ref.numel()} elements differ"
    if tdt == torch.bfloat16:
        assert L.bits_equal(out[:N, :K], w0.bfloat16())                     # the bf16 bits are torch's round-to-nearest-even
    assert g.guards_ok() and torch.equal(w, w0)
    print(f"[layout] toc3d_pack_weight {name} [{N}, {K}] -> [{Np}, {Kp}], {how}: {Np * Kp} elements equal bit for bit (padding exactly +0), guards and input unchanged")


@pytest.mark.parametrize("name,dt,tdt", DTYPES)
@pytest.mark.parametrize("Hd,K,Hp,Kp,wraps", L.PACK_SWIGLU)
def test_pack_swiglu(Hd, K, Hp, Kp, wraps, name, dt, tdt):
    how = _wraps("pack_swiglu", (Hp, Kp), wraps)
    ins = [L.rand_f32((Hd, K), 5, DEV), L.rand_f32((Hd, K), 6, DEV), L.rand_f32((Hd,), 7, DEV), L.rand_f32((Hd,), 8, DEV)]
    ins0 = [t.clone() for t in ins]
    gw, gb = Guarded(2 * Hp * Kp * _esz(tdt)), Guarded(2 * Hp * 4)
    out_w, out_b = gw.typed(tdt, 2 * Hp, Kp), gb.typed(torch.float32, 1, 2 * Hp)
    lib.call("toc3d_pack_swiglu", dt, *ins, Hd, K, out_w, out_b, Hp, Kp, S())
    torch.cuda.synchronize()
    ref_w, ref_b = L.ref_pack_swiglu(*ins0, Hp, Kp, tdt)
    assert L.bits_equal(out_w, ref_w), f"{int((L.bits(out_w) != L.bits(ref_w)).sum())} of {ref_w.numel()} weight elements differ"
    assert L.bits_equal(out_b[0], ref_b), f"{int((L.bits(out_b[0]) != L.bits(ref_b)).sum())} of {2 * Hp} bias elements differ"
    assert gw.guards_ok() and gb.guards_ok() and all(torch.equal(a, b) for a, b in zip(ins, ins0))
    print(f"[layout] toc3d_pack_swiglu {name} Hd={Hd} K={K} -> [{2 * Hp}, {Kp}] + bias [{2 * Hp}], {how}: weights and bias equal bit for bit "
          f"({Hp - Hd} padding units and {Kp - K} padding columns exactly +0), guards and inputs unchanged")


# ---- toc3d_im2col_3x3 / toc3d_conv3x3_nhwc at maps smaller than a tile -------------------------------------------------------------------------------------------------
CONV_DTYPES = DTYPES + [("fp32x3", lib.F32X3, torch.float32)]                  # F32X3: f32 buffers and packed weights, bf16 x 3 products (fused_args admits it for the conv)
EXTRA_ROWS = 3                                                                  # rows from M on: never written


def _served(fn):
    """-> None if the call returned a result, the message if the variant cannot serve it (any other failure is raised)."""
    try:
        fn()
        return None
    except RuntimeError as e:
        if "cannot serve" in str(e) or "bad epilogue" in str(e):
            return str(e)
        raise


@pytest.mark.parametrize("name,dt,tdt", CONV_DTYPES)
@pytest.mark.parametrize("V,h,w,C,Co,ldo", L.CONV)
def test_conv3x3_small_maps(V, h, w, C, Co, ldo, name, dt, tdt):
    """(a) toc3d_im2col_3x3 == ref_im2col_3x3 rounded to the dtype, ldo = 9C + 32 over the sentinel; (b) toc3d_conv3x3_nhwc == toc3d_im2col_3x3 +
    toc3d_linear_ex(EPI_RESIDUAL) on the same tile variant, bit for bit; (c) max|conv - f64| <= TOL_F32 * max|ref|.  h*w < BM for every tile: a tile holds several
    images, rows past M are clamped to M - 1, and an out-of-image tap must read the zero line, not the neighbouring row or image.  A variant either serves the
    case -- then (b) and (c) hold -- or refuses it ("cannot serve" / "bad epilogue or variant"), for the conv and for the GEMM alike; it never returns other bits.
    (A tile whose wide K-tile does not divide C is launched with the 128-byte K-tile of the same shape, launch_cfg in csrc/gemm_kernels.h: a result, held to (b) and (c).)"""
    M, K = V * h * w, 9 * C
    pdt = lib.F32 if dt == lib.F32X3 else dt
    x = L.rand_f32((V, h, w, C), seed=3, device=DEV)
    Wc, b = L.rand_f32((Co, C, 3, 3), seed=4, device=DEV, scale=K ** -0.5), L.rand_f32((Co,), seed=5, device=DEV)
    x_act = x.to(tdt).contiguous()
    x_act0, xf = x_act.clone(), x_act.float()
    # (a)
    ldc = K + 32
    gc = Guarded((M + EXTRA_ROWS) * ldc * _esz(tdt))
    col = gc.typed(tdt, M + EXTRA_ROWS, ldc)
    exp = _expect(col, L.ref_im2col_3x3(xf).to(tdt), M, K)
    lib.call("toc3d_im2col_3x3", pdt, xf, col, ldc, V, h, w, C, S())
    torch.cuda.synchronize()
    assert L.bits_equal(col, exp), f"(a) {int((L.bits(col) != L.bits(exp)).sum())} of {col.numel()} elements differ (sentinel rows and columns included)"
    assert gc.guards_ok()
    # the f64 reference, once per case and dtype
    ref64 = L.ref_conv3x3_f64(xf, Wc.to(tdt).float(), b)
    wp = pack(L.conv_weight_rows(Wc), pdt, tdt)
    zeros = torch.zeros(16, dtype=torch.uint8, device=DEV)
    served, worst = [], 0.0
    for v in L.CONV_VARIANTS + (L.CONV_VARIANTS_BF16 if dt == lib.BF16 else ()):
        gl, gv = Guarded((M + EXTRA_ROWS) * ldo * 4), Guarded((M + EXTRA_ROWS) * ldo * 4)
        lin, out = gl.typed(torch.float32, M + EXTRA_ROWS, ldo), gv.typed(torch.float32, M + EXTRA_ROWS, ldo)
        e_lin = _served(lambda: lib.call("toc3d_linear_ex", dt, lib.EPI_RESIDUAL, v, col, ldc, wp, wp.shape[1], b, lin, ldo, None, 0, 0, None, None, M, Co, K, 0, S()))
        e_conv = _served(lambda: lib.call("toc3d_conv3x3_nhwc", dt, v, x_act, C, wp, wp.shape[1], b, out, ldo, V, h, w, Co, zeros, S()))
        torch.cuda.synchronize()
        assert (e_lin is None) == (e_conv is None), f"variant {v}: the conv and the GEMM disagree on whether the tile serves: {e_conv!r} / {e_lin!r}"
        if e_conv is not None:
            assert is_sent(out) and gv.guards_ok(), f"variant {v} refused the case and still wrote"
            continue
        assert L.bits_equal(out, lin), f"(b) variant {v}: {int((L.bits(out) != L.bits(lin)).sum())} of {out.numel()} elements differ from im2col + GEMM"
        assert is_sent(out[M:]) and (ldo == Co or is_sent(out[:M, Co:])), f"variant {v}: rows from M on or columns [Cout, ldo) were written"
        assert gv.guards_ok() and gl.guards_ok(), f"variant {v}: a guard changed"
        ratio = L.conv_ratio(out[:M, :Co], ref64)
        worst = max(worst, ratio)
        note(f"conv3x3 {name}", ratio)
        assert ratio <= 1.0, f"(c) variant {v}: max|conv - f64| = {ratio:.3f} x TOL_F32 * max|ref|"
        served.append(v)
    assert 16 in served, "the default tile must serve every case"
    assert torch.equal(L.bits(x_act), L.bits(x_act0)) and L.bits_equal(col, exp)
    print(f"[layout] conv3x3 {name} V={V} {h}x{w} C={C} Cout={Co} ldo={ldo} (M={M}): im2col_3x3 == reference bit for bit over {M} x {K} (+32 sentinel columns, "
          f"{EXTRA_ROWS} sentinel rows); conv == im2col + GEMM bit for bit on {len(served)} tile variants {served}; worst max|conv - f64| = {worst:.3f} x TOL_F32 * max|ref|; "
          f"sentinel rows / columns, guards and inputs unchanged")
