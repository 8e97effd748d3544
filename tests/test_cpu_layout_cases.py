"""CPU: the restated references of tests/layout_cases.py are pinned to independent formulations, every "wrap" case provably takes a second trip of its capped
grid-stride loop (and every tail case stays inside the first), and every planted wrong variant is rejected by the very comparison tests/test_gpu_layout_kernels.py
applies -- bit equality, or the f64 bound of the implicit 3x3 conv -- on every case where the planted bug can act."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import epilogue_cases as E
import layout_cases as L


# ---- the references against independent formulations --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,Cin,H,W,p,wraps", [c for c in L.IM2COL if not c[-1]])
def test_ref_im2col_is_unfold(V, Cin, H, W, p, wraps):
    img = L.rand_f32((V, Cin, H, W), seed=1)
    unf = F.unfold(img, kernel_size=p, stride=p)                              # [V, Cin*p*p, h*w], channel-major (ch, py, px) blocks
    assert L.bits_equal(L.ref_im2col(img, p), unf.permute(0, 2, 1).reshape(-1, Cin * p * p).contiguous())


@pytest.mark.parametrize("V,h,w,C,Co,ldo", L.CONV)
def test_ref_im2col_3x3_and_ref_conv_agree_through_a_matmul(V, h, w, C, Co, ldo):
    x, Wc, b = L.rand_f32((V, h, w, C), seed=3), L.rand_f32((Co, C, 3, 3), seed=4, scale=(9 * C) ** -0.5), L.rand_f32((Co,), seed=5)
    cols = L.ref_im2col_3x3(x)
    assert L.bits_equal(cols, L._taps_3x3(x).reshape(-1, 9 * C))              # the slicing form against the index-arithmetic form
    conv = L.ref_conv3x3_f64(x, Wc, b)
    err = ((L.conv_from_cols(cols, Wc, b) - conv).abs().max() / conv.abs().max()).item()
    assert err < 1e-13, err


def test_ref_normalize_is_the_image_oracle(golden_dir):
    from oracle import image_oracle as I
    g = np.load(os.path.join(golden_dir, "image_norm.npz"))
    mean, std, div = g["mean"].tolist(), g["std"].tolist(), int(g["size_divisor"])
    for tag in "abcd":
        u8, to_rgb = g[f"{tag}_u8"], bool(g[f"{tag}_to_rgb"])
        exp = torch.from_numpy(I.prepare_images(u8, mean, std, to_rgb, div))
        got = L.ref_normalize(torch.from_numpy(u8), mean, std, to_rgb, exp.shape[2], exp.shape[3])
        assert L.bits_equal(got, exp), tag
        assert L.bits_equal(got, torch.from_numpy(g[f"{tag}_expected"])), tag


@pytest.mark.parametrize("Hd,K,Hp,Kp,wraps", [c for c in L.PACK_SWIGLU if not c[-1]])
def test_ref_pack_swiglu_unpacks_with_swiglu_units(Hd, K, Hp, Kp, wraps):
    """Pack, multiply by identity-like rows, unpack with epilogue_cases.swiglu_units: unit u of the hidden layer is silu(w1[u] . a + b1[u]) * (w2[u] . a + b2[u])."""
    w1, w2, b1, b2 = L.rand_f32((Hd, K), 5), L.rand_f32((Hd, K), 6), L.rand_f32((Hd,), 7), L.rand_f32((Hd,), 8)
    Wp, bp = L.ref_pack_swiglu(w1, w2, b1, b2, Hp, Kp, torch.float32)
    a = torch.zeros(K + 1, Kp)
    a[:K, :K] = torch.eye(K)                                                # row k picks column k of the weights; the last row only the bias
    z = a @ Wp.T + bp
    got = E.swiglu_units(z.clone(), Hd, Hp)
    z1, z2 = a[:, :K] @ w1.T + b1, a[:, :K] @ w2.T + b2
    # (silu over a strided view and over a contiguous tensor may differ in the last bit: the permutation is what is under test, so a mispaired unit is O(1) off)
    assert torch.allclose(got[:, :Hd], F.silu(z1) * z2, rtol=1e-6, atol=1e-7) and not got[:, Hd:].any()
    Wl, bl = torch.zeros(2 * Hp, Kp), torch.zeros(2 * Hp)                    # ... and bit for bit against the header's sentence, unit by unit
    for u in range(Hd):
        blk, i = divmod(u, 16)
        Wl[32 * blk + i, :K], Wl[32 * blk + 16 + i, :K], bl[32 * blk + i], bl[32 * blk + 16 + i] = w1[u], w2[u], b1[u], b2[u]
    assert L.bits_equal(Wp, Wl) and L.bits_equal(bp, bl)
    assert not Wp[:, K:].any() and not E.swiglu_units(z.clone(), Hp, Hp)[:, Hd:].any()      # padding units: zero weights AND zero bias -> silu(0) * 0 without the mask


# ---- wrap cases wrap ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,shape,wraps", L.wrap_checks())
def test_wrap_cases_take_a_second_trip_and_tail_cases_do_not(kernel, shape, wraps):
    items, cap = L.first_pass_items(kernel, shape), L.CAPS[kernel]
    assert items > cap if wraps else items < cap, (kernel, shape, items, cap)


def test_every_capped_kernel_has_a_wrap_case():
    assert {k for k, _, wr in L.wrap_checks() if wr} == set(L.CAPS) - {"copy_segments"}
    n16 = [L.first_pass_items("copy_segments", c) for c in L.COPY_SEGMENTS_MIXED]
    lanes = L.COPY_SEGS_LANES
    assert 3 * lanes in n16 and 3 * lanes + 1 in n16                          # the boundary of the four-deep body: no lane, then one lane
    big = L.MIB + 48 + 7
    assert (big, 0, 0) in L.COPY_SEGMENTS_MIXED and big // 16 == 4 * lanes + 3 and big % 16 == 7      # every lane one trip of the body, three lanes the plain loop, 7-byte tail
    assert max(n for n, _, _ in L.COPY_SEGMENTS_SMALL) // 16 <= 256 and len(L.COPY_SEGMENTS_MIXED) == 16 and len(L.COPY_SEGMENTS_17) == 17
    assert sum(1 for n, do, so in L.COPY_SEGMENTS_MIXED if n == 300001 and (do % 16 or so % 16)) == 3


# ---- planted variants are rejected ----------------------------------------------------------------------------------------------------------------------------------
def _reject(ref, planted, acted):
    """Each planted result differs from ref under bits_equal; a variant that returns None cannot act on this case.  -> the names that acted."""
    for name, wrong in planted.items():
        if wrong is None:
            continue
        assert wrong.shape == ref.shape and not L.bits_equal(wrong, ref), name
        acted.add(name)


ACTED = {k: set() for k in L.PLANTED}


@pytest.mark.parametrize("V,Cin,H,W,p,wraps", L.IM2COL)
def test_planted_im2col_variants_differ(V, Cin, H, W, p, wraps):
    img = L.rand_f32((V, Cin, H, W), seed=1)
    for tdt in (torch.float32, torch.bfloat16):
        _reject(L.ref_im2col(img, p).to(tdt), {k: None if f(img, p) is None else f(img, p).to(tdt) for k, f in L.PLANTED["im2col"].items()}, ACTED["im2col"])


@pytest.mark.parametrize("to_rgb", [False, True])
@pytest.mark.parametrize("V,H,W,Hp,Wp,wraps", L.NORMALIZE)
def test_planted_normalize_variants_differ(V, H, W, Hp, Wp, wraps, to_rgb):
    u8 = L.rand_u8((V, H, W, 3), seed=2)
    ref = L.ref_normalize(u8, L.IMG_NORM["mean"], L.IMG_NORM["std"], to_rgb, Hp, Wp)
    wrong = {k: f(u8, L.IMG_NORM["mean"], L.IMG_NORM["std"], to_rgb, Hp, Wp) for k, f in L.PLANTED["normalize"].items()}
    _reject(ref, wrong, ACTED["normalize"])
    for tdt in (torch.float32, torch.bfloat16):                               # ... and through the fused im2col
        _reject(L.ref_im2col(ref, 16).to(tdt), {k: None if v is None else L.ref_im2col(v, 16).to(tdt) for k, v in wrong.items()}, set())


@pytest.mark.parametrize("N,K,Np,Kp,wraps", L.PACK_WEIGHT)
def test_planted_pack_weight_variants_differ(N, K, Np, Kp, wraps):
    w = L.rand_f32((N, K), seed=3)
    for tdt in (torch.float32, torch.bfloat16):
        _reject(L.ref_pack_weight(w, Np, Kp, tdt), {k: f(w, Np, Kp, tdt) for k, f in L.PLANTED["pack_weight"].items()}, ACTED["pack_weight"])


@pytest.mark.parametrize("Hd,K,Hp,Kp,wraps", L.PACK_SWIGLU)
def test_planted_pack_swiglu_variants_differ(Hd, K, Hp, Kp, wraps):
    w1, w2, b1, b2 = L.rand_f32((Hd, K), 5), L.rand_f32((Hd, K), 6), L.rand_f32((Hd,), 7), L.rand_f32((Hd,), 8)
    for tdt in (torch.float32, torch.bfloat16):
        Wp, bp = L.ref_pack_swiglu(w1, w2, b1, b2, Hp, Kp, tdt)
        wrong = {k: f(w1, w2, b1, b2, Hp, Kp, tdt) for k, f in L.PLANTED["pack_swiglu"].items()}
        # the two outputs are compared separately on the device: a variant is rejected when either differs
        for name, pair in wrong.items():
            if pair is None:
                continue
            assert not (L.bits_equal(pair[0], Wp) and L.bits_equal(pair[1], bp)), name
            ACTED["pack_swiglu"].add(name)
        assert not L.bits_equal(wrong["groups_of_32"][0], Wp) and not L.bits_equal(wrong["groups_of_32"][1], bp)
        if wrong["pad_units_get_a_bias"] is not None:
            assert not L.bits_equal(wrong["pad_units_get_a_bias"][1], bp)


@pytest.mark.parametrize("V,T,C", L.NHWC)
def test_planted_transpose_variants_differ(V, T, C):
    import support
    x = L.rand_f32((V, T, C), seed=4)
    before = support.sent(V * C, T, device="cpu").view(V, C, T)
    _reject(L.ref_nhwc_to_nchw(x), {k: f(x, before) for k, f in L.PLANTED["nhwc_to_nchw"].items()}, ACTED["nhwc_to_nchw"])


@pytest.mark.parametrize("n,do,so,wraps", L.COPY_BYTES)
def test_planted_copy_bytes_variants_differ(n, do, so, wraps):
    src, before = L.rand_bytes(n, seed=n % 1000), torch.full((n,), L.PREFILL, dtype=torch.uint8)
    assert not (src == L.PREFILL).any()
    _reject(L.ref_copy(before, src), {k: f(before, src) for k, f in L.PLANTED["copy"].items()}, ACTED["copy"])


@pytest.mark.parametrize("table", ["COPY_SEGMENTS_MIXED", "COPY_SEGMENTS_SMALL", "COPY_SEGMENTS_17"])
def test_planted_copy_segments_variants_differ(table):
    for i, (n, do, so) in enumerate(getattr(L, table)):
        src, before = L.rand_bytes(n, seed=100 + i), torch.full((n,), L.PREFILL, dtype=torch.uint8)
        wrong = {k: f(before, src) for k, f in L.PLANTED["copy_segments"].items()}
        if do % 16 or so % 16:
            wrong["skips_a_stripe"] = None                                    # the byte loop has no four-deep body
        _reject(L.ref_copy(before, src), wrong, ACTED["copy_segments"])
        if table == "COPY_SEGMENTS_MIXED" and L.first_pass_items("copy_segments", (n, do, so)) > 3 * L.COPY_SEGS_LANES:
            assert wrong["skips_a_stripe"] is not None


@pytest.mark.parametrize("V,h,w,C,Co,ldo", L.CONV)
def test_planted_border_faults_differ_in_the_gather_and_exceed_the_conv_bound(V, h, w, C, Co, ldo):
    x, Wc, b = L.rand_f32((V, h, w, C), seed=3), L.rand_f32((Co, C, 3, 3), seed=4, scale=(9 * C) ** -0.5), L.rand_f32((Co,), seed=5)
    for tdt in (torch.float32, torch.bfloat16):
        xa, Wa = x.to(tdt).float(), Wc.to(tdt).float()
        cols, conv = L.ref_im2col_3x3(xa), L.ref_conv3x3_f64(xa, Wa, b)
        assert L.conv_ok(L.conv_from_cols(cols, Wa, b), conv)                  # the truth passes its own bar
        for name, f in L.PLANTED["im2col_3x3"].items():
            wrong = f(xa)
            if not L.gather_fault_applies(name, V, h, w):
                continue
            assert not L.bits_equal(wrong.to(tdt), cols.to(tdt)), name
            ratio = L.conv_ratio(L.conv_from_cols(wrong, Wa, b), conv)
            assert ratio > 100.0, (name, ratio)                                # not a near miss: orders of magnitude past TOL_F32 * max|ref|
            ACTED["im2col_3x3"].add(name)


def test_every_planted_variant_acted_on_some_case():
    """A variant that no case can tell from the truth would be a hole in the tables.  (Run on its own, this test first goes through the small cases itself.)"""
    if any(ACTED[ref] != set(table) for ref, table in L.PLANTED.items()):
        for c in L.IM2COL[:-1]:
            test_planted_im2col_variants_differ(*c)
        test_planted_normalize_variants_differ(*L.NORMALIZE[0], to_rgb=True)
        for c in L.PACK_WEIGHT[:-1]:
            test_planted_pack_weight_variants_differ(*c)
        for c in L.PACK_SWIGLU[:-1]:
            test_planted_pack_swiglu_variants_differ(*c)
        for c in L.NHWC:
            test_planted_transpose_variants_differ(*c)
        for c in L.COPY_BYTES[:6]:
            test_planted_copy_bytes_variants_differ(*c)
        test_planted_copy_segments_variants_differ("COPY_SEGMENTS_MIXED")
        for c in L.CONV:
            test_planted_border_faults_differ_in_the_gather_and_exceed_the_conv_bound(*c)
    for ref, table in L.PLANTED.items():
        assert ACTED[ref] == set(table), (ref, set(table) - ACTED[ref])
