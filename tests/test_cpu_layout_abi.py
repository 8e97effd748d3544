"""CPU: every refusal of the ten staging, layout and packing entry points (toc3d_copy_bytes, toc3d_copy_segments, toc3d_nhwc_to_nchw, toc3d_im2col_patches,
toc3d_im2col_patches_u8, toc3d_normalize_images, toc3d_pack_weight, toc3d_pack_swiglu, toc3d_im2col_3x3, toc3d_conv3x3_nhwc) is reached by a call that violates
only that condition, and names the entry and its reason in toc3d_last_error().  The checks run before any launch, so the device pointers are made-up aligned
addresses that are never dereferenced; only refusing calls, and the empty ones that return before the launch, are made.  (A call that is NOT refused would
launch: without a GPU it returns TOC3D_ERR_LAUNCH, so a missing check fails here.)  mean3 / std3 are host arrays the entries do read: those are real."""
import ctypes

import pytest

from support import A, _call, _refused
from toc3d_amd import lib

I31 = (1 << 31) - 1                          # the largest count the kernels' 32-bit indices hold
F32, BF16 = lib.F32, lib.BF16
MEAN = (ctypes.c_float * 3)(103.53, 116.28, 123.675)
STD = (ctypes.c_float * 3)(57.375, 57.12, 58.395)
STD0 = (ctypes.c_float * 3)(57.375, 0.0, 58.395)


# ---- toc3d_copy_bytes / toc3d_copy_segments ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args", [(A, A + 0x100, -1), (None, A, 16), (A, None, 16)])
def test_copy_bytes_refusals(args):
    _refused("toc3d_copy_bytes", (*args, None), "bad arguments")


def _segs(n, dst, src, nbytes):
    P, L64 = ctypes.c_void_p * max(n, 1), ctypes.c_int64 * max(n, 1)
    return n, P(*dst), P(*src), L64(*nbytes), None


@pytest.mark.parametrize("args", [(-1, A, A, A, None), (17, A, A, A, None), (1, None, A, A, None), (1, A, None, A, None), (1, A, A, None, None)])
def test_copy_segments_refuses_bad_counts_and_null_arrays(args):
    _refused("toc3d_copy_segments", args, "0 <= n <= 16 segments")


@pytest.mark.parametrize("dst,src,nbytes,bad", [
    ([A, A], [A, A], [16, -1], 1), ([None, A], [A, A], [16, 16], 0), ([A, A, A], [A, A, None], [0, 0, 5], 2),
])
def test_copy_segments_refuses_a_bad_segment_and_names_it(dst, src, nbytes, bad):
    _refused("toc3d_copy_segments", _segs(len(dst), dst, src, nbytes), f"bad segment {bad}")


def test_copy_empty_calls_return_before_the_launch():
    assert _call("toc3d_copy_bytes", None, None, 0, None)[0] == 0
    assert _call("toc3d_copy_segments", 0, None, None, None, None)[0] == 0
    assert _call("toc3d_copy_segments", *_segs(3, [None, A, None], [None, None, A], [0, 0, 0]))[0] == 0      # nothing but empty segments (null pointers allowed)


# ---- toc3d_nhwc_to_nchw ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args,reason", [
    ((None, A, 2, 100, 32), "bad arguments"), ((A, None, 2, 100, 32), "bad arguments"), ((A, A, 0, 100, 32), "bad arguments"), ((A, A, 2, 0, 32), "bad arguments"),
    ((A, A, 2, 100, 0), "bad arguments"), ((A, A, -1, 100, 32), "bad arguments"),
    ((A, A, 2, I31 + 1, 32), "too many tokens"), ((A, A, 2, 1 << 40, 32), "too many tokens"), ((A, A, 2, I31 - 30, 32), "too many tokens"),
    ((A, A, 65536, 100, 32), "grid too large"), ((A, A, 2, 100, 65535 * 32 + 1), "grid too large"), ((A, A, 2, 100, I31 + 1), "grid too large"),
    ((A, A, 2, 100, 1 << 62), "grid too large"),
])
def test_nhwc_to_nchw_refusals(args, reason):
    _refused("toc3d_nhwc_to_nchw", (*args, None), reason)


# ---- toc3d_im2col_patches -------------------------------------------------------------------------------------------------------------------------------------------
def _patches(dtype=F32, **o):
    a = dict(img=A, out=A, ldo=768, V=2, Cin=3, H=32, W=48, p=16)
    a.update(o)
    return (dtype, a["img"], a["out"], a["ldo"], a["V"], a["Cin"], a["H"], a["W"], a["p"], None)


@pytest.mark.parametrize("over,reason", [
    (dict(img=None), "null buffer"), (dict(out=None), "null buffer"),
    (dict(V=0), "must be positive"), (dict(V=-1), "must be positive"), (dict(Cin=0), "must be positive"), (dict(Cin=-3, ldo=768), "must be positive"),
    (dict(H=0), "must be positive"), (dict(W=0), "must be positive"), (dict(H=-32), "must be positive"), (dict(W=-48), "must be positive"),
    (dict(p=0), "multiples of patch"), (dict(p=-16), "multiples of patch"), (dict(p=6, H=36, W=48), "multiples of patch"), (dict(H=40), "multiples of patch"),
    (dict(W=40), "multiples of patch"),
    (dict(V=I31 + 1), "dimension too large"), (dict(H=1 << 32, p=4), "dimension too large"), (dict(W=1 << 32, p=4), "dimension too large"),
    (dict(Cin=(I31 >> 8) + 1, ldo=1 << 40), "dimension too large"), (dict(V=I31, Cin=1 << 20, H=1 << 20, W=1 << 20, p=4, ldo=1 << 40), "dimension too large"),
    (dict(ldo=767), "ldo too small"),
    (dict(img=A + 8), "16-byte aligned"),
])
def test_im2col_patches_refusals(over, reason):
    for dt in (F32, BF16):
        _refused("toc3d_im2col_patches", _patches(dt, **over), reason)


def test_im2col_patches_bad_dtype():
    for dt in (lib.F32X3, lib.F32X3P, 99):
        _refused("toc3d_im2col_patches", _patches(dt), "bad dtype")


# ---- toc3d_normalize_images / toc3d_im2col_patches_u8 -----------------------------------------------------------------------------------------------------------------
def _norm(**o):
    a = dict(img=A, V=2, H=33, W=47, mean=MEAN, std=STD, to_rgb=1, out=A, Hp=64, Wp=64)
    a.update(o)
    return (a["img"], a["V"], a["H"], a["W"], a["mean"], a["std"], a["to_rgb"], a["out"], a["Hp"], a["Wp"], None)


@pytest.mark.parametrize("over,reason", [
    (dict(img=None), "null buffer"), (dict(out=None), "null buffer"), (dict(mean=None), "null buffer"), (dict(std=None), "null buffer"),
    (dict(V=0), "bad dims"), (dict(H=0), "bad dims"), (dict(W=-1), "bad dims"), (dict(Hp=32), "bad dims"), (dict(Wp=44), "bad dims"), (dict(Wp=66), "bad dims"),
    (dict(V=I31 + 1), "dimension too large"), (dict(Hp=I31 + 1), "dimension too large"), (dict(Wp=1 << 31), "dimension too large"),
    (dict(H=1 << 31, Hp=1 << 31), "dimension too large"), (dict(W=1 << 31, Wp=1 << 31), "dimension too large"),
    (dict(V=I31, Hp=I31, Wp=I31 - 3), "dimension too large"),
    (dict(out=A + 4), "out must be 16-byte aligned"), (dict(out=A + 8), "out must be 16-byte aligned"),
    (dict(std=STD0), "zero std"),
])
def test_normalize_images_refusals(over, reason):
    _refused("toc3d_normalize_images", _norm(**over), reason)


def _u8(dtype=F32, **o):
    a = dict(img=A, V=2, H=33, W=47, mean=MEAN, std=STD, to_rgb=0, out=A, ldo=768, Hp=48, Wp=48, p=16)
    a.update(o)
    return (dtype, a["img"], a["V"], a["H"], a["W"], a["mean"], a["std"], a["to_rgb"], a["out"], a["ldo"], a["Hp"], a["Wp"], a["p"], None)


@pytest.mark.parametrize("over,reason", [
    (dict(img=None), "null buffer"), (dict(out=None), "null buffer"), (dict(mean=None), "null buffer"), (dict(std=None), "null buffer"),
    (dict(V=0), "bad dims"), (dict(H=0), "bad dims"), (dict(W=0), "bad dims"), (dict(p=0), "bad dims"), (dict(p=6, Hp=48, Wp=48), "bad dims"), (dict(Hp=32), "bad dims"),
    (dict(Wp=32), "bad dims"), (dict(Hp=56), "bad dims"), (dict(Wp=56), "bad dims"),
    (dict(V=I31 + 1), "dimension too large"), (dict(Hp=1 << 32), "dimension too large"), (dict(Wp=1 << 32), "dimension too large"),
    (dict(V=I31, Hp=I31 - 15, Wp=I31 - 15), "dimension too large"),
    (dict(ldo=767), "ldo < 3*patch*patch"),
    (dict(std=STD0), "zero std"),
])
def test_im2col_patches_u8_refusals(over, reason):
    for dt in (F32, BF16):
        _refused("toc3d_im2col_patches_u8", _u8(dt, **over), reason)


def test_im2col_patches_u8_bad_dtype():
    for dt in (lib.F32X3, 99):
        _refused("toc3d_im2col_patches_u8", _u8(dt), "bad dtype")


# ---- toc3d_pack_weight / toc3d_pack_swiglu ------------------------------------------------------------------------------------------------------------------------------
def _pw(dtype=F32, **o):
    a = dict(w=A, N=130, K=70, out=A, Np=256, Kp=128)
    a.update(o)
    return (dtype, a["w"], a["N"], a["K"], a["out"], a["Np"], a["Kp"], None)


@pytest.mark.parametrize("over,reason", [
    (dict(w=None), "bad arguments"), (dict(out=None), "bad arguments"), (dict(Np=128), "bad arguments"), (dict(Kp=64), "bad arguments"), (dict(N=0), "bad arguments"),
    (dict(K=0), "bad arguments"), (dict(N=-1), "bad arguments"), (dict(K=-1), "bad arguments"),
    (dict(Np=I31 + 1), "dimension too large"), (dict(Kp=I31 + 1), "dimension too large"), (dict(N=1 << 31, Np=1 << 31), "dimension too large"),
    (dict(K=1 << 31, Kp=1 << 31), "dimension too large"),
])
def test_pack_weight_refusals(over, reason):
    for dt in (F32, BF16):
        _refused("toc3d_pack_weight", _pw(dt, **over), reason)


def test_pack_weight_bad_dtype():
    for dt in (lib.F32X3, 99):
        _refused("toc3d_pack_weight", _pw(dt), "bad dtype")


def _ps(dtype=F32, **o):
    a = dict(w1=A, w2=A, b1=A, b2=A, Hd=17, K=70, out_w=A, out_b=A, Hp=64, Kp=128)
    a.update(o)
    return (dtype, a["w1"], a["w2"], a["b1"], a["b2"], a["Hd"], a["K"], a["out_w"], a["out_b"], a["Hp"], a["Kp"], None)


@pytest.mark.parametrize("over,reason", [
    *[({p: None}, "null buffer") for p in ("w1", "w2", "b1", "b2", "out_w", "out_b")],
    (dict(Hd=0), "Hd and K must be positive"), (dict(Hd=-1), "Hd and K must be positive"), (dict(K=0), "Hd and K must be positive"), (dict(K=-70), "Hd and K must be positive"),
    (dict(Hd=65), "Hp must be >= Hd and a multiple of 64"), (dict(Hp=96, Hd=17), "Hp must be >= Hd and a multiple of 64"), (dict(Kp=69), "Hp must be >= Hd and a multiple of 64"),
    (dict(Hp=1 << 30), "dimension too large"), (dict(Hd=1 << 30, Hp=1 << 30), "dimension too large"), (dict(Kp=I31 + 1), "dimension too large"),
    (dict(K=1 << 31, Kp=1 << 31), "dimension too large"),
])
def test_pack_swiglu_refusals(over, reason):
    for dt in (F32, BF16):
        _refused("toc3d_pack_swiglu", _ps(dt, **over), reason)


def test_pack_swiglu_bad_dtype():
    for dt in (lib.F32X3, 99):
        _refused("toc3d_pack_swiglu", _ps(dt), "bad dtype")


# ---- toc3d_im2col_3x3 / toc3d_conv3x3_nhwc ------------------------------------------------------------------------------------------------------------------------------
def _i3(dtype=F32, **o):
    a = dict(x=A, out=A, ldo=288, V=2, h=20, w=50, C=32)
    a.update(o)
    return (dtype, a["x"], a["out"], a["ldo"], a["V"], a["h"], a["w"], a["C"], None)


@pytest.mark.parametrize("over,reason", [
    (dict(V=-1), "negative dimension"), (dict(h=-20), "negative dimension"), (dict(w=-50), "negative dimension"), (dict(V=-2, h=-20), "negative dimension"),
    (dict(C=0, ldo=0), "channel count must be positive"), (dict(C=-32, ldo=288), "channel count must be positive"),
    (dict(C=I31 // 9 + 1, ldo=1 << 40), "channel count must be positive"), (dict(C=1 << 61, ldo=1 << 62), "channel count must be positive"),
    (dict(x=None), "bad arguments"), (dict(out=None), "bad arguments"), (dict(ldo=287), "bad arguments"),
    (dict(V=I31 + 1, h=1, w=1), "too many rows"), (dict(V=1 << 16, h=1 << 15, w=1), "too many rows"), (dict(V=3, h=1 << 15, w=1 << 15), "too many rows"),
    (dict(V=1 << 40, h=1 << 40, w=1 << 40), "too many rows"),
])
def test_im2col_3x3_refusals(over, reason):
    for dt in (F32, BF16):
        _refused("toc3d_im2col_3x3", _i3(dt, **over), reason)


def test_im2col_3x3_bad_dtype_and_empty_calls():
    for dt in (lib.F32X3, 99):
        _refused("toc3d_im2col_3x3", _i3(dt), "bad dtype")
    for o in (dict(V=0), dict(h=0), dict(w=0), dict(V=0, h=1 << 40)):            # nothing to do: success, no launch (include/toc3d.h)
        assert _call("toc3d_im2col_3x3", *_i3(**o))[0] == 0
    _refused("toc3d_im2col_3x3", _i3(V=0, x=None), "bad arguments")            # ... but the other checks come first


def _cv(dtype=F32, variant=16, **o):
    a = dict(x=A, C=64, W=A, ldw=576, bias=A, out=A, ldo=128, V=2, h=3, w=5, Cout=128, zeros=A)
    a.update(o)
    return (dtype, variant, a["x"], a["C"], a["W"], a["ldw"], a["bias"], a["out"], a["ldo"], a["V"], a["h"], a["w"], a["Cout"], a["zeros"], None)


@pytest.mark.parametrize("over,reason", [
    *[({p: None}, "toc3d_conv3x3_nhwc: bad arguments") for p in ("x", "W", "out", "zeros")],
    (dict(V=0), "toc3d_conv3x3_nhwc: bad arguments"), (dict(h=0), "toc3d_conv3x3_nhwc: bad arguments"), (dict(w=-1), "toc3d_conv3x3_nhwc: bad arguments"),
    (dict(h=32768), "toc3d_conv3x3_nhwc: bad arguments"), (dict(w=65536), "toc3d_conv3x3_nhwc: bad arguments"),
    (dict(C=96, ldw=864), "toc3d_conv3x3_nhwc: the channel count must be a multiple of 64"),
    (dict(V=(I31 // 15) + 1), "toc3d_conv3x3_nhwc: too many rows"), (dict(V=1 << 50), "toc3d_conv3x3_nhwc: too many rows"),
    (dict(V=2, h=32767, w=65535), "toc3d_conv3x3_nhwc: too many rows"),
    # the rest of the argument checks are toc3d_linear's (the conv is that call with EPI_CONV3X3): reached through this entry, named as toc3d_linear
    (dict(C=0, ldw=0), "toc3d_linear: bad dims"), (dict(C=-64), "toc3d_linear: bad dims"), (dict(Cout=0), "toc3d_linear: bad dims"),
    (dict(ldw=512), "toc3d_linear: leading dims smaller than K"), (dict(ldo=127), "toc3d_linear: ldo < N"), (dict(x=A + 8), "toc3d_linear: A/W must be 16-byte aligned"),
])
def test_conv3x3_nhwc_refusals(over, reason):
    for dt in (F32, BF16, lib.F32X3):
        _refused("toc3d_conv3x3_nhwc", _cv(dt, **over), reason, fn="toc3d_")


def test_conv3x3_nhwc_bad_dtype_and_split_k_variant():
    _refused("toc3d_conv3x3_nhwc", _cv(99), "bad dtype", fn="toc3d_linear")
    _refused("toc3d_conv3x3_nhwc", _cv(lib.F32X3P), "the 3x3 conv gathers f32 activations", fn="toc3d_linear")
    _refused("toc3d_conv3x3_nhwc", _cv(variant=2016), "split-K variant", fn="toc3d_linear")
