"""CPU: the camera ingest without a GPU -- the side header include/toc3d_ingest.h against the ctypes table that binds it and against the library's exports, the
refusals of its entry point on made-up and on real host pointers (the checks run before any launch), tests/golden/ingest_cases.npz (the REAL reference class on
Pillow, tools/gen_golden_ingest.py) against the numpy restatement built from ``resample_tables`` byte for byte, Pillow itself where it imports, the geometry of
the shipped configs, the camera update, and the refusals of the class.  Every test prints the figures it asserts on (run with -s)."""
import ctypes
import json
import re

import numpy as np
import pytest
import torch

import ingest_cases as IC
import toc3d_amd
from support import A, ERR_ARG, OldLibrary, header_sigs, raw_call
from toc3d_amd import lib
from toc3d_amd import preprocess as P

ENTRY = "toc3d_resize_crop_u8"
PTRS = ("src", "dst", "coef_h", "bounds_h", "coef_v", "bounds_v")


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------------------------------------
def test_ingest_header_ctypes_table_and_exports_agree():
    raw = open(lib.INGEST_HEADER_PATH).read()
    found = header_sigs(lib.header_text(lib.INGEST_HEADER_PATH), lib._INGEST_SIGS)
    print(f"toc3d_ingest.h declares {found}")
    assert found == lib._INGEST_SIGS and list(found) == [ENTRY]
    declared = set(re.findall(r"\b(toc3d_\w+)\s*\(", lib.header_text(lib.INGEST_HEADER_PATH)))
    assert declared == set(lib._INGEST_SIGS) | {"toc3d_ingest_abi"}, "nothing declared that the table does not bind"
    assert int(re.search(r"#define\s+TOC3D_INGEST_ABI\s+(\d+)", raw).group(1)) == lib.INGEST_ABI == 1
    defines = {k: int(v) for k, v in re.findall(r"#define\s+TOC3D_INGEST_(TILE_W|TILE_H|LDS_ROWS|MAX_KSIZE)\s+(\d+)", raw)}
    print(f"tile and LDS budget {defines}")
    assert defines == dict(TILE_W=lib.INGEST_TILE_W, TILE_H=lib.INGEST_TILE_H, LDS_ROWS=lib.INGEST_LDS_ROWS, MAX_KSIZE=lib.INGEST_MAX_KSIZE)
    assert "transform_3d.py:108-172" in raw and "Resample.c" in raw, "the header cites what it serves"
    assert re.search(r"every source index is clamped into the image", raw), "the header states the index clamp"
    dll = ctypes.CDLL(lib.LIB_PATH)
    assert all(hasattr(dll, n) for n in declared)
    dll.toc3d_ingest_abi.restype = ctypes.c_int
    assert dll.toc3d_ingest_abi() == 1
    # the other headers know nothing of it, and no name is bound twice
    for other in (lib.HEADER_PATH, lib.STREAMS_HEADER_PATH, lib.FOCAL_HEADER_PATH, lib.SAMPLED_HEADER_PATH, lib.SELECT_HEADER_PATH):
        assert "toc3d_ingest" not in open(other).read() and ENTRY not in open(other).read()
    assert not set(lib._INGEST_SIGS) & (set(lib._SIGS) | set(lib._STREAMS_SIGS) | set(lib._FOCAL_SIGS) | set(lib._SAMPLED_SIGS) | set(lib._SELECT_SIGS))
    assert lib.ABI_VERSION == 11 and lib.ABI_MINOR == 1


def test_exports():
    assert toc3d_amd.ResizeCropFlipRotImage is P.ResizeCropFlipRotImage and toc3d_amd.resample_tables is P.resample_tables
    assert {"ResizeCropFlipRotImage", "resample_tables", "prepare_images"} <= set(toc3d_amd.__all__)


def entry_args(**o):
    a = dict({p: A for p in PTRS}, src_stride=4800, V=6, H0=900, W0=1600, dst_stride=2400, fH=320, fW=800, ksize_h=9, ksize_v=9, max_span=70)
    a.update(o)
    return (a["src"], a["src_stride"], a["V"], a["H0"], a["W0"], a["dst"], a["dst_stride"], a["fH"], a["fW"], a["coef_h"], a["bounds_h"], a["ksize_h"],
            a["coef_v"], a["bounds_v"], a["ksize_v"], a["max_span"], None)


def test_call_binds_the_entry_point_and_an_old_library_is_told_to_rebuild(monkeypatch):
    with pytest.raises(RuntimeError, match=r"toc3d_resize_crop_u8 failed \(-1\): toc3d_resize_crop_u8: null buffer"):
        lib.call(ENTRY, *entry_args(src=None))
    assert getattr(lib.load(), ENTRY).argtypes == [lib._CT[c] for c in lib._INGEST_SIGS[ENTRY]], "bound with the table's argument types (int64 counts, not C ints)"

    monkeypatch.setattr(lib, "_lib", OldLibrary())
    with pytest.raises(RuntimeError, match=r"toc3d_ingest\.h.*rebuild the library"):
        lib.call(ENTRY, *entry_args())


@pytest.mark.parametrize("over,reason", [
    *[({p: None}, "null buffer") for p in PTRS],
    *[({d: 0}, "must be positive") for d in ("V", "H0", "W0", "fH", "fW")], (dict(V=-2), "must be positive"), (dict(fW=-800), "must be positive"),
    (dict(V=65536), "grid"), (dict(W0=1 << 30, src_stride=1 << 40), "31 bits"), (dict(fH=1 << 30), "31 bits"),
    (dict(src_stride=4799), "a stride smaller than a row"), (dict(dst_stride=2399), "a stride smaller than a row"), (dict(src_stride=0), "a stride smaller than a row"),
    (dict(dst_stride=-2400), "a stride smaller than a row"),
    (dict(ksize_h=0), "bad ksize"), (dict(ksize_v=0), "bad ksize"), (dict(ksize_h=lib.INGEST_MAX_KSIZE + 1), "LDS budget"), (dict(ksize_v=33), "LDS budget"),
    (dict(max_span=0), "bad max_span"), (dict(max_span=lib.INGEST_LDS_ROWS + 1), "LDS budget"), (dict(max_span=-5), "bad max_span"),
    ({}, "host pointer"),                     # every other check passed: the made-up pointers are not device memory
])
def test_entry_point_refusals(over, reason):
    rc, msg = raw_call(lib._INGEST_SIGS, ENTRY, entry_args(**over))
    print(f"{over}: rc {rc}, {msg!r}")
    assert rc == ERR_ARG and msg.startswith(ENTRY + ":") and reason in msg, (rc, msg)


def test_real_host_buffers_are_refused_and_left_alone():
    """Host memory that could be read and written: the entry point refuses it (not device memory) and touches none of it."""
    src = (ctypes.c_ubyte * (4 * 16 * 3))(*([7] * 192))
    dst = (ctypes.c_ubyte * (4 * 16 * 3))(*([9] * 192))
    tab = (ctypes.c_int32 * 64)(*([1] * 64))
    p = ctypes.addressof
    args = entry_args(src=p(src), dst=p(dst), src_stride=48, dst_stride=48, V=1, H0=4, W0=16, fH=4, fW=16, coef_h=p(tab), bounds_h=p(tab), ksize_h=1,
                      coef_v=p(tab), bounds_v=p(tab), ksize_v=1, max_span=4)
    rc, msg = raw_call(lib._INGEST_SIGS, ENTRY, args)
    print(f"rc {rc}, {msg!r}")
    assert rc == ERR_ARG and "host pointer" in msg
    assert bytes(dst) == bytes([9] * 192) and bytes(src) == bytes([7] * 192) and list(tab) == [1] * 64


# ---- the tables and the fixture --------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return np.load(IC.FIXTURE)


def test_tables_are_pillows():
    """Hand-checked rows: scale 2 away from the border has 8 taps, the bicubic at +-0.25 ... +-1.75 (source offsets +-0.5 ... +-3.5 times 1 / scale) normalised to 2^22; the border rows are cut and renormalised."""
    coef, bounds, ksize = P.resample_tables(1600, 800)
    print(f"ksize {ksize}, row 400 {coef[400].tolist()} at {bounds[400].tolist()}, row 0 {coef[0].tolist()} at {bounds[0].tolist()}")
    assert ksize == 9 and coef.dtype == bounds.dtype == np.int32 and coef.shape == (800, 9) and bounds.shape == (800, 2)
    assert bounds[400].tolist() == [797, 8] and coef[400, 8] == 0 and coef[400, :8].tolist() == coef[400, 7::-1].tolist(), "symmetric taps around the centre"
    w = [P._bicubic(t) for t in (-1.75, -1.25, -0.75, -0.25, 0.25, 0.75, 1.25, 1.75)]
    assert coef[400, :8].tolist() == [int((0.5 if v >= 0 else -0.5) + v / sum(w) * (1 << 22)) for v in w]
    assert abs(int(coef[400].sum()) - (1 << 22)) <= 4 and bounds[0].tolist() == [0, 5] and bounds[799].tolist() == [1595, 5]
    assert (np.abs(coef.astype(np.int64)).sum(1) * 255 + (1 << 21) < 2 ** 31).all(), "Pillow's int32 accumulator holds every row"
    sub = P.resample_tables(1600, 800, 130, 37)
    assert np.array_equal(sub[0], coef[130:167]) and np.array_equal(sub[1], bounds[130:167]) and sub[2] == 9, "a restricted range is the rows of the full table"
    up = P.resample_tables(64, 100)
    assert up[2] == 5 and int(up[1][:, 1].max()) <= 5
    for bad in ((0, 4, 0, 4), (4, 0, 0, 1), (8, 4, 2, 3), (8, 4, -1, 2), (8, 4, 0, 0)):
        with pytest.raises(ValueError, match="bad axis"):
            P.resample_tables(*bad)


@pytest.mark.parametrize("form", IC.FORMS)
@pytest.mark.parametrize("case", sorted(IC.CASES))
def test_restatement_equals_the_fixture_byte_for_byte(golden, case, form):
    c, tag = IC.CASES[case], f"{case}_{form}_"
    img = IC.frames(case, form)
    assert np.array_equal(img, golden[tag + "input"]), "the seeded input is the recorded one"
    m = P.ResizeCropFlipRotImage(IC.case_conf(case), training=False)
    resize, dims, crop = m.geometry()
    assert resize == float(golden[tag + "resize"]) and dims == tuple(golden[tag + "resize_dims"]) == c["resize_dims"] and crop == tuple(golden[tag + "crop"]) == c["crop"]
    t = m.host_tables()
    assert (t["h"][2], t["v"][2]) == c["ksize"]
    ref = golden[tag + "image"]
    got = IC.restated(img, t)
    # the same through resample_tables on BOTH axes (no one-tap identity for an axis of unchanged size)
    full = dict(h=P.resample_tables(c["W"], dims[0], crop[0], crop[2] - crop[0]), v=P.resample_tables(c["H"], dims[1], crop[1], crop[3] - crop[1]))
    got_full = IC.restated(img, full)
    diff, diff_full = int((got != ref).sum()), int((got_full != ref).sum())
    print(f"case {case} {form}: {img.shape} -> {ref.shape}, ksize {c['ksize']}, differing bytes {diff} (identity form) / {diff_full} (resampling tables on both axes) of {ref.size}; "
          f"output bytes at 0 / 255: {int((ref == 0).sum())} / {int((ref == 255).sum())}")
    assert ref.dtype == np.uint8 and ref.shape == (len(img),) + c["final_dim"] + (3,)
    assert diff == 0 and diff_full == 0
    if form == "stripes" and case == "d":      # upscaled, the bicubic over- and undershoots the 0 / 255 edges (at scale ~0.5 alternating lines average to 128)
        assert (ref[1:] == 0).any() and (ref[1:] == 255).any(), "the stripes reach the clamp at both ends"


@pytest.mark.parametrize("case", sorted(IC.CASES))
def test_restatement_equals_pillow(case):
    Image = pytest.importorskip("PIL.Image")
    m = P.ResizeCropFlipRotImage(IC.case_conf(case), training=False)
    _, dims, crop = m.geometry()
    for form in IC.FORMS:
        img = IC.frames(case, form)
        ref = np.stack([np.array(Image.fromarray(f).resize(dims).crop(crop)) for f in img])
        diff = int((IC.restated(img, m.host_tables()) != ref).sum())
        print(f"case {case} {form}: differing bytes against Pillow {diff}")
        assert diff == 0


@pytest.mark.parametrize("tag", sorted(IC.SCALES))
def test_other_resize_strengths_equal_pillow(tag):
    Image = pytest.importorskip("PIL.Image")
    (H, W), final_dim, ksize = IC.SCALES[tag]
    m = P.ResizeCropFlipRotImage(IC.conf(H, W, final_dim), training=False)
    _, dims, crop = m.geometry()
    t = m.host_tables()
    img = np.random.default_rng(ksize).integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    ref = np.stack([np.array(Image.fromarray(f).resize(dims).crop(crop)) for f in img])
    diff = int((IC.restated(img, t) != ref).sum())
    print(f"{tag}: {H} x {W} -> {final_dim}, resize_dims {dims}, crop {crop}, ksize {t['h'][2]}: differing bytes against Pillow {diff}")
    assert t["h"][2] == ksize and diff == 0


def test_fixture_meta_names_the_pillow_version():
    meta = json.load(open(IC.FIXTURE_META))
    print(meta["pillow"], meta["source"])
    assert re.fullmatch(r"\d+\.\d+(\.\d+)?", meta["pillow"]) and "ResizeCropFlipRotImage" in meta["source"]
    assert {k: tuple(v["final_dim"]) for k, v in meta["cases"].items()} == {k: v["final_dim"] for k, v in IC.CASES.items()}


# ---- the class -------------------------------------------------------------------------------------------------------------------------------------------------------
def test_geometry_of_the_shipped_configs():
    for final_dim, want in (((320, 800), (0.5, (800, 450), (0, 130, 800, 450))), ((800, 1600), (1.0, (1600, 900), (0, 100, 1600, 900)))):
        m = toc3d_amd.ResizeCropFlipRotImage(IC.conf(900, 1600, final_dim), training=False)
        print(final_dim, m.geometry(), m.ida_mat().tolist())
        assert m.geometry() == want
        ida = m.ida_mat()
        assert ida.dtype == torch.float32 and ida.tolist() == [[want[0], 0.0, -want[2][0]], [0.0, want[0], -want[2][1]], [0.0, 0.0, 1.0]]
        t = m.host_tables()
        assert P.tile_span(t["v"][1]) <= lib.INGEST_LDS_ROWS and max(t["h"][2], t["v"][2]) <= lib.INGEST_MAX_KSIZE


@pytest.mark.parametrize("form", IC.FORMS)
@pytest.mark.parametrize("case", sorted(IC.CASES))
def test_update_cameras_matches_the_fixture(golden, case, form):
    tag = f"{case}_{form}_"
    m = toc3d_amd.ResizeCropFlipRotImage(IC.case_conf(case), training=False)
    K, E = IC.cameras(case, form, len(golden[tag + "image"]))
    assert np.array_equal(K, golden[tag + "intrinsics_in"]) and np.array_equal(E, golden[tag + "extrinsics"])
    K0 = K.copy()
    new_k, l2i = m.update_cameras([k for k in K], [e for e in E])
    ida = m.ida_mat().numpy()
    print(f"case {case} {form}: ida_mat {ida.tolist()}, intrinsics {new_k[0].dtype}, lidar2img {l2i[0].dtype}")
    assert np.array_equal(ida, golden[tag + "ida_mat"]) and ida.dtype == golden[tag + "ida_mat"].dtype
    assert np.array_equal(K, K0), "the inputs are not changed"
    for name, got in (("intrinsics_out", np.stack(new_k)), ("lidar2img", np.stack(l2i))):
        ref = golden[tag + name]
        assert got.dtype == ref.dtype and got.shape == ref.shape and np.array_equal(got, ref), (name, float(np.abs(got - ref).max()))


def test_class_refusals():
    conf = IC.conf(900, 1600, (320, 800))
    with pytest.raises(NotImplementedError, match="training=False"):
        toc3d_amd.ResizeCropFlipRotImage(conf)                            # the reference's default is training=True
    with pytest.raises(NotImplementedError, match="training=False"):
        toc3d_amd.ResizeCropFlipRotImage(conf, training=True)
    with pytest.raises(NotImplementedError, match="rot_lim"):
        toc3d_amd.ResizeCropFlipRotImage(dict(conf, rot_lim=(-5.4, 5.4)), training=False)
    with pytest.raises(NotImplementedError, match="data_aug_conf"):
        toc3d_amd.ResizeCropFlipRotImage(None, training=False)
    with pytest.raises(ValueError, match="leaves the resized image"):
        toc3d_amd.ResizeCropFlipRotImage(dict(conf, bot_pct_lim=(0.9, 0.9)), training=False)         # crop_h < 0: Pillow would pad with zeros
    m = toc3d_amd.ResizeCropFlipRotImage(conf, training=False)
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        m(torch.zeros(6, 900, 1600, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        m(np.zeros((6, 900, 1600, 3), dtype=np.uint8))

    class OnDevice(torch.Tensor):             # shape and dtype checks come after the device's: a stand-in that claims to be on the device
        is_cuda = True
    for bad in (torch.zeros(6, 900, 1600, 3), torch.zeros(6, 900, 1600, 4, dtype=torch.uint8), torch.zeros(6, 3, 900, 1600, dtype=torch.uint8),
                torch.zeros(900, 1600, 3, dtype=torch.uint8), torch.zeros(6, 450, 800, 3, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="expected uint8 HWC frames"):
            m(bad.as_subclass(OnDevice))
    # a resize too strong for the kernel's LDS: refused when the tables are made, before any launch
    strong = toc3d_amd.ResizeCropFlipRotImage(IC.conf(3200, 640, (32, 64)), training=False)
    with pytest.raises(ValueError, match="LDS budget"):
        strong._device_tables("cpu")
