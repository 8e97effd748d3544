"""GPU: toc3d_resize_crop_u8 and toc3d_amd.ResizeCropFlipRotImage against Pillow's bytes -- every case of tests/golden/ingest_cases.npz (the REAL reference
class) byte for byte, with guard bytes around the destination, destination rows wider than the image (4-byte and byte store forms) and the source pointer off by
1 and by 3 bytes; 6 x 900 x 1600 frames to both shipped sizes against the numpy restatement (tests/ingest_cases.py; tests/test_cpu_ingest.py holds it to Pillow);
tables with out-of-range entries against the clamps the header states; the same call twice; and a tiny-config backbone frame fed the ingest's output against the
same frame fed the restatement's bytes.  The bar everywhere is zero differing bytes.  Every test prints the figures it asserts on (run with -s)."""
import numpy as np
import pytest
import torch

import ingest_cases as IC
import toc3d_amd
from support import DEV, S
from toc3d_amd import configs, lib, synth
from toc3d_amd import preprocess as P

pytestmark = pytest.mark.gpu
GUARD, FILL = 256, 0xA5


@pytest.fixture(scope="module")
def golden():
    return np.load(IC.FIXTURE)


@pytest.fixture(scope="module")
def big():
    """The 6 x 900 x 1600 frames and their restated outputs at both shipped sizes, computed once."""
    img = IC.big_frames()
    return img, {tag: IC.restated_case(IC.conf(900, 1600, fd), img) for tag, fd in IC.BIG.items()}


def dev_tables(t):
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    (ch, bh, kh), (cv, bv, kv) = t["h"], t["v"]
    return dv(ch), dv(bh), kh, dv(cv), dv(bv), kv


def run_entry(img, tables, fH, fW, src_off=0, dst_off=0, dst_pad=0, max_span=None):
    """The entry point on a source that starts ``src_off`` bytes into its buffer and a destination that starts ``dst_off`` bytes behind a 256-byte guard, with
    rows ``dst_pad`` bytes wider than the image.  -> (output (V, fH, fW, 3), number of guard / padding bytes that changed)."""
    V, H0, W0, _ = img.shape
    src = torch.full((src_off + img.size,), 0x5A, dtype=torch.uint8, device=DEV)
    src[src_off:] = torch.from_numpy(img.reshape(-1)).to(DEV)
    stride = fW * 3 + dst_pad
    body = V * fH * stride
    dst = torch.full((GUARD + dst_off + body + GUARD,), FILL, dtype=torch.uint8, device=DEV)
    ch, bh, kh, cv, bv, kv = dev_tables(tables)
    span = P.tile_span(tables["v"][1]) if max_span is None else max_span
    lib.call("toc3d_resize_crop_u8", src[src_off:], W0 * 3, V, H0, W0, dst[GUARD + dst_off:], stride, fH, fW, ch, bh, kh, cv, bv, kv, span, S())
    torch.cuda.synchronize()
    host = dst.cpu().numpy()
    rows = host[GUARD + dst_off:GUARD + dst_off + body].reshape(V, fH, stride)
    touched = int((host[:GUARD + dst_off] != FILL).sum() + (host[GUARD + dst_off + body:] != FILL).sum() + (rows[:, :, fW * 3:] != FILL).sum())
    return rows[:, :, :fW * 3].reshape(V, fH, fW, 3), touched


# (source offset, destination offset, row padding): contiguous; 4-byte stores into padded rows, source off by 1; byte stores (odd start and stride), source off by 3
LAYOUTS = ((0, 0, 0), (1, 0, 8), (3, 1, 5), (0, 0, 4), (1, 4, 3))


@pytest.mark.parametrize("form", IC.FORMS)
@pytest.mark.parametrize("case", sorted(IC.CASES))
def test_fixture_cases_byte_for_byte(golden, case, form):
    tag = f"{case}_{form}_"
    img, ref = IC.frames(case, form), golden[tag + "image"]
    m = toc3d_amd.ResizeCropFlipRotImage(IC.case_conf(case), training=False)
    fH, fW = IC.CASES[case]["final_dim"]
    t = m.host_tables()
    for src_off, dst_off, dst_pad in LAYOUTS:
        got, touched = run_entry(img, t, fH, fW, src_off, dst_off, dst_pad)
        diff = int((got != ref).sum())
        wide = (dst_off % 4 == 0) and ((fW * 3 + dst_pad) % 4 == 0)
        print(f"case {case} {form}: source +{src_off}, destination +{dst_off}, rows +{dst_pad} ({'4-byte' if wide else 'byte'} stores): {diff} of {ref.size} bytes differ, "
              f"{touched} guard or padding bytes written")
        assert diff == 0 and touched == 0
    # resampling tables on both axes (no one-tap identity) give the same bytes
    c = IC.CASES[case]
    full = dict(h=P.resample_tables(c["W"], c["resize_dims"][0], c["crop"][0], fW), v=P.resample_tables(c["H"], c["resize_dims"][1], c["crop"][1], fH))
    got, touched = run_entry(img, full, fH, fW, 0, 0, 4)
    assert int((got != ref).sum()) == 0 and touched == 0
    # the class, on the contiguous tensor: 4-D and 5-D, the workspace and out=
    x = torch.from_numpy(img).to(DEV)
    y = m(x)
    assert y.dtype == torch.uint8 and tuple(y.shape) == ref.shape and np.array_equal(y.cpu().numpy(), ref)
    y5 = m(x[None])
    assert tuple(y5.shape) == (1,) + ref.shape and np.array_equal(y5[0].cpu().numpy(), ref)
    assert m(x).data_ptr() == y.data_ptr(), "the per-shape workspace is reused"
    out = torch.full(ref.shape, FILL, dtype=torch.uint8, device=DEV)
    assert m(x, out=out) is out and np.array_equal(out.cpu().numpy(), ref)
    with pytest.raises(ValueError, match="out= must be"):
        m(x, out=out[..., :2])


@pytest.mark.parametrize("tag", sorted(IC.BIG))
def test_six_camera_frames_to_the_shipped_sizes(big, tag):
    img, refs = big
    ref = refs[tag]
    fH, fW = IC.BIG[tag]
    m = toc3d_amd.ResizeCropFlipRotImage(IC.conf(900, 1600, (fH, fW)), training=False)
    x = torch.from_numpy(img).to(DEV)
    got = m(x.view(1, 6, 900, 1600, 3)).cpu().numpy()[0]
    diff = int((got != ref).sum())
    print(f"6 x 900 x 1600 -> {fH} x {fW}: {diff} of {ref.size} bytes differ; restated bytes at 0 / 255: {int((ref == 0).sum())} / {int((ref == 255).sum())}; "
          f"tile span {P.tile_span(m.host_tables()['v'][1])} rows")
    assert ref.shape == (6, fH, fW, 3) and diff == 0
    assert (ref[3] == 0).any() and (ref[3] == 255).any(), "the checkerboard view reaches the clamp at both ends"
    # guards and padded rows at this size, byte stores from a source off by 3
    got, touched = run_entry(img, m.host_tables(), fH, fW, 3, 1, 7)
    assert int((got != ref).sum()) == 0 and touched == 0


@pytest.mark.parametrize("tag", sorted(IC.SCALES))
def test_other_resize_strengths(tag):
    """ksize 7 and 11 (4-byte source forms of their own), 13 (none: bytes), and a 9-tap case two tiles wide whose second tile is partial."""
    (H, W), (fH, fW), ksize = IC.SCALES[tag]
    m = toc3d_amd.ResizeCropFlipRotImage(IC.conf(H, W, (fH, fW)), training=False)
    t = m.host_tables()
    assert t["h"][2] == ksize
    img = np.random.default_rng(ksize).integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    img[1, :, (np.arange(W) // 3) % 2 == 0] = 0
    img[1, :, (np.arange(W) // 3) % 2 == 1] = 255
    ref = IC.restated(img, t)
    for layout in LAYOUTS:
        got, touched = run_entry(img, t, fH, fW, *layout)
        diff = int((got != ref).sum())
        print(f"{tag}: {H} x {W} -> {fH} x {fW}, ksize {ksize}, layout {layout}: {diff} of {ref.size} bytes differ, {touched} guard or padding bytes written")
        assert diff == 0 and touched == 0


def test_the_same_call_twice_gives_the_same_bytes(big):
    img, refs = big
    m = toc3d_amd.ResizeCropFlipRotImage(IC.conf(900, 1600, (320, 800)), training=False)
    x = torch.from_numpy(img).to(DEV)
    a = m(x).clone()
    b = m(x)
    assert torch.equal(a, b) and np.array_equal(b.cpu().numpy(), refs["320x800"])


def clamped_reference(img, tables, max_span):
    """The header's INDEX RANGE paragraph as code, for an output smaller than one tile: first indices clamped into the image, tap counts into [0, ksize] and,
    along a row, to the taps that lie in the image; intermediate rows into the rows the workgroup holds."""
    (ch, bh, kh), (cv, bv, kv) = tables["h"], tables["v"]
    V, H0, W0, _ = img.shape
    cl = lambda v, lo, hi: max(lo, min(hi, int(v)))
    r0 = cl(bv[0, 0], 0, H0 - 1)
    nrows = cl(cl(bv[-1, 0], 0, H0 - 1) + cl(bv[-1, 1], 0, kv) - r0, 1, min(max_span, H0 - r0))
    out = np.zeros((V, len(bv), len(bh), 3), dtype=np.uint8)
    for v in range(V):
        inter = np.zeros((nrows, len(bh), 3), dtype=np.int64)
        for x in range(len(bh)):
            xmin = cl(bh[x, 0], 0, W0 - 1)
            cnt = cl(bh[x, 1], 0, min(kh, W0 - xmin))                       # taps beyond the image are dropped
            acc = np.full((nrows, 3), 1 << 21, dtype=np.int64)
            for t in range(cnt):
                acc += img[v, r0:r0 + nrows, xmin + t].astype(np.int64) * int(ch[x, t])
            inter[:, x] = np.clip(acc >> 22, 0, 255)
        for y in range(len(bv)):
            ymin, cnt = cl(bv[y, 0], 0, H0 - 1) - r0, cl(bv[y, 1], 0, kv)
            acc = np.full((len(bh), 3), 1 << 21, dtype=np.int64)
            for t in range(cnt):
                acc += inter[cl(ymin + t, 0, nrows - 1)] * int(cv[y, t])
            out[v, y] = np.clip(acc >> 22, 0, 255)
    return out


def test_out_of_range_table_entries_are_clamped():
    """First indices before and beyond the image, tap counts negative and above ksize, a max_span smaller than the taps span: the bytes the clamps define, and
    nothing written outside the destination rows."""
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (2, 20, 24, 3), dtype=np.uint8)
    ch, bh, kh = P.resample_tables(24, 12)
    cv, bv, kv = P.resample_tables(20, 10)
    bh, bv = bh.copy(), bv.copy()
    bh[0], bh[3], bh[7], bh[11] = (-50, 9), (10 ** 9, 5), (4, 1000), (20, -3)
    bv[2], bv[5], bv[9] = (-7, 9), (2 * 10 ** 9, 9), (17, 50)
    t = dict(h=(ch, bh, kh), v=(cv, bv, kv))
    for span in (lib.INGEST_LDS_ROWS, 20, 6):
        ref = clamped_reference(img, t, span)
        for layout in ((0, 0, 0), (1, 1, 3)):                               # the 4-byte source form (24 * 3 bytes a row, ksize 9) and the byte form
            got, touched = run_entry(img, t, 10, 12, *layout, max_span=span)
            diff = int((got != ref).sum())
            print(f"max_span {span}, layout {layout}: {diff} of {ref.size} bytes differ, {touched} guard or padding bytes written")
            assert diff == 0 and touched == 0


def test_backbone_frame_on_the_ingest_output_equals_the_restated_bytes(big):
    """Raw frames -> ingest -> a backbone built with img_norm_cfg (uint8 straight into the patch-embedding im2col), against the same backbone fed the
    restatement's bytes: the same features and kept sets, bit for bit."""
    img, refs = big
    norm = dict(mean=[103.530, 116.280, 123.675], std=[57.375, 57.120, 58.395], to_rgb=False)
    cfg = configs.get("toc3d_tiny")
    bb = toc3d_amd.build_backbone(dict(cfg, precision="fp32", img_norm_cfg=norm))
    bb.load_state_dict(synth.make_state_dict(cfg), strict=True)
    bb = bb.to(DEV).eval()
    inp = synth.make_inputs(cfg, views_per_frame=2)
    d = lambda t: t.to(DEV)

    def frame(x):
        o = bb(x, temp_queries=d(inp["temp_queries"]), prev_exists=True, temp_ref_points=d(inp["temp_ref_points"]), temp_vel=d(inp["temp_vel"]),
               temp_timestamp=d(inp["temp_timestamp"]), temp_ego_pose=d(inp["temp_ego_pose"]), ego_pose_inv=d(inp["ego_pose_inv"]), gumbel_noise=inp["gumbel"])
        return o.img_feats["last_feat"].clone(), [k.clone() for k in o.keep_idx]

    ingest = toc3d_amd.ResizeCropFlipRotImage(IC.conf(900, 1600, (320, 800)), training=False)
    views = (0, 3)                                                         # a natural view and the checkerboard
    fa, ka = frame(ingest(torch.from_numpy(img[list(views)]).to(DEV)))
    fb, kb = frame(torch.from_numpy(refs["320x800"][list(views)]).to(DEV))
    print(f"features {tuple(fa.shape)}, max |difference| {float((fa - fb).abs().max())}")
    assert tuple(fa.shape) == (2, cfg["embed_dim"], 20, 50) and torch.equal(fa, fb)
    assert all(torch.equal(a, b) for a, b in zip(ka, kb))
