"""GPU: toc3d_box_segments, toc3d_box_segments_bev, toc3d_segments_render and toc3d_amd.BoxVis -- the render against the integer restatement of
tests/box_vis_cases.py, byte for byte, over hand-made and random segment tables, five thicknesses, three source forms and the access widths, with guard bytes
around the output; the geometry against the float64 restatement, decisions wherever their margin exceeds their error bound and untouched ends within a bound
counted from the implementation's roundings; the whole path; 6 x 320 x 800 with 300 boxes; the same call twice; and the detector with the visualisation
switched on against one without it, bit for bit, with the files it writes decoded and compared.  Every test prints the figures it asserts on (run with -s)."""
import os

import numpy as np
import pytest
import torch

import box_vis_cases as BC
import detector_cases as DC
import toc3d_amd
import token_vis_cases as TC
from support import DEV, S, guarded, to_dev, touched
from toc3d_amd import lib, synth

pytestmark = pytest.mark.gpu
THIN = 1.0                                   # a decision whose margin is below its own error bound may go the other way in float32
dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- the render, exact -----------------------------------------------------------------------------------------------------------------------------------------------
# (source offset in bytes, source row padding, destination offset).  Everything aligned (the wide forms where W allows); an f32 source 4 bytes off a 16-byte
# boundary / a u8 source at an odd address with rows padded by 5, the destination aligned; source rows padded up to a multiple of 4 (u8 dwords, also where
# W % 4 != 0: the last quad of a row falls back), the destination at an odd address (bytes)
LAYOUTS = ((0, 0, 0), (1, 5, 0), (0, "dword", 1))


def call_render(kind, src, stride, V, H, W, norm, segi, cidx, t, dst_off=0, bg=(0, 0, 0), palette=BC.PALETTE):
    nseg = segi.shape[1]
    obuf, out = guarded(V * H * W * 3, dst_off)
    d_segi, d_cidx = (dv(segi.astype(np.int32)), dv(cidx.astype(np.uint8))) if nseg else (None, None)
    mean, std, to_rgb = (norm["mean"], norm["std"], norm["to_rgb"]) if norm is not None else ([0.0] * 3, [1.0] * 3, False)
    lib.call("toc3d_segments_render", src, kind, stride, V, H, W, *mean, *std, int(to_rgb), *bg, d_segi, d_cidx, nseg, dv(palette), len(palette), t, BC.GUARD, out, S())
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(V, H, W, 3), touched(obuf, V * H * W * 3, dst_off)


def f32_source(img, src_off):
    off = 4 * min(src_off, 1)
    buf = torch.zeros(off + img.size * 4, dtype=torch.uint8, device=DEV)
    buf[off:] = dv(img.reshape(-1).view(np.uint8))
    return buf[off:]


def u8_source(raw, src_off, pad):
    V, H, W, _ = raw.shape
    stride = -(-(3 * W) // 4) * 4 + 4 if pad == "dword" else 3 * W + pad
    buf = torch.full((src_off + V * H * stride,), 0x5A, dtype=torch.uint8, device=DEV)
    rows = buf[src_off:].view(V * H, stride)
    rows[:, :3 * W] = dv(raw.reshape(V * H, 3 * W))
    return buf[src_off:], stride


@pytest.mark.parametrize("t", BC.THICKNESSES)
@pytest.mark.parametrize("name", BC.RENDER_CASES)
def test_render_equals_the_restatement(name, t):
    c = BC.render_case(name)
    H, W, segi, cidx = c["H"], c["W"], c["segi"], c["cidx"]
    assert H % lib.BOXES_TILE_H and W % lib.BOXES_TILE_W and H > lib.BOXES_TILE_H and W > lib.BOXES_TILE_W, "no multiple of the tile, two tiles each way"
    assert (W % 4 == 0) == (name == "w4")
    img, raw = BC.render_sources(H, W, 5400 + len(name))
    total = worst = 0
    for norm in (TC.SHIPPED_NORM, TC.RGB_NORM, None):
        want = BC.render_restated(BC.base_f32(img, norm), segi, cidx, BC.PALETTE, t)
        for layout in LAYOUTS:
            got, g = call_render(0, f32_source(img, layout[0]), 0, 2, H, W, norm, segi, cidx, t, layout[2])
            diff = int((got != want).sum())
            total, worst = total + 1, max(worst, diff)
            assert diff == 0 and g == 0, (name, t, "f32", norm, layout, diff, g)
    want = BC.render_restated(BC.base_u8(raw), segi, cidx, BC.PALETTE, t)
    for layout in LAYOUTS:
        src, stride = u8_source(raw, layout[0], layout[1])
        for norm in (TC.SHIPPED_NORM, TC.RGB_NORM):
            got, g = call_render(1, src, stride, 2, H, W, norm, segi, cidx, t, layout[2])
            diff = int((got != want).sum())
            total, worst = total + 1, max(worst, diff)
            assert diff == 0 and g == 0, (name, t, "u8", layout, diff, g)
    base = np.empty((2, H, W, 3), dtype=np.uint8)
    base[:] = (250, 128, 3)
    want = BC.render_restated(base, segi, cidx, BC.PALETTE, t)
    for dst_off in (0, 1):
        got, g = call_render(2, None, 0, 2, H, W, None, segi, cidx, t, dst_off, bg=(250, 128, 3))
        diff = int((got != want).sum())
        total, worst = total + 1, max(worst, diff)
        assert diff == 0 and g == 0, (name, t, "none", dst_off, diff, g)
    drawn = int(BC.coloured(want, base).sum())
    print(f"{name} {H} x {W}, thickness {t}: {total} renders (f32 / u8 / none, three layouts), at most {worst} bytes differ; {drawn} of {2 * H * W} pixels coloured")
    assert (drawn == 0) == (name == "empty")


def test_render_overlaps_take_the_smaller_index_in_both_orders():
    c = BC.render_case("odd")
    base = np.zeros((2, c["H"], c["W"], 3), dtype=np.uint8)
    got, _ = call_render(2, None, 0, 2, c["H"], c["W"], None, c["segi"], c["cidx"], 1)
    # (24, 20, 40, 20) is there twice, colour 0 then 8, behind a 255 entry; view 1 holds the segments in the other order
    assert got[0, 20, 35].tolist() == list(BC.PALETTE[0]) and got[1, 20, 35].tolist() == list(BC.PALETTE[8])
    assert got[0, 18, 35].tolist() == [0, 0, 0], "a 255 entry draws nothing"
    assert np.array_equal(got, BC.render_restated(base, c["segi"], c["cidx"], BC.PALETTE, 1))


# ---- the geometry, against float64 ----------------------------------------------------------------------------------------------------------------------------------
def call_camera(c, near=BC.NEAR, thr=BC.THR, t=2):
    n, V = len(c["scores"]), c["proj"].shape[0]
    fb, segf = guarded(V * n * 12 * 16)
    ib, segi = guarded(V * n * 12 * 16)
    cb, cidx = guarded(V * n * 12)
    boxes = dv(c["boxes"]) if n else None
    lib.call("toc3d_box_segments", boxes, c["boxes"].shape[1], dv(c["scores"]) if n else None, dv(c["labels"]) if n else None, n, thr, 10, dv(c["proj"]), V, near,
             c["H"], c["W"], BC.GUARD, t, segf, segi, cidx, S())
    torch.cuda.synchronize()
    g = touched(fb, V * n * 192) + touched(ib, V * n * 192) + touched(cb, V * n * 12)
    return (segf.cpu().numpy().view(np.float32).reshape(V, n, 12, 4), segi.cpu().numpy().view(np.int32).reshape(V, n, 12, 4), cidx.cpu().numpy().reshape(V, n, 12), g)


def call_bev(c, size=BC.BEV_S, range_m=BC.BEV_RANGE, thr=BC.THR, t=2):
    n = len(c["scores"])
    fb, segf = guarded(n * 5 * 16)
    ib, segi = guarded(n * 5 * 16)
    cb, cidx = guarded(n * 5)
    lib.call("toc3d_box_segments_bev", dv(c["boxes"]) if n else None, c["boxes"].shape[1], dv(c["scores"]) if n else None, dv(c["labels"]) if n else None, n, thr, 10,
             size, range_m, BC.GUARD, t, segf, segi, cidx, S())
    torch.cuda.synchronize()
    g = touched(fb, n * 80) + touched(ib, n * 80) + touched(cb, n * 5)
    return segf.cpu().numpy().view(np.float32).reshape(n, 5, 4), segi.cpu().numpy().view(np.int32).reshape(n, 5, 4), cidx.cpu().numpy().reshape(n, 5), g


def compare_tables(tag, segf, segi, cidx, ref):
    """The device's tables against the float64 run -> (segments compared for the decision, left out, ends compared, worst fraction of the bound)."""
    assert np.array_equal(segi, np.rint(segf).astype(np.int32)), f"{tag}: segi is rint of the device's own segf"
    off = cidx == 255
    assert (segf[off] == 0).all() and (segi[off] == 0).all(), f"{tag}: a segment that is not drawn has its coordinates written as 0"
    sure = ref["margin"] > THIN
    assert np.array_equal(cidx[sure], ref["cidx"][sure]), f"{tag}: cidx where the margins exceed the bound"
    ends = sure & ~ref["touched"] & (ref["cidx"] != 255)
    frac = 0.0
    if ends.any():
        err, bound = np.abs(segf[ends].astype(np.float64) - ref["segf"][ends]), ref["bound"][ends]
        assert bound.max() < 0.01, f"{tag}: the bound itself is small (largest {bound.max():.2e} pixels)"
        frac = float((err / bound).max())
        assert frac <= 1.0, f"{tag}: an untouched end is {frac:.3f} of its bound away"
    return int(sure.sum()), int((~sure).sum()), int(ends.sum()) * 4, frac


@pytest.mark.parametrize("name", BC.GEOMETRY_CASES)
def test_geometry_against_float64(name):
    """THE BOUND of an end that no clip touched (tests/box_vis_cases.py, U = 2^-24): a corner coordinate is within U (12 r + |c|), r = (|dx| + |dy|) / 2 -- sincosf
    within 2 ulp (4 U each on |lx| + |ly| <= r), two products, a difference and a sum of one rounding each, taken as 12 U r, and U |c| for the last sum; z within
    U |z|.  A row of h is within sum_j |P_ij| dc_j + 4 U sum_j |P_ij c_j| (a product and three sums on every term, fused or not).  A pixel is within
    1.05 (dh_x + |p| dh_z) / h_z + U |p|.  The top-down ends: the corner error times the scale plus 3 U (S / 2 + |c| scale), times 1.05.  Written down before
    the first run, not fitted; the test prints the worst fraction of it."""
    c = BC.geometry_case(name)
    segf, segi, cidx, g = call_camera(c)
    ref = BC.camera_segments64(c["boxes"], c["scores"], c["labels"], c["proj"], c["H"], c["W"])
    cam = compare_tables(f"{name} camera", segf, segi, cidx, ref)
    bsegf, bsegi, bcidx, bg = call_bev(c)
    bref = BC.bev_segments64(c["boxes"], c["scores"], c["labels"], BC.BEV_S, BC.BEV_RANGE)
    bev = compare_tables(f"{name} bev", bsegf, bsegi, bcidx, bref)
    print(f"{name}: camera {cam[0]} decisions equal, {cam[1]} left out, {cam[2]} untouched coordinates, worst {cam[3]:.3f} of the bound; "
          f"bev {bev[0]} / {bev[1]} / {bev[2]} / {bev[3]:.3f}; {g + bg} guard bytes written; drawn {int((cidx != 255).sum())} + {int((bcidx != 255).sum())}")
    assert g == 0 and bg == 0
    assert cam[1] + bev[1] <= 0.02 * max(1, cidx.size + bcidx.size)
    if name == "hand":
        assert cam[2] >= 2 * 12 * 4 and (cidx[0, 2] == 255).all() and (cidx[0, 5:8] == 255).all() and 0 < (cidx[0, 1] != 255).sum()
        kept = segf[cidx != 255]
        assert (kept[:, [0, 2]] >= -16).all() and (kept[:, [0, 2]] <= c["W"] + 15).all() and (kept[:, [1, 3]] >= -16).all() and (kept[:, [1, 3]] <= c["H"] + 15).all()
    if name == "empty":
        assert cidx.size == 0 and bcidx.size == 0


def test_geometry_takes_a_row_stride_and_other_thresholds():
    c = BC.geometry_case("random_a")
    wide = np.full((len(c["scores"]), 13), np.nan, dtype=np.float32)       # rows 13 apart; what lies behind column 6 is not read
    wide[:, :7] = c["boxes"][:, :7]
    a = call_camera(c)
    b = call_camera(dict(c, boxes=wide))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
    ref = BC.camera_segments64(c["boxes"], c["scores"], c["labels"], c["proj"], c["H"], c["W"], thr=0.6, near=1.5)
    segf, segi, cidx, _ = call_camera(c, near=1.5, thr=0.6)
    out = compare_tables("thr 0.6, near 1.5", segf, segi, cidx, ref)
    print(f"a row stride of 13 gives the same tables; at score_thr 0.6 and near 1.5: {out[0]} decisions equal, {out[1]} left out, worst {out[3]:.3f} of the bound")
    assert (cidx[:, c["scores"] < 0.6] == 255).all()


# ---- the whole path ---------------------------------------------------------------------------------------------------------------------------------------------------
def render_class(vis, imgs, c, norm, bev=True):
    r = vis.render(imgs, dv(c["boxes"]), dv(c["scores"]), dv(c["labels"]), dv(c["proj"]), norm, bev=bev)
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()}


def token_vis_ori(imgs, norm):
    """TokenVis.render(...)['ori'] of the same images: masks of zeros on the token grid at patch 16."""
    V = imgs.shape[0]
    H, W = (imgs.shape[1:3] if imgs.dtype == torch.uint8 else imgs.shape[2:4])
    hp, wp = -(-H // 16), -(-W // 16)
    r = toc3d_amd.TokenVis(16).render(imgs, [torch.zeros(V, hp, wp, 1, device=DEV)], None, None, norm)
    return r["ori"].cpu().numpy()


@pytest.mark.parametrize("form,norm", [("f32", "shipped"), ("f32", "rgb"), ("f32", None), ("u8", "shipped"), ("u8", "rgb")])
@pytest.mark.parametrize("name", ["hand", "random_a", "empty"])
def test_whole_path(name, form, norm):
    norm = dict(shipped=TC.SHIPPED_NORM, rgb=TC.RGB_NORM).get(norm)
    c = BC.geometry_case(name)
    H, W = c["H"], c["W"]
    rng = np.random.default_rng(77)
    if form == "u8":
        H, W = H - 2, W - 2                                                 # frames that do not fill the token grid
        c = dict(c, H=H, W=W)
        raw = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
        imgs, base = dv(raw), BC.base_u8(raw)
    else:
        img = rng.uniform(-2.5, 2.8, (2, 3, H, W)).astype(np.float32)
        imgs, base = dv(img), BC.base_f32(img, norm)
    vis = toc3d_amd.BoxVis(bev_size=BC.BEV_S, bev_range=BC.BEV_RANGE, thickness=2)
    r = render_class(vis, imgs, c, norm)
    n = len(c["scores"])
    assert r["views"].shape == (2, H, W, 3) and r["bev"].shape == (BC.BEV_S, BC.BEV_S, 3) and r["segi"].shape == (2, n, 12, 4) and r["bev_cidx"].shape == (n, 5)
    # (a) the pixels are the restatement's of the device's own tables
    want = BC.render_restated(base, r["segi"].reshape(2, -1, 4), r["cidx"].reshape(2, -1), BC.PALETTE, 2)
    white = np.full((1, BC.BEV_S, BC.BEV_S, 3), 255, dtype=np.uint8)
    want_bev = BC.render_restated(white, r["bev_segi"].reshape(1, -1, 4), r["bev_cidx"].reshape(1, -1), BC.PALETTE, 2)
    diff = int((r["views"] != want).sum()) + int((r["bev"] != want_bev[0]).sum())
    # (b) against the all-float64 pipeline: every pixel one coloured and the other did not lies within one pixel of a pixel the other coloured
    ref = BC.camera_segments64(c["boxes"], c["scores"], c["labels"], c["proj"], H, W)
    bref = BC.bev_segments64(c["boxes"], c["scores"], c["labels"], BC.BEV_S, BC.BEV_RANGE)
    want64 = BC.render_restated(base, np.rint(ref["segf"]).reshape(2, -1, 4), ref["cidx"].reshape(2, -1), BC.PALETTE, 2)
    bev64 = BC.render_restated(white, np.rint(bref["segf"]).reshape(1, -1, 4), bref["cidx"].reshape(1, -1), BC.PALETTE, 2)
    far = BC.within_one_pixel(BC.coloured(r["views"], base), BC.coloured(want64, base)) + BC.within_one_pixel(BC.coloured(r["bev"][None], white), BC.coloured(bev64, white))
    # (c) the base is TokenVis's ori: channel-reversed when to_rgb is false, cropped to the frame for u8
    ori = token_vis_ori(imgs, norm)[:, :H, :W]
    to_rgb = norm is not None and norm["to_rgb"]
    ori = ori if to_rgb else ori[..., ::-1]
    plain = render_class(vis, imgs, BC.geometry_case("empty"), norm, bev=False)
    base_diff = int((plain["views"] != ori).sum()) + int((base != ori).sum())
    blank = ~BC.coloured(want, base)
    print(f"{name} {form} {'no norm' if norm is None else 'to_rgb ' + str(to_rgb)}: {diff} bytes differ from the restatement on the device's tables; "
          f"{int(BC.coloured(want, base).sum())} + {int(BC.coloured(want_bev, white).sum())} pixels coloured, {far} further than one pixel from the float64 pipeline's; "
          f"base against TokenVis ori: {base_diff} bytes")
    assert diff == 0 and far == 0 and base_diff == 0 and plain["bev"] is None
    assert np.array_equal(r["views"][blank], ori[blank]), "an uncovered pixel keeps its base byte"
    if name != "empty":
        assert BC.coloured(want, base).sum() > 100 and BC.coloured(want_bev, white).sum() > 100


# ---- size and repeatability ----------------------------------------------------------------------------------------------------------------------------------------
def test_six_views_at_the_shipped_size_and_the_same_call_twice():
    c = BC.big_case()
    vis = toc3d_amd.BoxVis()
    img = dv(c["img"])
    r = render_class(vis, img, c, TC.SHIPPED_NORM)
    assert r["views"].shape == (6, 320, 800, 3) and r["bev"].shape == (640, 640, 3) and r["segi"].shape == (6, 300, 12, 4)
    base = BC.base_f32(c["img"], TC.SHIPPED_NORM)
    want = BC.render_restated(base, r["segi"].reshape(6, -1, 4), r["cidx"].reshape(6, -1), BC.PALETTE, 2)
    white = np.full((1, 640, 640, 3), 255, dtype=np.uint8)
    want_bev = BC.render_restated(white, r["bev_segi"].reshape(1, -1, 4), r["bev_cidx"].reshape(1, -1), BC.PALETTE, 2)
    diff = int((r["views"] != want).sum()) + int((r["bev"] != want_bev[0]).sum())
    drawn = int((r["cidx"] != 255).sum())
    print(f"6 x 320 x 800, 300 boxes: {drawn} of {r['cidx'].size} camera segments and {int((r['bev_cidx'] != 255).sum())} top-down ones drawn, "
          f"{int(BC.coloured(want, base).sum())} pixels coloured; {diff} bytes differ from the restatement on the device's tables")
    assert diff == 0 and drawn > 1000
    ptr = vis.render(img, dv(c["boxes"]), dv(c["scores"]), dv(c["labels"]), dv(c["proj"]), TC.SHIPPED_NORM)["views"].data_ptr()
    again = render_class(vis, img, c, TC.SHIPPED_NORM)
    assert vis.render(img, dv(c["boxes"]), dv(c["scores"]), dv(c["labels"]), dv(c["proj"]), TC.SHIPPED_NORM)["views"].data_ptr() == ptr, "the per-shape workspace is reused"
    assert all(np.array_equal(r[k], again[k]) for k in ("views", "bev", "segi", "cidx", "bev_segi", "bev_cidx")) and np.array_equal(r["segf"].view(np.int32), again["segf"].view(np.int32))
    # lidar2img as the frame carries it: (1, V, 4, 4), float64, on the host; boxes as an object with .tensor
    class Boxes:
        tensor = dv(c["boxes"])
    other = vis.render(img[None], Boxes(), dv(c["scores"]), dv(c["labels"]), torch.from_numpy(c["proj"].astype(np.float64))[None], TC.SHIPPED_NORM)
    assert np.array_equal(other["views"].cpu().numpy(), r["views"]) and np.array_equal(other["bev"].cpu().numpy(), r["bev"])


# ---- the detector ------------------------------------------------------------------------------------------------------------------------------------------------
TINY = synth.DETECTOR_TINY
run, assert_same_bits = DC.run, DC.assert_same_bits


def build_detector(precision, norm=None):
    return DC.build_detector(TINY, precision, norm=norm)


def check_files(folder, img, dec, l2i, norm, V=6):
    """The files under ``folder`` decode to what an independent BoxVis makes of the frame's decoded lists -> (files, boxes, pixels coloured)."""
    assert sorted(os.listdir(folder)) == sorted([f"view{v}_pred.png" for v in range(V)] + ["bev_pred.png"])
    boxes = getattr(dec["boxes_3d"], "tensor", dec["boxes_3d"])
    r = toc3d_amd.BoxVis(score_thr=0.0).render(img, torch.as_tensor(boxes).to(DEV), torch.as_tensor(dec["scores_3d"]).to(DEV), torch.as_tensor(dec["labels_3d"]).to(DEV), l2i, norm)
    views, bev = r["views"].cpu().numpy(), r["bev"].cpu().numpy()
    for v in range(V):
        assert np.array_equal(TC.decode_png(open(os.path.join(folder, f"view{v}_pred.png"), "rb").read()), views[v]), f"view {v}"
    assert np.array_equal(TC.decode_png(open(os.path.join(folder, "bev_pred.png"), "rb").read()), bev)
    white = np.full_like(bev, 255)
    return V + 1, int(boxes.shape[0]), int((r["cidx"] != 255).sum().item()), int(BC.coloured(bev[None], white[None]).sum())


@pytest.mark.parametrize("precision", ["fp32x3", "bf16"])
def test_detector_keeps_its_bits_and_writes_frame_one(tmp_path, monkeypatch, precision):
    monkeypatch.chdir(tmp_path)
    frames = []
    for fr in synth.detector_inputs(TINY)[:3]:
        metas = [dict(fr["img_metas"][0], img_norm_cfg=TC.SHIPPED_NORM)]
        frames.append(dict(img_metas=metas, gumbel=fr["gumbel"], dev=to_dev(fr)))
    plain = run(build_detector(precision), frames)
    assert not os.path.exists(tmp_path / "box_vis"), "off: nothing is written"
    det = build_detector(precision).enable_box_vis(num_sample=1, start_id=1, out_path="box_vis", score_thr=0.0)
    got = run(det, frames)
    assert_same_bits(got, plain)
    assert det.box_vis_cur_id == 2 and det.box_vis_num_sample == 0 and sorted(os.listdir(tmp_path / "box_vis")) == ["1"], "exactly the directory of frame 1"
    files, n, drawn, bev_px = check_files(tmp_path / "box_vis" / "1", frames[1]["dev"]["img"][0], plain[1][0]["dec"], frames[1]["dev"]["lidar2img"], TC.SHIPPED_NORM)
    print(f"{precision}: three frames equal a detector without the visualisation bit for bit; {files} files of frame 1 decode to an independent render of its {n} "
          f"decoded boxes ({drawn} camera segments drawn, {bev_px} top-down pixels coloured)")
    assert n > 0 and bev_px > 0


def test_detector_on_uint8_frames_with_both_visualisations(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(21)
    frames = []
    for fr in synth.detector_inputs(TINY)[:3]:
        dev = to_dev(fr)
        dev["img"] = torch.from_numpy(rng.integers(0, 256, (1, 6, 318, 796, 3), dtype=np.uint8)).to(DEV)
        frames.append(dict(img_metas=fr["img_metas"], gumbel=fr["gumbel"], dev=dev))                       # no img_norm_cfg in the metas: the backbone's is taken
    norm = dict(TC.RGB_NORM)
    plain = run(build_detector("fp32x3", norm), frames)
    det = build_detector("fp32x3", norm).enable_box_vis(num_sample=1, start_id=1, out_path="box_vis", score_thr=0.0).enable_token_vis(1, 0, "token_vis")
    got = run(det, frames)
    assert_same_bits(got, plain)
    assert sorted(os.listdir(tmp_path / "token_vis")) == ["0"] and sorted(os.listdir(tmp_path / "box_vis")) == ["1"], "each with its own counter"
    files, n, drawn, bev_px = check_files(tmp_path / "box_vis" / "1", frames[1]["dev"]["img"][0], plain[1][0]["dec"], frames[1]["dev"]["lidar2img"], norm)
    view = TC.decode_png(open(tmp_path / "box_vis" / "1" / "view0_pred.png", "rb").read())
    raw = frames[1]["dev"]["img"][0, 0].cpu().numpy()
    same = (view == raw[..., ::-1]).all(axis=-1)
    print(f"uint8 frames 318 x 796: {files} files, {n} boxes, {drawn} camera segments drawn; {int((~same).sum())} pixels of view 0 are not the frame's own")
    assert view.shape == (318, 796, 3) and same.mean() > 0.5, "cropped to the frame; red first: the raw frame's channels reversed"


def test_detector_streams_step(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    steps, _ = synth.detector_stream_steps(TINY, seeds=(0, 1), new_scene_at=(3, 2))
    frames = [dict(img_metas=[dict(m, img_norm_cfg=TC.SHIPPED_NORM) for m in st["img_metas"]], gumbel=st["gumbel"], dev=to_dev(st)) for st in steps[:1]]
    plain = run(build_detector("fp32x3"), frames, streams=True)
    det = build_detector("fp32x3").enable_box_vis(num_sample=1, start_id=0, out_path="box_vis", score_thr=0.0)
    got = run(det, frames, streams=True)
    assert_same_bits(got, plain)
    assert sorted(os.listdir(tmp_path / "box_vis" / "0")) == ["stream0", "stream1"] and det.box_vis_cur_id == 1
    for b in range(2):
        files, n, drawn, bev_px = check_files(tmp_path / "box_vis" / "0" / f"stream{b}", frames[0]["dev"]["img"][b], plain[0][b]["dec"], frames[0]["dev"]["lidar2img"][b],
                                              TC.SHIPPED_NORM)
        print(f"stream {b}: {files} files decode to an independent render of its {n} decoded boxes ({drawn} camera segments drawn)")
        assert n > 0
