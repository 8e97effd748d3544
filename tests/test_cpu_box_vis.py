"""CPU: the box overlays without a GPU -- the side header include/toc3d_boxes.h against the ctypes table that binds it and the library's exports; the refusals of
its three entry points on made-up and on real host pointers (the checks run before any launch); the integer coverage rule against a brute-force float64
point-to-segment distance; corner order and the twelve edges against a hand-computed box; the share of segments the float64 restatement leaves out for a thin
margin; BoxVis.write; and the detector hook's frame counting on recording fakes.  Every test prints the figures it asserts on (run with -s)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import box_vis_cases as BC
import toc3d_amd
import token_vis_cases as TC
from support import A, ERR_ARG, FakeNeck, OldLibrary, header_sigs, raw_call
from toc3d_amd import box_vis as BV
from toc3d_amd import lib, synth

CAM, BEV, RENDER = "toc3d_box_segments", "toc3d_box_segments_bev", "toc3d_segments_render"


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------------------------------------
def test_boxes_header_ctypes_table_and_exports_agree():
    raw = open(lib.BOXES_HEADER_PATH).read()
    txt = lib.header_text(lib.BOXES_HEADER_PATH)
    found = header_sigs(txt, lib._BOXES_SIGS)
    print(f"toc3d_boxes.h declares {found}")
    assert found == lib._BOXES_SIGS and list(found) == [CAM, BEV, RENDER]
    declared = set(re.findall(r"\b(toc3d_\w+)\s*\(", txt))
    assert declared == set(lib._BOXES_SIGS) | {"toc3d_boxes_abi"}, "nothing declared that the table does not bind"
    define = lambda n: int(re.search(rf"#define\s+{n}\s+(\d+)", raw).group(1))
    assert define("TOC3D_BOXES_ABI") == lib.BOXES_ABI == 1
    assert (define("TOC3D_BOXES_CAMERA_EDGES"), define("TOC3D_BOXES_BEV_EDGES")) == (lib.BOXES_CAMERA_EDGES, lib.BOXES_BEV_EDGES) == (12, 5)
    assert (define("TOC3D_BOXES_MAX_SIDE"), define("TOC3D_BOXES_MAX_GUARD"), define("TOC3D_BOXES_MAX_THICKNESS")) == (8192, 16, 15)
    assert (lib.BOXES_MAX_SIDE, lib.BOXES_MAX_GUARD, lib.BOXES_MAX_THICKNESS) == (8192, 16, 15)
    assert (define("TOC3D_BOXES_TILE_W"), define("TOC3D_BOXES_TILE_H")) == (lib.BOXES_TILE_W, lib.BOXES_TILE_H)
    assert "image_vis.py:61-126" in raw and "lidar_box3d.py:50-90" in raw, "the header cites what it serves"
    dll = ctypes.CDLL(lib.LIB_PATH)
    assert all(hasattr(dll, n) for n in declared)
    dll.toc3d_boxes_abi.restype = ctypes.c_int
    assert dll.toc3d_boxes_abi() == 1
    # the other headers know nothing of it, no name is bound twice, and the 11.1 surface stays where it is
    others = (lib.HEADER_PATH, lib.STREAMS_HEADER_PATH, lib.FOCAL_HEADER_PATH, lib.SAMPLED_HEADER_PATH, lib.SELECT_HEADER_PATH, lib.INGEST_HEADER_PATH, lib.VIS_HEADER_PATH)
    for other in others:
        text = open(other).read()
        assert "toc3d_boxes" not in text and not any(n in text for n in lib._BOXES_SIGS)
    tables = (lib._SIGS, lib._STREAMS_SIGS, lib._FOCAL_SIGS, lib._SAMPLED_SIGS, lib._SELECT_SIGS, lib._INGEST_SIGS, lib._VIS_SIGS, lib._BOXES_SIGS)
    names = [n for t in tables for n in t]
    assert len(names) == len(set(names)), "no name is bound twice across the tables"
    assert list(lib._VIS_SIGS) == ["toc3d_token_alpha", "toc3d_token_vis_render"], "toc3d_vis.h keeps its two entry points"
    assert lib.ABI_VERSION == 11 and lib.ABI_MINOR == 1
    main = open(lib.HEADER_PATH).read()
    assert int(re.search(r"#define\s+TOC3D_ABI_VERSION\s+(\d+)", main).group(1)) == 11 and int(re.search(r"#define\s+TOC3D_ABI_MINOR\s+(\d+)", main).group(1)) == 1
    l = lib.load()
    l.toc3d_abi_minor.restype = ctypes.c_int
    assert l.toc3d_abi_version() == 11 and l.toc3d_abi_minor() == 1


def test_exports():
    assert toc3d_amd.BoxVis is BV.BoxVis and "BoxVis" in toc3d_amd.__all__
    assert {"TokenVis", "token_selection_vis", "build_vis_detector"} <= set(toc3d_amd.__all__)
    assert np.array_equal(np.asarray(BV.DEFAULT_PALETTE, dtype=np.uint8), BC.PALETTE) and len(BV.DEFAULT_PALETTE) == 10
    assert BV.DEFAULT_PALETTE[0] == (255, 158, 0) and BV.DEFAULT_PALETTE[5] == (112, 128, 144) and BV.DEFAULT_PALETTE[8] == (0, 0, 230) and BV.DEFAULT_PALETTE[9] == (47, 79, 79)


def cam_args(**o):
    a = dict(boxes=A, box_stride=9, scores=A, labels=A, n=300, thr=0.25, ncol=10, proj=A, V=6, near=0.1, H=320, W=800, guard=16, t=2, segf=A, segi=A, cidx=A)
    a.update(o)
    return tuple(a[k] for k in ("boxes", "box_stride", "scores", "labels", "n", "thr", "ncol", "proj", "V", "near", "H", "W", "guard", "t", "segf", "segi", "cidx")) + (None,)


def bev_args(**o):
    a = dict(boxes=A, box_stride=9, scores=A, labels=A, n=300, thr=0.25, ncol=10, S=640, range_m=51.2, guard=16, t=2, segf=A, segi=A, cidx=A)
    a.update(o)
    return tuple(a[k] for k in ("boxes", "box_stride", "scores", "labels", "n", "thr", "ncol", "S", "range_m", "guard", "t", "segf", "segi", "cidx")) + (None,)


def render_args(**o):
    a = dict(src=A, kind=0, src_stride=0, V=6, H=320, W=800, mean=(103.53, 116.28, 123.675), std=(57.375, 57.12, 58.395), to_rgb=0, bg=(255, 255, 255), segi=A, cidx=A,
             nseg=3600, palette=A, ncol=10, t=2, guard=16, out=A)
    a.update(o)
    return (a["src"], a["kind"], a["src_stride"], a["V"], a["H"], a["W"], *a["mean"], *a["std"], a["to_rgb"], *a["bg"], a["segi"], a["cidx"], a["nseg"], a["palette"],
            a["ncol"], a["t"], a["guard"], a["out"], None)


ARGS = {CAM: cam_args, BEV: bev_args, RENDER: render_args}


def test_call_binds_the_entry_points_and_an_old_library_is_told_to_rebuild(monkeypatch):
    with pytest.raises(RuntimeError, match=r"toc3d_box_segments failed \(-1\): toc3d_box_segments: null buffer"):
        lib.call(CAM, *cam_args(boxes=None))
    for name in lib._BOXES_SIGS:
        assert getattr(lib.load(), name).argtypes == [lib._CT[c] for c in lib._BOXES_SIGS[name]], "bound with the table's argument types"

    monkeypatch.setattr(lib, "_lib", OldLibrary())
    with pytest.raises(RuntimeError, match=r"toc3d_boxes\.h.*rebuild the library"):
        lib.call(RENDER, *render_args())


U8 = dict(kind=1, src_stride=2400)
GEOM_COMMON = [
    *[({p: None}, "null buffer") for p in ("boxes", "scores", "labels", "segf", "segi", "cidx")],
    (dict(n=-1), "must not be negative"), (dict(t=0), "bad thickness"), (dict(t=16), "bad thickness"),
    (dict(guard=0), "bad guard"), (dict(guard=17), "bad guard"), (dict(t=15, guard=7), "bad guard"), (dict(t=3, guard=1), "bad guard"),
    (dict(box_stride=6), "a stride smaller than a row"), (dict(box_stride=-9), "a stride smaller than a row"),
    (dict(ncol=0), "bad num_colors"), (dict(ncol=255), "bad num_colors"),
    ({}, "host pointer"),
]


@pytest.mark.parametrize("name,over,reason", [
    *[(CAM, o, r) for o, r in GEOM_COMMON], *[(BEV, o, r) for o, r in GEOM_COMMON],
    (CAM, dict(proj=None), "null buffer"), *[(CAM, {d: 0}, "must be positive") for d in ("V", "H", "W")], (CAM, dict(H=-3), "must be positive"),
    (CAM, dict(H=8193), "at most 8192"), (CAM, dict(W=8193), "at most 8192"), (CAM, dict(V=65536), "grid"), (CAM, dict(n=1 << 31), "grid"),
    (CAM, dict(V=60000, n=3000), "grid"),
    (BEV, dict(S=0), "must be positive"), (BEV, dict(S=-640), "must be positive"), (BEV, dict(S=8193), "at most 8192"), (BEV, dict(n=1 << 31), "grid"),
    (BEV, dict(range_m=0.0), "bad range_m"), (BEV, dict(range_m=-51.2), "bad range_m"), (BEV, dict(range_m=float("nan")), "bad range_m"),
    (BEV, dict(range_m=float("inf")), "bad range_m"),
    *[(RENDER, {p: None}, "null buffer") for p in ("src", "out", "palette", "segi", "cidx")], (RENDER, dict(U8, src=None), "null buffer"),
    (RENDER, dict(kind=3), "bad src_kind"), (RENDER, dict(kind=-1), "bad src_kind"),
    (RENDER, dict(nseg=-1), "must not be negative"), (RENDER, dict(nseg=(1 << 31) - 256), "below 2^31 - 256"),
    *[(RENDER, {d: 0}, "must be positive") for d in ("V", "H", "W")], (RENDER, dict(W=-800), "must be positive"),
    (RENDER, dict(H=8193), "at most 8192"), (RENDER, dict(W=8193), "at most 8192"), (RENDER, dict(V=65536), "grid"),
    (RENDER, dict(t=0), "bad thickness"), (RENDER, dict(t=16), "bad thickness"), (RENDER, dict(t=-2), "bad thickness"),
    (RENDER, dict(guard=0), "bad guard"), (RENDER, dict(guard=17), "bad guard"), (RENDER, dict(t=15, guard=7), "bad guard"),
    (RENDER, dict(U8, src_stride=2399), "a stride smaller than a row"), (RENDER, dict(U8, src_stride=0), "a stride smaller than a row"),
    (RENDER, dict(src=A + 2), "4-byte boundary"), (RENDER, dict(segi=A + 2), "4-byte boundary"),
    (RENDER, dict(ncol=0), "bad num_colors"), (RENDER, dict(ncol=255), "bad num_colors"),
    (RENDER, dict(kind=2, src=None, bg=(256, 0, 0)), "bad background"), (RENDER, dict(kind=2, src=None, bg=(0, 0, -1)), "bad background"),
    (RENDER, {}, "host pointer"), (RENDER, U8, "host pointer"), (RENDER, dict(kind=2, src=None), "host pointer"),
    (RENDER, dict(nseg=0, segi=None, cidx=None), "host pointer"), (RENDER, dict(t=15, guard=8), "host pointer"), (RENDER, dict(t=1, guard=1), "host pointer"),
])
def test_entry_point_refusals(name, over, reason):
    rc, msg = raw_call(lib._BOXES_SIGS, name, ARGS[name](**over))
    print(f"{name} {over}: rc {rc}, {msg!r}")
    assert rc == ERR_ARG and msg.startswith(name + ":") and reason in msg, (rc, msg)


def test_no_boxes_is_legal_for_the_geometry():
    """n == 0: nothing is launched, no pointer is looked at (none is device memory here), and the call succeeds."""
    for name in (CAM, BEV):
        rc, msg = raw_call(lib._BOXES_SIGS, name, ARGS[name](n=0))
        assert rc == 0, (name, rc, msg)
        rc, msg = raw_call(lib._BOXES_SIGS, name, ARGS[name](n=0, boxes=None, scores=None, labels=None, segf=None, segi=None, cidx=None))
        assert rc == 0, (name, rc, msg)


def test_real_host_buffers_are_refused_and_left_alone():
    """Host memory that could be read and written: every entry point refuses it (not device memory) and touches none of it."""
    p = ctypes.addressof
    boxes = (ctypes.c_float * 18)(*([1.0] * 18))
    scores = (ctypes.c_float * 2)(0.9, 0.8)
    labels = (ctypes.c_int64 * 2)(0, 1)
    proj = (ctypes.c_float * 16)(*([1.0] * 16))
    segf, segi, cidx = (ctypes.c_float * 96)(*([7.0] * 96)), (ctypes.c_int32 * 96)(*([7] * 96)), (ctypes.c_ubyte * 24)(*([9] * 24))
    untouched = lambda: list(segf) == [7.0] * 96 and list(segi) == [7] * 96 and bytes(cidx) == bytes([9] * 24) and list(boxes) == [1.0] * 18
    rc, msg = raw_call(lib._BOXES_SIGS, CAM, cam_args(boxes=p(boxes), scores=p(scores), labels=p(labels), n=2, proj=p(proj), V=1, H=16, W=16, segf=p(segf), segi=p(segi), cidx=p(cidx)))
    print(f"rc {rc}, {msg!r}")
    assert rc == ERR_ARG and "host pointer" in msg and untouched()
    rc, msg = raw_call(lib._BOXES_SIGS, BEV, bev_args(boxes=p(boxes), scores=p(scores), labels=p(labels), n=2, S=16, segf=p(segf), segi=p(segi), cidx=p(cidx)))
    assert rc == ERR_ARG and "host pointer" in msg and untouched()
    src = (ctypes.c_ubyte * 768)(*([7] * 768))
    pal = (ctypes.c_ubyte * 30)(*([5] * 30))
    out = (ctypes.c_ubyte * 768)(*([9] * 768))
    rc, msg = raw_call(lib._BOXES_SIGS, RENDER, render_args(src=p(src), kind=1, src_stride=48, V=1, H=16, W=16, segi=p(segi), cidx=p(cidx), nseg=24, palette=p(pal), out=p(out)))
    print(f"rc {rc}, {msg!r}")
    assert rc == ERR_ARG and "host pointer" in msg and untouched()
    assert bytes(out) == bytes([9] * 768) and bytes(src) == bytes([7] * 768) and bytes(pal) == bytes([5] * 30)


# ---- the coverage rule ------------------------------------------------------------------------------------------------------------------------------------------------
# d has an odd component (or is zero) and t is odd: 4 (p.p) = t^2 has no integer solution (even = odd), and 4 c^2 = t^2 dd needs dd divisible by 4, that is both
# components even -- so no pixel lies ON the threshold, and with |4 c^2 - t^2 dd| >= 1 none lies near it at these sizes
COVER_SEGMENTS = [(7, 6, 7, 6), (3, 9, 24, 9), (12, 2, 12, 21), (4, 4, 21, 15), (26, 3, 5, 18), (-3, -2, 8, 7), (20, 20, 35, 27), (0, 0, 29, 23), (15, 11, 16, 11)]


@pytest.mark.parametrize("t", [1, 3, 5, 15])
def test_integer_coverage_equals_the_float64_distance(t):
    H, W = 24, 30
    worst, total = np.inf, 0
    for seg in COVER_SEGMENTS:
        d = (seg[2] - seg[0], seg[3] - seg[1])
        assert d == (0, 0) or d[0] % 2 or d[1] % 2
        rule = BC.coverage(H, W, seg, t)
        brute, margin = BC.distance_coverage(H, W, seg, t)
        worst, total = min(worst, margin), total + int(rule.sum())
        assert margin > 1e-9, (seg, t, margin)
        assert np.array_equal(rule, brute), (seg, t)
    print(f"t = {t}: {len(COVER_SEGMENTS)} segments on {H} x {W}, {total} covered pixels, every one as the float64 distance says; smallest |distance - t/2| = {worst:.3e}")
    assert total > 0


def test_coverage_at_even_thickness_includes_the_threshold():
    """t = 2: a pixel at distance exactly 1 is covered (<=): a horizontal stroke is three rows high, a dot is a plus of five pixels."""
    line = BC.coverage(9, 12, (2, 4, 9, 4), 2)
    assert line[3:6, 2:10].all() and line.sum() == 3 * 8 + 2, "three rows of eight, and the two cap pixels at distance 1 beyond the ends"
    dot = BC.coverage(5, 5, (2, 2, 2, 2), 2)
    assert dot.sum() == 5 and dot[2, 1:4].all() and dot[1:4, 2].all()
    assert BC.coverage(5, 5, (2, 2, 2, 2), 1).sum() == 1


def test_the_winner_is_the_smallest_drawn_index():
    base = np.zeros((1, 8, 8, 3), dtype=np.uint8)
    segi = np.array([[(1, 3, 6, 3), (3, 1, 3, 6), (1, 3, 6, 3), (3, 1, 3, 6)]])
    out = BC.render_restated(base, segi, np.array([[255, 8, 5, 0]]), BC.PALETTE, 1)
    assert out[0, 3, 3].tolist() == list(BC.PALETTE[8]) and out[0, 3, 1].tolist() == list(BC.PALETTE[5]) and out[0, 1, 3].tolist() == list(BC.PALETTE[8])
    assert BC.coloured(out, base).sum() == 11
    # a segment with an end beyond the guard, and a colour beyond the palette, are not drawn
    out = BC.render_restated(base, np.array([[(-17, 3, 6, 3), (1, 1, 6, 1)]]), np.array([[0, 10]]), BC.PALETTE, 1)
    assert not BC.coloured(out, base).any()


# ---- the geometry -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_corner_order_and_edges_against_a_hand_computed_box():
    """A 4 x 2 x 1 box at (10, 20, -1) turned by 90 degrees: its length lies along +y afterwards.  Corner k of lidar_box3d.py:50-90, by hand."""
    box = np.array([[10.0, 20.0, -1.0, 4.0, 2.0, 1.0, np.pi / 2]])
    got = BC.corners64(box)[0]
    # local (x, y, z) of the offsets: (-2,-1,0) (-2,-1,1) (-2,1,1) (-2,1,0) (2,-1,0) (2,-1,1) (2,1,1) (2,1,0); turned by 90 degrees: (x, y) -> (-y, x)
    want = np.array([(11, 18, -1), (11, 18, 0), (9, 18, 0), (9, 18, -1), (11, 22, -1), (11, 22, 0), (9, 22, 0), (9, 22, -1)], dtype=np.float64)
    print(f"largest difference to the hand-computed corners: {np.abs(got - want).max():.2e}")
    assert np.abs(got - want).max() < 1e-12
    assert BC.EDGES == ((0, 1), (0, 3), (0, 4), (1, 2), (1, 5), (3, 2), (3, 7), (4, 5), (4, 7), (2, 6), (5, 6), (6, 7))
    # the twelve edges are the twelve pairs of corners that differ in one offset: four along each axis, every corner on three of them
    assert sorted(int(np.abs(BC.OFFSETS[a] - BC.OFFSETS[b]).sum()) for a, b in BC.EDGES) == [1] * 12 and len(set(map(frozenset, BC.EDGES))) == 12
    assert np.bincount(np.array(BC.EDGES).reshape(-1)).tolist() == [3] * 8
    lengths = sorted(round(float(np.linalg.norm(got[a] - got[b])), 9) for a, b in BC.EDGES)
    assert lengths == [1.0] * 4 + [2.0] * 4 + [4.0] * 4
    # the top-down footprint (0,3) (3,7) (7,4) (4,0) is the bottom face in order, and edge (4,7) is the front (+x of the box, +y here)
    assert all(int(np.abs(BC.OFFSETS[a] - BC.OFFSETS[b]).sum()) == 1 and BC.OFFSETS[a][2] == BC.OFFSETS[b][2] == 0 for a, b in BC.BEV_EDGES)
    bev = BC.bev_segments64(np.concatenate([box, np.zeros((1, 2))], axis=1), [0.9], [0], 100, range_m=50.0)
    assert np.allclose(bev["segf"][0, 4], (50 - 20, 50 - 10, 50 - 22, 50 - 10)), "the heading stroke: from the centre towards +y, which is left on the panel"
    assert bev["cidx"][0].tolist() == [0] * 5


def test_corners_equal_the_reference_fixture():
    """tests/golden/box_vis_cases.npz: the reference's own LiDARInstance3DBoxes.corners on the boxes of every case (tools/gen_golden_box_vis.py)."""
    z = np.load(BC.FIXTURE)
    worst = total = 0
    for name in ("hand", "random_a", "random_b", "big"):
        boxes = (BC.big_case() if name == "big" else BC.geometry_case(name))["boxes"].astype(np.float64)
        assert np.array_equal(z[f"{name}_boxes"], boxes, equal_nan=True), "the seeded inputs"
        want = z[f"{name}_corners"]
        with np.errstate(all="ignore"):
            got = BC.corners64(boxes)
        ok = np.isfinite(want).all(axis=(1, 2))
        assert np.array_equal(ok, np.isfinite(got).all(axis=(1, 2))) and (ok.all() or name == "hand"), "only the NaN box of the hand case is not finite"
        worst, total = max(worst, float(np.abs(got[ok] - want[ok]).max())), total + int(ok.sum())
    print(f"{total} boxes: the restated corners differ from the reference's by at most {worst:.2e}")
    assert worst < 1e-12 and total == 8 + 8 + 8 + 300


def test_camera_restatement_on_the_hand_case():
    c = BC.geometry_case("hand")
    r = BC.camera_segments64(c["boxes"], c["scores"], c["labels"], c["proj"], c["H"], c["W"])
    drawn = (r["cidx"][0] != 255).sum(axis=1).tolist()
    print(f"view 0 draws {drawn} of each box's twelve edges; view 1 {(r['cidx'][1] != 255).sum(axis=1).tolist()}")
    assert drawn[0] == 12 and drawn[8] == 12 and not r["touched"][0, 0].any(), "fully in view"
    assert 0 < drawn[1] <= 12 and r["touched"][0, 1].any(), "straddles the near plane: clipped, not dropped"
    assert drawn[2] == 0 and drawn[4] == 0 and drawn[5] == 0 and drawn[6] == 0 and drawn[7] == 0, "behind, outside, low score, bad label, NaN"
    assert 0 < drawn[3] < 12 or r["touched"][0, 3].any(), "partly outside the rectangle"
    seg = r["segf"][0][r["cidx"][0] != 255]
    assert (seg[:, [0, 2]] >= -16).all() and (seg[:, [0, 2]] <= c["W"] - 1 + 16).all() and (seg[:, [1, 3]] >= -16).all() and (seg[:, [1, 3]] <= c["H"] - 1 + 16).all()
    assert (r["cidx"][0, 0] == 0).all() and (r["cidx"][0, 8] == 9).all()
    # the near-plane end has depth `near`: the clipped box's pixels stay finite and bounded by the rectangle (mmdet3d's clamp would put them at 1e5 and beyond)
    assert np.isfinite(r["segf"]).all()


THIN = 1.0                                   # a decision whose margin is below its own error bound may go the other way in float32


def test_thin_margins_are_at_most_two_percent():
    total = thin = 0
    for name in BC.GEOMETRY_CASES:
        c = BC.geometry_case(name)
        r = BC.camera_segments64(c["boxes"], c["scores"], c["labels"], c["proj"], c["H"], c["W"])
        b = BC.bev_segments64(c["boxes"], c["scores"], c["labels"], BC.BEV_S, BC.BEV_RANGE)
        total += r["margin"].size + b["margin"].size
        thin += int((r["margin"] <= THIN).sum()) + int((b["margin"] <= THIN).sum())
    big = BC.big_case()
    r = BC.camera_segments64(big["boxes"], big["scores"], big["labels"], big["proj"], big["H"], big["W"])
    thin_big = int((r["margin"] <= THIN).sum())
    print(f"{thin} of {total} segments of the small cases and {thin_big} of {r['margin'].size} of the 300-box case have a decision margin below their error bound")
    assert total > 300 and thin <= 0.02 * total and thin_big <= 0.02 * r["margin"].size


# ---- BoxVis on the host ---------------------------------------------------------------------------------------------------------------------------------------------
def test_write_names_and_channel_order(tmp_path):
    rng = np.random.default_rng(4)
    views, bev = rng.integers(0, 256, (3, 5, 7, 3), dtype=np.uint8), rng.integers(0, 256, (6, 6, 3), dtype=np.uint8)
    views[0, 0, 0] = (255, 0, 1)                                            # red first
    vis = toc3d_amd.BoxVis()
    out = str(tmp_path / "a" / "nested") + "/"
    names = vis.write(dict(views=torch.from_numpy(views), bev=torch.from_numpy(bev)), out)
    assert [os.path.basename(n) for n in names] == ["view0_pred.png", "view1_pred.png", "view2_pred.png", "bev_pred.png"] and sorted(os.listdir(out)) == sorted(map(os.path.basename, names))
    for v in range(3):
        assert np.array_equal(TC.decode_png(open(os.path.join(out, f"view{v}_pred.png"), "rb").read()), views[v]), "stored in array order: red first"
    assert np.array_equal(TC.decode_png(open(os.path.join(out, "bev_pred.png"), "rb").read()), bev)
    assert TC.decode_png(open(os.path.join(out, "view0_pred.png"), "rb").read())[0, 0].tolist() == [255, 0, 1]
    out2 = str(tmp_path / "b") + "/"
    names = vis.write(dict(views=torch.from_numpy(views), bev=None), out2, views=range(1, 3))
    assert [os.path.basename(n) for n in names] == ["view0_pred.png", "view1_pred.png"], "a range of views is numbered from 0; no panel, no file"
    assert np.array_equal(TC.decode_png(open(os.path.join(out2, "view0_pred.png"), "rb").read()), views[1])


def test_constructor_refusals_and_no_cpu_path():
    for kw, what in ((dict(thickness=0), "thickness"), (dict(thickness=16), "thickness"), (dict(thickness=2.5), "thickness"), (dict(bev_size=0), "bev_size"),
                     (dict(bev_size=8193), "bev_size"), (dict(bev_range=0.0), "bev_range"), (dict(palette=[(1, 2)]), "palette"), (dict(palette=[(0, 0, 256)]), "palette"),
                     (dict(palette=[(0, 0, 0)] * 255), "palette"), (dict(bev_background=(0, 0)), "bev_background"), (dict(bev_background=(0, 0, 300)), "bev_background")):
        with pytest.raises(ValueError, match=what):
            toc3d_amd.BoxVis(**kw)
    vis = toc3d_amd.BoxVis()
    assert (vis.score_thr, vis.thickness, vis.near, vis.bev_size, vis.bev_range, vis.bev_background) == (0.25, 2, 0.1, 640, 51.2, (255, 255, 255))
    assert np.array_equal(vis.palette, BC.PALETTE)
    with pytest.raises(RuntimeError, match="only compute path"):
        vis.render(torch.zeros(1, 3, 16, 16), torch.zeros(0, 9), torch.zeros(0), torch.zeros(0, dtype=torch.int64), torch.eye(4)[None])


# ---- the detector: which frames are drawn ------------------------------------------------------------------------------------------------------------------------------
class FakeBackbone(nn.Module):
    pruning_loc, pruning_num_queries, patch_size, img_norm_cfg = [3, 6, 9], 64, 16, None

    def __init__(self, log):
        super().__init__()
        self.log = log

    def forward(self, x, **kw):
        self.log.append(("backbone",))
        return toc3d_amd.ToC3DViTReturnType({"last_feat": torch.zeros(x.shape[0], 8, 2, 5)}, ["m0", "m1", "m2"], None, ["k0", "k1", "k2"], ["d0", "d1", "d2"])


class FakeHead(nn.Module):
    embed_dims = 256

    def __init__(self, log):
        super().__init__()
        self.log = log

    def backbone_queries(self, n, prev_exists, batch_size=1):
        return dict(temp_queries=torch.zeros(batch_size, n, 256), temp_ref_points=None, temp_timestamp=None, temp_ego_pose=None, temp_vel=None, prev_exists=False)

    def img_feats_rows_buffer(self, B, N, h, w, device=None):
        return "rows", 64, lib.F32X3P

    def reset_memory(self):
        pass

    def forward(self, memory_center, img_metas, topk_indexes=None, img_feats_rows=False, **data):
        self.log.append(("head",))
        return dict(all_cls_scores="cls", all_bbox_preds="box", dn_mask_dict=None)

    def get_bboxes(self, outs, img_metas, rescale=False):
        self.log.append(("get_bboxes",))
        return [[torch.full((3, 9), float(i)), torch.arange(3.0) + i, torch.arange(3) + i] for i, _ in enumerate(img_metas)]


class FakeBoxVis:
    """Records what the detector hands to BoxVis."""
    def __init__(self, log):
        self.log = log

    def render(self, img, boxes, scores, labels, lidar2img, cfg):
        self.log.append(("render", tuple(img.shape), float(boxes[0, 0]), float(scores[0]), int(labels[0]), tuple(lidar2img.shape), float(lidar2img[0, 0, 0]), cfg))
        return dict(views="views", bev="bev")

    def write(self, rendered, path, views=None):
        assert rendered == dict(views="views", bev="bev") and views is None
        self.log.append(("write", path))


class FakeTokenVis:
    def __init__(self, log):
        self.log = log

    def render(self, img, masks, keeps, drops, cfg):
        self.log.append(("token_render",))
        return dict(ori=torch.zeros(6, 1, 1, 3))

    def write(self, rendered, path, fix_colors=False, views=None):
        self.log.append(("token_write", path))


def fake_detector(log):
    det = toc3d_amd.build_detector(synth.detector_cfg(synth.DETECTOR_TINY))
    det.img_backbone, det.img_neck, det.pts_bbox_head = FakeBackbone(log), FakeNeck(log), FakeHead(log)
    return det


def frame(det, norm="cfg", **over):
    metas = [dict(scene_token="a", pad_shape=[(32, 80, 3)], img_norm_cfg=norm)]
    data = dict(img=torch.zeros(1, 6, 3, 32, 80), intrinsics=torch.zeros(1, 6, 4, 4), lidar2img=torch.full((1, 6, 4, 4), 2.0), timestamp=torch.zeros(1, dtype=torch.float64),
                ego_pose=torch.eye(4)[None], ego_pose_inv=torch.eye(4)[None])
    data.update(over)
    return det.simple_test(metas, **{k: v for k, v in data.items() if v is not None})


@pytest.mark.parametrize("start,num,drawn,cur_id", [(0, 2, [0, 1], 2), (1, 1, [1], 2), (5, 1, [], 4)])
def test_which_frames_are_drawn(start, num, drawn, cur_id):
    log = []
    det = fake_detector(log)
    assert not det.box_vis and det._box_vis is None
    assert det.enable_box_vis(num_sample=num, start_id=start, out_path="out/boxes", thickness=3, bev_size=128) is det and det.box_vis and det.box_vis_cur_id == 0
    assert isinstance(det._box_vis, toc3d_amd.BoxVis) and det._box_vis.thickness == 3 and det._box_vis.bev_size == 128, "the keywords reach BoxVis"
    det._box_vis = FakeBoxVis(log)
    seen = []
    for f in range(4):
        del log[:]
        out = frame(det)
        names = [e[0] for e in log]
        hit = f in drawn
        assert names == ["backbone", "neck", "head", "get_bboxes"] + (["render", "write"] if hit else []), (f, names)     # from what get_bboxes returned
        if hit:
            assert log[4][1:] == ((6, 3, 32, 80), 0.0, 0.0, 0, (6, 4, 4), 2.0, "cfg") and log[5][1] == f"./out/boxes/{f}/"
            seen.append(f)
        assert list(out[0]) == ["pts_bbox"] and torch.equal(torch.as_tensor(out[0]["pts_bbox"]["scores_3d"]), torch.arange(3.0))
    print(f"(start_id, num_sample) = ({start}, {num}): frames {seen} drawn, counter {det.box_vis_cur_id}, samples left {det.box_vis_num_sample}")
    assert seen == drawn and det.box_vis_cur_id == cur_id and det.box_vis_num_sample == num - len(drawn)
    assert det.cur_id == 0 and not det.token_select_vis, "a counter of its own: the token overlays' is not touched"


def test_disable_streams_both_visualisations_and_the_missing_matrix():
    log = []
    det = fake_detector(log)
    frame(det, lidar2img=None)                                              # not enabled: a frame without lidar2img is nobody's business
    det.enable_box_vis(num_sample=3, out_path="v")
    det._box_vis = FakeBoxVis(log)
    det.disable_box_vis()
    del log[:]
    frame(det)
    assert [e[0] for e in log] == ["backbone", "neck", "head", "get_bboxes"] and det.box_vis_cur_id == 0, "off: nothing drawn, nothing counted"
    det.enable_box_vis(num_sample=3, out_path="v")
    det._box_vis = FakeBoxVis(log)
    with pytest.raises(ValueError, match="no lidar2img"):
        frame(det, lidar2img=None)
    assert det.box_vis_cur_id == 0 and det.box_vis_num_sample == 3
    # two streams in one step: counted once, a sub-directory per stream, each with its own boxes, views, matrices and metas
    for step in range(2):
        del log[:]
        metas = [dict(scene_token="a", pad_shape=[(32, 80, 3)]), dict(scene_token="b", pad_shape=[(32, 80, 3)], img_norm_cfg="other")]
        l2i = torch.stack([torch.full((6, 4, 4), 2.0), torch.full((6, 4, 4), 3.0)])
        out = det.simple_test_streams(metas, img=torch.zeros(2, 6, 3, 32, 80), intrinsics=torch.zeros(2, 6, 4, 4), lidar2img=l2i,
                                      timestamp=torch.zeros(2, dtype=torch.float64), ego_pose=torch.eye(4)[None].repeat(2, 1, 1), ego_pose_inv=torch.eye(4)[None].repeat(2, 1, 1))
        assert len(out) == 2
        evs = [e for e in log if e[0] in ("render", "write")]
        assert [e[0] for e in evs] == ["render", "write", "render", "write"]
        assert evs[0][1:] == ((6, 3, 32, 80), 0.0, 0.0, 0, (6, 4, 4), 2.0, None) and evs[1][1] == f"./v/{step}/stream0/"
        assert evs[2][1:] == ((6, 3, 32, 80), 1.0, 1.0, 1, (6, 4, 4), 3.0, "other") and evs[3][1] == f"./v/{step}/stream1/"
    assert det.box_vis_cur_id == 2 and det.box_vis_num_sample == 1
    # both visualisations at once: each with its own counter and folder
    log2 = []
    both = fake_detector(log2)
    both.enable_token_vis(vis_num_sample=1, vis_start_id=0, vis_out_path="tok").enable_box_vis(num_sample=1, start_id=1, out_path="box")
    both._token_vis, both._box_vis = FakeTokenVis(log2), FakeBoxVis(log2)
    frame(both)
    frame(both)
    assert [e for e in log2 if e[0] in ("token_write", "write")] == [("token_write", "./tok/0/"), ("write", "./box/1/")]
    assert (both.cur_id, both.box_vis_cur_id, both.vis_num_sample, both.box_vis_num_sample) == (1, 2, 0, 0)
