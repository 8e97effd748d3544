"""CPU: the token selection overlays without a GPU -- the side header include/toc3d_vis.h against the ctypes table that binds it and the library's exports, the
refusals of its two entry points on made-up and on real host pointers (the checks run before any launch), tests/golden/token_vis_cases.npz (the REAL reference
function on a stand-in mmcv, tools/gen_golden_token_vis.py) against the numpy restatement value for value, the alpha and padding bytes, the set of pixel values
on which a fused multiply-add would round differently, the PNG writer through a decoder of the test's own (and Pillow where it imports), the detector's frame
counting on recording fakes, and ``build_vis_detector`` on a shipped block.  Every test prints the figures it asserts on (run with -s)."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import toc3d_amd
import token_vis_cases as TC
from support import A, ERR_ARG, FakeNeck, OldLibrary, header_sigs, raw_call
from toc3d_amd import configs, lib, synth
from toc3d_amd import token_vis as TV

ALPHA, RENDER = "toc3d_token_alpha", "toc3d_token_vis_render"


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------------------------------------
def test_vis_header_ctypes_table_and_exports_agree():
    raw = open(lib.VIS_HEADER_PATH).read()
    found = header_sigs(lib.header_text(lib.VIS_HEADER_PATH), lib._VIS_SIGS)
    print(f"toc3d_vis.h declares {found}")
    assert found == lib._VIS_SIGS and list(found) == [ALPHA, RENDER]
    declared = set(re.findall(r"\b(toc3d_\w+)\s*\(", lib.header_text(lib.VIS_HEADER_PATH)))
    assert declared == set(lib._VIS_SIGS) | {"toc3d_vis_abi"}, "nothing declared that the table does not bind"
    assert int(re.search(r"#define\s+TOC3D_VIS_ABI\s+(\d+)", raw).group(1)) == lib.VIS_ABI == 1
    assert int(re.search(r"#define\s+TOC3D_VIS_MAX_TOKENS\s+(\d+)", raw).group(1)) == lib.VIS_MAX_TOKENS >= 5000, "covers 1600 x 800 at patch 16"
    assert "token_select_vis.py:27-80" in raw and "petr3d.py:562-579" in raw, "the header cites what it serves"
    assert "two roundings, no FMA contraction" in raw and "76, not 77" in raw
    dll = ctypes.CDLL(lib.LIB_PATH)
    assert all(hasattr(dll, n) for n in declared)
    dll.toc3d_vis_abi.restype = ctypes.c_int
    assert dll.toc3d_vis_abi() == 1
    # the other headers know nothing of it, no name is bound twice, and the 11.1 surface stays where it is
    others = (lib.HEADER_PATH, lib.STREAMS_HEADER_PATH, lib.FOCAL_HEADER_PATH, lib.SAMPLED_HEADER_PATH, lib.SELECT_HEADER_PATH, lib.INGEST_HEADER_PATH)
    for other in others:
        assert "toc3d_vis" not in open(other).read() and ALPHA not in open(other).read() and RENDER not in open(other).read()
    tables = (lib._SIGS, lib._STREAMS_SIGS, lib._FOCAL_SIGS, lib._SAMPLED_SIGS, lib._SELECT_SIGS, lib._INGEST_SIGS)
    assert not any(set(lib._VIS_SIGS) & set(t) for t in tables)
    assert lib.ABI_VERSION == 11 and lib.ABI_MINOR == 1
    main = open(lib.HEADER_PATH).read()
    assert int(re.search(r"#define\s+TOC3D_ABI_VERSION\s+(\d+)", main).group(1)) == 11 and int(re.search(r"#define\s+TOC3D_ABI_MINOR\s+(\d+)", main).group(1)) == 1
    l = lib.load()
    l.toc3d_abi_minor.restype = ctypes.c_int
    assert l.toc3d_abi_version() == 11 and l.toc3d_abi_minor() == 1


def test_exports():
    assert toc3d_amd.TokenVis is TV.TokenVis and toc3d_amd.token_selection_vis is TV.token_selection_vis
    assert {"TokenVis", "token_selection_vis", "build_vis_detector"} <= set(toc3d_amd.__all__)


def alpha_args(**o):
    a = dict(mask=A, keep=A, keep_stride=1000, K=500, V=6, T=1000, min_alpha=0.3, max_alpha=1.0, alpha_mask=A, alpha_keep=A)
    a.update(o)
    return tuple(a[k] for k in ("mask", "keep", "keep_stride", "K", "V", "T", "min_alpha", "max_alpha", "alpha_mask", "alpha_keep")) + (None,)


def render_args(**o):
    a = dict(src=A, src_u8=0, src_stride=0, V=6, H0=320, W0=800, H=320, W=800, patch=16, alpha=A, A=6, mean=(103.53, 116.28, 123.675), std=(57.375, 57.12, 58.395),
             to_rgb=0, ori=A, rgba=A)
    a.update(o)
    return (a["src"], a["src_u8"], a["src_stride"], a["V"], a["H0"], a["W0"], a["H"], a["W"], a["patch"], a["alpha"], a["A"], *a["mean"], *a["std"], a["to_rgb"],
            a["ori"], a["rgba"], None)


def test_call_binds_the_entry_points_and_an_old_library_is_told_to_rebuild(monkeypatch):
    with pytest.raises(RuntimeError, match=r"toc3d_token_alpha failed \(-1\): toc3d_token_alpha: null buffer"):
        lib.call(ALPHA, *alpha_args(mask=None))
    for name in (ALPHA, RENDER):
        assert getattr(lib.load(), name).argtypes == [lib._CT[c] for c in lib._VIS_SIGS[name]], "bound with the table's argument types"

    monkeypatch.setattr(lib, "_lib", OldLibrary())
    with pytest.raises(RuntimeError, match=r"toc3d_vis\.h.*rebuild the library"):
        lib.call(RENDER, *render_args())


U8 = dict(src_u8=1, H0=300, W0=790, src_stride=2370)


@pytest.mark.parametrize("name,over,reason", [
    (ALPHA, dict(mask=None), "null buffer"), (ALPHA, dict(alpha_mask=None), "null buffer"), (ALPHA, dict(keep=None), "null buffer"),
    (ALPHA, dict(V=0), "must be positive"), (ALPHA, dict(T=0), "must be positive"), (ALPHA, dict(T=-4), "must be positive"), (ALPHA, dict(K=-1), "not negative"),
    (ALPHA, dict(V=1 << 31), "grid"), (ALPHA, dict(T=lib.VIS_MAX_TOKENS + 1), "TOC3D_VIS_MAX_TOKENS"), (ALPHA, dict(keep_stride=499), "a stride smaller than a row"),
    (ALPHA, dict(keep_stride=-1000), "a stride smaller than a row"),
    (ALPHA, {}, "host pointer"), (ALPHA, dict(keep=None, K=0), "host pointer"), (ALPHA, dict(keep=None, alpha_keep=None), "host pointer"),
    *[(RENDER, {p: None}, "null buffer") for p in ("src", "alpha", "ori", "rgba")],
    *[(RENDER, {d: 0}, "must be positive") for d in ("A", "V", "H0", "W0", "H", "W", "patch")], (RENDER, dict(patch=-16), "must be positive"),
    (RENDER, dict(V=65536), "grid"), (RENDER, dict(H=1 << 20, W=1 << 20, H0=1 << 20, W0=1 << 20), "grid"),
    (RENDER, dict(H=328, H0=328), "multiples of patch"), (RENDER, dict(W=808, W0=808), "multiples of patch"), (RENDER, dict(patch=7), "multiples of patch"),
    (RENDER, dict(U8, H0=321), "inside the padded"), (RENDER, dict(U8, W0=801, src_stride=2403), "inside the padded"),
    (RENDER, dict(H0=304), "H0 == H and W0 == W"), (RENDER, dict(W0=784), "H0 == H and W0 == W"),
    (RENDER, dict(H=1600, W=1600, H0=1600, W0=1600), "TOC3D_VIS_MAX_TOKENS"), (RENDER, dict(patch=2), "TOC3D_VIS_MAX_TOKENS"),
    (RENDER, dict(U8, src_stride=2369), "a stride smaller than a row"), (RENDER, dict(U8, src_stride=0), "a stride smaller than a row"),
    (RENDER, dict(src=A + 2), "4-byte boundary"),
    (RENDER, {}, "host pointer"), (RENDER, U8, "host pointer"), (RENDER, dict(U8, src=A + 1), "host pointer"),
])
def test_entry_point_refusals(name, over, reason):
    rc, msg = raw_call(lib._VIS_SIGS, name, (alpha_args if name == ALPHA else render_args)(**over))
    print(f"{name} {over}: rc {rc}, {msg!r}")
    assert rc == ERR_ARG and msg.startswith(name + ":") and reason in msg, (rc, msg)


def test_real_host_buffers_are_refused_and_left_alone():
    """Host memory that could be read and written: both entry points refuse it (not device memory) and touch none of it."""
    p = ctypes.addressof
    mask = (ctypes.c_float * 4)(*([1.0] * 4))
    keep = (ctypes.c_int64 * 4)(*([0] * 4))
    am, ak = (ctypes.c_ubyte * 4)(*([9] * 4)), (ctypes.c_ubyte * 4)(*([9] * 4))
    rc, msg = raw_call(lib._VIS_SIGS, ALPHA, alpha_args(mask=p(mask), keep=p(keep), keep_stride=2, K=2, V=2, T=2, alpha_mask=p(am), alpha_keep=p(ak)))
    print(f"rc {rc}, {msg!r}")
    assert rc == ERR_ARG and "host pointer" in msg and bytes(am) == bytes(ak) == bytes([9] * 4)
    src = (ctypes.c_ubyte * (16 * 16 * 3))(*([7] * 768))
    alpha = (ctypes.c_ubyte * 16)(*([5] * 16))
    ori, rgba = (ctypes.c_ubyte * 768)(*([9] * 768)), (ctypes.c_ubyte * 1024)(*([9] * 1024))
    rc, msg = raw_call(lib._VIS_SIGS, RENDER, render_args(src=p(src), src_u8=1, src_stride=48, V=1, H0=16, W0=16, H=16, W=16, alpha=p(alpha), A=1, ori=p(ori), rgba=p(rgba)))
    print(f"rc {rc}, {msg!r}")
    assert rc == ERR_ARG and "host pointer" in msg
    assert bytes(ori) == bytes([9] * 768) and bytes(rgba) == bytes([9] * 1024) and bytes(src) == bytes([7] * 768) and bytes(alpha) == bytes([5] * 16)


# ---- the fixture and the restatement ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return np.load(TC.FIXTURE), json.load(open(TC.FIXTURE_META))


def golden_key(case, name, kind):
    base = name[:-4]
    if base.endswith("_ori"):
        base = base.split("_layer")[0] + "_ori"
    return f"{case}_{kind}_{base}"


@pytest.mark.parametrize("case", sorted(TC.CASES))
def test_restatement_equals_the_fixture(golden, case):
    z, meta = golden
    c = TC.CASES[case]
    inp = TC.inputs(c, TC.case_seed(case))
    assert np.array_equal(z[f"{case}_in_raw"], inp["raw"]) and np.array_equal(z[f"{case}_in_img"].view(np.int32), inp["img"].view(np.int32)), "the seeded inputs"
    for l, m in enumerate(inp["masks"]):
        assert np.array_equal(z[f"{case}_in_mask{l}"], m)
        if inp["keeps"] is not None:
            assert np.array_equal(z[f"{case}_in_keep{l}"], inp["keeps"][l]) and np.array_equal(z[f"{case}_in_drop{l}"], inp["drops"][l])
    files = TC.restated(inp["img"], inp["masks"], inp["keeps"], inp["drops"], c["norm"], c["patch"])
    assert [n for n, _ in files] == meta["cases"][case]["files"], "file names, in the order the reference writes them"
    L, per_view = len(inp["masks"]), (3 if c["K"] is not None else 2)
    assert len(files) == c["V"] * L * per_view
    nf = nb = 0
    for name, arr in files:
        want_f, want_b = z[golden_key(case, name, "f")], z[golden_key(case, name, "b")]
        nf += int((arr.view(np.int32) != want_f.view(np.int32)).sum())
        nb += int((TC.to_bytes(arr) != want_b).sum())
    u8 = TC.restated_u8(inp["raw"], inp["masks"], inp["keeps"], inp["drops"], c["norm"], c["patch"])
    nu = sum(int((TC.to_bytes(a) != z[golden_key(case, n, "b")]).sum()) for n, a in u8)
    print(f"case {case}: {len(files)} files; {nf} float32 values, {nb} bytes differ from the fixture; the uint8 form differs in {nu} bytes")
    assert nf == 0 and nb == 0 and nu == 0
    assert "LIMITATION" in meta and "OpenCV" in meta["LIMITATION"]


def test_alpha_and_padding_bytes():
    a = TC.to_bytes(TC.token_alpha([0.0, 1.0, 0.25, 0.5]))
    print(f"alpha bytes of m = 0, 1, 0.25, 0.5 at the defaults: {a.tolist()}; 255 * 0.3f = {float(TC.token_alpha([0.0])[0])!r}")
    assert a.tolist()[:2] == [76, 255] and float(TC.token_alpha([0.0])[0]) == 76.5, "a dropped token is 76: 76.5 rounds half to even"
    assert a.tolist()[2:] == [121, 166]
    pad = TC.to_bytes(np.rint(TC.f32(TC.SHIPPED_NORM["mean"])))
    assert pad.tolist()[::-1] == [124, 116, 104], "array channels 2 / 1 / 0 of the shipped means"
    # ... which is what a zero-padded normalised image denormalises to
    assert TC.to_bytes(TC.imdenormalize(np.zeros((1, 1, 3), np.float32), TC.SHIPPED_NORM["mean"], TC.SHIPPED_NORM["std"], to_bgr=False)).reshape(-1).tolist() == pad.tolist()


def test_fma_sensitive_set():
    x, c = TC.fma_sensitive()
    n = TC.SHIPPED_NORM
    sd, mu = TC.f32(n["std"])[c], TC.f32(n["mean"])[c]
    two = TC.to_bytes(TC.two_roundings(x, sd, mu))
    fu, safe = TC.fused(x, sd, mu)
    print(f"{len(x)} values on which two roundings and a fused multiply-add differ after rounding; per channel {np.bincount(c).tolist()}")
    assert len(x) == 190 and len(x) >= 16 and safe.all() and (two != TC.to_bytes(fu)).all()
    assert x.dtype == np.float32 and set(c.tolist()) == {0, 1, 2}
    x2, c2 = TC.fma_sensitive()
    assert np.array_equal(x, x2) and np.array_equal(c, c2), "a fixed seed"


# ---- the PNG writer --------------------------------------------------------------------------------------------------------------------------------------------------
decode_png = TC.decode_png                  # a decoder for what the writer makes, shared with the GPU tests


@pytest.mark.parametrize("shape", [(5, 7, 3), (4, 6, 4), (1, 1, 3), (3, 5, 4), (16, 33, 3)])
def test_png_writer_round_trips(tmp_path, shape):
    """RGB and RGBA, widths whose row bytes are no multiple of 4 (7 x 3 = 21, 33 x 3 = 99), the blue-first convention and file order."""
    arr = np.random.default_rng(sum(shape)).integers(0, 256, shape, dtype=np.uint8)
    assert np.array_equal(decode_png(TV.encode_png(arr)), arr)
    path = str(tmp_path / "a.png")
    TV.write_png(path, arr)                                                 # cv2.imwrite's convention: array channel 0 is blue
    got = decode_png(open(path, "rb").read())
    assert np.array_equal(got[..., 0], arr[..., 2]) and np.array_equal(got[..., 1], arr[..., 1]) and np.array_equal(got[..., 2], arr[..., 0])
    assert shape[2] == 3 or np.array_equal(got[..., 3], arr[..., 3]), "alpha stays last"
    TV.write_png(path, arr, blue_first=False)
    assert np.array_equal(decode_png(open(path, "rb").read()), arr)
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        img = Image.open(path)
        assert img.mode == ("RGB" if shape[2] == 3 else "RGBA") and np.array_equal(np.asarray(img), arr)
    with pytest.raises(ValueError, match="encode_png"):
        TV.encode_png(arr.astype(np.float32))


def test_write_names_order_and_colours(tmp_path):
    """TokenVis.write on arrays of the restatement (CPU tensors: the writer does not care): the reference's names in its order, ori once per stage, the
    blue-first files and fix_colors for both conventions."""
    for case, fix, plain_order in (("two", False, False), ("two", True, True), ("p8", True, False), ("plain", False, False)):
        c = TC.CASES[case]
        inp = TC.inputs(c, TC.case_seed(case))
        files = TC.restated(inp["img"], inp["masks"], inp["keeps"], inp["drops"], c["norm"], c["patch"])
        ori, masks, keep = TC.planes(files, c["V"], len(inp["masks"]), c["K"] is not None)
        t = lambda a: None if a is None else torch.from_numpy(a)
        out = str(tmp_path / f"{case}{int(fix)}" / "nested") + "/"
        names = toc3d_amd.TokenVis(c["patch"]).write(dict(ori=t(ori), masks=t(masks), keepidx=t(keep), to_rgb=c["norm"]["to_rgb"]), out, fix_colors=fix)
        assert [os.path.basename(n) for n in names] == [n for n, _ in files] and sorted(os.listdir(out)) == sorted(n for n, _ in files)
        for n, arr in files:
            got, want = decode_png(open(os.path.join(out, n), "rb").read()), TC.to_bytes(arr)
            if not plain_order:
                want = np.concatenate([want[..., 2::-1], want[..., 3:]], axis=-1)
            assert np.array_equal(got, want), (case, n)
        # true colours: the file's red plane is the raw frame's red plane (raw frames are BGR as cv2.imread gives them; to_rgb swapped them for the network)
        if fix:
            got = decode_png(open(os.path.join(out, "view0_layer0_ori.png"), "rb").read())
            H0, W0 = c["raw"]
            assert np.array_equal(got[:H0, :W0, 0], inp["raw"][0, :, :, 2]) and np.array_equal(got[:H0, :W0, 2], inp["raw"][0, :, :, 0])


# ---- the detector: which frames are rendered ----------------------------------------------------------------------------------------------------------------------
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
        return [[torch.zeros(3, 9), torch.arange(3.0), torch.arange(3)] for _ in img_metas]


class FakeVis:
    """Records what the detector hands to TokenVis."""
    def __init__(self, log, views):
        self.log, self.views = log, views

    def render(self, img, masks, keeps, drops, cfg):
        self.log.append(("render", tuple(img.shape), masks, keeps, drops, cfg))
        return dict(ori=torch.zeros(self.views, 1, 1, 3))

    def write(self, rendered, path, fix_colors=False, views=None):
        self.log.append(("write", path, None if views is None else list(views)))


def fake_detector(log, views=6):
    det = toc3d_amd.build_detector(synth.detector_cfg(synth.DETECTOR_TINY))
    det.img_backbone, det.img_neck, det.pts_bbox_head = FakeBackbone(log), FakeNeck(log), FakeHead(log)
    return det


def frame(det, scene="a", norm="cfg"):
    metas = [dict(scene_token=scene, pad_shape=[(32, 80, 3)], img_norm_cfg=norm)]
    return det.simple_test(metas, img=torch.zeros(1, 6, 3, 32, 80), intrinsics=torch.zeros(1, 6, 4, 4), lidar2img=torch.zeros(1, 6, 4, 4),
                           timestamp=torch.zeros(1, dtype=torch.float64), ego_pose=torch.eye(4)[None], ego_pose_inv=torch.eye(4)[None])


@pytest.mark.parametrize("start,num,rendered,cur_id", [(0, 2, [0, 1], 2), (1, 1, [1], 2), (5, 1, [], 4)])
def test_which_frames_are_rendered(start, num, rendered, cur_id):
    log = []
    det = fake_detector(log)
    assert det.enable_token_vis(vis_num_sample=num, vis_start_id=start, vis_out_path="out/vis") is det and det.token_select_vis and det.cur_id == 0
    assert isinstance(det._token_vis, toc3d_amd.TokenVis) and det._token_vis.patch_size == 16
    det._token_vis = FakeVis(log, 6)
    seen = []
    for f in range(4):
        del log[:]
        out = frame(det)
        names = [e[0] for e in log]
        hit = f in rendered
        assert names == ["backbone", "neck"] + (["render", "write"] if hit else []) + ["head"], (f, names)      # :562-579: after extract_img_feat, before the head
        if hit:
            r, w = log[2], log[3]
            assert r[1:] == ((1, 6, 3, 32, 80), ["m0", "m1", "m2"], ["k0", "k1", "k2"], ["d0", "d1", "d2"], "cfg") and w[1:] == (f"./out/vis/{f}/", None)
            seen.append(f)
        assert list(out[0]) == ["pts_bbox"]
    print(f"(vis_start_id, vis_num_sample) = ({start}, {num}): frames {seen} rendered, cur_id {det.cur_id}, samples left {det.vis_num_sample}")
    assert seen == rendered and det.cur_id == cur_id, "the counter stops once the samples are used up"
    assert det.vis_num_sample == num - len(rendered)


def test_disable_streams_and_the_dense_backbone():
    log = []
    det = fake_detector(log)
    det.enable_token_vis(vis_num_sample=3, vis_out_path="v")
    det._token_vis = FakeVis(log, 12)
    det.disable_token_vis()
    frame(det)
    assert [e[0] for e in log] == ["backbone", "neck", "head"] and det.cur_id == 0, "off: nothing rendered, nothing counted"
    det.enable_token_vis(vis_num_sample=3, vis_out_path="v")
    det._token_vis = FakeVis(log, 12)
    # two streams in one step: counted once, a sub-directory per stream with that stream's views
    for step in range(2):
        del log[:]
        metas = [dict(scene_token="a", pad_shape=[(32, 80, 3)]), dict(scene_token="b", pad_shape=[(32, 80, 3)], img_norm_cfg="other")]
        out = det.simple_test_streams(metas, img=torch.zeros(2, 6, 3, 32, 80), intrinsics=torch.zeros(2, 6, 4, 4), lidar2img=torch.zeros(2, 6, 4, 4),
                                      timestamp=torch.zeros(2, dtype=torch.float64), ego_pose=torch.eye(4)[None].repeat(2, 1, 1), ego_pose_inv=torch.eye(4)[None].repeat(2, 1, 1))
        assert len(out) == 2
        evs = [e for e in log if e[0] in ("render", "write")]
        assert [e[0] for e in evs] == ["render", "write", "write"] and evs[0][1] == (2, 6, 3, 32, 80) and evs[0][5] is None, "stream 0's metas carry no img_norm_cfg"
        assert evs[1][1:] == (f"./v/{step}/stream0/", list(range(0, 6))) and evs[2][1:] == (f"./v/{step}/stream1/", list(range(6, 12)))
    assert det.cur_id == 2 and det.vis_num_sample == 1
    dense = toc3d_amd.build_detector(dict(synth.detector_cfg(synth.DETECTOR_TINY), img_backbone=dict(configs.EVA_TINY)))
    with pytest.raises(ValueError, match="a dense backbone has no masks"):
        dense.enable_token_vis()
    assert not dense.token_select_vis


def test_build_vis_detector_on_a_shipped_block():
    """The model block of projects/configs/token_vis_ToC3D/ToC3D_faster.py:35-43 -- the ToC3D_faster block plus token_select_vis, vis_num_sample and vis_start_id --
    at tiny sizes: the constructor keeps refusing the keyword, the builder takes the block unchanged."""
    block = dict(synth.detector_cfg(synth.DETECTOR_TINY), token_select_vis=True, vis_num_sample=80, vis_start_id=0)
    with pytest.raises(NotImplementedError, match="enable_token_vis"):
        toc3d_amd.build_detector(block)
    keys = sorted(block)
    det = toc3d_amd.build_vis_detector(block)
    assert sorted(block) == keys and block["token_select_vis"] is True, "the caller's block is not changed"
    assert isinstance(det, toc3d_amd.Petr3D) and det.token_select_vis and (det.vis_num_sample, det.vis_start_id, det.vis_out_path, det.cur_id) == (80, 0, "./token_vis", 0)
    assert det._token_vis.patch_size == det.img_backbone.patch_size == 16
    off = toc3d_amd.build_vis_detector(dict(block, token_select_vis=False, vis_out_path="elsewhere"), precision="bf16")
    assert not off.token_select_vis and off._token_vis is None and off.vis_num_sample == 80 and off.vis_out_path == "elsewhere" and off.precision == "bf16"
    plain = toc3d_amd.build_vis_detector(synth.detector_cfg(synth.DETECTOR_TINY))
    assert not plain.token_select_vis
    # the pixels have no CPU path
    with pytest.raises(RuntimeError, match="only compute path"):
        toc3d_amd.TokenVis().render(torch.zeros(1, 3, 16, 16), [torch.zeros(1, 1, 1, 1)])
