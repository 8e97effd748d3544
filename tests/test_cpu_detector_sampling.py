"""CPU: the detector with token selection (toc3d_amd.Petr3D(aux_2d_only=False)) and the entry point it adds, without a GPU -- the side header
include/toc3d_select.h against the ctypes table that binds it and against the library's exports, a library without the symbol is told to rebuild, every refusal
of toc3d_focal_sample_weight on made-up host pointers (the checks run before any launch), construction (the roi head is built, precision reaches it, the head takes
topk_indexes, the ValueErrors), the state dict (the union plus the sixteen img_roi_head names), strict loading in both modes, derived state, and -- on recording
fakes -- the sequencing of four frames: the location is built once, select_rows runs before the head, its topk_indexes are passed through, reset_memory fires on
the scene change."""
import ctypes
import json
import os
import re

import pytest
import torch
import torch.nn as nn

import toc3d_amd
from support import A, ERR_ARG, FakeNeck, OldLibrary, header_sigs, raw_call
from toc3d_amd import FocalHead, lib, synth
from toc3d_amd.detector import Petr3D

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TINY = synth.DETECTOR_TINY_ROI


def tiny(**over):
    return toc3d_amd.build_detector(dict(synth.detector_cfg(TINY), aux_2d_only=False, **over))


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------------------------------------
def test_select_header_ctypes_table_and_exports_agree():
    raw = open(lib.SELECT_HEADER_PATH).read()
    found = header_sigs(lib.header_text(lib.SELECT_HEADER_PATH), lib._SELECT_SIGS)
    print(f"toc3d_select.h declares {found}")
    assert found == lib._SELECT_SIGS and list(found) == ["toc3d_focal_sample_weight"]
    declared = set(re.findall(r"\b(toc3d_\w+)\s*\(", lib.header_text(lib.SELECT_HEADER_PATH)))
    assert declared == set(lib._SELECT_SIGS) | {"toc3d_select_abi"}, "nothing declared that the table does not bind"
    assert int(re.search(r"#define\s+TOC3D_SELECT_ABI\s+(\d+)", raw).group(1)) == lib.SELECT_ABI == 1
    assert "focal_head.py:159-160, 178-180" in raw and "petr3d.py:524-525" in raw, "the header cites the reference lines it serves"
    dll = ctypes.CDLL(lib.LIB_PATH)
    assert all(hasattr(dll, n) for n in declared)
    dll.toc3d_select_abi.restype = ctypes.c_int
    assert dll.toc3d_select_abi() == 1
    # the pinned headers know nothing of it, and no header was folded
    for path in (lib.HEADER_PATH, lib.STREAMS_HEADER_PATH, lib.FOCAL_HEADER_PATH, lib.SAMPLED_HEADER_PATH):
        assert "toc3d_focal_sample_weight" not in open(path).read() and "toc3d_select" not in open(path).read(), path
    assert not set(lib._SELECT_SIGS) & (set(lib._SIGS) | set(lib._STREAMS_SIGS) | set(lib._FOCAL_SIGS) | set(lib._SAMPLED_SIGS))
    assert (lib.ABI_VERSION, lib.ABI_MINOR, lib.FOCAL_ABI, lib.SAMPLED_ABI, lib.STREAMS_ABI) == (11, 1, 1, 1, 1)


PTRS = ("x", "stats", "gamma", "beta", "w_cls", "b_cls", "weight")


def weight_args(dtype=lib.F32, **o):
    a = dict({p: A for p in PTRS}, ldx=256, V=6, T=1000, E=256, NC=10)
    a.update(o)
    return (dtype, a["x"], a["ldx"], a["stats"], a["gamma"], a["beta"], a["w_cls"], a["b_cls"], a["V"], a["T"], a["E"], a["NC"], a["weight"], None)


def test_call_binds_the_entry_point_and_an_old_library_is_told_to_rebuild(monkeypatch):
    with pytest.raises(RuntimeError, match=r"toc3d_focal_sample_weight failed \(-1\): toc3d_focal_sample_weight: null buffer"):
        lib.call("toc3d_focal_sample_weight", *weight_args(x=None))
    for n, sig in lib._SELECT_SIGS.items():
        assert getattr(lib.load(), n).argtypes == [lib._CT[c] for c in sig], "bound with the table's argument types (int64 counts, not C ints)"

    monkeypatch.setattr(lib, "_lib", OldLibrary())
    with pytest.raises(RuntimeError, match=r"toc3d_select\.h.*rebuild the library"):
        lib.call("toc3d_focal_sample_weight", *weight_args())


@pytest.mark.parametrize("dtype,over,reason", [
    *[(lib.F32, {p: None}, "null buffer") for p in PTRS],
    (lib.BF16, {}, "bad dtype"), (lib.F32X3P, {}, "bad dtype"), (99, {}, "bad dtype"),
    (lib.F32, dict(V=0), "must be positive"), (lib.F32, dict(T=0), "must be positive"), (lib.F32, dict(T=-5), "must be positive"), (lib.F32, dict(E=0), "must be positive"),
    (lib.F32, dict(NC=0), "must be positive"), (lib.F32, dict(E=48), "embed_dims % 32 != 0"), (lib.F32, dict(E=250), "embed_dims % 32 != 0"),
    (lib.F32, dict(E=2048, ldx=2048), "above 1024"), (lib.F32, dict(NC=65), "num_classes above 64"),
    (lib.F32, dict(E=1024, ldx=1024, NC=16), "64 KB of LDS"), (lib.F32, dict(E=256, NC=64), "64 KB of LDS"),
    (lib.F32, dict(ldx=252), "leading dimension"), (lib.F32, dict(ldx=258), "leading dimension"),
    (lib.F32, dict(x=A + 4), "aligned"), (lib.F32, dict(gamma=A + 8), "aligned"), (lib.F32, dict(beta=A + 4), "aligned"), (lib.F32, dict(w_cls=A + 4), "aligned"),
    (lib.F32, dict(T=1 << 31), "too many"), (lib.F32, dict(V=1 << 31, T=32), "too many"),
])
def test_sample_weight_refusals(dtype, over, reason):
    rc, msg = raw_call(lib._SELECT_SIGS, "toc3d_focal_sample_weight", weight_args(dtype, **over))
    print(f"{over or dtype}: rc {rc}, {msg!r}")
    assert rc == ERR_ARG and msg.startswith("toc3d_focal_sample_weight:") and reason in msg, (rc, msg)


# ---- construction ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_roi_head_is_built_and_the_head_takes_its_tokens():
    det = tiny()
    assert isinstance(det, Petr3D) and isinstance(det.img_roi_head, FocalHead) and det.with_img_roi_head and not det.aux_2d_only and not det.training
    roi = det.img_roi_head
    assert (roi.num_classes, roi.in_channels, roi.embed_dims, roi.infer_ratio, roi.precision) == (3, 64, 64, 0.3, "fp32x3")
    assert det.pts_bbox_head.token_sampling and det.img_neck.out_channels == 64
    assert tiny(precision="bf16").img_roi_head.precision == "bf16", "precision is handed down as for the other parts"
    # the default path is what it was: no module, a head that refuses topk_indexes, None from forward_roi_head
    plain = toc3d_amd.build_detector(synth.detector_cfg(TINY))
    assert not hasattr(plain, "img_roi_head") and not plain.with_img_roi_head and not plain.pts_bbox_head.token_sampling
    assert plain.forward_roi_head(None) == {"topk_indexes": None}
    # aux_2d_only=False without a roi head runs that path too (:319, `not self.with_img_roi_head`)
    none = tiny(img_roi_head=None)
    assert not none.with_img_roi_head and not none.pts_bbox_head.token_sampling and none.forward_roi_head(None) == {"topk_indexes": None}
    assert none._select_tokens([dict(pad_shape=[(320, 800, 3)])], dict(img_feats=torch.zeros(1, 6, 64, 20, 50))) == (None, None)
    # the shipped block with the one keyword changed
    assert synth.detector_cfg() == synth.detector_cfg(synth.DETECTOR_FULL_ROI), "sizes with a roi key of no overrides build the shipped block"


def test_refusals_at_construction_and_at_the_first_frame():
    with pytest.raises(ValueError, match="out_channels 64 != img_roi_head's in_channels 128"):
        tiny(img_roi_head=dict(synth.detector_cfg(TINY)["img_roi_head"], in_channels=128))
    # what FocalHead refuses about its own config is said first, with its exception: DETECTOR_TINY's 32-channel neck
    with pytest.raises(NotImplementedError, match="toc3d_amd.FocalHead: in_channels=32"):
        toc3d_amd.build_detector(dict(synth.detector_cfg(synth.DETECTOR_TINY), aux_2d_only=False))
    with pytest.raises(NotImplementedError):
        tiny(img_roi_head=dict(type="YOLOXHeadCustom"))
    # a selection that keeps no token: detected at the first frame, before anything is launched (the fakes would log it)
    det, log = tiny(img_roi_head=dict(synth.detector_cfg(TINY)["img_roi_head"], infer_ratio=0.0001)), []
    det.img_backbone, det.img_neck, det.pts_bbox_head = FakeBackbone(log), FakeNeck(log), FakeHead(log)
    data = dict(img=torch.zeros(1, 6, 3, 32, 80), intrinsics=torch.zeros(1, 6, 4, 4), lidar2img=torch.zeros(1, 6, 4, 4), timestamp=torch.zeros(1, dtype=torch.float64),
                ego_pose=torch.eye(4)[None], ego_pose_inv=torch.eye(4)[None])
    metas = [dict(scene_token="a", pad_shape=[(32, 80, 3)])]
    with pytest.raises(ValueError, match=r"int\(60 tokens \* infer_ratio 0.0001\) = 0 tokens"):
        det.simple_test(metas, **data)
    with pytest.raises(ValueError, match="= 0 tokens"):
        det.simple_test_streams(metas, **data)
    assert log == [], "nothing ran"
    with pytest.raises(ValueError, match="= 0 tokens"):          # ... and in front of the roi head's launches for a caller that comes in through simple_test_pts
        det.simple_test_pts(metas, img_feats=torch.zeros(1, 6, 64, 2, 5), **data)
    assert log == []


# ---- state -----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_state_dict_is_the_union_plus_the_sixteen_roi_names():
    spec = json.load(open(os.path.join(GOLDEN, "focal_head_state_dict_spec.json")))
    det, plain = tiny(), toc3d_amd.build_detector(synth.detector_cfg(TINY))
    got, base = {k: list(v.shape) for k, v in det.state_dict().items()}, {k: list(v.shape) for k, v in plain.state_dict().items()}
    roi = {k: v for k, v in got.items() if k.startswith("img_roi_head.")}
    assert len(roi) == 16 and [k[len("img_roi_head."):] for k in roi] == list(spec["tiny"]) and {k[len("img_roi_head."):]: v for k, v in roi.items()} == spec["tiny"]
    assert {k: v for k, v in got.items() if k not in roi} == base
    sd = synth.detector_state_dict(TINY)
    assert {k: list(v.shape) for k, v in sd.items()} == got
    # sizes that do not ask for them get no roi keys: the existing helpers' results are unchanged
    assert not any(k.startswith("img_roi_head.") for k in synth.detector_state_dict(synth.DETECTOR_TINY))
    # the shipped sizes: 620 + 4 + 16 + 251 names (shapes from the specs; the ViT-L weights are not drawn here)
    full = toc3d_amd.build_detector(dict(synth.detector_cfg(), aux_2d_only=False))
    names = list(full.state_dict())
    assert len(names) == 620 + 4 + 16 + 251 and {k[len("img_roi_head."):]: list(v.shape) for k, v in full.state_dict().items() if k.startswith("img_roi_head.")} == spec["full"]
    assert (full.img_roi_head.infer_ratio, full.img_roi_head.in_channels, full.pts_bbox_head.token_sampling) == (1.0, 256, True)


def test_strict_loading_in_both_modes_and_derived_state():
    sd = synth.detector_state_dict(TINY)
    det = tiny()
    det.prev_scene_token, det._location = "a", ("key", "tensor")
    assert str(det.load_state_dict(sd, strict=True)) == "<All keys matched successfully>"
    assert det.prev_scene_token is None and det._location is None, "new weights: the scene and the location start over"
    assert all(torch.equal(v, sd[k]) for k, v in det.state_dict().items())
    without = {k: v for k, v in sd.items() if not k.startswith("img_roi_head.")}
    with pytest.raises(RuntimeError, match=r'Missing key\(s\) in state_dict: "img_roi_head.cls.weight"'):
        det.load_state_dict(without, strict=True)
    with pytest.raises(RuntimeError, match=r'Unexpected key\(s\) in state_dict: "img_roi_head.x"'):
        det.load_state_dict(dict(sd, **{"img_roi_head.x": torch.zeros(3)}), strict=True)
    res = det.load_state_dict(without, strict=False)
    assert len(res.missing_keys) == 16 and not res.unexpected_keys
    # without the module the keys are dropped as before, whatever they hold
    plain = toc3d_amd.build_detector(synth.detector_cfg(TINY))
    res = plain.load_state_dict(dict(sd, **{"img_roi_head.x": torch.zeros(3)}), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert str(plain.load_state_dict(without, strict=True)) == "<All keys matched successfully>"
    # load_state_dict, .to() and init_weights() drop the roi head's derived state, and the detector's
    roi = det.img_roi_head
    for drop in (lambda: det.load_state_dict(sd), lambda: det.to("cpu"), det.init_weights):
        roi._packed, roi._ws, roi._states = "packed", {1: 2}, {3: 4}
        det._location, det.prev_scene_token = ("key", "tensor"), "a"
        drop()
        assert roi._packed is None and roi._ws == {} and roi._states == {} and det._location is None and det.prev_scene_token is None
    assert float(roi.cls.bias.detach()[0]) == pytest.approx(-4.59511985013459), "init_weights reaches the roi head (focal_head.py:136-138)"


# ---- sequencing, on recording fakes --------------------------------------------------------------------------------------------------------------------------------
class FakeBackbone(nn.Module):
    pruning_loc, pruning_num_queries = [3, 6, 9], 64

    def __init__(self, log):
        super().__init__()
        self.log = log

    def forward(self, x, **kw):
        self.log.append(("backbone", tuple(x.shape), kw["prev_exists"]))
        return toc3d_amd.ToC3DViTReturnType({"last_feat": torch.zeros(x.shape[0], 8, 2, 5)}, ["m0", "m1", "m2"], None, ["k0", "k1", "k2"], ["d0", "d1", "d2"])


class FakeHead(nn.Module):
    def __init__(self, log):
        super().__init__()
        self.log, self.bank, self.rows = log, None, {}

    def backbone_queries(self, n, prev_exists, batch_size=1):
        return dict(temp_queries=torch.zeros(batch_size, n, 256), temp_ref_points=None, temp_timestamp=None, temp_ego_pose=None, temp_vel=None, prev_exists=prev_exists)

    def img_feats_rows_buffer(self, B, N, h, w, device=None):
        return self.rows.setdefault((B, N, h, w), torch.zeros(B * N * h * w, 64, dtype=torch.bfloat16)), 64, lib.BF16

    def reset_memory(self):
        self.log.append(("reset",))

    def forward(self, memory_center, img_metas, topk_indexes=None, img_feats_rows=False, **data):
        self.log.append(("head", memory_center, topk_indexes, img_feats_rows, data["prev_exists"].tolist()))
        return dict(all_cls_scores="cls", all_bbox_preds="box", dn_mask_dict=None)

    def get_bboxes(self, outs, img_metas, rescale=False):
        return [[torch.zeros(3, 9), torch.arange(3.0), torch.arange(3)] for _ in img_metas]


class FakeRoi(nn.Module):
    in_channels, infer_ratio = 64, 0.3

    def __init__(self, log, precision):
        super().__init__()
        self.log, self.precision = log, precision

    def select_rows(self, location, rows, ld, B, N, h, w):
        self.log.append(("select_rows", location, rows, ld, (B, N, h, w)))
        return dict(topk_indexes="topk%d" % len(self.log), sample_weight=None)

    def select(self, location, **data):
        self.log.append(("select", location, sorted(data)))
        return dict(topk_indexes="topk%d" % len(self.log), sample_weight=None)

    def forward(self, *a, **k):
        raise AssertionError("simple_test takes the selection-only path")

    forward_rows = forward


class Neck64(FakeNeck):
    """FakeNeck with the accessor of the plain-f32 conv rows."""
    def conv_rows(self, V, h, w):
        self.log.append(("conv_rows", V, h, w))
        self.o0 = getattr(self, "o0", torch.zeros(V * h * w, 64))
        return self.o0, 64


@pytest.mark.parametrize("precision", ["bf16", "fp32x3"])
def test_sequencing_over_four_frames_with_a_scene_change(precision):
    det, log = tiny(precision=precision), []
    det.img_backbone, det.img_neck, det.pts_bbox_head, det.img_roi_head = FakeBackbone(log), Neck64(log), FakeHead(log), FakeRoi(log, precision)
    built = []
    prepare = det.prepare_location
    det.prepare_location = lambda metas, **d: (built.append(1), prepare(metas, **d))[1]
    data = lambda: dict(img=torch.zeros(1, 6, 3, 32, 80), intrinsics=torch.zeros(1, 6, 4, 4), lidar2img=torch.zeros(1, 6, 4, 4), timestamp=torch.zeros(1, dtype=torch.float64),
                        ego_pose=torch.eye(4)[None], ego_pose_inv=torch.eye(4)[None])
    locations = []
    for f, scene in enumerate(["a", "a", "a", "b"]):
        del log[:]
        out = det.simple_test([dict(scene_token=scene, pad_shape=[(32, 80, 3)])], **data())
        prev = f in (1, 2)
        names = [e[0] for e in log]
        rows_from = [] if precision == "bf16" else ["conv_rows"]
        assert names == ["backbone", "neck"] + rows_from + ["select_rows"] + ([] if prev else ["reset"]) + ["head"], (f, names)
        sel, hd = log[names.index("select_rows")], log[-1]
        # select_rows runs before the head, on the neck's rows of this frame: the head's bf16 rows, or the neck's own plain-f32 conv rows
        assert sel[4] == (1, 6, 2, 5) and sel[3] == 64
        assert sel[2] is (det.pts_bbox_head.rows[(1, 6, 2, 5)] if precision == "bf16" else det.img_neck.o0)
        # its topk_indexes are passed through, with the location, on the fanned rows
        assert hd[2] == "topk%d" % (names.index("select_rows") + 1)
        assert hd[1] is sel[1] and tuple(hd[1].shape) == (6, 2, 5, 2) and hd[3] is True and hd[4] == [1.0 if prev else 0.0]
        locations.append(sel[1])
        assert len(out) == 1 and set(out[0]["pts_bbox"]) == {"boxes_3d", "scores_3d", "labels_3d"}
    assert built == [1] and all(l is locations[0] for l in locations), "the location is built once and kept as derived state"
    # a tensor that is not the fanned one goes through select; another pad_shape builds another location
    del log[:]
    det.simple_test_pts([dict(scene_token="b", pad_shape=[(32, 80, 3)])], img_feats=torch.zeros(1, 6, 4, 2, 5), **data())
    assert [e[0] for e in log] == ["select", "head"] and log[0][2] == ["img_feats"] and log[1][2] == "topk1" and log[1][3] is False and log[0][1] is locations[0]
    det.simple_test_pts([dict(scene_token="b", pad_shape=[(64, 80, 3)])], img_feats=torch.zeros(1, 6, 4, 2, 5), **data())
    assert built == [1, 1] and log[-2][1] is not locations[0]
    # two streams: one selection per step for both samples
    del log[:]
    two = {k: torch.cat([v, v]) for k, v in data().items()}
    det.simple_test_streams([dict(scene_token="a", pad_shape=[(32, 80, 3)]), dict(scene_token="b", pad_shape=[(32, 80, 3)])], **two)
    names = [e[0] for e in log]
    assert names == ["reset", "backbone", "neck"] + rows_from + ["select_rows", "head"] and log[names.index("select_rows")][4] == (2, 6, 2, 5)
    assert log[-1][2] == "topk%d" % (names.index("select_rows") + 1) and tuple(log[-1][1].shape) == (12, 2, 5, 2)
