"""CPU: the assembled detector (toc3d_amd.Petr3D) without a GPU -- the ABI minor and the refusals of the entry point it adds, the shipped config block builds it,
its state dict is the prefixed union of the three parts' (the reference's names and shapes), everything it does not implement says so, and -- with the three
parts replaced by recording fakes -- the sequencing of four frames with a scene change: scene token, prev_exists, reset_memory, the unwrapping of forward_test and
the shape of what simple_test returns."""
import ctypes
import json
import os
import re

import pytest
import torch
import torch.nn as nn

import toc3d_amd
from support import FakeNeck
from toc3d_amd import configs, lib, synth
from toc3d_amd.detector import Petr3D


def shipped_block():
    """The ``model=dict(type='Petr3D', ...)`` block of projects/configs/ToC3D/ToC3D_faster.py:35-166, key for key (num_frame_losses = 1, point_cloud_range and
    voxel_size substituted; the pts_bbox_head block is tests/test_cpu_head.py's, held to synth.head_cfg() there)."""
    point_cloud_range, voxel_size, num_frame_losses = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0], [0.2, 0.2, 8], 1
    return dict(
        type="Petr3D", num_frame_head_grads=num_frame_losses, num_frame_backbone_grads=num_frame_losses, num_frame_losses=num_frame_losses, use_grid_mask=True,
        img_backbone=dict(type="ToC3DEVAViT", img_size=320, patch_size=16, window_size=16, global_window_size=20, in_chans=3, embed_dim=1024, depth=24, num_heads=16,
                          mlp_ratio=4 * 2 / 3, global_attn_indexes=(2, 5, 8, 11, 14, 17, 20, 23), qkv_bias=True, drop_path_rate=0.3, use_act_checkpoint=True, xattn=False,
                          use_checkpoint=False, rope=True, rope_acc=True, pc_range=point_cloud_range, pruning_num_queries=64, pruning_loc=[6, 12, 18],
                          accelerate_global=True, token_ratio=[0.5, 0.4, 0.3],
                          token_selection_loss=dict(type="TokenSelectionLoss", semantic_loss=dict(type="GaussianFocalLoss", loss_weight=5.0))),
        img_neck=dict(type="CPFPN", in_channels=[1024], out_channels=256, num_outs=2),
        img_roi_head=dict(type="FocalHead", num_classes=10, in_channels=256, loss_cls2d=dict(type="QualityFocalLoss", use_sigmoid=True, beta=2.0, loss_weight=2.0),
                          loss_centerness=dict(type="GaussianFocalLoss", reduction="mean", loss_weight=1.0), loss_bbox2d=dict(type="L1Loss", loss_weight=5.0),
                          loss_iou2d=dict(type="GIoULoss", loss_weight=2.0), loss_centers2d=dict(type="L1Loss", loss_weight=10.0),
                          train_cfg=dict(assigner2d=dict(type="HungarianAssigner2D", cls_cost=dict(type="FocalLossCost", weight=2.),
                                                         reg_cost=dict(type="BBoxL1Cost", weight=5.0, box_format="xywh"),
                                                         iou_cost=dict(type="IoUCost", iou_mode="giou", weight=2.0), centers2d_cost=dict(type="BBox3DL1Cost", weight=10.0)))),
        pts_bbox_head=synth.head_cfg(),
        train_cfg=dict(pts=dict(grid_size=[512, 512, 1], voxel_size=voxel_size, point_cloud_range=point_cloud_range, out_size_factor=4,
                                assigner=dict(type="HungarianAssigner3D", cls_cost=dict(type="FocalLossCost", weight=2.0), reg_cost=dict(type="BBox3DL1Cost", weight=0.25),
                                              iou_cost=dict(type="IoUCost", weight=0.0), pc_range=point_cloud_range))))


def tiny(**over):
    return toc3d_amd.build_detector(dict(synth.detector_cfg(synth.DETECTOR_TINY), **over))


@pytest.fixture(scope="module")
def shipped():
    """The detector of the shipped block, built once (ViT-L on the CPU takes seconds); the tests that share it do not change it."""
    return toc3d_amd.build_detector(shipped_block())


# ---- the ABI: major 11, minor 1 -------------------------------------------------------------------------------------------------------------------------------
def test_abi_major_stays_and_the_minor_counts_the_added_entry_point():
    raw = open(lib.HEADER_PATH).read()
    assert int(re.search(r"#define\s+TOC3D_ABI_VERSION\s+(\d+)", raw).group(1)) == lib.ABI_VERSION == 11
    assert int(re.search(r"#define\s+TOC3D_ABI_MINOR\s+(\d+)", raw).group(1)) == lib.ABI_MINOR == 1
    l = lib.load()
    l.toc3d_abi_minor.restype = ctypes.c_int
    assert l.toc3d_abi_version() == 11 and l.toc3d_abi_minor() == 1
    assert "toc3d_neck_rows_fanout" in lib._SIGS and "toc3d_neck_rows_fanout" in lib.header_functions() and "toc3d_abi_minor" in lib.header_functions()
    note = raw[raw.index("#ifdef __cplusplus"):raw.index("#define TOC3D_ABI_MINOR")]
    assert "changed or removed" in note and "added" in note, "the header says which change moves which number"


def test_load_refuses_a_library_with_a_lower_minor_or_none(monkeypatch):
    class Old:                                             # a build from before the minor existed
        def __init__(self, minor):
            self.toc3d_abi_version = lambda: 11
            if minor is not None:
                self.toc3d_abi_minor = lambda: minor
    for minor in (None, 0):
        monkeypatch.setattr(lib, "_lib", None)
        monkeypatch.setattr(ctypes, "CDLL", lambda path, m=minor: Old(m))
        with pytest.raises(RuntimeError, match=r"ABI version 11\.[?0], this package binds ABI 11\.1 .*rebuild the library"):
            lib.load()
    monkeypatch.undo()
    assert lib.load().toc3d_abi_version() == 11


def fanout(dtype, x, ldx, nchw, rows, ld, V, T, C):
    l = lib.load()
    rc = l.toc3d_neck_rows_fanout(dtype, x, ldx, nchw, rows, ld, V, T, C, None)
    return rc, l.toc3d_last_error().decode()


def test_fanout_refusals_without_a_gpu():
    """Every refusal returns before a launch, so host pointers do: nothing is read or written through them."""
    buf = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(buf) + 127) & ~127             # 128-byte aligned
    x, nchw, rows = base, base + 1024, base + 2048
    ok = dict(dtype=lib.F32X3P, x=x, ldx=32, nchw=nchw, rows=rows, ld=64, V=1, T=1, C=32)
    call = lambda **over: fanout(**dict(ok, **over))
    for over, msg in ((dict(x=None), "null buffer"), (dict(nchw=None), "null buffer"), (dict(rows=None), "null buffer"),
                      (dict(ldx=31), "bad leading dimensions"), (dict(ld=0, dtype=lib.F32), "bad leading dimensions"), (dict(ld=31, dtype=lib.BF16), "bad leading dimensions"),
                      (dict(V=65536), "V <= 65535"), (dict(V=0), "bad dims"), (dict(T=0), "bad dims"), (dict(C=-1), "bad dims"), (dict(T=1 << 31), "bad dims"),
                      (dict(dtype=lib.F32X3), "bad dtype"), (dict(dtype=lib.F32X3W), "bad dtype"), (dict(dtype=99), "bad dtype"),
                      # planes rows: 128-byte aligned, leading dimension a multiple of 32
                      (dict(rows=rows + 64), "128-byte boundaries"), (dict(rows=rows + 4), "128-byte boundaries"), (dict(ld=48), "128-byte boundaries"),
                      (dict(ld=36), "128-byte boundaries")):
        rc, err = call(**over)
        assert rc == -1 and err.startswith("toc3d_neck_rows_fanout:") and msg in err, (over, rc, err)
    with pytest.raises(RuntimeError, match=r"toc3d_neck_rows_fanout failed \(-1\): toc3d_neck_rows_fanout: null buffer"):
        lib.call("toc3d_neck_rows_fanout", lib.F32, None, 32, None, None, 32, 1, 1, 32, None)


# ---- construction -------------------------------------------------------------------------------------------------------------------------------------------
def test_shipped_config_block_builds_unchanged(shipped):
    assert shipped_block() == synth.detector_cfg(), "synth.detector_cfg() is the shipped block"
    det = shipped
    assert isinstance(det, Petr3D) and not det.training and toc3d_amd.DETECTORS.get("Petr3D") is Petr3D and "Petr3D" in toc3d_amd.__all__
    assert type(det.img_backbone).__name__ == "ToC3DEVAViT" and type(det.img_neck).__name__ == "CPFPN" and type(det.pts_bbox_head).__name__ == "StreamPETRHead"
    assert det.img_backbone.precision == det.img_neck.precision == det.pts_bbox_head.precision == "fp32x3"
    assert det.query_backbone_selection and det.use_grid_mask and det.aux_2d_only and det.stride == 16 and det.position_level == 0 and det.prev_scene_token is None
    assert det.pts_bbox_head.train_cfg is None and det.pts_bbox_head.test_cfg is None            # MVXTwoStageDetector hands the head the pts slice; the head keeps none at eval
    assert not hasattr(det, "img_roi_head") and det.forward_roi_head(None) == {"topk_indexes": None}
    # every keyword of petr3d.py:27-55, and precision, which reaches the three parts
    every = dict(use_grid_mask=False, pts_voxel_layer=None, pts_voxel_encoder=None, pts_middle_encoder=None, pts_fusion_layer=None, pts_backbone=None, pts_neck=None,
                 img_rpn_head=None, test_cfg=dict(pts=dict(max_per_img=300)), num_frame_head_grads=2, num_frame_backbone_grads=2, num_frame_losses=2, stride=16,
                 position_level=0, aux_2d_only=True, single_test=True, pretrained=None, token_select_vis=False, vis_num_sample=20, vis_start_id=0,
                 vis_out_path="./token_vis", test_time_print=True, precision="bf16")
    d2 = tiny(**every)
    assert d2.img_backbone.precision == d2.img_neck.precision == d2.pts_bbox_head.precision == d2.pts_bbox_head._tokens.precision == "bf16"
    assert d2.pts_bbox_head.test_cfg == dict(max_per_img=300) and d2.single_test
    dense = tiny(img_backbone=dict(configs.EVA_TINY))
    assert type(dense.img_backbone).__name__ == "EVA_ViT" and not dense.query_backbone_selection


def test_what_is_not_implemented_says_so():
    for over in (dict(aux_2d_only=False), dict(token_select_vis=True), dict(position_level=1), dict(pts_backbone=dict(type="SECOND")), dict(img_rpn_head=dict(type="RPN")),
                 dict(img_roi_head=dict(type="YOLOXHeadCustom")), dict(precision="fp32")):
        with pytest.raises(NotImplementedError):
            tiny(**over)
    with pytest.raises(ValueError, match="out_channels 32 != the head's in_channels 256"):
        tiny(pts_bbox_head=synth.head_cfg())
    # backbones and necks other than this package's are refused at construction
    class Other(nn.Module):
        def __init__(self, **kw):
            super().__init__()
    from toc3d_amd import registry                     # (the registries the builders use now)
    registry.BACKBONES.register_module(name="_OtherBackbone", module=Other)
    registry.NECKS.register_module(name="_OtherNeck", module=Other)
    try:
        with pytest.raises(NotImplementedError, match="this package's EVA_ViT / ToC3DEVAViT, CPFPN and StreamPETRHead only"):
            tiny(img_backbone=dict(type="_OtherBackbone"))
        with pytest.raises(NotImplementedError, match="CPFPN and StreamPETRHead only"):
            tiny(img_neck=dict(type="_OtherNeck", out_channels=32))
    finally:
        registry.BACKBONES.module_dict.pop("_OtherBackbone", None)
        registry.NECKS.module_dict.pop("_OtherNeck", None)
    det = tiny()
    with pytest.raises(NotImplementedError, match="training mode"):
        det.train()
    assert not det.training and det.eval() is det
    with pytest.raises(NotImplementedError, match="forward_train"):
        det.forward_train(img_metas=None)
    with pytest.raises(NotImplementedError, match="return_loss=True"):
        det(img_metas=[[]], img=[torch.zeros(1)])
    with pytest.raises(NotImplementedError, match="return_loss=True"):
        det.forward(return_loss=True)
    with pytest.raises(RuntimeError, match="no CPU"):
        det.extract_img_feat(torch.zeros(1, 6, 3, 320, 800), prev_exists=False, ego_pose_inv=torch.eye(4)[None])


# ---- state dict ---------------------------------------------------------------------------------------------------------------------------------------------
def union_spec(golden_dir, backbone="toc3d_faster", head="full", neck=configs.CPFPN_CFG):
    spec = {"img_backbone." + k: v for k, v in json.load(open(os.path.join(golden_dir, "state_dict_spec.json")))[backbone].items()}
    cin, cout = neck["in_channels"][0], neck["out_channels"]
    spec.update({"img_neck.lateral_convs.0.conv.weight": [cout, cin, 1, 1], "img_neck.lateral_convs.0.conv.bias": [cout],
                 "img_neck.fpn_convs.0.conv.weight": [cout, cout, 3, 3], "img_neck.fpn_convs.0.conv.bias": [cout]})
    spec.update({"pts_bbox_head." + k: v for k, v in json.load(open(os.path.join(golden_dir, "head_state_dict_spec.json")))[head].items()})
    return spec


def test_state_dict_is_the_prefixed_union_of_the_parts(golden_dir, shipped):
    spec = union_spec(golden_dir)
    assert len(spec) == 620 + 4 + 251
    det = shipped
    got = {k: list(v.shape) for k, v in det.state_dict().items()}
    assert got == spec, (sorted(set(got) ^ set(spec))[:8], [k for k in got if k in spec and got[k] != spec[k]][:8])
    assert not any(k.startswith(("img_roi_head.", "grid_mask.")) for k in got)
    # the tiny detector: the tiny backbone's and neck's names; the head's at its own sizes
    t = {k: list(v.shape) for k, v in tiny().state_dict().items()}
    ts = union_spec(golden_dir, "toc3d_tiny", "tiny", configs.CPFPN_TINY)
    assert set(t) == set(ts) and all(t[k] == ts[k] for k in t if not k.startswith("pts_bbox_head."))
    assert {k: list(v.shape) for k, v in synth.detector_state_dict(synth.DETECTOR_TINY).items()} == t


def test_load_state_dict_forgives_the_roi_head_and_nothing_else():
    det = tiny()
    sd = synth.detector_state_dict(synth.DETECTOR_TINY)
    det.prev_scene_token = "a"
    assert str(det.load_state_dict(sd, strict=True)) == "<All keys matched successfully>"
    assert det.prev_scene_token is None, "new weights: the scene starts over"
    assert all(torch.equal(v, sd[k]) for k, v in det.state_dict().items())
    with_roi = dict(sd, **{"img_roi_head.x": torch.zeros(3), "img_roi_head.cls.weight": torch.zeros(10, 256, 1, 1)})
    res = det.load_state_dict(with_roi, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    with pytest.raises(RuntimeError, match=r'Unexpected key\(s\) in state_dict: "pts_bbox_head.y"'):
        det.load_state_dict(dict(with_roi, **{"pts_bbox_head.y": torch.zeros(1)}), strict=True)
    with pytest.raises(RuntimeError, match="Unexpected key"):
        det.load_state_dict(dict(sd, **{"img_roi_headx.w": torch.zeros(1)}), strict=True)
    short = dict(sd)
    short.pop("img_neck.fpn_convs.0.conv.bias")
    with pytest.raises(RuntimeError, match="Missing key"):
        det.load_state_dict(short, strict=True)
    # derived state belongs to the parts and goes with a move as well
    det.prev_scene_token = "a"
    det.pts_bbox_head.__dict__["_bank"] = object()
    det.to("cpu")
    assert det.prev_scene_token is None and det.pts_bbox_head._bank is None
    det.prev_scene_token = "a"
    det.init_weights()
    assert det.prev_scene_token is None


# ---- sequencing, on recording fakes ----------------------------------------------------------------------------------------------------------------------------
class FakeBackbone(nn.Module):
    pruning_loc, pruning_num_queries = [3, 6, 9], 64

    def __init__(self, log):
        super().__init__()
        self.log = log

    def forward(self, x, **kw):
        self.log.append(("backbone", tuple(x.shape), kw["prev_exists"], tuple(kw["temp_queries"].shape), tuple(kw["ego_pose_inv"].shape), kw.get("gumbel_noise")))
        feats = torch.zeros(x.shape[0], 8, 2, 5)
        return toc3d_amd.ToC3DViTReturnType({"last_feat": feats}, ["m0", "m1", "m2"], None, ["k0", "k1", "k2"], ["d0", "d1", "d2"])


class FakeHead(nn.Module):
    embed_dims = 256

    def __init__(self, log):
        super().__init__()
        self.log, self.bank, self.rows = log, None, {}

    def backbone_queries(self, n, prev_exists, batch_size=1):
        self.log.append(("queries", n, prev_exists, batch_size, self.bank))
        mid = bool(prev_exists) and self.bank is not None
        return dict(temp_queries=torch.zeros(batch_size, n, 256), temp_ref_points=None, temp_timestamp=None, temp_ego_pose=None, temp_vel=None, prev_exists=mid)

    def img_feats_rows_buffer(self, B, N, h, w, device=None):
        return self.rows.setdefault((B, N, h, w), "rows(%d,%d,%d,%d)" % (B, N, h, w)), 64, lib.F32X3P       # one buffer per shape, as the workspace is

    def reset_memory(self):
        self.log.append(("reset",))
        self.bank = None

    def forward(self, memory_center, img_metas, topk_indexes=None, img_feats_rows=False, **data):
        self.log.append(("head", topk_indexes, img_feats_rows, sorted(data), data["prev_exists"].tolist(), tuple(data["img_feats"].shape), tuple(data["intrinsics"].shape),
                         tuple(data["timestamp"].shape)))
        self.bank = "bank%d" % len(self.log)
        return dict(all_cls_scores="cls", all_bbox_preds="box", dn_mask_dict=None)

    def get_bboxes(self, outs, img_metas, rescale=False):
        self.log.append(("get_bboxes", outs["all_cls_scores"], len(img_metas)))
        return [[torch.zeros(3, 9), torch.arange(3.0), torch.arange(3)]]


def test_sequencing_over_four_frames_with_a_scene_change():
    det, log = tiny(), []
    det.img_backbone, det.img_neck, det.pts_bbox_head = FakeBackbone(log), FakeNeck(log), FakeHead(log)
    scenes = ["a", "a", "a", "b"]
    for f, scene in enumerate(scenes):
        del log[:]
        metas = [[dict(scene_token=scene, pad_shape=[(32, 80, 3)])]]
        wrap = lambda t: [[t]]                              # the nested lists of the test-time pipeline (petr3d.py:514-518)
        out = det(return_loss=False, img_metas=metas, rescale=True, img=[torch.zeros(1, 6, 3, 32, 80)], intrinsics=wrap(torch.zeros(6, 4, 4)),
                  lidar2img=wrap(torch.zeros(6, 4, 4)), timestamp=wrap(torch.zeros((), dtype=torch.float64)), ego_pose=wrap(torch.eye(4)), ego_pose_inv=wrap(torch.eye(4)),
                  gumbel_noise="noise" if f == 1 else None)
        prev = f in (1, 2)
        names = [e[0] for e in log]
        assert names == ["queries", "backbone", "neck"] + ([] if prev else ["reset"]) + ["head", "get_bboxes"], (f, names)
        # prev_exists: decided by the scene token before the backbone runs (:546-549), a Python bool all the way; the bank it reads is the previous frame's
        q, bb, nk, hd = log[0], log[1], log[2], log[-2]
        assert q[1:4] == (64, prev, 1) and type(q[2]) is bool and (q[4] is not None) == (f > 0)
        assert bb[1] == (6, 3, 32, 80) and bb[2] is prev and bb[3] == (1, 64, 256) and bb[4] == (1, 4, 4) and bb[5] == ("noise" if f == 1 else None)
        # the neck fans out into the head's own rows buffer for this (B, N, h, w)
        assert nk[1:] == ((6, 8, 2, 5), "rows(1,6,2,5)", 64, lib.F32X3P)
        # the head: topk_indexes None, on the rows, prev_exists as the reference's tensor, every data key unwrapped to a leading 1
        assert hd[1] is None and hd[2] is True and hd[4] == [1.0 if prev else 0.0] and hd[5] == (1, 6, 4, 2, 5) and hd[6] == (1, 6, 4, 4) and hd[7] == (1,)
        assert hd[3] == sorted(["img", "img_feats", "intrinsics", "lidar2img", "timestamp", "ego_pose", "ego_pose_inv", "prev_exists"])
        assert det.prev_scene_token == scene
        # [dict(pts_bbox=dict(boxes_3d, scores_3d, labels_3d))] on the CPU
        assert isinstance(out, list) and len(out) == 1 and list(out[0]) == ["pts_bbox"] and set(out[0]["pts_bbox"]) == {"boxes_3d", "scores_3d", "labels_3d"}
        assert tuple(out[0]["pts_bbox"]["boxes_3d"].shape) == (3, 9) and out[0]["pts_bbox"]["labels_3d"].tolist() == [0, 1, 2]
        assert det.last_frame["keep_idxes"] == ["k0", "k1", "k2"] and det.last_frame["token_masks"] == ["m0", "m1", "m2"]
    # extract_img_feat returns the reference's five; a tensor it did not return goes to the head without the rows flag
    del log[:]
    feats, masks, attn, keep, drop = det.extract_img_feat(torch.zeros(1, 6, 3, 32, 80), 1, prev_exists=True, ego_pose_inv=torch.eye(4)[None])
    assert tuple(feats.shape) == (1, 6, 4, 2, 5) and masks == ["m0", "m1", "m2"] and attn is None and keep == ["k0", "k1", "k2"] and drop == ["d0", "d1", "d2"]
    assert det.extract_img_feat(None) == (None, None, None, None, None)
    assert tuple(det.prepare_location([dict(pad_shape=[(32, 80, 3)])], img_feats=feats).shape) == (6, 2, 5, 2)
    data = dict(img=torch.zeros(1, 6, 3, 32, 80), intrinsics=torch.zeros(1, 6, 4, 4), lidar2img=torch.zeros(1, 6, 4, 4), timestamp=torch.zeros(1, dtype=torch.float64))
    det.simple_test_pts([dict(scene_token="b", pad_shape=[(32, 80, 3)])], img_feats=feats.clone(), **data)
    assert log[-2][0] == "head" and log[-2][2] is False and log[-2][4] == [1.0]
    det.extract_img_feat(torch.zeros(1, 6, 3, 32, 80), 1, prev_exists=True, ego_pose_inv=torch.eye(4)[None])
    det.simple_test_pts([dict(scene_token="b", pad_shape=[(32, 80, 3)])], img_feats=feats, **data)
    assert log[-2][2] is False, "an older tensor of extract_img_feat is not the one whose rows sit in the workspace"
    newest, *_ = det.extract_img_feat(torch.zeros(1, 6, 3, 32, 80), 1, prev_exists=True, ego_pose_inv=torch.eye(4)[None])
    det.pts_bbox_head.rows.clear()                          # the head alone got new weights: its workspace is another buffer now
    det.simple_test_pts([dict(scene_token="b", pad_shape=[(32, 80, 3)])], img_feats=newest, **data)
    assert log[-2][2] is False
    newest, *_ = det.extract_img_feat(torch.zeros(1, 6, 3, 32, 80), 1, prev_exists=True, ego_pose_inv=torch.eye(4)[None])
    det.simple_test_pts([dict(scene_token="b", pad_shape=[(32, 80, 3)])], img_feats=newest, **data)
    assert log[-2][2] is True
