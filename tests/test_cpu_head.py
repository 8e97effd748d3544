"""CPU: the assembled head (toc3d_amd.StreamPETRHead) without a GPU -- the shipped config block builds it, its state dict is the reference's
(tests/golden/head_state_dict_spec.json, read off the reference's own modules by tools/gen_golden_head_e2e.py), it is registered under the reference's type
name, everything it does not implement says so, and copies / moves drop the derived state."""
import copy
import json
import os
import pickle

import pytest
import torch

import toc3d_amd
from toc3d_amd import synth
from toc3d_amd.head import StreamPETRHead

TINY = synth.HEAD_TINY


def shipped_block():
    """The ``pts_bbox_head=dict(...)`` block of projects/configs/ToC3D/ToC3D_faster.py:96-154, key for key (point_cloud_range and voxel_size substituted)."""
    point_cloud_range, voxel_size = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0], [0.2, 0.2, 8]
    return dict(
        type="StreamPETRHead", num_classes=10, in_channels=256, num_query=644, memory_len=1024, topk_proposals=256, num_propagated=256, with_ego_pos=True,
        match_with_velo=False, scalar=10, noise_scale=1.0, dn_weight=1.0, split=0.75, LID=True, with_position=True,
        position_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], code_weights=[2.0, 2.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0],
        transformer=dict(type="PETRTemporalTransformer", decoder=dict(
            type="PETRTransformerDecoder", return_intermediate=True, num_layers=6, transformerlayers=dict(
                type="PETRTemporalDecoderLayer",
                attn_cfgs=[dict(type="MultiheadAttention", embed_dims=256, num_heads=8, dropout=0.1), dict(type="PETRMultiheadAttention", embed_dims=256, num_heads=8, dropout=0.1)],
                feedforward_channels=2048, ffn_dropout=0.1, with_cp=True, operation_order=("self_attn", "norm", "cross_attn", "norm", "ffn", "norm")))),
        bbox_coder=dict(type="NMSFreeCoder", post_center_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], pc_range=point_cloud_range, max_num=300, voxel_size=voxel_size,
                        num_classes=10),
        loss_cls=dict(type="FocalLoss", use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=2.0), loss_bbox=dict(type="L1Loss", loss_weight=0.25),
        loss_iou=dict(type="GIoULoss", loss_weight=0.0))


@pytest.fixture(scope="module")
def spec(golden_dir):
    return json.load(open(os.path.join(golden_dir, "head_state_dict_spec.json")))


def tiny(**over):
    return toc3d_amd.build_head(dict(synth.head_cfg(TINY), **over))


def test_shipped_config_block_builds_unchanged():
    cfg = shipped_block()
    assert cfg == synth.head_cfg(), "synth.head_cfg() is the shipped block"
    h = toc3d_amd.build_head(cfg)
    assert isinstance(h, StreamPETRHead) and h.precision == toc3d_amd.gemm.DEFAULT_PRECISION == "fp32x3" and h._tokens.precision == "fp32x3"
    assert (h.num_query, h.memory_len, h.topk_proposals, h.num_propagated, h.num_pred, h.code_size, h.cls_out_channels) == (644, 1024, 256, 256, 6, 10, 10)
    assert h.transformer.num_layers == 6 and h.bbox_coder.max_num == 300 and h.test_cfg == dict(max_per_img=100) and h.train_cfg is None
    assert h.pc_range.tolist() == pytest.approx(cfg["bbox_coder"]["pc_range"]) and h.code_weights.tolist() == cfg["code_weights"] == h.match_costs.tolist()
    # every keyword of the reference's __init__, the training-only ones included, is accepted
    extra = dict(stride=16, embed_dims=256, num_reg_fcs=2, with_dn=True, match_costs=[1.0] * 10, sync_cls_avg_factor=True, depth_step=0.8, depth_num=64, depth_start=1,
                 noise_trans=0.0, init_cfg=None, normedlinear=False, code_size=10, test_cfg=dict(max_per_img=300),
                 train_cfg=dict(assigner=dict(type="HungarianAssigner3D", cls_cost=dict(type="FocalLossCost", weight=2.0))))
    h2 = toc3d_amd.build_head(dict(synth.head_cfg(TINY), **extra), precision="bf16", launch_mode="eager", levels="last")
    assert h2.test_cfg == dict(max_per_img=300) and h2.match_costs.tolist() == [1.0] * 10
    assert (h2.precision, h2.transformer.precision, h2._outputs.precision, h2._queries.precision, h2._tokens.precision) == ("bf16",) * 5
    assert h2._outputs.levels == "last" and h2._outputs.launch_mode == h2._queries.launch_mode == h2.transformer.launch_mode == "eager"


@pytest.mark.parametrize("tag,sizes", [("full", None), ("tiny", TINY)])
def test_state_dict_is_the_references(spec, tag, sizes):
    h = toc3d_amd.build_head(synth.head_cfg(sizes))
    got = {k: list(v.shape) for k, v in h.state_dict().items()}
    assert got == spec[tag], (sorted(set(got) ^ set(spec[tag])), [k for k in got if k in spec[tag] and got[k] != spec[tag][k]])
    sd = synth.head_state_dict(sizes)
    assert {k: list(v.shape) for k, v in sd.items()} == spec[tag]
    assert str(h.load_state_dict(sd, strict=True)) == "<All keys matched successfully>"
    back = h.state_dict()
    assert all(torch.equal(back[k], sd[k]) for k in sd)
    # one set of tensors: the modules that run the steps hold the head's Parameter objects, and nothing twice
    assert h._tokens.position_encoder[0].weight is h.position_encoder[0].weight and h._queries.ego_pose_pe.gamma.weight is h.ego_pose_pe.gamma.weight
    assert h._outputs.cls_branches[5][6].bias is h.cls_branches[0][6].bias and h._queries.reference_points.weight is h.reference_points.weight
    assert len({id(p) for p in h.parameters()}) == len(list(h.parameters()))
    # the token kernel's depth bins are the head's coords_d parameter, bound once; the token module's own state dict did not grow by it
    assert h._tokens._coords_d_owner is h.coords_d and "coords_d" not in h._tokens.state_dict() and not any("owner" in k for k in h._tokens.state_dict())
    assert [n for n, p in h.named_parameters() if n in ("code_weights", "match_costs", "pc_range", "position_range", "coords_d") and not p.requires_grad] == \
        ["code_weights", "match_costs", "pc_range", "position_range", "coords_d"]
    # ... under a detector's prefix as well
    det = torch.nn.Module()
    det.pts_bbox_head = h
    assert str(det.load_state_dict({"pts_bbox_head." + k: v for k, v in sd.items()}, strict=True)) == "<All keys matched successfully>"


def test_old_style_keys_load():
    """streampetr_head.py:547-562: checkpoints from before version 2 name the attentions ``self_attn`` / ``multihead_attn`` and the last norm ``decoder.norm``."""
    sd = synth.head_state_dict(TINY)
    old = {}
    for k, v in sd.items():
        k = k.replace(".attentions.0.", ".self_attn.").replace(".attentions.1.", ".multihead_attn.").replace(".decoder.post_norm.", ".decoder.norm.")
        old["pts_bbox_head." + k] = v
    assert any(".self_attn." in k for k in old) and any(".multihead_attn." in k for k in old) and any(".decoder.norm." in k for k in old)
    det = torch.nn.Module()
    det.pts_bbox_head = tiny()
    assert str(det.load_state_dict(old, strict=True)) == "<All keys matched successfully>"
    back = det.pts_bbox_head.state_dict()
    assert all(torch.equal(back[k], sd[k]) for k in sd)
    # a state dict this version saved carries version 2 and is not renamed: its (new-style) keys load, old-style ones would be unexpected
    saved = det.state_dict()
    assert saved._metadata["pts_bbox_head"]["version"] == 2
    det.load_state_dict(saved, strict=True)
    renamed = type(saved)((k.replace(".attentions.0.", ".self_attn."), v) for k, v in saved.items())
    renamed._metadata = saved._metadata
    with pytest.raises(RuntimeError, match="Unexpected key"):
        det.load_state_dict(renamed, strict=True)
    # the ranges the kernels take from the config must be the checkpoint's
    bad = dict(sd, pc_range=sd["pc_range"] * 2)
    with pytest.raises(RuntimeError, match="differs from the config"):
        tiny().load_state_dict(bad)
    with pytest.raises(RuntimeError, match="position_range"):
        tiny().load_state_dict(dict(sd, position_range=sd["position_range"] * 1.05))
    # ... the same geometry rounded by a half / bf16 checkpoint is not a different one
    rounded = dict(sd, pc_range=sd["pc_range"].bfloat16().float(), position_range=sd["position_range"].half().float())
    assert not torch.equal(rounded["pc_range"], sd["pc_range"])
    tiny().load_state_dict(rounded, strict=True)


def test_registered_under_the_references_name():
    assert toc3d_amd.HEADS.get("StreamPETRHead") is StreamPETRHead is toc3d_amd.StreamPETRHead
    assert {"StreamPETRHead", "HEADS", "build_head"} <= set(toc3d_amd.__all__)
    h = toc3d_amd.build_head(synth.head_cfg(TINY), precision="bf16")
    assert type(h) is StreamPETRHead and h.precision == "bf16"
    assert type(h.transformer) is toc3d_amd.PETRTemporalTransformer and type(h.bbox_coder) is toc3d_amd.NMSFreeCoder and h._outputs.bbox_coder is h.bbox_coder


@pytest.mark.parametrize("over,match", [
    (dict(precision="fp32"), "precision 'fp32' is not implemented"), (dict(precision="fp32x6"), "precision 'fp32x6' is not implemented"),
    (dict(normedlinear=True), "normedlinear=True"), (dict(num_reg_fcs=3), "num_reg_fcs=3"), (dict(embed_dims=128), "embed_dims"),
    (dict(loss_cls=dict(type="CrossEntropyLoss", use_sigmoid=False)), "softmax classifier"),
    (dict(loss_cls=None), "softmax classifier"),              # the reference's default loss_cls has no use_sigmoid: num_classes + 1 outputs
    (dict(transformer=dict(synth.decoder_cfg(), encoder=dict(type="x"))), "an encoder"),
    (dict(levels="first"), "levels='first'"), (dict(code_size=9), "code_size=9"),
])
def test_what_is_not_implemented_says_so(over, match):
    with pytest.raises(NotImplementedError, match=match):
        tiny(**over)


def test_refusals_at_call_time():
    h = tiny().eval()
    inp = synth.head_inputs(TINY, synth.HEAD_TINY_SHAPE)
    data, metas = inp["frames"][0], inp["img_metas"]
    with pytest.raises(NotImplementedError, match="topk_indexes"):
        h(None, metas, torch.zeros(2, 5, 1, dtype=torch.int64), **data)
    with pytest.raises(RuntimeError, match="CUDA/HIP"):                    # no CPU path: the token module's error, before anything is allocated
        h(None, metas, None, **data)
    assert h._bank is None and h.memory_embedding is None and h.memory_velo is None
    with pytest.raises(RuntimeError, match="no CPU path"):                 # ... and the bank's, for the memory methods and the backbone's slice
        h.pre_update_memory(data)
    with pytest.raises(RuntimeError, match="no CPU path"):
        h.backbone_queries(8, False, batch_size=2)
    h.train()
    with pytest.raises(RuntimeError, match="training mode"):
        h(None, metas, None, **data)
    with pytest.raises(ValueError, match="needs transformer="):
        StreamPETRHead(num_classes=10)


def test_copies_and_moves_drop_the_derived_state():
    h = tiny()
    h.load_state_dict(synth.head_state_dict(TINY))
    parts = (h, h._tokens, h._queries, h._outputs, h.transformer)
    marker = object()

    def dirty():
        h._bank = marker
        for p in parts[1:]:
            p._packed = marker
        h._queries._fresh = marker

    def clean(x):
        return x._bank is None and all(p._packed is None for p in (x._tokens, x._queries, x._outputs, x.transformer)) and x._queries._fresh is None
    dirty()
    c = copy.deepcopy(h)
    assert clean(c) and not clean(h), "a copy starts without derived state; the original keeps its own"
    assert c._tokens.position_encoder is c.position_encoder and c.position_encoder is not h.position_encoder and c._outputs.bbox_coder is c.bbox_coder
    assert c._tokens._coords_d_owner is c.coords_d and c.coords_d is not h.coords_d
    assert all(torch.equal(a, b) for a, b in zip(c.state_dict().values(), h.state_dict().values()))
    p = pickle.loads(pickle.dumps(h))
    assert clean(p) and p._queries.reference_points is p.reference_points and p._outputs.cls_branches is p.cls_branches and p._tokens._coords_d_owner is p.coords_d
    assert h.to("cpu") is h and clean(h)
    dirty()
    h.load_state_dict(synth.head_state_dict(TINY, seed=1))
    assert clean(h)
    dirty()
    h.reset_memory()
    assert h._bank is None and h._tokens._packed is marker, "reset_memory drops the bank alone"
    dirty()
    h.init_weights()
    assert clean(h) and not h.pseudo_reference_points.weight.requires_grad
