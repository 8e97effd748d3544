"""CPU: the host side of toc3d_amd.HeadOutputs / toc3d_amd.NMSFreeCoder (state-dict names, aliasing of the levels, documented exceptions, registry) and the
plain-torch restatement of branches + decoding (tests/head_outputs_cases.py) that pins tests/golden/head_outputs_*.npz -- output of the REAL reference (tools/gen_golden_head_outputs.py) -- to
something checkable where the reference does not exist.  tests/test_gpu_head_outputs.py uses the same restatement as its control."""
import json
import os

import numpy as np
import pytest
import torch

import toc3d_amd
from head_outputs_cases import group_errors, restated_branches, restated_decode, rows_without_inf
from support import rel_max
from toc3d_amd import synth


# ---- module surface ---------------------------------------------------------------------------------------------------------------------------
def test_state_dict_names_order_shapes_and_strict_load(golden_dir):
    spec = json.load(open(os.path.join(golden_dir, "head_outputs_state_dict_spec.json")))
    for tag, sizes in (("tiny", synth.HEAD_OUTPUTS_TINY), ("full", synth.HEAD_OUTPUTS_FULL)):
        m = toc3d_amd.HeadOutputs(**sizes)
        assert {k: list(v.shape) for k, v in m.state_dict().items()} == spec[tag]
        assert list(m.state_dict()) == list(spec[tag])                                  # the reference's order too
        sd = synth.head_outputs_state_dict(sizes)
        res = m.load_state_dict(sd, strict=True)
        assert not res.missing_keys and not res.unexpected_keys
        assert all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())
    assert len(spec["full"]) == 96 and spec["full"]["cls_branches.5.6.weight"] == [10, 256] and spec["full"]["reg_branches.0.4.weight"] == [10, 256]
    assert "cls_branches.3.4.bias" in spec["full"] and "reg_branches.5.2.bias" in spec["full"] and "reg_branches.0.1.weight" not in spec["full"]


def test_the_levels_alias_one_module_as_in_the_reference():
    m = toc3d_amd.HeadOutputs(**synth.HEAD_OUTPUTS_FULL)
    assert len(m.cls_branches) == len(m.reg_branches) == 6
    assert all(b is m.cls_branches[0] for b in m.cls_branches) and all(b is m.reg_branches[0] for b in m.reg_branches)
    assert len(list(m.parameters())) == 16                                              # one copy: 5 x 2 class-tower tensors, 3 x 2 box-tower tensors
    # torch's behaviour for shared modules: a checkpoint whose levels disagree loads, and the last level's tensors are the ones kept
    sd = dict(synth.head_outputs_state_dict(synth.HEAD_OUTPUTS_FULL))
    sd["cls_branches.5.6.bias"] = sd["cls_branches.5.6.bias"] + 1.0
    m.load_state_dict(sd, strict=True)
    assert torch.equal(m.cls_branches[0][6].bias, sd["cls_branches.5.6.bias"])
    m.init_weights()
    assert torch.allclose(m.cls_branches[2][6].bias, torch.full((10,), -4.59512))       # bias_init_with_prob(0.01)


@pytest.mark.parametrize("over,what", [(dict(normedlinear=True), "NormedLinear"), (dict(num_reg_fcs=3), "num_reg_fcs=3"), (dict(levels="first"), "levels='first'"),
                                       (dict(embed_dims=100), "embed_dims=100"), (dict(embed_dims=1024), "64 KB of LDS"), (dict(code_size=9), "code_size=9")])
def test_configs_outside_the_family_are_refused(over, what):
    with pytest.raises(NotImplementedError, match="not implemented") as e:
        toc3d_amd.HeadOutputs(**dict(synth.HEAD_OUTPUTS_FULL, **over))
    assert what in str(e.value)


@pytest.mark.parametrize("precision", ["fp32", "fp32x6"])
def test_other_precisions_name_the_two_that_work(precision):
    with pytest.raises(NotImplementedError, match="'bf16' or 'fp32x3'"):
        toc3d_amd.HeadOutputs(precision=precision, **synth.HEAD_OUTPUTS_FULL)
    assert toc3d_amd.HeadOutputs().precision == "fp32x3" and toc3d_amd.HeadOutputs().levels == "all"


def test_cpu_tensors_and_missing_pieces_raise_the_documented_exceptions():
    sizes, shape = synth.HEAD_OUTPUTS_TINY, synth.HEAD_OUTPUTS_TINY_SHAPE
    m = toc3d_amd.HeadOutputs(**sizes)
    inp = synth.head_outputs_inputs(sizes, shape)
    with pytest.raises(RuntimeError, match="no CPU"):
        m(inp["outs_dec"], inp["reference_points"])
    with pytest.raises(ValueError, match="do not fit embed_dims=64"):          # the shapes are checked before the device
        m(inp["outs_dec"], inp["reference_points"][:, :5])
    preds = dict(all_cls_scores=torch.zeros(1, 2, 32, 10), all_bbox_preds=torch.zeros(1, 2, 32, 10))
    with pytest.raises(RuntimeError, match="needs a bbox_coder"):
        m.get_bboxes(preds)
    with pytest.raises(NotImplementedError, match="only support post_center_range is not None"):          # the reference's own refusal (nms_free_coder.py:86-89)
        toc3d_amd.NMSFreeCoder(pc_range=synth.PC_RANGE).decode(preds)
    coder = toc3d_amd.build_bbox_coder(synth.bbox_coder_cfg(max_num=20))
    with pytest.raises(RuntimeError, match="no CPU"):
        coder.decode(preds)
    with pytest.raises(ValueError, match="num_classes=10"):
        coder.decode_fixed(torch.zeros(2, 32, 7), torch.zeros(2, 32, 10))


def test_registry_builds_the_coder_from_the_shipped_config():
    cfg = dict(type="NMSFreeCoder", post_center_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0],              # projects/configs/ToC3D/ToC3D_faster.py:140-146, verbatim
               pc_range=[-51.2, -51.2, -5.0, 51.2, 51.2, 3.0], max_num=300, voxel_size=[0.2, 0.2, 8], num_classes=10)
    assert "NMSFreeCoder" in toc3d_amd.BBOX_CODERS.module_dict
    c = toc3d_amd.build_bbox_coder(cfg)
    assert isinstance(c, toc3d_amd.NMSFreeCoder) and (c.max_num, c.num_classes, c.score_threshold) == (300, 10, None)
    assert c.post_center_range == cfg["post_center_range"] and c.pc_range == cfg["pc_range"] and c.voxel_size == [0.2, 0.2, 8]
    assert cfg == synth.bbox_coder_cfg()                                                  # the seeded config maker hands out the same block
    m = toc3d_amd.HeadOutputs(bbox_coder=cfg, pc_range=cfg["pc_range"], **synth.HEAD_OUTPUTS_FULL)
    assert isinstance(m.bbox_coder, toc3d_amd.NMSFreeCoder) and m.bbox_coder.max_num == 300 and m.pc_range == cfg["pc_range"]
    assert toc3d_amd.NMSFreeCoder(pc_range=cfg["pc_range"]).max_num == 100                # the reference's defaults


# ---- the restatement against the reference's fixtures ------------------------------------------------------------------------------------------
def test_restatement_reproduces_the_tiny_fixture(golden_dir):
    """<= 1e-5 relative (max-abs error / max-abs reference) per output group, the bound SURVEY.md section 8d sets for restatements; nan_to_num exactly; the decode of
    the last level through the narrowed post_center_range with the reference's index lists exactly."""
    g = np.load(os.path.join(golden_dir, "head_outputs_tiny.npz"))
    sizes, shape = synth.HEAD_OUTPUTS_TINY, synth.HEAD_OUTPUTS_TINY_SHAPE
    inp = synth.head_outputs_inputs(sizes, shape)
    assert torch.isnan(inp["outs_dec"]).sum() == 3 and torch.isinf(inp["outs_dec"]).sum() == 2 and torch.isfinite(inp["outs_dec"][-1]).sum() == inp["outs_dec"][-1].numel() - 2
    with torch.no_grad():
        clean, cls, box = restated_branches(synth.head_outputs_state_dict(sizes), inp)
    assert clean.shape == (2, 2, 32, 64) == g["outs_dec"].shape and cls.shape == (2, 2, 32, 10) == g["all_cls_scores"].shape == box.shape
    assert np.array_equal(clean.numpy(), g["outs_dec"]) and np.isfinite(g["outs_dec"]).all() and np.abs(g["outs_dec"]).max() == np.finfo(np.float32).max
    rows = rows_without_inf(inp)
    assert int((~rows).sum()) == 2 and bool(rows[-1].all())
    errs = group_errors(cls, box, g["all_cls_scores"], g["all_bbox_preds"], rows)
    print({k: f"{e:.2e}" for k, e in errs.items()})
    assert max(errs.values()) <= 1e-5, errs
    pcr, K = g["post_center_range"].tolist(), int(g["max_num"])
    for b in range(2):
        bb, sc, lb, idx, topk = restated_decode(torch.from_numpy(g["all_cls_scores"][-1, b]), torch.from_numpy(g["all_bbox_preds"][-1, b]), K, pcr)
        assert np.array_equal(topk.numpy(), g[f"dec{b}_topk"]) and np.array_equal(idx.numpy(), g[f"dec{b}_index"]) and np.array_equal(lb.numpy(), g[f"dec{b}_labels"])
        assert 0 < len(idx) < K                                                          # the mask drops some and keeps some
        assert rel_max(sc, g[f"dec{b}_scores"]) <= 1e-5 and all(rel_max(bb[:, i], g[f"dec{b}_bboxes"][:, i]) <= 1e-5 for i in range(9))


def test_restatement_reproduces_the_full_fixture(golden_dir):
    g = np.load(os.path.join(golden_dir, "head_outputs_full.npz"))
    sizes, shape, seed = synth.HEAD_OUTPUTS_FULL, synth.HEAD_OUTPUTS_FULL_SHAPE, int(g["seed"])
    with torch.no_grad():
        _, cls, box = restated_branches(synth.head_outputs_state_dict(sizes, seed=seed), synth.head_outputs_inputs(sizes, shape, seed=seed))
    assert cls.shape == (6, 1, 900, 10) == g["all_cls_scores"].shape == box.shape == g["all_bbox_preds"].shape
    errs = group_errors(cls, box, g["all_cls_scores"], g["all_bbox_preds"])
    errs64 = group_errors(g["last_cls_f64"], g["last_bbox_f64"], g["all_cls_scores"][-1], g["all_bbox_preds"][-1])
    print({k: f"{e:.2e}" for k, e in errs.items()}, "f64 run vs f32 run:", {k: f"{e:.2e}" for k, e in errs64.items()})
    assert max(errs.values()) <= 1e-5 and max(errs64.values()) <= 1e-5, (errs, errs64)
    # the fixture's two promised properties: a boundary gap of hundreds of f32 ulps, finite logits
    s = np.sort(1.0 / (1.0 + np.exp(-g["all_cls_scores"][-1, 0].astype(np.float64))).ravel())[::-1]
    assert s[299] - s[300] >= 1e-5 and np.isfinite(g["all_cls_scores"]).all()
    bb, sc, lb, idx, _ = restated_decode(torch.from_numpy(g["all_cls_scores"][-1, 0]), torch.from_numpy(g["all_bbox_preds"][-1, 0]), int(g["max_num"]),
                                         g["post_center_range"].tolist())
    assert len(idx) == 300 and np.array_equal(idx.numpy(), g["dec_index"]) and np.array_equal(lb.numpy(), g["dec_labels"])
    assert rel_max(sc, g["dec_scores"]) <= 1e-5 and all(rel_max(bb[:, i], g["dec_bboxes"][:, i]) <= 1e-5 for i in range(9))
    assert g["decode_f32_err"].shape == (10,) and (g["decode_f32_err"][[0, 1, 2, 7, 8]] == 0).all() and g["decode_f32_err"].max() < 2e-6
