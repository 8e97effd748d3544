"""CPU: FocalHead without a GPU -- the plain-torch restatement (tests/focal_head_cases.py) against the fixtures of the REAL reference
(tools/gen_golden_focal_head.py), the module's state dict against the reference's names and shapes, the registry, every refusal of the constructor and of the
forward, the side header include/toc3d_focal.h against the ctypes table that binds it and against the library's exports, and every refusal of the two entry points
on made-up host pointers (the checks run before any launch).  Every test prints the figures it asserts on (run with -s)."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import focal_head_cases as FC
import toc3d_amd
from support import A, ERR_ARG, OldLibrary, header_sigs, raw_call
from toc3d_amd import FocalHead, lib, registry, synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32_ROUNDING = 2e-6                          # the restatement and the reference spell the same f32 formulas: they differ by the order of a few roundings


# ---- the restatement pins the fixtures -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["tiny", "full"])
def test_restatement_equals_the_golden(tag):
    sizes, shape = FC.SIZES[tag]
    gold = np.load(os.path.join(GOLDEN, f"focal_head_{tag}.npz"))
    seed = int(gold["seed"])
    sd, inp = synth.focal_head_state_dict(sizes, seed=seed), synth.focal_head_inputs(sizes, shape, seed=seed)
    out = FC.restated_forward(sd, inp, float(gold["infer_ratio"]))
    B, N, T = shape["B"], shape["N"], shape["h"] * shape["w"]
    K = int(N * T * sizes["infer_ratio"])
    want = dict(enc_cls_scores=(B * N, T, sizes["num_classes"]), enc_bbox_preds=(B * N, T, 4), pred_centers2d=(B * N, T, 2), centerness=(B * N, T, 1),
                topk_indexes=(B, K, 1), sample_weight=(B, N * T, 1))
    for k, s in want.items():
        assert tuple(gold[k].shape) == s == tuple(out[k].shape), (k, gold[k].shape, out[k].shape)
        assert gold[k].dtype == (np.int64 if k == "topk_indexes" else np.float32)
    errs = FC.group_errors(out, {k: torch.from_numpy(gold[k]) for k in FC.ARITH})
    print(f"{tag}: restatement vs golden {errs}; K = {K}")
    assert max(errs.values()) <= F32_ROUNDING, errs
    assert torch.equal(out["topk_indexes"], torch.from_numpy(gold["topk_indexes"]))
    # the premises of the GPU index test, as the generator asserted them
    w = torch.from_numpy(gold["sample_weight"]).reshape(B, -1)
    _, share = FC.index_band(w, K, gold["band_half_width_f64"])
    srt = torch.sort(w, dim=1, descending=True).values
    assert bool((share <= 0.005).all()) and bool((srt[:, K - 1] > srt[:, K]).all())
    assert (K, tag) in ((9, "tiny"), (3000, "full"))


def test_geometry_clamps_and_pixel_centres():
    loc = torch.tensor([[0.1, 0.9], [0.5, 0.5]])
    boxes, centers = FC.geometry(loc, torch.tensor([[30.0, -30.0, 30.0, -30.0], [-30.0, -30.0, -30.0, -30.0]]), torch.zeros(2, 2))
    print(boxes, centers)
    # row 0: x1 = 0.1 - 1 -> 0, y1 = 0.9 - 0 = 0.9, x2 = 0.1 + 1 -> 1, y2 = 0.9 + 0
    assert torch.allclose(boxes[0], torch.tensor([0.5, 0.9, 1.0, 0.0]), atol=1e-6) and torch.allclose(boxes[1], torch.tensor([0.5, 0.5, 0.0, 0.0]), atol=1e-6)
    assert torch.allclose(centers, loc, atol=1e-6), "a zero offset returns the location"


# ---- the module ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_state_dict_names_and_shapes_equal_the_reference():
    spec = json.load(open(os.path.join(GOLDEN, "focal_head_state_dict_spec.json")))
    for tag, (sizes, _) in FC.SIZES.items():
        m = FocalHead(**sizes)
        got = {k: list(v.shape) for k, v in m.state_dict().items()}
        assert got == spec[tag] and list(got) == list(spec[tag]), (tag, got)
        sd = synth.focal_head_state_dict(sizes)
        assert {k: list(v.shape) for k, v in sd.items()} == spec[tag]
        m.load_state_dict(sd, strict=True)
        with pytest.raises(RuntimeError, match="Missing key|Unexpected key"):
            m.load_state_dict(dict(sd, extra=torch.zeros(1)), strict=True)
        with pytest.raises(RuntimeError, match="Missing key"):
            m.load_state_dict({k: v for k, v in sd.items() if k != "ltrb.bias"}, strict=True)
    names = list(spec["full"])
    print(names)
    assert names == ["cls.weight", "cls.bias", "shared_reg.0.weight", "shared_reg.0.bias", "shared_reg.1.weight", "shared_reg.1.bias", "shared_cls.0.weight",
                     "shared_cls.0.bias", "shared_cls.1.weight", "shared_cls.1.bias", "centerness.weight", "centerness.bias", "ltrb.weight", "ltrb.bias",
                     "center2d.weight", "center2d.bias"]
    m = FocalHead(num_classes=10)
    assert float(m.cls.bias.detach()[0]) == pytest.approx(-4.59511985013459) and float(m.centerness.bias.detach()[0]) == pytest.approx(-4.59511985013459)


def test_derived_state_is_dropped_with_the_weights():
    m = FocalHead(**synth.FOCAL_HEAD_TINY)
    for drop in (lambda: m.load_state_dict(synth.focal_head_state_dict(synth.FOCAL_HEAD_TINY)), lambda: m.to("cpu"), m.init_weights):
        m._packed, m._ws, m._states = "packed", {1: 2}, {3: 4}
        drop()
        assert m._packed is None and m._ws == {} and m._states == {}


def test_shipped_img_roi_head_builds_through_the_registry():
    cfg = synth.detector_cfg()["img_roi_head"]
    m = registry.build_head(cfg)
    assert isinstance(m, FocalHead) and toc3d_amd.HEADS.get("FocalHead") is FocalHead and "FocalHead" in toc3d_amd.__all__
    assert not m.training and (m.num_classes, m.in_channels, m.embed_dims, m.stride, m.infer_ratio) == (10, 256, 256, 16, 1.0)
    assert m.precision == "fp32x3" and m.launch_mode == "plan" and m.train_cfg == cfg["train_cfg"]
    assert not any(hasattr(m, k) for k in ("loss_cls2d", "loss_bbox2d", "assigner2d", "sampler")), "losses, assigner and sampler: accepted, nothing built"
    assert registry.build_head(dict(cfg, precision="bf16", infer_ratio=0.5, launch_mode="eager")).precision == "bf16"


def test_refusals():
    name = "toc3d_amd.FocalHead"
    for kw, exc in ((dict(use_hybrid_tokens=True), NotImplementedError), (dict(in_channels=96), NotImplementedError), (dict(embed_dims=96), NotImplementedError),
                    (dict(embed_dims=32), NotImplementedError), (dict(embed_dims=48), NotImplementedError), (dict(infer_ratio=1.5), ValueError),
                    (dict(infer_ratio=-0.1), ValueError), (dict(precision="fp32"), NotImplementedError), (dict(num_classes=0), NotImplementedError)):
        with pytest.raises(exc, match=name) as e:
            FocalHead(**dict(dict(num_classes=10), **kw))
        print(kw, "->", str(e.value)[:90])
    m = FocalHead(**synth.FOCAL_HEAD_TINY)
    with pytest.raises(NotImplementedError, match=name):
        m.train()
    with pytest.raises(NotImplementedError, match=name):
        m.train(True)
    assert m.eval() is m and m.train(False) is m and not m.training
    inp = synth.focal_head_inputs(synth.FOCAL_HEAD_TINY, synth.FOCAL_HEAD_TINY_SHAPE)
    with pytest.raises(RuntimeError, match="no CPU"):
        m(inp["location"], img_feats=inp["img_feats"])
    with pytest.raises(RuntimeError, match="no CPU"):
        m(inp["location"].tolist(), img_feats=inp["img_feats"])
    with pytest.raises(RuntimeError, match="no CPU"):
        m.forward_rows(inp["location"], torch.zeros(30, 64), 64, 1, 2, 3, 5)
    with pytest.raises(ValueError, match=name):
        m(inp["location"], img_feats=inp["img_feats"][:, :, :32])
    with pytest.raises(ValueError, match=name):
        m(inp["location"][:1], img_feats=inp["img_feats"])
    m.training = True                          # set behind train()'s back
    with pytest.raises(NotImplementedError, match=name):
        m(inp["location"], img_feats=inp["img_feats"])


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------------------------------------
def test_focal_header_ctypes_table_and_exports_agree():
    raw = open(lib.FOCAL_HEADER_PATH).read()
    found = header_sigs(lib.header_text(lib.FOCAL_HEADER_PATH), lib._FOCAL_SIGS)
    print(f"toc3d_focal.h declares {found}")
    assert found == lib._FOCAL_SIGS and list(found) == ["toc3d_focal_gn_stats", "toc3d_focal_heads"]
    declared = set(re.findall(r"\b(toc3d_\w+)\s*\(", lib.header_text(lib.FOCAL_HEADER_PATH)))
    assert declared == set(lib._FOCAL_SIGS) | {"toc3d_focal_abi"}, "nothing declared that the table does not bind"
    assert int(re.search(r"#define\s+TOC3D_FOCAL_ABI\s+(\d+)", raw).group(1)) == lib.FOCAL_ABI == 1
    assert "dense_heads/focal_head.py:124,129" in raw and "focal_head.py:159-180" in raw and "misc.py:26-43" in raw, "the header cites the reference lines it serves"
    dll = ctypes.CDLL(lib.LIB_PATH)
    assert all(hasattr(dll, n) for n in declared)
    dll.toc3d_focal_abi.restype = ctypes.c_int
    assert dll.toc3d_focal_abi() == 1
    # the pinned headers know nothing of it
    assert "toc3d_focal" not in open(lib.HEADER_PATH).read() and "toc3d_focal" not in open(lib.STREAMS_HEADER_PATH).read()
    assert not set(lib._FOCAL_SIGS) & (set(lib._SIGS) | set(lib._STREAMS_SIGS))


def test_call_binds_the_entry_points_and_an_old_library_is_told_to_rebuild(monkeypatch):
    with pytest.raises(RuntimeError, match=r"toc3d_focal_gn_stats failed \(-1\).*null buffer"):
        lib.call("toc3d_focal_gn_stats", lib.F32, None, 128, 1, 15, 64, 2, 1e-5, None, None)
    for n, sig in lib._FOCAL_SIGS.items():
        assert getattr(lib.load(), n).argtypes == [lib._CT[c] for c in sig], "bound with the table's argument types (int64 counts, not C ints)"

    monkeypatch.setattr(lib, "_lib", OldLibrary())
    with pytest.raises(RuntimeError, match=r"toc3d_focal\.h.*rebuild the library"):
        lib.call("toc3d_focal_heads", *heads_args())


STATS_PTRS, HEADS_PTRS = ("x", "stats"), ("x", "stats", "gamma", "beta", "w_cls", "b_cls", "w_reg", "b_reg", "location", "cls", "box", "ctr2d", "ctrness", "weight")


def stats_args(dtype=lib.F32, **o):
    a = dict({p: A for p in STATS_PTRS}, ldx=512, V=6, T=1000, E=256, branches=2)
    a.update(o)
    return (dtype, a["x"], a["ldx"], a["V"], a["T"], a["E"], a["branches"], 1e-5, a["stats"], None)


def heads_args(dtype=lib.F32, **o):
    a = dict({p: A for p in HEADS_PTRS}, ldx=512, V=6, T=1000, E=256, NC=10, ld_cls=10)
    a.update(o)
    return (dtype, a["x"], a["ldx"], a["stats"], a["gamma"], a["beta"], a["w_cls"], a["b_cls"], a["w_reg"], a["b_reg"], a["location"], a["V"], a["T"], a["E"], a["NC"],
            a["cls"], a["ld_cls"], a["box"], a["ctr2d"], a["ctrness"], a["weight"], None)


COMMON = [(lib.BF16, {}, "bad dtype"), (lib.F32X3P, {}, "bad dtype"), (99, {}, "bad dtype"),
          (lib.F32, dict(V=0), "must be positive"), (lib.F32, dict(T=0), "must be positive"), (lib.F32, dict(T=-5), "must be positive"),
          (lib.F32, dict(E=0), "must be positive"), (lib.F32, dict(E=48), "embed_dims % 32 != 0"), (lib.F32, dict(E=250), "embed_dims % 32 != 0"),
          (lib.F32, dict(E=2048, ldx=4096), "above 1024")]


@pytest.mark.parametrize("dtype,over,reason", [
    *[(lib.F32, {p: None}, "null buffer") for p in STATS_PTRS], *COMMON,
    (lib.F32, dict(branches=0), "must be positive"), (lib.F32, dict(ldx=511), "ldx below"), (lib.F32, dict(T=1 << 31), "too many"),
])
def test_gn_stats_refusals(dtype, over, reason):
    rc, msg = raw_call(lib._FOCAL_SIGS, "toc3d_focal_gn_stats", stats_args(dtype, **over))
    print(f"{over or dtype}: rc {rc}, {msg!r}")
    assert rc == ERR_ARG and "toc3d_focal_gn_stats" in msg and reason in msg, (rc, msg)


@pytest.mark.parametrize("dtype,over,reason", [
    *[(lib.F32, {p: None}, "null buffer") for p in HEADS_PTRS], *COMMON,
    (lib.F32, dict(NC=0), "must be positive"), (lib.F32, dict(NC=65), "num_classes above 64"), (lib.F32, dict(E=1024, ldx=2048, NC=10), "64 KB of LDS"),
    (lib.F32, dict(ldx=508), "leading dimension"), (lib.F32, dict(ldx=514), "leading dimension"), (lib.F32, dict(ld_cls=9), "leading dimension"),
    (lib.F32, dict(x=A + 4), "aligned"), (lib.F32, dict(box=A + 8), "aligned"), (lib.F32, dict(location=A + 4), "aligned"), (lib.F32, dict(T=1 << 31), "too many"),
])
def test_heads_refusals(dtype, over, reason):
    rc, msg = raw_call(lib._FOCAL_SIGS, "toc3d_focal_heads", heads_args(dtype, **over))
    print(f"{over or dtype}: rc {rc}, {msg!r}")
    assert rc == ERR_ARG and "toc3d_focal_heads" in msg and reason in msg, (rc, msg)
