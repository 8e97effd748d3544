"""GPU: the assembled detector (toc3d_amd.Petr3D) and the kernel it adds.

(a) toc3d_neck_rows_fanout bit for bit against toc3d_nhwc_to_nchw followed by toc3d_nchw_to_rows, for BF16, F32 and F32X3P: one token, C no multiple of 32,
    T no multiple of the tile, more than one workgroup, the shipped shape; every path of the kernel -- 16-byte and element-wise input, 16-byte and element-wise
    NCHW stores (T % 4, C % 4, ldx % 4, a pointer off 16 bytes); padding columns keep their sentinel, planes buffers are compared whole;
(b) the detector equals the hand-written chain -- separately built backbone, neck and head with the same weights, looping through ``backbone_queries`` -- bit for
    bit over four frames with a scene change, in "fp32x3" and "bf16", in the plan launch mode and eagerly;
(d) the same at the shipped sizes (ViT-L at 6 x 320 x 800, CPFPN_CFG, HEAD_FULL), two frames, "fp32x3", with the shipped tile table;
(e) determinism, the scene change, load_state_dict, and ``data['img_feats']`` = a separate ``CPFPN.forward``.
There is NO test against a fixture of the reference's own ``Petr3D``: tools/gen_golden_detector.py runs the reference's ``simple_test`` over these four frames in f32
and in f64, and on none of the seeds 0 .. 63 does the stream, or frame 0 alone, meet the fixture's near-tie condition (every cut's gap >= 100 x the largest
|f32 - f64| of its scores; the best seed reaches 0.23 x on frame 0, and the reference's f32 and f64 runs keep different token sets on all 64).  A fixture that
misses its condition is not committed (the generator's docstring has the figures).  The parts are held to the reference by their own fixtures; (b) and (d) hold the
detector to the parts.
Every test prints the figures it asserts on (run with -s)."""
import pytest
import torch

import detector_cases as DC
import toc3d_amd
from detector_cases import BANK, schedule, weights
from support import DEV, to_dev
from toc3d_amd import lib, synth

pytestmark = pytest.mark.gpu
TINY = synth.DETECTOR_TINY
S = lambda: torch.cuda.current_stream().cuda_stream
SENTINEL = -7.0

# (V, T, C, ldx, ld_rows); the last three go beyond the issue's list to reach the element-wise input path (C % 4, ldx % 4) and a pointer off 16 bytes
FANOUT_SHAPES = [(1, 1, 32, 32, 64), (2, 31, 40, 64, 64), (2, 31, 40, 64, 40), (3, 33, 32, 32, 32), (2, 1000, 32, 32, 64), (12, 1000, 256, 256, 256),
                 (2, 33, 30, 31, 32), (2, 36, 30, 32, 64), ("off", 36, 32, 32, 64)]
DTYPES = {"bf16": (lib.BF16, torch.bfloat16), "f32": (lib.F32, torch.float32), "f32x3p": (lib.F32X3P, torch.float32)}


# planes rows take a leading dimension that is a multiple of 32: the ld_rows = 40 case is for the plain dtypes
FANOUT_CASES = [(n, s) for n in DTYPES for s in FANOUT_SHAPES if not (n == "f32x3p" and s[4] % 32)]


@pytest.mark.parametrize("name,shape", FANOUT_CASES, ids=lambda v: v if isinstance(v, str) else "x".join(str(e) for e in v))
def test_a_fanout_kernel_bit_for_bit(name, shape):
    dt, tdt = DTYPES[name]
    V, T, C, ldx, ld = shape
    off = V == "off"                                       # x and nchw start 4 bytes off a 16-byte boundary: the element-wise forms of both halves
    V = 2 if off else V
    g = torch.Generator().manual_seed(V * 1000 + T + C)
    xbuf = torch.randn(V * T * ldx + 1, generator=g).to(DEV)
    x = xbuf[1:] if off else xbuf[:-1]
    x = x.view(V * T, ldx)
    dense = x[:, :C].contiguous()
    # the two launches the kernel replaces
    nchw_ref = torch.full((V, C, T), SENTINEL, device=DEV)
    lib.call("toc3d_nhwc_to_nchw", dense, nchw_ref, V, T, C, S())
    fill = 0.0 if name == "f32x3p" else SENTINEL
    rows_ref = torch.full((V * T, ld), fill, dtype=tdt, device=DEV)
    lib.call("toc3d_nchw_to_rows", dt, nchw_ref, rows_ref, ld, V, C, T, S())
    # one pass
    nbuf = torch.full((V * C * T + 1,), SENTINEL, device=DEV)
    nchw = (nbuf[1:] if off else nbuf[:-1]).view(V, C, T)
    rows = torch.full((V * T, ld), fill, dtype=tdt, device=DEV)
    lib.call("toc3d_neck_rows_fanout", dt, x, ldx, nchw, rows, ld, V, T, C, S())
    torch.cuda.synchronize()
    bits = lambda t: t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)
    assert torch.equal(bits(nchw), bits(nchw_ref)), f"{name} {shape}: NCHW bits differ from toc3d_nhwc_to_nchw"
    assert torch.equal(bits(nchw), bits(dense.view(V, T, C).permute(0, 2, 1)))
    assert torch.equal(bits(rows), bits(rows_ref)), f"{name} {shape}: rows differ from toc3d_nchw_to_rows (valid columns, padding or planes)"
    assert float(nbuf[0 if off else -1]) == SENTINEL, "the element next to the NCHW tensor was written"
    if name != "f32x3p":
        assert torch.equal(bits(rows[:, :C]), bits(dense.to(tdt))) and bool((rows[:, C:].float() == SENTINEL).all()), f"{name} {shape}: padding columns were touched"
    else:
        assert bool((bits(rows) != 0).any())            # (the planes buffer was pre-zeroed and is compared whole above)


# ---- the detector and the chain ------------------------------------------------------------------------------------------------------------------------------
def build_detector(sizes, precision, launch_mode="plan"):
    return DC.build_detector(sizes, precision, launch_mode)


def build_chain(sizes, precision, launch_mode="plan"):
    cfg, sd = synth.detector_cfg(sizes), weights(sizes)
    pick = lambda pre: {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}
    backbone = toc3d_amd.build_backbone(dict(cfg["img_backbone"], precision=precision))
    backbone.load_state_dict(pick("img_backbone."), strict=True)
    neck = toc3d_amd.build_neck(dict(cfg["img_neck"], precision=precision))
    neck.load_state_dict(pick("img_neck."), strict=True)
    head = toc3d_amd.build_head(cfg["pts_bbox_head"], precision=precision, launch_mode=launch_mode)
    head.load_state_dict(pick("pts_bbox_head."), strict=True)
    backbone, neck, head = (m.to(DEV).eval() for m in (backbone, neck, head))
    schedule(backbone, neck, sizes, precision, launch_mode)
    return backbone, neck, head


def run_detector(det, frames):
    """simple_test over the stream -> per frame (keep_idxes, img_feats, head outputs, bank, decoded lists)."""
    seen = []
    hook = det.pts_bbox_head.register_forward_hook(lambda m, a, out: seen.append(out))
    res = []
    try:
        for fr in frames:
            result = det.simple_test(fr["img_metas"], gumbel_noise=fr["gumbel"], **to_dev(fr))
            assert isinstance(result, list) and len(result) == 1 and set(result[0]) == {"pts_bbox"} and set(result[0]["pts_bbox"]) == {"boxes_3d", "scores_3d", "labels_3d"}
            last = det.last_frame
            res.append(dict(keep=[k.clone() for k in last["keep_idxes"]], img_feats=last["img_feats"].clone(), out=seen[-1],
                            bank={k: getattr(det.pts_bbox_head, k).clone() for k in BANK}, dec=result[0]["pts_bbox"]))
    finally:
        hook.remove()
    return res


def run_chain(parts, frames):
    """The hand-written chain of INTEGRATION.md: backbone, neck, head, get_bboxes, the bank's proposals handed to the next frame's backbone."""
    backbone, neck, head = parts
    res, scene = [], None
    for fr in frames:
        data, metas = to_dev(fr), fr["img_metas"]
        prev = metas[0]["scene_token"] == scene
        scene = metas[0]["scene_token"]
        q = head.backbone_queries(backbone.pruning_num_queries, prev, 1)
        out = backbone(data["img"][0], ego_pose_inv=data["ego_pose_inv"], gumbel_noise=fr["gumbel"], **q)
        feats = neck(list(out.img_feats.values()))[0]
        data["img_feats"] = feats.view(1, *feats.shape)
        if not prev:
            head.reset_memory()
        data["prev_exists"] = data["img"].new_ones(1) if prev else data["img"].new_zeros(1)
        outs = head(None, metas, None, **data)
        (bboxes, scores, labels), = head.get_bboxes(outs, metas)
        res.append(dict(keep=[k.clone() for k in out.keep_idx], img_feats=data["img_feats"].clone(), out=outs, bank={k: getattr(head, k).clone() for k in BANK},
                        dec=dict(boxes_3d=bboxes.cpu(), scores_3d=scores.cpu(), labels_3d=labels.cpu())))
    return res


def assert_same(tag, a, b):
    assert len(a) == len(b)
    for f, (x, y) in enumerate(zip(a, b)):
        assert len(x["keep"]) == len(y["keep"]) == 3 and all(torch.equal(p, q) for p, q in zip(x["keep"], y["keep"])), f"{tag} frame {f}: kept token sets differ"
        assert torch.equal(x["img_feats"], y["img_feats"]), f"{tag} frame {f}: img_feats differ"
        for k in ("all_cls_scores", "all_bbox_preds"):
            assert torch.equal(x["out"][k], y["out"][k]), f"{tag} frame {f}: {k} differs"
        for k in BANK:
            assert torch.equal(x["bank"][k], y["bank"][k]), f"{tag} frame {f}: {k} differs"
        for k in ("boxes_3d", "scores_3d", "labels_3d"):
            assert torch.equal(torch.as_tensor(x["dec"][k]), torch.as_tensor(y["dec"][k])), f"{tag} frame {f}: decoded {k} differ"
        print(f"[{tag}] frame {f}: kept sets, img_feats, outputs, bank and {x['dec']['labels_3d'].shape[0]} decoded boxes equal bit for bit")


@pytest.mark.parametrize("launch_mode", ["plan", "eager"])
@pytest.mark.parametrize("precision", ["fp32x3", "bf16"])
def test_b_detector_is_the_hand_chain_bit_for_bit(precision, launch_mode):
    frames = synth.detector_inputs(TINY)
    assert [f["img_metas"][0]["scene_token"] for f in frames] == ["a", "a", "a", "b"]
    det = build_detector(TINY, precision, launch_mode)
    got = run_detector(det, frames)
    want = run_chain(build_chain(TINY, precision, launch_mode), frames)
    assert tuple(got[0]["img_feats"].shape) == (1, 6, 32, 20, 50) and tuple(got[0]["out"]["all_cls_scores"].shape) == (2, 1, 96, 10)
    assert tuple(got[1]["bank"]["memory_embedding"].shape) == (1, 160 + 64, 256)
    assert_same(f"tiny {precision} {launch_mode}", got, want)
    assert torch.isfinite(got[-1]["out"]["all_bbox_preds"]).all()
    # the frames behind a scene start read real proposals: the kept sets of frames 1 and 2 are not those of a frame that had none
    assert det.pts_bbox_head.topk_proposals == det.img_backbone.pruning_num_queries == 64


def test_d_shipped_sizes_detector_is_the_chain_bit_for_bit():
    sizes = synth.DETECTOR_FULL
    frames = synth.detector_inputs(sizes)
    assert len(frames) == 2 and tuple(frames[0]["data"]["img"].shape) == (1, 6, 3, 320, 800)
    det = build_detector(sizes, "fp32x3")
    assert det.img_backbone._tuned, "the shipped tile table serves this shape"
    got = run_detector(det, frames)
    del det
    want = run_chain(build_chain(sizes, "fp32x3"), frames)
    assert tuple(got[0]["img_feats"].shape) == (1, 6, 256, 20, 50) and tuple(got[0]["out"]["all_cls_scores"].shape) == (6, 1, 900, 10)
    assert_same("full fp32x3", got, want)


def test_e_state_and_determinism():
    frames = synth.detector_inputs(TINY)
    det = build_detector(TINY, "fp32x3")
    calls = []
    fwd = det.img_backbone.forward
    det.img_backbone.forward = lambda *a, **k: (calls.append(k["prev_exists"]), fwd(*a, **k))[1]
    first = run_detector(det, frames)
    # a new scene token resets the bank, and the backbone then gets prev_exists = False -- as the Python bool it is
    assert calls == [False, True, True, False] and all(type(c) is bool for c in calls)
    assert det.prev_scene_token == "b"
    # ... so frame 3 is what a detector that has seen nothing computes for it
    det.prev_scene_token = None
    det.pts_bbox_head.reset_memory()
    assert_same("scene start alone", first[3:], run_detector(det, frames[3:]))
    assert calls[4:] == [False]
    del calls[:]
    # the same stream again: frame 0 carries scene "a" again, so it starts over by itself
    again = run_detector(det, frames)
    assert_same("again", first, again)
    assert calls == [False, True, True, False]
    # data['img_feats'] carries the bits of a separate CPFPN.forward on the backbone's features
    backbone, neck, head = build_chain(TINY, "fp32x3")
    fr = frames[0]
    out = backbone(fr["data"]["img"][0].to(DEV), ego_pose_inv=fr["data"]["ego_pose_inv"].to(DEV), gumbel_noise=fr["gumbel"], **head.backbone_queries(64, False, 1))
    assert torch.equal(neck(list(out.img_feats.values()))[0], first[0]["img_feats"][0])
    # load_state_dict drops derived state and the scene
    assert det.pts_bbox_head._bank is not None and det.img_neck._packed is not None and det.img_backbone._packed is not None
    det.load_state_dict(weights(TINY), strict=True)
    assert det.prev_scene_token is None and det.last_frame is None and det.pts_bbox_head._bank is None and det.img_neck._packed is None
    assert det.img_backbone._packed is None and det.pts_bbox_head._tokens._packed is None
    third = run_detector(det, frames)
    assert_same("reloaded", first, third)
    # a tensor that is not the one extract_img_feat returned last goes through the head's own transpose: the same bits
    fr = frames[3]
    data, dec = to_dev(fr), []
    for own in (True, False):
        det.prev_scene_token = None                     # a scene start both times
        feats, *_ = det.extract_img_feat(data["img"], 1, prev_exists=False, ego_pose_inv=data["ego_pose_inv"], gumbel_noise=fr["gumbel"])
        dec.append(det.simple_test_pts(fr["img_metas"], img_feats=feats if own else feats.clone(), **data)[0])
    assert dec[0]["labels_3d"].numel() > 0 and all(torch.equal(dec[0][k], dec[1][k]) for k in ("boxes_3d", "scores_3d", "labels_3d"))
