"""GPU: the assembled head with ``token_sampling=True`` -- ``forward(..., topk_indexes=...)`` end to end.

(a) the tiny stream of tests/golden/head_sampled_tiny.npz -- the REAL reference's own forward with a seeded index list per frame and sample (K = 7 of 24 tokens;
    tools/gen_golden_head_sampled.py), four frames, free-running in "fp32x3" -- at the bars tests/test_gpu_head.py holds head_tiny.npz to: the kept proposal sets
    and the decoded labels / query order are the fixture's, outputs and bank below 1e-3 rel max (timestamps and poses below 1e-4).  The bank is compared
    entry for entry, so the fixture's seed also meets the near-tie condition on the ORDER of the kept proposals (the generator's docstring has the figures of
    the seed that met the cut condition alone: two kept scores 2.9e-7 apart, their bank rows swapped, every output of that frame within 7e-5);
(b) the head is the hand-written chain of its modules on the same lists, bit for bit;  (c) ``img_feats_rows=True`` gives the same bits as the path without it;
(d) the shipped sizes, K = 3000 of 6000: both outputs of frame 0 against the REAL reference (head_sampled_full_frame0.npz; bar 1e-3, as for head_full_frame0.npz);
(e) a head built without the keyword still raises on a list.
Every test prints the figures it asserts on (run with -s)."""
import os

import numpy as np
import pytest
import torch

import sampled_cases as SC
import toc3d_amd
from head_queries_cases import BANK
from support import DEV, rel_max_zero_ok
from toc3d_amd import synth

pytestmark = pytest.mark.gpu
TINY, TINY_SHAPE = synth.HEAD_TINY, synth.HEAD_TINY_SHAPE


def build(sizes, seed=0, **kw):
    h = toc3d_amd.build_head(synth.head_cfg(sizes), **kw)
    h.load_state_dict(synth.head_state_dict(sizes, seed=seed), strict=True)
    return h.to(DEV).eval()


def stream(h, sizes, shape, lists, seed=0, frames=None, **kw):
    """Free-running on the per-frame lists: per frame (outputs, bank after post_update_memory, decode_fixed of the last level)."""
    inp = synth.head_inputs(sizes, shape, seed=seed)
    res = []
    for f, data in enumerate(inp["frames"][:frames]):
        out = h(None, inp["img_metas"], lists[f].to(DEV), **{k: v.to(DEV) for k, v in data.items()}, **kw)
        bank = {k: getattr(h, k).clone() for k in BANK}
        dec = h.bbox_coder.decode_fixed(out["all_cls_scores"][-1], out["all_bbox_preds"][-1], sub_half_height=True)
        res.append((out, bank, dec))
    return res, inp


def tiny_lists(g=None, frames=4):
    g = np.load(os.path.join(SC.GOLDEN, "head_sampled_tiny.npz")) if g is None else g
    return [torch.from_numpy(g[f"f{f}_topk_indexes"]) for f in range(frames)]


def test_a_tiny_stream_fp32x3_against_the_reference():
    g, g64 = np.load(os.path.join(SC.GOLDEN, "head_sampled_tiny.npz")), np.load(os.path.join(SC.GOLDEN, "head_sampled_tiny_f64.npz"))
    mg = g["margins"]
    assert bool((mg[..., 0] >= float(g["margin_required"]) * mg[..., 1]).all()), "the fixture states its near-tie condition and meets it"
    og = g["order_margins"]                     # ... and the one on the ORDER of the kept proposals, which decides the order of the bank rows compared below
    assert og.shape == (4, 2, 2) and bool((og[..., 0] >= float(g["margin_required"]) * og[..., 1]).all())
    seed, lists = int(g["seed"]), tiny_lists(g)
    assert all(tuple(t.shape) == (2, 7, 1) and t.dtype == torch.int64 and int(t.max()) < 24 for t in lists) and not torch.equal(lists[0], lists[1])
    h = build(TINY, seed, token_sampling=True)
    assert h.precision == "fp32x3" and h.token_sampling
    res, inp = stream(h, TINY, TINY_SHAPE, lists, seed)
    assert len(res) == 4 and g["f0_all_cls_scores"].shape == (2, 2, 28, 10) and g["f3_memory_embedding"].shape == (2, 36, 256)
    K = TINY["topk_proposals"]
    for f, (out, bank, dec) in enumerate(res):
        cls, box = out["all_cls_scores"], out["all_bbox_preds"]
        score = cls[-1].sigmoid().max(-1).values
        kept = torch.sort(score, dim=1, descending=True, stable=True).indices[:, :K].sort(1).values.cpu()
        assert torch.equal(kept, torch.from_numpy(g[f"f{f}_proposal_set"])), f"frame {f}: the kept proposal set differs from the reference's"
        pairs = [("all_cls_scores", cls, 1e-3), ("all_bbox_preds", box, 1e-3)]
        pairs += [(k, bank[k], 1e-4 if k in ("memory_timestamp", "memory_egopose") else 1e-3) for k in BANK]
        for k, v, tol in pairs:
            e, e64 = rel_max_zero_ok(v, g[f"f{f}_{k}"]), rel_max_zero_ok(v, g64[f"f{f}_{k}"])
            print(f"[tiny sampled fp32x3] frame {f} {k}: rel max vs the f32 reference {e:.2e} (vs its f64 twin {e64:.2e}), bar {tol:.0e}")
            assert e < tol, (f, k, e)
        boxes, scores, labels, qidx, counts = (t.cpu() for t in dec)
        for b in range(cls.shape[1]):
            n = int(counts[b])
            assert n == g[f"f{f}_b{b}_labels"].shape[0], f"frame {f} sample {b}: {n} boxes decoded, the reference keeps {g[f'f{f}_b{b}_labels'].shape[0]}"
            assert torch.equal(labels[b, :n], torch.from_numpy(g[f"f{f}_b{b}_labels"])) and torch.equal(qidx[b, :n], torch.from_numpy(g[f"f{f}_b{b}_query"])), \
                f"frame {f} sample {b}: decoded labels / query order differ from the reference's"
            eb, es = rel_max_zero_ok(boxes[b, :n], g[f"f{f}_b{b}_bboxes"]), rel_max_zero_ok(scores[b, :n], g[f"f{f}_b{b}_scores"])
            print(f"[tiny sampled fp32x3] frame {f} sample {b}: {n} boxes, rel max boxes {eb:.2e} scores {es:.2e}")
            assert eb < 1e-3 and es < 1e-3
    # the sampled stream is not the full-token one: the list reaches the decoder
    full = build(TINY, seed)(None, inp["img_metas"], None, **{k: v.to(DEV) for k, v in inp["frames"][0].items()})
    assert not torch.equal(full["all_cls_scores"], res[0][0]["all_cls_scores"])


@pytest.mark.parametrize("precision", ["fp32x3", "bf16"])
def test_b_head_is_the_chain_of_its_modules_bit_for_bit(precision):
    sizes, shape = TINY, TINY_SHAPE
    cfg, sd, lists = synth.head_cfg(sizes), synth.head_state_dict(sizes), tiny_lists(frames=2)
    h = build(sizes, precision=precision, token_sampling=True)
    pick = lambda *pre: {k: v for k, v in sd.items() if k.startswith(pre)}
    tokens = toc3d_amd.HeadTokenEmbedding(in_channels=sizes["in_channels"], embed_dims=256, depth_num=64, depth_start=1, LID=True, stride=16,
                                          position_range=cfg["position_range"], precision=precision)
    tokens.load_state_dict(pick("position_encoder.", "memory_embed.", "spatial_alignment.", "featurized_pe."), strict=True)
    queries = toc3d_amd.HeadQueries(num_query=sizes["num_query"], memory_len=sizes["memory_len"], num_propagated=sizes["num_propagated"], embed_dims=256,
                                    with_ego_pos=True, pc_range=synth.PC_RANGE, precision=precision)
    queries.load_state_dict(pick("reference_points.", "query_embedding.", "time_embedding.", "ego_pose_pe.", "ego_pose_memory."), strict=True)
    decoder = toc3d_amd.build_transformer(cfg["transformer"], precision=precision)
    decoder.load_state_dict({k[len("transformer."):]: v for k, v in pick("transformer.").items()}, strict=True)
    outputs = toc3d_amd.HeadOutputs(num_classes=10, embed_dims=256, num_reg_fcs=2, code_size=10, num_pred=6, pc_range=synth.PC_RANGE, bbox_coder=cfg["bbox_coder"],
                                    precision=precision)
    outputs.load_state_dict(pick("cls_branches.", "reg_branches."), strict=True)
    tokens, queries, decoder, outputs = (m.to(DEV).eval() for m in (tokens, queries, decoder, outputs))
    bank = toc3d_amd.TemporalMemory(sizes["memory_len"], sizes["topk_proposals"], sizes["num_propagated"], 256, synth.PC_RANGE, sd["pseudo_reference_points.weight"],
                                    device=DEV)
    res, inp = stream(h, sizes, shape, lists, frames=2)
    for f, data in enumerate(inp["frames"][:2]):
        data = {k: v.to(DEV) for k, v in data.items()}
        memory, pos_embed, cone = tokens(data["img_feats"], data["intrinsics"], data["lidar2img"], inp["img_metas"][0]["pad_shape"][0], topk_indexes=lists[f].to(DEV))
        assert tuple(memory.shape) == (2, 7, 256)
        bank.pre_update_memory(data)
        tgt, query_pos, reference_points, temp_memory, temp_pos, rec_ego_pose = queries.forward_from(bank)
        outs_dec, _, _ = decoder(memory, tgt, query_pos, pos_embed, None, temp_memory, temp_pos)
        outs_dec, all_cls_scores, all_bbox_preds = outputs(outs_dec, reference_points)
        bank.post_update_memory(data, rec_ego_pose, all_cls_scores, all_bbox_preds, outs_dec)
        out, hbank, _ = res[f]
        assert torch.equal(out["all_cls_scores"], all_cls_scores) and torch.equal(out["all_bbox_preds"], all_bbox_preds), f"{precision} frame {f}: outputs differ"
        for k in BANK:
            assert torch.equal(hbank[k], getattr(bank, k)), f"{precision} frame {f}: {k} differs"


def test_c_img_feats_rows_gives_the_same_bits():
    lists = tiny_lists(frames=2)
    want, inp = stream(build(TINY, token_sampling=True), TINY, TINY_SHAPE, lists, frames=2)
    h = build(TINY, token_sampling=True)
    B, N, hh, ww = (TINY_SHAPE[k] for k in ("B", "N", "h", "w"))
    for f, data in enumerate(inp["frames"][:2]):
        data = {k: v.to(DEV) for k, v in data.items()}
        rows, ld, dt = h.img_feats_rows_buffer(B, N, hh, ww)
        toc3d_amd.lib.call("toc3d_nchw_to_rows", dt, data["img_feats"].float().contiguous(), rows, ld, B * N, TINY["in_channels"], hh * ww, toc3d_amd.lib.stream_ptr())
        out = h(None, inp["img_metas"], lists[f].to(DEV), img_feats_rows=True, **dict(data, img_feats=torch.empty_like(data["img_feats"])))
        for k in ("all_cls_scores", "all_bbox_preds"):
            assert torch.equal(out[k], want[f][0][k]), f"frame {f}: {k} with img_feats_rows=True differs"
        for k in BANK:
            assert torch.equal(getattr(h, k), want[f][1][k]), f"frame {f}: {k} with img_feats_rows=True differs"


def test_d_shipped_sizes_frame0_fp32x3_against_the_reference():
    g = np.load(os.path.join(SC.GOLDEN, "head_sampled_full_frame0.npz"))
    seed, rows, topk = int(g["seed"]), int(g["row_step"]), torch.from_numpy(g["f0_topk_indexes"])
    assert tuple(topk.shape) == (1, 3000, 1) and int(topk.max()) < 6000 and len(set(topk.flatten().tolist())) == 3000
    h = build(synth.HEAD_FULL, seed, token_sampling=True)
    assert h.precision == "fp32x3"
    res, inp = stream(h, synth.HEAD_FULL, synth.HEAD_FULL_SHAPE, [topk], seed, frames=1)
    assert tuple(inp["frames"][0]["img_feats"].shape) == (1, 6, 256, 20, 50) and inp["frames"][0]["prev_exists"].tolist() == [0.0]
    out = res[0][0]
    assert tuple(out["all_cls_scores"].shape) == (6, 1, 900, 10) and tuple(out["all_bbox_preds"].shape) == (6, 1, 900, 10)
    for k in ("all_cls_scores", "all_bbox_preds"):
        for key, v in ((f"f0_{k}_last", out[k][-1]), (f"f0_{k}", out[k][:-1, :, ::rows])):
            e, e64 = rel_max_zero_ok(v, g[key]), rel_max_zero_ok(v, g["f64_" + key])
            print(f"[full sampled fp32x3] frame 0 {key}: rel max vs the f32 reference {e:.2e} (vs its f64 twin {e64:.2e}), bar 1e-03")
            assert tuple(v.shape) == g[key].shape and e < 1e-3, (key, e)


def test_e_keyword_off_still_raises_on_the_device():
    h = build(TINY)
    inp = synth.head_inputs(TINY, TINY_SHAPE)
    data = {k: v.to(DEV) for k, v in inp["frames"][0].items()}
    with pytest.raises(NotImplementedError, match="topk_indexes.*token_sampling"):
        h(None, inp["img_metas"], tiny_lists(frames=1)[0].to(DEV), **data)
    assert h._bank is None, "refused before anything ran"
    out = h(None, inp["img_metas"], None, **data)
    assert tuple(out["all_cls_scores"].shape) == (2, 2, 28, 10)
