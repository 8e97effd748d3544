"""GPU: the assembled head (toc3d_amd.StreamPETRHead) end to end.

(a) the tiny stream of tests/golden/head_tiny.npz -- the REAL reference's own forward / get_bboxes over four frames (tools/gen_golden_head_e2e.py), B = 2, sample 1
    starting a new scene at frame 2 -- free-running (the head's own bank feeds the next frame, no teacher forcing) in "fp32x3": the kept proposal sets and the decoded
    labels / query order are the fixture's, outputs and bank below 1e-3 rel max (timestamps and poses below 1e-4), with the error against the f64 twin printed;
(b) the head is the hand-written chain of INTEGRATION.md on separately built modules that carry the same weights, bit for bit, in "fp32x3" and "bf16";
(c) the shipped sizes (B 1, 6 x 20 x 50 tokens, 644 + 256 queries, 1024 entries, six layers), fp32x3: both outputs of frame 0 against the REAL reference
    (tests/golden/head_full_frame0.npz: the last level whole, every 8th query row of the others; bar 1e-3, the f64 twin printed) -- what no top-k cut has touched.
    The two-frame STREAM at these sizes has no reference fixture: no seed of the generator's search met the near-tie condition at 900 queries
    (tools/gen_golden_head_e2e.py states the figures), and a fixture that misses its condition is not committed.  The stream -- the bank, the second frame, the
    decoded lists -- is held at the shipped sizes by (b) instead, bit for bit against the chain of the modules;
(d) determinism, reset_memory, load_state_dict;  (e) shapes, levels="last".
Every test prints the figures it asserts on (run with -s)."""
import os

import numpy as np
import pytest
import torch

import toc3d_amd
from head_queries_cases import BANK
from support import DEV, rel_max_zero_ok
from toc3d_amd import synth

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TINY, TINY_SHAPE = synth.HEAD_TINY, synth.HEAD_TINY_SHAPE


def build(sizes, seed=0, **kw):
    h = toc3d_amd.build_head(synth.head_cfg(sizes), **kw)
    h.load_state_dict(synth.head_state_dict(sizes, seed=seed), strict=True)
    return h.to(DEV).eval()


def stream(h, sizes, shape, seed=0, frames=None):
    """Free-running: per frame (outputs, bank after post_update_memory, decode_fixed of the last level)."""
    inp = synth.head_inputs(sizes, shape, seed=seed)
    res = []
    for data in inp["frames"][:frames]:
        out = h(None, inp["img_metas"], None, **{k: v.to(DEV) for k, v in data.items()})
        bank = {k: getattr(h, k).clone() for k in BANK}
        dec = h.bbox_coder.decode_fixed(out["all_cls_scores"][-1], out["all_bbox_preds"][-1], sub_half_height=True)
        res.append((out, bank, dec))
    return res, inp


def check_against_fixture(tag, res, g, g64, sizes, rows=None):
    K, worst = sizes["topk_proposals"], {}
    for f, (out, bank, dec) in enumerate(res):
        cls, box = out["all_cls_scores"], out["all_bbox_preds"]
        # the proposals post_update_memory kept: the same set as the reference's, so the bank rows below are compared entry for entry
        score = cls[-1].sigmoid().max(-1).values
        kept = torch.sort(score, dim=1, descending=True, stable=True).indices[:, :K].sort(1).values.cpu()
        assert torch.equal(kept, torch.from_numpy(g[f"f{f}_proposal_set"])), f"{tag} frame {f}: the kept proposal set differs from the reference's"
        pairs = []
        for k, v in (("all_cls_scores", cls), ("all_bbox_preds", box)):
            if rows:
                pairs += [(k + "_last", v[-1], 1e-3), (k, v[:-1, :, ::rows], 1e-3)]
            else:
                pairs.append((k, v, 1e-3))
        for k in BANK:
            pairs.append((k, bank[k][:, ::rows] if rows else bank[k], 1e-4 if k in ("memory_timestamp", "memory_egopose") else 1e-3))
        for k, v, tol in pairs:
            e, e64 = rel_max_zero_ok(v, g[f"f{f}_{k}"]), rel_max_zero_ok(v, g64[f"f{f}_{k}"])
            worst[k] = max(worst.get(k, 0.0), e)
            print(f"[{tag}] frame {f} {k}: rel max vs the f32 reference {e:.2e} (vs its f64 twin {e64:.2e}), bar {tol:.0e}")
            assert e < tol, (tag, f, k, e)
        ref_pt = torch.from_numpy(g[f"f{f}_memory_reference_point"])
        got_pt = (bank["memory_reference_point"][:, ::rows] if rows else bank["memory_reference_point"]).cpu()
        row_err = (got_pt - ref_pt).abs().amax(-1) / ref_pt.abs().max()
        assert bool((row_err < 1e-3).all()), f"{tag} frame {f}: reference points of bank rows {row_err.argmax().item()} differ ({row_err.max().item():.2e})"
        boxes, scores, labels, qidx, counts = (t.cpu() for t in dec)
        for b in range(cls.shape[1]):
            n = int(counts[b])
            assert n == g[f"f{f}_b{b}_labels"].shape[0], f"{tag} frame {f} sample {b}: {n} boxes decoded, the reference keeps {g[f'f{f}_b{b}_labels'].shape[0]}"
            assert torch.equal(labels[b, :n], torch.from_numpy(g[f"f{f}_b{b}_labels"])) and torch.equal(qidx[b, :n], torch.from_numpy(g[f"f{f}_b{b}_query"])), \
                f"{tag} frame {f} sample {b}: decoded labels / query order differ from the reference's"
            eb, es = rel_max_zero_ok(boxes[b, :n], g[f"f{f}_b{b}_bboxes"]), rel_max_zero_ok(scores[b, :n], g[f"f{f}_b{b}_scores"])
            print(f"[{tag}] frame {f} sample {b}: {n} boxes, rel max boxes {eb:.2e} scores {es:.2e}")
            assert eb < 1e-3 and es < 1e-3
    return worst


def test_a_tiny_stream_fp32x3_against_the_reference():
    g, g64 = np.load(os.path.join(GOLDEN, "head_tiny.npz")), np.load(os.path.join(GOLDEN, "head_tiny_f64.npz"))
    mg = g["margins"]
    assert bool((mg[..., 0] >= float(g["margin_required"]) * mg[..., 1]).all()), "the fixture states its near-tie condition and meets it"
    seed = int(g["seed"])
    h = build(TINY, seed)
    assert h.precision == "fp32x3"
    res, inp = stream(h, TINY, TINY_SHAPE, seed)
    assert len(res) == 4 and inp["frames"][2]["prev_exists"].tolist() == [1.0, 0.0]
    assert g["f0_all_cls_scores"].shape == (2, 2, 28, 10) and g["f3_memory_embedding"].shape == (2, 36, 256)
    check_against_fixture("tiny fp32x3", res, g, g64, TINY)
    # get_bboxes hands out the same survivors per sample as lists
    out, _, dec = res[-1]
    for b, (bboxes, scores, labels) in enumerate(h.get_bboxes(out, inp["img_metas"])):
        n = int(dec[4][b])
        assert torch.equal(bboxes, dec[0][b, :n]) and torch.equal(scores, dec[1][b, :n]) and torch.equal(labels, dec[2][b, :n])


@pytest.mark.parametrize("size,precision", [("tiny", "fp32x3"), ("tiny", "bf16"), ("full", "fp32x3")])
def test_b_head_is_the_chain_of_its_modules_bit_for_bit(size, precision):
    """Two frames; "full" = the shipped sizes (B 1, 6 x 20 x 50 tokens, 644 + 256 queries, 1024 entries, six layers): the M = 6000 token-side launches and the
    six-layer stream through the bank, held to the modules that are each checked against the reference at these sizes."""
    sizes, shape = (TINY, TINY_SHAPE) if size == "tiny" else (synth.HEAD_FULL, synth.HEAD_FULL_SHAPE)
    cfg = synth.head_cfg(sizes)
    sd = synth.head_state_dict(sizes)
    h = build(sizes, precision=precision)
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
    res, inp = stream(h, sizes, shape, frames=2)
    assert tuple(res[0][0]["all_cls_scores"].shape) == ((2, 2, 28, 10) if size == "tiny" else (6, 1, 900, 10))
    for f, data in enumerate(inp["frames"][:2]):
        data = {k: v.to(DEV) for k, v in data.items()}
        # the chain of INTEGRATION.md, by hand
        memory, pos_embed, cone = tokens(data["img_feats"], data["intrinsics"], data["lidar2img"], inp["img_metas"][0]["pad_shape"][0])
        bank.pre_update_memory(data)
        tgt, query_pos, reference_points, temp_memory, temp_pos, rec_ego_pose = queries.forward_from(bank)
        outs_dec, _, _ = decoder(memory, tgt, query_pos, pos_embed, None, temp_memory, temp_pos)
        outs_dec, all_cls_scores, all_bbox_preds = outputs(outs_dec, reference_points)
        bank.post_update_memory(data, rec_ego_pose, all_cls_scores, all_bbox_preds, outs_dec)
        bbox_list = outputs.get_bboxes(dict(all_cls_scores=all_cls_scores, all_bbox_preds=all_bbox_preds), inp["img_metas"])
        out, hbank, dec = res[f]
        assert torch.equal(out["all_cls_scores"], all_cls_scores) and torch.equal(out["all_bbox_preds"], all_bbox_preds), f"{size} {precision} frame {f}: outputs differ"
        for k in BANK:
            assert torch.equal(hbank[k], getattr(bank, k)), f"{precision} frame {f}: {k} differs"
        for b, (bboxes, scores, labels) in enumerate(bbox_list):
            n = int(dec[4][b])
            assert torch.equal(bboxes, dec[0][b, :n]) and torch.equal(scores, dec[1][b, :n]) and torch.equal(labels, dec[2][b, :n])
    assert out["dn_mask_dict"] is None and torch.isfinite(out["all_bbox_preds"]).all()


def test_c_shipped_sizes_frame0_fp32x3_against_the_reference():
    g = np.load(os.path.join(GOLDEN, "head_full_frame0.npz"))
    seed, rows = int(g["seed"]), int(g["row_step"])
    h = build(synth.HEAD_FULL, seed)
    assert h.precision == "fp32x3"
    res, inp = stream(h, synth.HEAD_FULL, synth.HEAD_FULL_SHAPE, seed, frames=1)
    assert tuple(inp["frames"][0]["img_feats"].shape) == (1, 6, 256, 20, 50) and inp["frames"][0]["prev_exists"].tolist() == [0.0]
    out = res[0][0]
    assert tuple(out["all_cls_scores"].shape) == (6, 1, 900, 10) and tuple(out["all_bbox_preds"].shape) == (6, 1, 900, 10)
    for k in ("all_cls_scores", "all_bbox_preds"):
        for key, v in ((f"f0_{k}_last", out[k][-1]), (f"f0_{k}", out[k][:-1, :, ::rows])):
            e, e64 = rel_max_zero_ok(v, g[key]), rel_max_zero_ok(v, g["f64_" + key])
            print(f"[full fp32x3] frame 0 {key}: rel max vs the f32 reference {e:.2e} (vs its f64 twin {e64:.2e}), bar 1e-03")
            assert tuple(v.shape) == g[key].shape and e < 1e-3, (key, e)


def test_d_determinism_reset_and_reload():
    h = build(TINY)
    first, _ = stream(h, TINY, TINY_SHAPE)
    assert h._queries.fresh_builds == 1

    def same(a, b):
        return all(torch.equal(x[0][k], y[0][k]) for x, y in zip(a, b) for k in ("all_cls_scores", "all_bbox_preds")) and \
            all(torch.equal(x[1][k], y[1][k]) for x, y in zip(a, b) for k in BANK)
    h.reset_memory()
    assert h.memory_embedding is None
    again, _ = stream(h, TINY, TINY_SHAPE)
    assert same(first, again), "reset_memory() and the same stream: other bits"
    assert h._queries.fresh_builds == 1 and h._tokens._packed is not None
    # without a reset the bank goes on: frame 0 of the stream says prev_exists = 0 for every sample, so it starts over by itself
    third, _ = stream(h, TINY, TINY_SHAPE)
    assert same(first, third)
    packed = h.transformer._packed
    h.load_state_dict(synth.head_state_dict(TINY), strict=True)
    assert h._bank is None and h._tokens._packed is None and h._queries._fresh is None and h._outputs._packed is None and h.transformer._packed is None
    fourth, _ = stream(h, TINY, TINY_SHAPE)
    assert same(first, fourth), "the same weights loaded again: other bits"
    assert h._queries.fresh_builds == 2 and h.transformer._packed is not packed
    other = build(TINY)
    assert same(first, stream(other, TINY, TINY_SHAPE)[0]), "a second head built from the same weights: other bits"


def test_e_shapes_levels_and_bank_attributes():
    inp = synth.head_inputs(TINY, TINY_SHAPE)
    B, Q = 2, TINY["num_query"] + TINY["num_propagated"]
    outs = {}
    for levels in ("all", "last"):
        h = build(TINY, levels=levels)
        assert all(getattr(h, k) is None for k in BANK)
        center = torch.rand(4, 3, 4, 2, device=DEV)
        keep = center.clone()
        data = {k: v.to(DEV) for k, v in inp["frames"][0].items()}
        out = h(center, inp["img_metas"], None, **data)
        assert torch.equal(center, keep), "memory_center is left as it is"
        L = 2 if levels == "all" else 1
        assert set(out) == {"all_cls_scores", "all_bbox_preds", "dn_mask_dict"} and out["dn_mask_dict"] is None
        assert tuple(out["all_cls_scores"].shape) == (L, B, Q, 10) and tuple(out["all_bbox_preds"].shape) == (L, B, Q, 10)
        n = TINY["memory_len"] + TINY["topk_proposals"]
        assert [tuple(getattr(h, k).shape) for k in BANK] == [(B, n, 256), (B, n, 3), (B, n, 1), (B, n, 4, 4), (B, n, 2)] and h.memory_timestamp.dtype == torch.float64
        bl = h.get_bboxes(out, inp["img_metas"])
        assert len(bl) == B and all(len(x) == 3 and x[0].shape[1] == 9 and x[0].shape[0] == x[1].shape[0] == x[2].shape[0] <= 20 and x[2].dtype == torch.int64 for x in bl)
        q = h.backbone_queries(5, data["prev_exists"].new_ones(B))
        assert q["prev_exists"] is True and tuple(q["temp_queries"].shape) == (B, 5, 256) and tuple(q["temp_ego_pose"].shape) == (B, 5, 4, 4)
        outs[levels] = out
    assert torch.equal(outs["all"]["all_cls_scores"][-1], outs["last"]["all_cls_scores"][0]) and torch.equal(outs["all"]["all_bbox_preds"][-1], outs["last"]["all_bbox_preds"][0])
