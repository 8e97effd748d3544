"""GPU: FocalHead.select_rows / select -- the selection-only frame (conv of the class tower alone, one-branch statistics, toc3d_focal_sample_weight, the
ranking) -- against FocalHead.forward_rows' ``topk_indexes`` and ``sample_weight``, bit for bit.

This is the check of the conv variant: the class-only conv (N = E) must give the class-tower columns of the two-tower conv (N = 2E) bit for bit, so it is launched
with the tile variant of the full-width shape; where that variant is 0 (the library's heuristic, M >= 16k rows: the B = 4 case) the selection runs the full-width
conv and reads its first E columns.  Sizes: FOCAL_HEAD_TINY (B = 1, N = 2, 3 x 5), B = 2 of it, the shipped 6 x 20 x 50 at infer_ratio 0.5, and B = 4 of the
shipped shape; both precisions, plan and eager, three frames with changing inputs (eager, recorded, replayed in the plan mode).

Against the fixtures of the REAL reference (tests/golden/focal_head_{tiny,full}.npz): the top-K sets of ``select`` are held to the band rule and the limits of
tests/test_gpu_focal_head.py -- a token whose golden sample_weight lies outside a band of 2 x OUR measured max error around the golden K-th value is in our set
exactly when it is in the golden's, and the band holds at most 0.5 % (fp32x3) / 10 % (bf16) of the tokens.  Every test prints the figures it asserts on."""
import os

import numpy as np
import pytest
import torch

import focal_head_cases as FC
from support import DEV, S, same_bits
from toc3d_amd import FocalHead, lib, synth
from toc3d_amd import focal_head as focal_head_module

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BAND_MAX_SHARE = {"fp32x3": 0.005, "bf16": 0.10}                     # tests/test_gpu_focal_head.py's limits
SHAPES = dict(tiny=(synth.FOCAL_HEAD_TINY, synth.FOCAL_HEAD_TINY_SHAPE), tiny_b2=(synth.FOCAL_HEAD_TINY, dict(synth.FOCAL_HEAD_TINY_SHAPE, B=2)),
              full=(synth.FOCAL_HEAD_FULL, synth.FOCAL_HEAD_FULL_SHAPE), full_b4=(synth.FOCAL_HEAD_FULL, dict(synth.FOCAL_HEAD_FULL_SHAPE, B=4)))


def build(sizes, precision, launch_mode, seed=0):
    m = FocalHead(**sizes, precision=precision, launch_mode=launch_mode)
    m.load_state_dict(synth.focal_head_state_dict(sizes, seed=seed))
    return m.to(DEV)


def token_rows(m, feats):
    B, N, C, h, w = feats.shape
    rows = torch.zeros(B * N * h * w, C, dtype=torch.bfloat16 if m.precision == "bf16" else torch.float32, device=DEV)
    lib.call("toc3d_nchw_to_rows", lib.BF16 if m.precision == "bf16" else lib.F32, feats.to(DEV).contiguous(), rows, C, B * N, C, h * w, S())
    return rows


@pytest.mark.parametrize("launch_mode", ["plan", "eager"])
@pytest.mark.parametrize("precision", ["fp32x3", "bf16"])
@pytest.mark.parametrize("tag", list(SHAPES))
def test_select_equals_forward_rows_bit_for_bit(tag, precision, launch_mode):
    sizes, shape = SHAPES[tag]
    B, N, h, w, C, E = shape["B"], shape["N"], shape["h"], shape["w"], sizes["in_channels"], sizes["embed_dims"]
    M, n = B * N * h * w, N * h * w
    K = int(n * sizes["infer_ratio"])
    m = build(sizes, precision, launch_mode)
    variant = focal_head_module.gemm.small_m_variant(M, 2 * E, 9 * C, False)
    assert (variant == 0) == (tag == "full_b4"), "B = 4 of the shipped shape is the case the library's heuristic serves"
    rows = None
    for frame in range(3):
        inp = synth.focal_head_inputs(sizes, shape, seed=200 + frame)
        loc = inp["location"].to(DEV)
        rows = token_rows(m, inp["img_feats"]) if rows is None else rows.copy_(token_rows(m, inp["img_feats"]))     # one buffer: the recorded plans name it
        want = m.forward_rows(loc, rows, C, B, N, h, w)
        got = m.select_rows(loc, rows, C, B, N, h, w)
        assert set(got) == {"topk_indexes", "sample_weight"}
        assert got["topk_indexes"].dtype == torch.int64 and tuple(got["topk_indexes"].shape) == (B, K, 1) and tuple(got["sample_weight"].shape) == (B, n, 1)
        assert same_bits(got["sample_weight"], want["sample_weight"]), f"frame {frame}: {int((got['sample_weight'] != want['sample_weight']).sum())} weights differ"
        assert torch.equal(got["topk_indexes"], want["topk_indexes"]), f"frame {frame}: topk_indexes differ"
        sel = m.select(loc, img_feats=inp["img_feats"].to(DEV))
        assert same_bits(sel["sample_weight"], want["sample_weight"]) and torch.equal(sel["topk_indexes"], want["topk_indexes"]), f"frame {frame}: select differs"
        W = m._ws[(B, N, h, w)]
        assert all(t.data_ptr() not in (W["select"]["weight"].data_ptr(), W["select"]["order"].data_ptr(), W["weight"].data_ptr(), W["order"].data_ptr())
                   for t in got.values()), "the outputs are freshly allocated"
    print(f"[{tag} {precision} {launch_mode}] M = {M}, K = {K} of {n}, conv variant {variant}: select_rows and select equal forward_rows over three frames")
    names = [name for name, _ in m._select_launches((B, N, h, w), m._ws[(B, N, h, w)], rows, K)]
    assert names == ["conv3x3", "gn_stats", "sample_weight", "rank_desc"]
    state = m._states.get(("select_rows", (B, N, h, w), K, rows.data_ptr()))
    if launch_mode == "plan":
        assert state["cplan"] is not None and state["cplan"].num_launches == 4, "the four launches, replayed from one plan of their own"
        assert m._states[("rows", (B, N, h, w), K, rows.data_ptr())]["cplan"].num_launches == 4, "forward_rows keeps its own plan"
        assert m._states[("select", (B, N, h, w), K)]["cplan"].num_launches == 5, "select: nchw_to_rows + the four"
    else:
        assert state is None or state.get("cplan") is None


@pytest.mark.parametrize("precision", ["fp32x3", "bf16"])
@pytest.mark.parametrize("tag", ["tiny", "full"])
def test_plan_replay_and_eager_give_the_same_bits_over_three_frames(tag, precision):
    sizes, shape = SHAPES[tag]
    B, N, h, w, C = shape["B"], shape["N"], shape["h"], shape["w"], sizes["in_channels"]
    plan, eager = build(sizes, precision, "plan"), build(sizes, precision, "eager")
    rows, seen = None, []
    for frame in range(3):                               # frame 0 launches eagerly in both, 1 records, 2 replays
        inp = synth.focal_head_inputs(sizes, shape, seed=300 + frame)
        loc = inp["location"].to(DEV)
        rows = token_rows(plan, inp["img_feats"]) if rows is None else rows.copy_(token_rows(plan, inp["img_feats"]))
        a, b = plan.select_rows(loc, rows, C, B, N, h, w), eager.select_rows(loc, rows, C, B, N, h, w)
        assert same_bits(a["sample_weight"], b["sample_weight"]) and torch.equal(a["topk_indexes"], b["topk_indexes"]), f"frame {frame}"
        seen.append(a["sample_weight"].cpu())
    state, = plan._states.values()
    assert state["cplan"] is not None and state["cplan"].num_launches == 4 and all(s.get("cplan") is None for s in eager._states.values())
    assert not torch.equal(seen[1], seen[2]), "the inputs changed between the recorded and the replayed frame"


def test_no_ranking_when_nothing_is_kept_and_the_refusals_are_forward_rows():
    sizes, shape = SHAPES["tiny"]
    m = build(dict(sizes, infer_ratio=0.0), "fp32x3", "eager")
    inp = synth.focal_head_inputs(sizes, shape)
    B, N, h, w, C = 1, 2, 3, 5, 64
    rows = token_rows(m, inp["img_feats"])
    out = m.select_rows(inp["location"].to(DEV), rows, C, B, N, h, w)
    assert tuple(out["topk_indexes"].shape) == (1, 0, 1) and out["topk_indexes"].dtype == torch.int64
    assert [name for name, _ in m._select_launches((B, N, h, w), m._ws[(B, N, h, w)], rows, 0)] == ["conv3x3", "gn_stats", "sample_weight"]
    assert same_bits(out["sample_weight"], m.forward_rows(inp["location"].to(DEV), rows, C, B, N, h, w)["sample_weight"])
    name = "toc3d_amd.FocalHead"
    with pytest.raises(ValueError, match=name):
        m.select_rows(inp["location"].to(DEV), rows.to(torch.bfloat16), C, B, N, h, w)
    with pytest.raises(ValueError, match=name):
        m.select_rows(inp["location"][:1].to(DEV), rows, C, B, N, h, w)
    with pytest.raises(ValueError, match=name):
        m.select(inp["location"].to(DEV), img_feats=inp["img_feats"][:, :, :32].to(DEV))
    with pytest.raises(RuntimeError, match="no CPU"):
        m.select(inp["location"], img_feats=inp["img_feats"])


def test_row_plans_stay_within_max_row_states():
    sizes, shape = SHAPES["tiny"]
    m = build(sizes, "fp32x3", "plan")
    inp = synth.focal_head_inputs(sizes, shape)
    loc = inp["location"].to(DEV)
    bufs = [token_rows(m, inp["img_feats"]) for _ in range(focal_head_module.MAX_ROW_STATES + 2)]
    for rows in bufs:
        m.select_rows(loc, rows, 64, 1, 2, 3, 5)
    assert len(m._states) == focal_head_module.MAX_ROW_STATES and all(k[0] == "select_rows" for k in m._states)
    assert [k[3] for k in m._states] == [b.data_ptr() for b in bufs[2:]], "the oldest recordings went first"


@pytest.mark.parametrize("precision", ["fp32x3", "bf16"])
@pytest.mark.parametrize("tag", ["tiny", "full"])
def test_selected_sets_against_the_golden(tag, precision):
    sizes, shape = FC.SIZES[tag]
    gold = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(GOLDEN, f"focal_head_{tag}.npz")).items()}
    seed = int(gold["seed"])
    inp = synth.focal_head_inputs(sizes, shape, seed=seed)
    m = build(sizes, precision, "plan", seed=seed)
    for _ in range(3):                                   # eager warm-up, recording, replay: the replayed frame is the one checked
        out = {k: v.cpu() for k, v in m.select(inp["location"].to(DEV), img_feats=inp["img_feats"].to(DEV)).items()}
    B, n = shape["B"], shape["N"] * shape["h"] * shape["w"]
    K = int(n * sizes["infer_ratio"])
    wg, wo = gold["sample_weight"].reshape(B, n), out["sample_weight"].reshape(B, n)
    half = 2.0 * (wo.double() - wg.double()).abs().max(1).values
    outside, share = FC.index_band(wg, K, half)
    ours, theirs = FC.membership(out["topk_indexes"], n), FC.membership(gold["topk_indexes"], n)
    wrong = int(((ours != theirs) & outside).sum())
    print(f"[{tag} {precision}] K = {K} of {n}: band half-width {half.tolist()} holds {share.tolist()} of the tokens (limit {BAND_MAX_SHARE[precision]}); "
          f"{int((ours != theirs).sum())} tokens differ in membership, {wrong} of them outside the band")
    assert bool((share <= BAND_MAX_SHARE[precision]).all()), "the band of our own error is too wide to decide anything"
    assert wrong == 0
    assert bool((ours.sum(1) == K).all()), "K distinct indices per sample"
    assert torch.equal(out["topk_indexes"].view(B, K), torch.sort(wo, dim=1, descending=True, stable=True).indices[:, :K])
