"""GPU: HeadTokenEmbedding on sampled tokens (``topk_indexes``).

Against tests/golden/head_tokens_sampled.npz -- the REAL reference's position_embeding with topk_indexes, topk_gather, MLN and SELayer_Linear
(tools/gen_golden_head_tokens_sampled.py) -- at the bars the full-token tests hold head_tokens.npz to in each precision: fp32x3 1e-3 rel max
(tests/test_gpu_head_tokens_x3.py), fp32 2e-4 and bf16 6e-2 (the token-embedding tests of tests/test_gpu_e2e.py, restated), cone 1e-5 in all three.
Bit for bit: a permutation of all LEN tokens against the ``None`` run's rows (the launches have the same M, hence the same tiles: a difference is a finding about
row-position dependence, not a tolerance question), forward against forward_rows, a second frame.  ``None`` launches exactly what it launched before the list
existed (counted through lib.call).  A GEMM row tail (300 tokens, K = 131) and the shipped size (6000 tokens, K = 3000) at the fp32x3 bar."""
import os

import numpy as np
import pytest
import torch

import sampled_cases as SC
import toc3d_amd
from toc3d_amd import lib, synth

from support import DEV, rel_max

pytestmark = pytest.mark.gpu
BARS = {"fp32x3": 1e-3, "fp32": 2e-4, "bf16": 6e-2}
CONE_BAR = 1e-5


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(SC.GOLDEN, "head_tokens_sampled.npz"))


@pytest.mark.parametrize("precision", list(BARS))
def test_matches_reference_golden(golden, precision):
    CFG, B, N, H, W, K = SC.CFG, SC.B, SC.N, SC.H, SC.W, SC.K
    topk = torch.from_numpy(golden["topk_indexes"])
    m = SC.build_tokens(precision)
    inp = synth.head_tokens_inputs(CFG, B, N, H, W)
    memory, pos, cone = SC.run_tokens(m, inp, H, W, CFG["stride"], topk)
    assert tuple(memory.shape) == tuple(pos.shape) == (B, K, CFG["embed_dims"]) and tuple(cone.shape) == (B, K, 8)
    e_cone, e_mem, e_pos = (rel_max(a, torch.from_numpy(golden[k])) for a, k in ((cone, "cone"), (memory, "memory"), (pos, "pos_embed")))
    print(f"[head tokens sampled {precision}] rel max err vs the reference: cone {e_cone:.2e} memory {e_mem:.2e} pos_embed {e_pos:.2e} (bars {CONE_BAR:.0e}, {BARS[precision]:.0e})")
    assert e_cone < CONE_BAR and e_mem < BARS[precision] and e_pos < BARS[precision]
    # (B, K) lists are taken as (B, K, 1) ones are; a second frame on the same inputs gives the same bits
    again = SC.run_tokens(m, inp, H, W, CFG["stride"], topk.view(B, K))
    assert all(torch.equal(a, b) for a, b in zip((memory, pos, cone), again)), "a second frame on the same inputs returns other bits"
    # the None run of the same module is untouched by the sampled workspaces, and the sampled rows are near its rows
    full = SC.run_tokens(m, inp, H, W, CFG["stride"])
    e_full = rel_max(full[0], torch.from_numpy(golden["full_memory"]))
    print(f"[head tokens sampled {precision}] the None run vs the reference's full outputs: memory {e_full:.2e}")
    assert tuple(full[0].shape) == (B, N * H * W, CFG["embed_dims"]) and e_full < BARS[precision]


@pytest.mark.parametrize("precision", list(BARS))
def test_permutation_rows_are_the_none_runs_rows(precision):
    CFG, B, N, H, W = SC.CFG, SC.B, SC.N, SC.H, SC.W
    LEN = N * H * W
    m = SC.build_tokens(precision)
    inp = synth.head_tokens_inputs(CFG, B, N, H, W)
    perm = SC.index_families(B, LEN, seed=5)["permutation"]
    assert perm[0].tolist() != perm[1].tolist() and perm[0].tolist() != list(range(LEN))
    full = SC.run_tokens(m, inp, H, W, CFG["stride"])
    got = SC.run_tokens(m, inp, H, W, CFG["stride"], perm)
    for name, f, s in zip(("memory", "pos_embed", "cone"), full, got):
        want = SC.gather_rows(f, perm.to(DEV))
        bad = (want != s).any(-1).sum().item()
        assert torch.equal(want, s), f"{precision} {name}: {bad} of {B * LEN} permuted rows differ from the None run's rows (row-position dependence)"
    again = SC.run_tokens(m, inp, H, W, CFG["stride"])
    assert all(torch.equal(a, b) for a, b in zip(full, again)), "the None run after a sampled one returns other bits"


@pytest.mark.parametrize("precision", ["fp32x3", "bf16"])
def test_forward_rows_gives_forwards_bits(golden, precision):
    CFG, B, N, H, W, K = SC.CFG, SC.B, SC.N, SC.H, SC.W, SC.K
    topk = torch.from_numpy(golden["topk_indexes"]).to(DEV)
    inp = synth.head_tokens_inputs(CFG, B, N, H, W)
    m = SC.build_tokens(precision)
    want = SC.run_tokens(m, inp, H, W, CFG["stride"], topk)
    other = SC.build_tokens(precision)                                   # its feature rows come from a producer: here toc3d_nchw_to_rows, by hand
    rows, ld, dt = other.feat_workspace(B, N, H, W, DEV)
    assert tuple(rows.shape) == (B * N * H * W, ld), "feat_workspace stays the full-token buffer"
    lib.call("toc3d_nchw_to_rows", dt, inp["feats"].to(DEV).float().contiguous(), rows, ld, B * N, CFG["in_channels"], H * W, lib.stream_ptr())
    got = other.forward_rows((B, N, H, W), inp["intrinsics"].to(DEV), inp["lidar2img"].to(DEV), (H * CFG["stride"], W * CFG["stride"], 3), DEV, topk_indexes=topk)
    assert all(torch.equal(a, b) for a, b in zip(want, got)), f"{precision}: forward_rows and forward differ on the same list"
    assert other.feat_workspace(B, N, H, W, DEV)[0] is rows and set(other._ws) == {(B, N, H, W), (B, N, H, W, K)}, "workspaces are keyed by K as well"


def test_refusals_on_the_device():
    CFG, B, N, H, W = SC.CFG, SC.B, SC.N, SC.H, SC.W
    m = SC.build_tokens("fp32x3")
    inp = synth.head_tokens_inputs(CFG, B, N, H, W)
    for bad, exc in ((torch.zeros(B, 0, 1, dtype=torch.int64), ValueError), (torch.zeros(B, N * H * W + 1, dtype=torch.int64), ValueError),
                     (torch.zeros(B, 3, dtype=torch.int32), ValueError), (torch.zeros(B + 1, 3, 1, dtype=torch.int64), ValueError)):
        with pytest.raises(exc, match="toc3d_amd.HeadTokenEmbedding"):
            SC.run_tokens(m, inp, H, W, CFG["stride"], bad)
    with pytest.raises(RuntimeError, match="CUDA/HIP"):                    # a list on the CPU beside inputs on the device
        m(inp["feats"].to(DEV), inp["intrinsics"].to(DEV), inp["lidar2img"].to(DEV), (48, 64, 3), topk_indexes=torch.zeros(B, 3, 1, dtype=torch.int64))


X3_NONE = ["toc3d_head_frustum_inputs", "toc3d_linear_fused", "toc3d_linear_fused", "toc3d_nchw_to_rows"] + ["toc3d_linear_fused"] * 5 + \
          ["toc3d_mln_apply", "toc3d_linear_fused", "toc3d_linear_fused", "toc3d_se_gate"]
F32_NONE = ["toc3d_head_frustum_inputs", "toc3d_linear", "toc3d_relu_inplace", "toc3d_linear", "toc3d_nchw_to_rows", "toc3d_linear", "toc3d_relu_inplace",
            "toc3d_linear", "toc3d_linear", "toc3d_relu_inplace", "toc3d_linear", "toc3d_linear", "toc3d_mln_apply", "toc3d_linear", "toc3d_relu_inplace",
            "toc3d_linear", "toc3d_se_gate"]


def sampled_list(names):
    """What a list changes: the frustum kernel's sampled form, and the row gather behind toc3d_nchw_to_rows."""
    out = []
    for n in names:
        out.append("toc3d_head_frustum_inputs_sampled" if n == "toc3d_head_frustum_inputs" else n)
        if n == "toc3d_nchw_to_rows":
            out.append("toc3d_gather_token_rows")
    return out


@pytest.mark.parametrize("precision,none_list", [("fp32x3", X3_NONE), ("fp32", F32_NONE)])
def test_none_launches_what_it_launched_before(golden, monkeypatch, precision, none_list):
    CFG, B, N, H, W, K = SC.CFG, SC.B, SC.N, SC.H, SC.W, SC.K
    topk = torch.from_numpy(golden["topk_indexes"])
    inp = synth.head_tokens_inputs(CFG, B, N, H, W)
    m = SC.build_tokens(precision)
    SC.run_tokens(m, inp, H, W, CFG["stride"]), SC.run_tokens(m, inp, H, W, CFG["stride"], topk)        # packs the weights: the counted frames are launches only
    calls, real = [], lib.call
    monkeypatch.setattr(lib, "call", lambda name, *a: (calls.append((name, a)), real(name, *a))[1])
    SC.run_tokens(m, inp, H, W, CFG["stride"])
    names = [n for n, _ in calls]
    assert names == none_list, names
    M_full = B * N * H * W
    if precision == "fp32":
        assert all(a[14] == M_full for n, a in calls if n == "toc3d_linear")
    del calls[:]
    SC.run_tokens(m, inp, H, W, CFG["stride"], topk)
    assert [n for n, _ in calls] == sampled_list(none_list)
    by = {n: a for n, a in calls}
    assert by["toc3d_mln_apply"][4] == B * K and by["toc3d_se_gate"][3] == B * K * CFG["embed_dims"], "the row kernels behind the gather run at M = B*K"
    assert by["toc3d_gather_token_rows"][4:8] == (B, N * H * W, K, CFG["in_channels"])
    if precision == "fp32":
        assert all(a[14] == B * K for n, a in calls if n == "toc3d_linear"), "the nine GEMMs run at M = B*K"


def test_row_tail_300_tokens_131_listed():
    """300 tokens, K = 131: two 128-row tiles with a 3-row tail at embed_dims 256 -- fp32x3 against the fp32 module on the same weights and list at the fp32x3
    bar, cone bit-equal."""
    cfg = dict(synth.HEAD_TOKENS_CFG, in_channels=40)
    inp = synth.head_tokens_inputs(cfg, 1, 2, 10, 15, seed=2)
    g = torch.Generator().manual_seed(131)
    topk = torch.randperm(300, generator=g)[:131].view(1, 131, 1)
    a, b = (SC.run_tokens(SC.build_tokens(p, cfg), inp, 10, 15, 16, topk) for p in ("fp32x3", "fp32"))
    e_mem, e_pos = rel_max(a[0], b[0]), rel_max(a[1], b[1])
    print(f"[head tokens sampled fp32x3, 131 of 300 tokens] rel max vs fp32: memory {e_mem:.2e} pos_embed {e_pos:.2e}")
    assert tuple(a[0].shape) == (1, 131, 256) and e_mem < 1e-3 and e_pos < 1e-3 and torch.equal(a[2], b[2])


def test_shipped_size_3000_of_6000_against_the_oracle():
    """One frame at 6 x 20 x 50 = 6000 tokens, K = 3000, fp32x3, against the oracle restatement on the host, gathered, at the fp32x3 bar."""
    from oracle import head_tokens_oracle as HO
    cfg = synth.HEAD_TOKENS_CFG
    sd = synth.head_tokens_state_dict(cfg, seed=1)
    inp = synth.head_tokens_inputs(cfg, 1, 6, 20, 50, seed=1)
    g = torch.Generator().manual_seed(3000)
    idx = torch.randperm(6000, generator=g)[:3000].view(1, 3000)
    m = toc3d_amd.HeadTokenEmbedding(precision="fp32x3", **cfg)
    m.load_state_dict(sd)
    memory, pos, cone = SC.run_tokens(m.to(DEV).eval(), inp, 20, 50, 16, idx.view(1, 3000, 1))
    assert tuple(memory.shape) == tuple(pos.shape) == (1, 3000, 256) and tuple(cone.shape) == (1, 3000, 8)
    with torch.no_grad():
        _, rc = HO.position_embedding(sd, cfg, inp["intrinsics"], inp["lidar2img"], 20, 50, 320, 800)
        rm, rp = HO.token_embeddings(sd, cfg, inp["feats"], inp["intrinsics"], inp["lidar2img"], 320, 800)
    e_mem, e_pos, e_cone = rel_max(memory, SC.gather_rows(rm, idx)), rel_max(pos, SC.gather_rows(rp, idx)), rel_max(cone, SC.gather_rows(rc, idx))
    print(f"[head tokens sampled fp32x3, 3000 of 6000 tokens] rel max vs the oracle: memory {e_mem:.2e} pos_embed {e_pos:.2e} cone {e_cone:.2e}")
    assert e_mem < 1e-3 and e_pos < 1e-3 and e_cone < CONE_BAR
