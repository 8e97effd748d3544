"""GPU: the token side of the head in "fp32x3" -- the row kernels' (hi, lo) planes output and HeadTokenEmbedding(precision="fp32x3").

Row kernels (toc3d_head_frustum_inputs, toc3d_nchw_to_rows, toc3d_mln_apply with TOC3D_DTYPE_F32X3P) at 1, 5 and 24 tokens: the planes image holds the f32 kernel's
output in the planes' representation -- hi = bf16(x), lo = bf16(x - hi) (x - hi is exact in f32, so the residual x - hi - lo is the bf16 rounding error of the
remainder) --, the plain f32 outputs are the bits of the F32 dtype's, and nothing outside the valid rows and columns is written (canaries).
The module: against tests/golden/head_tokens.npz at the project's fp32x3 bar (1e-3 rel max; cone 1e-5), and its launch list -- no toc3d_relu_inplace on "fp32x3",
the parent's sequence with its four ReLU launches on "fp32"."""
import os

import numpy as np
import pytest
import torch

import toc3d_amd
from toc3d_amd import lib, synth

from support import DEV, S, bits, canary, is_canary, planes_decode, rel_max, rnd

pytestmark = pytest.mark.gpu
TOKENS = {1: (1, 1, 1, 1), 5: (1, 1, 1, 5), 24: (2, 2, 2, 3)}          # tokens -> (B, N, h, w)


def check_planes(tag, planes, plain, M, width):
    """planes [rows, ld] (canary-filled before the launch) against the F32 kernel's plain [rows, ld] (likewise): columns [0, width) of rows [0, M)."""
    hi, lo = planes_decode(planes)
    x = plain[:M, :width]
    want_hi = x.to(torch.bfloat16).float()
    assert torch.equal(hi[:M, :width], want_hi), f"{tag}: hi plane is not bf16(x)"
    assert torch.equal(lo[:M, :width], (x - want_hi).to(torch.bfloat16).float()), f"{tag}: lo plane is not bf16(x - hi)"
    rem = (x - want_hi).double()
    assert bool(((rem - lo[:M, :width].double()).abs() <= 2.0 ** -8 * rem.abs()).all()), f"{tag}: residual outside bf16 of the remainder"
    # nothing else was written, in either layout: the canary decodes to hi = lo = 9.0
    assert bool(is_canary(plain[M:]).all()) and bool(is_canary(plain[:M, width:]).all()), f"{tag}: the F32 kernel wrote outside [0, {M}) x [0, {width})"
    assert bool(is_canary(planes[M:]).all()), f"{tag}: rows >= {M} of the planes buffer were written"
    assert bool((hi[:M, width:] == 9.0).all()) and bool((lo[:M, width:] == 9.0).all()), f"{tag}: columns >= {width} of the planes buffer were written"


@pytest.mark.parametrize("D", [64, 33])
@pytest.mark.parametrize("tokens", list(TOKENS))
def test_frustum_inputs_planes(tokens, D):
    B, N, h, w = TOKENS[tokens]
    cfg = dict(synth.HEAD_TOKENS_TINY, depth_num=D)
    inp = synth.head_tokens_inputs(cfg, B, N, h, w, seed=tokens)
    m = toc3d_amd.HeadTokenEmbedding(**cfg)                                 # (for coords_d and the host position_range)
    i2l = torch.linalg.inv(inp["lidar2img"].reshape(B * N, 4, 4)).contiguous().to(DEV)
    intr = inp["intrinsics"].reshape(B * N, 4, 4).contiguous().to(DEV)
    cd = m.coords_d.to(DEV)
    M, ld = tokens, (3 * D + 63) // 64 * 64
    out = {}
    for name, dt in (("f32", lib.F32), ("planes", lib.F32X3P)):
        pin, ca, cone = canary(M + 3, ld, torch.float32), canary(M + 3, 64, torch.float32), canary(M + 3, 8, torch.float32)
        lib.call("toc3d_head_frustum_inputs", dt, i2l, intr, cd, m._pr, B, N, h, w, D, 16, h * 16, w * 16, pin, ld, ca, 64, cone, S())
        out[name] = (pin, ca, cone)
    tag = f"frustum {tokens} tokens D={D}"
    check_planes(tag + " pos_in", out["planes"][0], out["f32"][0], M, 3 * D)
    check_planes(tag + " cone_act", out["planes"][1], out["f32"][1], M, 8)
    assert torch.equal(bits(out["planes"][2]), bits(out["f32"][2])), f"{tag}: the f32 cone depends on the dtype"
    assert bool(is_canary(out["f32"][2][M:]).all()) and torch.equal(out["f32"][2][:M], out["f32"][1][:M, :8])


@pytest.mark.parametrize("C", [32, 40])
@pytest.mark.parametrize("tokens", list(TOKENS))
def test_nchw_to_rows_planes(tokens, C):
    V, hw = {1: (1, 1), 5: (1, 5), 24: (4, 6)}[tokens]
    x = rnd(V, C, hw, seed=tokens + C).to(DEV).contiguous()
    out = {}
    for name, dt in (("f32", lib.F32), ("planes", lib.F32X3P)):
        o = canary(tokens + 3, 64, torch.float32)
        lib.call("toc3d_nchw_to_rows", dt, x, o, 64, V, C, hw, S())
        out[name] = o
    assert torch.equal(out["f32"][:tokens, :C], x.permute(0, 2, 1).reshape(tokens, C))
    check_planes(f"nchw_to_rows {tokens} tokens C={C}", out["planes"], out["f32"], tokens, C)


@pytest.mark.parametrize("E", [64, 256])
@pytest.mark.parametrize("tokens", list(TOKENS))
def test_mln_apply_planes(tokens, E):
    M = tokens
    x, g, b = (3.0 * rnd(M, E, seed=1 + E) + 0.5).to(DEV), (1.0 + 0.3 * rnd(M, E, seed=2 + E)).to(DEV), rnd(M, E, seed=3 + E).to(DEV)
    out = {}
    for name, dt in (("f32", lib.F32), ("planes", lib.F32X3P)):
        o, oa = canary(M + 3, E, torch.float32), canary(M + 3, E + 32, torch.float32)
        lib.call("toc3d_mln_apply", dt, x, g, b, M, E, o, oa, E + 32, S())
        out[name] = (o, oa)
    tag = f"mln_apply {M} rows E={E}"
    assert torch.equal(bits(out["planes"][0]), bits(out["f32"][0])), f"{tag}: the f32 output depends on the dtype"
    assert torch.equal(out["f32"][0][:M], out["f32"][1][:M, :E]) and bool(is_canary(out["f32"][0][M:]).all())
    ref = g.double() * torch.nn.functional.layer_norm(x.double(), (E,), eps=1e-5) + b.double()
    assert rel_max(out["f32"][0][:M], ref) < 1e-5
    check_planes(tag, out["planes"][1], out["f32"][1], M, E)


# ---- the module ----------------------------------------------------------------------------------------------------------------------------------------------
def build(precision, cfg):
    m = toc3d_amd.HeadTokenEmbedding(precision=precision, **cfg)
    m.load_state_dict(synth.head_tokens_state_dict(cfg), strict=True)
    return m.to(DEV).eval()


def run(m, inp, H, W, stride):
    return m(inp["feats"].to(DEV), inp["intrinsics"].to(DEV), inp["lidar2img"].to(DEV), (H * stride, W * stride, 3))


def test_fp32x3_matches_reference_golden(golden_dir):
    from oracle.gen_golden_head import CFG, B, N, H, W
    g = np.load(os.path.join(golden_dir, "head_tokens.npz"))
    m = build("fp32x3", CFG)
    inp = synth.head_tokens_inputs(CFG, B, N, H, W)
    memory, pos, cone = run(m, inp, H, W, CFG["stride"])
    e_cone, e_mem, e_pos = rel_max(cone, torch.from_numpy(g["cone"])), rel_max(memory, torch.from_numpy(g["memory"])), rel_max(pos, torch.from_numpy(g["pos_embed"]))
    print(f"[head tokens fp32x3] rel max err vs the reference: cone {e_cone:.2e} memory {e_mem:.2e} pos_embed {e_pos:.2e}")
    assert e_cone < 1e-5 and e_mem < 1e-3 and e_pos < 1e-3
    again = run(m, inp, H, W, CFG["stride"])
    assert all(torch.equal(a, b) for a, b in zip((memory, pos, cone), again)), "a second frame on the same inputs returns other bits"
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        m(inp["feats"], inp["intrinsics"], inp["lidar2img"], (64, 96))


PARENT_SEQUENCE = ["toc3d_head_frustum_inputs", "toc3d_linear", "toc3d_relu_inplace", "toc3d_linear", "toc3d_nchw_to_rows", "toc3d_linear", "toc3d_relu_inplace",
                   "toc3d_linear", "toc3d_linear", "toc3d_relu_inplace", "toc3d_linear", "toc3d_linear", "toc3d_mln_apply", "toc3d_linear", "toc3d_relu_inplace",
                   "toc3d_linear", "toc3d_se_gate"]


def test_launch_lists(monkeypatch):
    """Counted through lib.call: "fp32x3" issues nine GEMMs with the ReLU in four epilogues and no toc3d_relu_inplace; "fp32" and "bf16" keep the sequence they had
    before the epilogue existed (two launches per Linear + ReLU), in their own dtype."""
    from oracle.gen_golden_head import CFG, B, N, H, W
    inp = synth.head_tokens_inputs(CFG, B, N, H, W)
    mods = {p: build(p, CFG) for p in ("fp32x3", "fp32", "bf16")}
    outs = {p: run(m, inp, H, W, CFG["stride"]) for p, m in mods.items()}     # packs the weights: the counted frame is launches only
    calls, real = [], lib.call
    monkeypatch.setattr(lib, "call", lambda name, *a: (calls.append((name, a)), real(name, *a))[1])
    for p, m in mods.items():
        del calls[:]
        got = run(m, inp, H, W, CFG["stride"])
        names = [n for n, _ in calls]
        assert all(torch.equal(a, b) for a, b in zip(got, outs[p])), p
        if p == "fp32x3":
            assert "toc3d_relu_inplace" not in names and "toc3d_linear" not in names
            gemms = [a for n, a in calls if n == "toc3d_linear_fused"]
            assert [a[1] for a in gemms] == [lib.EPI_BIAS_RELU, lib.EPI_RESIDUAL, lib.EPI_BIAS_RELU, lib.EPI_RESIDUAL, lib.EPI_BIAS_RELU, lib.EPI_RESIDUAL, lib.EPI_RESIDUAL,
                                             lib.EPI_BIAS_RELU, lib.EPI_RESIDUAL]
            # A in planes where a row kernel wrote it, plain behind a ReLU epilogue; W in planes throughout
            assert [a[0] for a in gemms] == [lib.F32X3WA, lib.F32X3W] * 3 + [lib.F32X3W, lib.F32X3WA, lib.F32X3W]
            assert [n for n in names if n != "toc3d_linear_fused"] == ["toc3d_head_frustum_inputs", "toc3d_nchw_to_rows", "toc3d_mln_apply", "toc3d_se_gate"]
            assert all(a[0] == lib.F32X3P for n, a in calls if n in ("toc3d_head_frustum_inputs", "toc3d_nchw_to_rows", "toc3d_mln_apply"))
        else:
            dt = lib.F32 if p == "fp32" else lib.BF16
            assert names == PARENT_SEQUENCE and names.count("toc3d_relu_inplace") == 4
            assert all(a[0] == dt for n, a in calls if n != "toc3d_se_gate")
            assert [a[1] for n, a in calls if n == "toc3d_linear"] == [lib.EPI_BIAS, lib.EPI_RESIDUAL] * 2 + [lib.EPI_BIAS, lib.EPI_RESIDUAL, lib.EPI_RESIDUAL, lib.EPI_BIAS, lib.EPI_RESIDUAL]
    # the same weights, three precisions: fp32x3 sits with fp32, far inside what bf16 does
    e3, eb = rel_max(outs["fp32x3"][0], outs["fp32"][0]), rel_max(outs["bf16"][0], outs["fp32"][0])
    print(f"[head tokens] memory rel max vs fp32: fp32x3 {e3:.2e}, bf16 {eb:.2e}")
    assert e3 < 1e-3 and torch.equal(outs["fp32x3"][2], outs["fp32"][2])


def test_fp32x3_more_than_one_tile():
    """300 tokens (three 128-row tiles, a row tail) at embed_dims 256: against the fp32 module on the same weights, at the fp32x3 bar."""
    cfg = dict(synth.HEAD_TOKENS_CFG, in_channels=40)
    inp = synth.head_tokens_inputs(cfg, 1, 2, 10, 15, seed=2)
    a, b = run(build("fp32x3", cfg), inp, 10, 15, 16), run(build("fp32", cfg), inp, 10, 15, 16)
    e_mem, e_pos = rel_max(a[0], b[0]), rel_max(a[1], b[1])
    print(f"[head tokens fp32x3, 300 tokens] rel max vs fp32: memory {e_mem:.2e} pos_embed {e_pos:.2e}")
    assert e_mem < 1e-3 and e_pos < 1e-3 and torch.equal(a[2], b[2])


def test_fp32x3_shipped_size_against_the_oracle_and_fp32():
    """The shipped sizes -- 6 views x 20 x 50 = 6000 tokens, 256 channels, E 256, 64 LID bins: the M = 6000 launches of the assembled head, the default-tile
    N = 1024, K = 192 EPI_BIAS_RELU GEMM on planes among them -- against the oracle on the host (the reference-derived numbers of
    test_gpu_e2e.py::test_head_token_embedding_full_size_matches_oracle) at the fp32x3 bar, and against the fp32 module on the same weights."""
    from oracle import head_tokens_oracle as HO
    cfg = synth.HEAD_TOKENS_CFG
    sd = synth.head_tokens_state_dict(cfg, seed=1)
    inp = synth.head_tokens_inputs(cfg, 1, 6, 20, 50, seed=1)
    outs = {}
    for precision in ("fp32x3", "fp32"):
        m = toc3d_amd.HeadTokenEmbedding(precision=precision, **cfg)
        m.load_state_dict(sd)
        outs[precision] = run(m.to(DEV).eval(), inp, 20, 50, 16)
    memory, pos, cone = outs["fp32x3"]
    assert tuple(memory.shape) == (1, 6000, 256) and tuple(pos.shape) == (1, 6000, 256) and tuple(cone.shape) == (1, 6000, 8)
    with torch.no_grad():
        rm, rp = HO.token_embeddings(sd, cfg, inp["feats"], inp["intrinsics"], inp["lidar2img"], 320, 800)
    e_mem, e_pos = rel_max(memory, rm), rel_max(pos, rp)
    f_mem, f_pos = rel_max(memory, outs["fp32"][0]), rel_max(pos, outs["fp32"][1])
    print(f"[head tokens fp32x3, 6000 tokens] rel max vs the oracle: memory {e_mem:.2e} pos_embed {e_pos:.2e}; vs the fp32 module: {f_mem:.2e} {f_pos:.2e}")
    assert e_mem < 1e-3 and e_pos < 1e-3 and f_mem < 1e-3 and f_pos < 1e-3 and torch.equal(cone, outs["fp32"][2])
