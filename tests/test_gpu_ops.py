"""GPU: every C-ABI entry point against the oracle / plain torch fp32 on the same seeded inputs.

Tolerances: index outputs bit-exact; f32 path 1e-5..1e-4 relative (summation order only); bf16 path is
compared with a reference that sees the same bf16-rounded operands, so only accumulation order and the
final bf16 rounding (2^-8 relative) differ.
"""
import os

import numpy as np
import pytest
import torch

from oracle import toc3d_oracle as O
from support import DEV, S, _pack_scorer, _run_topk, as_act, pack, planes_decode, relerr, rnd, ru, to_planes
from toc3d_amd import configs, lib, synth

pytestmark = pytest.mark.gpu
DTYPES = [("fp32", lib.F32, torch.float32), ("bf16", lib.BF16, torch.bfloat16)]


# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dt,tdt", DTYPES)
@pytest.mark.parametrize("M,N,K", [(300, 200, 128), (128, 128, 64), (1000, 384, 192), (6000, 1024, 768), (37, 3072, 1024)])
def test_linear_bias_gelu_residual(name, dt, tdt, M, N, K):
    A, W, b = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5), rnd(N, seed=3)
    res = rnd(M, N, seed=4)
    Ar, Wr = (A.to(tdt).float(), W.to(tdt).float())           # what the kernel sees
    ref = Ar.double() @ Wr.double().T + b.double()
    a_d, w_d = as_act(A, tdt), pack(W, dt, tdt)
    Kp = a_d.shape[1]
    tol_out = 1e-5 if dt == lib.F32 else 6e-3
    out = torch.full((M, N + 8), 7.0, dtype=tdt, device=DEV)
    lib.call("toc3d_linear", dt, lib.EPI_BIAS, a_d, Kp, w_d, Kp, b.to(DEV), out, N + 8, None, 0, 0, None, None, M, N, Kp, 0, S())
    assert relerr(out[:, :N].float(), ref) < tol_out
    assert (out[:, N:].float() == 7.0).all(), "wrote outside [0, N)"
    lib.call("toc3d_linear", dt, lib.EPI_GELU, a_d, Kp, w_d, Kp, b.to(DEV), out, N + 8, None, 0, 0, None, None, M, N, Kp, 0, S())
    assert relerr(out[:, :N].float(), torch.nn.functional.gelu(ref)) < tol_out
    # residual epilogue, in place, with representative-row capture (period 5) and modular residual rows
    o32 = res.to(DEV).clone()
    period = 5
    rep = torch.zeros(M // period + 1, N, device=DEV)
    rep_index = torch.full((M,), -1, dtype=torch.int32)
    rep_index[period - 1::period] = torch.arange(len(rep_index[period - 1::period]), dtype=torch.int32)
    lib.call("toc3d_linear", dt, lib.EPI_RESIDUAL, a_d, Kp, w_d, Kp, b.to(DEV), o32, N, o32, N, 0, rep, rep_index.to(DEV), M, N, Kp, 0, S())
    assert relerr(o32, res.double() + ref) < 2e-5
    rows = torch.arange(period - 1, M, period)
    assert relerr(rep[: len(rows)], ref[rows]) < 2e-5
    pos = rnd(7, N, seed=5)
    o2 = torch.empty(M, N, device=DEV)
    lib.call("toc3d_linear", dt, lib.EPI_RESIDUAL, a_d, Kp, w_d, Kp, b.to(DEV), o2, N, pos.to(DEV), N, 7, None, None, M, N, Kp, 0, S())
    assert relerr(o2, ref + pos.double()[torch.arange(M) % 7]) < 2e-5
    o3 = torch.empty(M, N, device=DEV)
    lib.call("toc3d_linear", dt, lib.EPI_RESIDUAL, a_d, Kp, w_d, Kp, None, o3, N, None, 0, 0, None, None, M, N, Kp, 0, S())
    assert relerr(o3, ref - b.double()) < 2e-5


@pytest.mark.parametrize("name,dt,tdt", DTYPES)
@pytest.mark.parametrize("M,Hd,K", [(257, 341, 128), (700, 2730, 1024)])
def test_linear_swiglu(name, dt, tdt, M, Hd, K):
    A = rnd(M, K, seed=1)
    w1, w2 = rnd(Hd, K, seed=2, scale=K ** -0.5), rnd(Hd, K, seed=3, scale=K ** -0.5)
    b1, b2 = rnd(Hd, seed=4), rnd(Hd, seed=5)
    Hp = ru(Hd, 64)
    w12 = torch.empty(2 * Hp, K, dtype=tdt, device=DEV)
    b12 = torch.empty(2 * Hp, device=DEV)
    lib.call("toc3d_pack_swiglu", dt, w1.to(DEV), w2.to(DEV), b1.to(DEV), b2.to(DEV), Hd, K, w12, b12, Hp, K, S())
    a_d = as_act(A, tdt)
    out = torch.full((M, Hp), 3.0, dtype=tdt, device=DEV)
    lib.call("toc3d_linear", dt, lib.EPI_SWIGLU, a_d, K, w12, K, b12, out, Hp, None, 0, 0, None, None, M, 2 * Hp, K, Hd, S())
    Ar = A.to(tdt).double()
    x1 = Ar @ w1.to(tdt).double().T + b1.double()
    x2 = Ar @ w2.to(tdt).double().T + b2.double()
    ref = torch.nn.functional.silu(x1) * x2
    assert relerr(out[:, :Hd].float(), ref) < (1e-5 if dt == lib.F32 else 6e-3)
    assert (out[:, Hd:].float() == 0).all(), "hidden padding must be written as zeros"


@pytest.mark.parametrize("name,dt,tdt", DTYPES)
def test_patch_embed_and_abs_pos(name, dt, tdt, golden_dir):
    cfg = configs.get("toc3d_tiny")
    sd = synth.make_state_dict(cfg)
    img = synth.make_inputs(cfg, views_per_frame=2)["x"]
    V, C = 2, cfg["embed_dim"]
    h, w = 20, 50
    pe = sd["pos_embed"][0, 1:].contiguous().to(DEV)
    pos = torch.empty(h * w, C, device=DEV)
    lib.call("toc3d_abs_pos_bicubic", pe, 14, C, pos, h, w, S())
    ref_pos = O.abs_pos(sd["pos_embed"], True, (h, w)).reshape(h * w, C)
    assert relerr(pos, ref_pos) < 1e-5
    g = np.load(os.path.join(golden_dir, "units.npz"))
    for hh, ww in ((20, 50), (40, 100), (50, 100)):
        o = torch.empty(hh * ww, 16, device=DEV)
        lib.call("toc3d_abs_pos_bicubic", torch.from_numpy(g["abs_pos.in"])[0, 1:].contiguous().to(DEV), 14, 16, o, hh, ww, S())
        assert relerr(o.view(1, hh, ww, 16), torch.from_numpy(g[f"abs_pos.{hh}x{ww}"])) < 1e-5
    col = torch.empty(V * h * w, 768, dtype=tdt, device=DEV)
    lib.call("toc3d_im2col_patches", dt, img.to(DEV), col, 768, V, 3, 320, 800, 16, S())
    wp = pack(sd["patch_embed.proj.weight"].reshape(C, -1), dt, tdt)
    x = torch.empty(V * h * w, C, device=DEV)
    lib.call("toc3d_linear", dt, lib.EPI_RESIDUAL, col, 768, wp, 768, sd["patch_embed.proj.bias"].to(DEV), x, C, pos, C, h * w, None, None,
             V * h * w, C, 768, 0, S())
    ref = O.stem(sd, cfg, img).reshape(-1, C)
    assert relerr(x, ref) < (1e-5 if dt == lib.F32 else 1e-2)


@pytest.mark.parametrize("name,dt,tdt", DTYPES)
@pytest.mark.parametrize("C", [128, 1024])
def test_layernorm_rows(name, dt, tdt, C):
    M = 203
    x, gw, gb = rnd(M + 5, C, seed=1) * 3 + 0.5, 1 + 0.1 * rnd(C, seed=2), 0.1 * rnd(C, seed=3)
    idx = torch.randint(0, M + 5, (M,), generator=torch.Generator().manual_seed(4)).int()
    idx[::17] = -1
    scale = torch.rand(M + 5, generator=torch.Generator().manual_seed(5))
    out = torch.empty(M, C, dtype=tdt, device=DEV)
    tol = 2e-5 if dt == lib.F32 else 5e-3
    lib.call("toc3d_layernorm_rows", dt, x.to(DEV), C, None, None, gw.to(DEV), gb.to(DEV), 1e-6, out, C, M, C, S())
    assert relerr(out.float(), O.layer_norm(x[:M], gw, gb)) < tol
    lib.call("toc3d_layernorm_rows", dt, x.to(DEV), C, idx.to(DEV), scale.to(DEV), gw.to(DEV), gb.to(DEV), 1e-5, out, C, M, C, S())
    src = torch.where(idx[:, None] >= 0, x[idx.clamp_min(0).long()] * scale[idx.clamp_min(0).long()][:, None], torch.zeros(M, C))
    assert relerr(out.float(), O.layer_norm(src, gw, gb, 1e-5)) < tol


@pytest.mark.parametrize("name,dt,tdt", DTYPES)
@pytest.mark.parametrize("n,ld", [(341, 384), (2730, 2752), (100, 128)])
def test_layernorm_act(name, dt, tdt, n, ld):
    M = 131
    x, gw, gb = rnd(M, n, seed=1) * 2 + 0.3, 1 + 0.1 * rnd(n, seed=2), 0.1 * rnd(n, seed=3)
    xd = as_act(x, tdt, ld)
    out = torch.full((M, ld), 5.0, dtype=tdt, device=DEV)
    lib.call("toc3d_layernorm_act", dt, xd, ld, gw.to(DEV), gb.to(DEV), 1e-6, out, ld, M, n, S())
    ref = O.layer_norm(x.to(tdt).float(), gw, gb)
    assert relerr(out[:, :n].float(), ref) < (2e-5 if dt == lib.F32 else 5e-3)
    assert (out[:, n:].float() == 0).all()


# ---------------------------------------------------------------------------------------------------
def _attention_ref(x_rows, sd, pre, heads, cos, sin):
    return O.attention(x_rows[None], sd, pre, heads, cos, sin)[0]


@pytest.mark.parametrize("name,dt,tdt", DTYPES)
@pytest.mark.parametrize("L", [16, 20])
def test_window_attention_dense_with_virtual_pads(name, dt, tdt, L):
    """Block.forward attention part (eva_vit.py:249-262): LN -> zero-pad -> window attention; pads folded analytically."""
    cfg = configs.get("toc3d_tiny")
    sd = synth.make_state_dict(cfg)
    C, heads, V, h, w = cfg["embed_dim"], cfg["num_heads"], 2, 20, 50
    pre = "blocks.2.attn." if L == 20 else "blocks.0.attn."
    y = rnd(V, h, w, C, seed=7)                                     # stands for LN1(x)
    yw, pad_hw = O.window_partition(y, L)
    nB = yw.shape[0]
    # reference up to (not including) proj: recompute attention core with identity proj
    sd2 = dict(sd)
    sd2[pre + "proj.weight"], sd2[pre + "proj.bias"] = torch.eye(C), torch.zeros(C)
    ref = O.attention(yw.reshape(nB, L * L, C), sd2, pre, heads, sd[pre + "rope.freqs_cos"], sd[pre + "rope.freqs_sin"])
    ref = O.window_unpartition(ref.reshape(nB, L, L, C), L, pad_hw, (h, w)).reshape(-1, C)
    # device: qkv of the real tokens only
    wqkv = torch.cat([sd[pre + "q_proj.weight"], sd[pre + "k_proj.weight"], sd[pre + "v_proj.weight"]])
    bqkv = torch.cat([sd[pre + "q_bias"], torch.zeros(C), sd[pre + "v_bias"]])
    M = V * h * w
    a_d = as_act(y.reshape(M, C), tdt)
    qkv = torch.empty(M, 3 * C, dtype=tdt, device=DEV)
    lib.call("toc3d_linear", dt, lib.EPI_BIAS, a_d, C, pack(wqkv, dt, tdt), C, bqkv.to(DEV), qkv, 3 * C, None, 0, 0, None, None, M, 3 * C, C, 0, S())
    nW, N = nB, L * L
    rows = torch.empty(nW, N, dtype=torch.int32, device=DEV)
    slots, count, npad = torch.empty_like(rows), torch.empty(nW, dtype=torch.int32, device=DEV), torch.empty(nW, dtype=torch.int32, device=DEV)
    lib.call("toc3d_window_map_dense", V, h, w, L, rows, slots, count, npad, S())
    assert int(count.sum()) == M and int((count + npad).min()) == N
    out = torch.zeros(M, C, dtype=tdt, device=DEV)
    lib.call("toc3d_window_attention", dt, qkv, 3 * C, out, C, rows, slots, count, None, npad, None, N, nW, int(count.max()), heads,
             sd[pre + "rope.freqs_cos"].to(DEV), sd[pre + "rope.freqs_sin"].to(DEV), L, sd[pre + "v_bias"].to(DEV), 64 ** -0.5, S())
    err = relerr(out.float(), ref)
    assert err < (5e-5 if dt == lib.F32 else 3e-2), err


@pytest.mark.parametrize("name,dt,tdt", DTYPES)
def test_window_attention_is_bit_stable_with_co_resident_workgroups(name, dt, tdt):
    """Regression for the packed-FP32 erratum (LABNOTES.md): with more attention workgroups than CUs (several per CU) the
    bf16 kernel built with v_pk_fma_f32 returned slightly different K tiles from launch to launch.  Same inputs, many
    launches, every output must be bit-identical -- and equal to the launch made on an otherwise idle GPU."""
    V, h, w, L, C, heads = 12, 20, 50, 16, 128, 2
    M, N = V * h * w, L * L
    nW = V * 2 * 4
    qkv = as_act(rnd(M, 3 * C, seed=3), tdt)
    rows = torch.empty(nW, N, dtype=torch.int32, device=DEV)
    slots, count, npad = torch.empty_like(rows), torch.empty(nW, dtype=torch.int32, device=DEV), torch.empty(nW, dtype=torch.int32, device=DEV)
    lib.call("toc3d_window_map_dense", V, h, w, L, rows, slots, count, npad, S())
    cosT, sinT, vb = rnd(N, 64, seed=4).to(DEV), rnd(N, 64, seed=5).to(DEV), rnd(C, seed=6).to(DEV)
    outs = [torch.zeros(M, C, dtype=tdt, device=DEV) for _ in range(12)]
    for o in outs:
        lib.call("toc3d_window_attention", dt, qkv, 3 * C, o, C, rows, slots, count, None, npad, None, N, nW, int(count.max()), heads,
                 cosT, sinT, L, vb, 0.125, S())
    torch.cuda.synchronize()
    for o in outs[1:]:
        assert torch.equal(o.view(torch.uint8), outs[0].view(torch.uint8))


@pytest.mark.parametrize("name,dt,tdt", DTYPES)
@pytest.mark.parametrize("n", [77, 129, 201])
def test_window_attention_selected_slots(name, dt, tdt, n):
    """ToC3DEVAAttention (toc3d_eva_vit.py:484-518): compact rows, RoPE rows gathered by slot index."""
    cfg = configs.get("toc3d_tiny")
    sd = synth.make_state_dict(cfg)
    C, heads, nW = cfg["embed_dim"], cfg["num_heads"], 5
    pre = "blocks.5.attn."
    cosT, sinT = sd[pre + "rope.freqs_cos"], sd[pre + "rope.freqs_sin"]        # 400-row table
    y = rnd(nW, n, C, seed=11)
    g = torch.Generator().manual_seed(12)
    slots = torch.stack([torch.randperm(400, generator=g)[:n] for _ in range(nW)])
    sd2 = dict(sd)
    sd2[pre + "proj.weight"], sd2[pre + "proj.bias"] = torch.eye(C), torch.zeros(C)
    ref = O.attention(y, sd2, pre, heads, cosT[slots], sinT[slots]).reshape(-1, C)
    wqkv = torch.cat([sd[pre + "q_proj.weight"], sd[pre + "k_proj.weight"], sd[pre + "v_proj.weight"]])
    bqkv = torch.cat([sd[pre + "q_bias"], torch.zeros(C), sd[pre + "v_bias"]])
    M = nW * n
    qkv = torch.empty(M, 3 * C, dtype=tdt, device=DEV)
    lib.call("toc3d_linear", dt, lib.EPI_BIAS, as_act(y.reshape(M, C), tdt), C, pack(wqkv, dt, tdt), C, bqkv.to(DEV), qkv, 3 * C, None, 0, 0,
             None, None, M, 3 * C, C, 0, S())
    rows = torch.arange(M, dtype=torch.int32).reshape(nW, n).to(DEV)
    count = torch.full((nW,), n, dtype=torch.int32, device=DEV)
    out = torch.zeros(M, C, dtype=tdt, device=DEV)
    lib.call("toc3d_window_attention", dt, qkv, 3 * C, out, C, rows, slots.int().to(DEV), count, None, None, None, n, nW, n, heads,
             cosT.to(DEV), sinT.to(DEV), 20, None, 64 ** -0.5, S())
    err = relerr(out.float(), ref)
    assert err < (5e-5 if dt == lib.F32 else 3e-2), err


# ---------------------------------------------------------------------------------------------------
def test_rank_desc_is_a_stable_descending_sort():
    g = torch.Generator().manual_seed(3)
    for B, n in ((6, 1000), (2, 5000), (3, 17)):
        sc = torch.randn(B, n, generator=g)
        sc[:, ::7] = sc[:, 3:4]                                   # plenty of exact ties
        sc[0, : n // 2] = -1e6
        sc[1, 1], sc[1, 5], sc[1, 9] = 0.0, -0.0, 0.0             # signed zeros compare equal: slot order decides
        sc[1, 2], sc[1, 11] = float("-inf"), float("inf")
        order = torch.empty(B, n, dtype=torch.int64, device=DEV)
        lib.call("toc3d_rank_desc", sc.to(DEV), B, n, order, S())
        ref = torch.sort(sc, dim=1, descending=True, stable=True)[1]
        assert torch.equal(order.cpu(), ref)


@pytest.mark.parametrize("L,ratio", [(16, 0.5), (16, 0.3), (20, 0.4), (20, 0.7), (7, 0.5), (14, 0.6), (33, 0.3), (64, 0.1)])
def test_window_topk_matches_oracle(L, ratio):
    V, h, w = 3, 20, 50
    g = torch.Generator().manual_seed(5)
    scores = -torch.rand(V, h, w, generator=g) * 4
    scores[1, :5] = scores[1, 0, 0]                                  # ties among real tokens
    N = L * L
    k = int(N * ratio)
    sw, _ = O.window_partition(scores[..., None], L, pad_value=O.PAD_SCORE)
    nW = sw.shape[0]
    sw = sw.reshape(nW, N)
    s_sorted, ref_order = O.sort_desc_stable(sw)
    b = _run_topk(scores, V, h, w, L, k)
    assert torch.equal(b["order"].cpu().long(), ref_order)
    idx_img = torch.arange(V * h * w, dtype=torch.float32).reshape(V, h, w, 1)
    iw, _ = O.window_partition(idx_img, L, pad_value=-1)
    ref_tok = torch.gather(iw.reshape(nW, N), 1, ref_order).long()
    assert torch.equal(b["tok"].cpu().long(), ref_tok)
    fast = s_sorted[:, k:]
    assert (b["wgt"][:, :k] == 0).all()
    assert relerr(b["wgt"][:, k:], fast / fast.sum(dim=1, keepdim=True)) < 1e-5
    # compact kept set: kept real tokens in sorted order, representative last; kept pads become virtual keys
    tok, prow, crow, repi = (b[x].cpu().long() for x in ("tok", "prow", "crow_tok", "rep_index"))
    arows, aslots, cq, ck, rep_row = (b[x].cpu().long() for x in ("arows", "aslots", "acount_q", "acount_k", "rep_row"))
    off = 0
    for i in range(nW):
        real_kept = [p for p in range(k) if ref_tok[i, p] >= 0]
        n_real = int((ref_tok[i] >= 0).sum())
        cap = min(k, n_real) + 1
        assert cq[i] == cap and ck[i] == k + 1 and rep_row[i] == off + cap - 1
        assert crow[off:off + cap - 1].tolist() == [int(ref_tok[i, p]) for p in real_kept]
        assert crow[off + cap - 1] == -2 and repi[off + cap - 1] == i and (repi[off:off + cap - 1] == -1).all()
        assert prow[i, real_kept].tolist() == list(range(off, off + cap - 1))
        pads_kept = [p for p in range(k) if ref_tok[i, p] < 0]
        assert (prow[i, pads_kept] == -1).all()
        assert arows[i, :cap].tolist() == list(range(off, off + cap))
        assert aslots[i, :cap - 1].tolist() == [int(ref_order[i, p]) for p in real_kept] and aslots[i, cap - 1] == k
        assert (arows[i, cap:] == -1).all() and aslots[i, cap:].tolist() == [int(ref_order[i, p]) for p in pads_kept]
        off += cap
    assert off == b["ms"]


@pytest.mark.parametrize("name,dt,tdt", DTYPES)
@pytest.mark.parametrize("C,L,ratio", [(128, 16, 0.5), (1024, 20, 0.3)])
def test_gather_merge_ln_and_scatter(name, dt, tdt, C, L, ratio):
    V, h, w = 2, 20, 50
    g = torch.Generator().manual_seed(9)
    x = torch.randn(V, h, w, C, generator=g)
    scores = -torch.rand(V, h, w, generator=g) * 3 - 0.1
    gw, gb = 1 + 0.1 * rnd(C, seed=2), 0.1 * rnd(C, seed=3)
    N = L * L
    k = int(N * ratio)
    xw, pad_hw = O.window_partition(x, L)
    sw, _ = O.window_partition(scores[..., None], L, pad_value=O.PAD_SCORE)
    nW = xw.shape[0]
    xw, sw = xw.reshape(nW, N, C), sw.reshape(nW, N)
    s_sorted, order = O.sort_desc_stable(sw)
    slow = O.gather_rows(xw, order[:, :k])
    rep = O.merge_tokens(O.gather_rows(xw, order[:, k:]), s_sorted[:, k:])
    ref_short = torch.cat([slow, rep], 1)                            # (nW, k+1, C), pads included
    ref_ln = O.layer_norm(ref_short, gw, gb)
    b = _run_topk(scores, V, h, w, L, k)
    ms = b["ms"]
    xd = x.reshape(-1, C).to(DEV).contiguous()
    short = torch.empty(ms, C, device=DEV)
    a = torch.empty(ms, C, dtype=tdt, device=DEV)
    lib.call("toc3d_gather_merge_ln", dt, xd, C, b["tok"], b["wgt"], b["crow_tok"], b["rep_row"], nW, N, k, ms, gw.to(DEV), gb.to(DEV), 1e-6,
             short, a, C, S())
    # map compact rows back to (window, position) of the reference's padded layout
    prow, rep_row = b["prow"].cpu().long(), b["rep_row"].cpu().long()
    for i in range(nW):
        kept = (prow[i, :k] >= 0).nonzero()[:, 0]
        rows_i = torch.cat([prow[i, kept], rep_row[i:i + 1]])
        pos_i = torch.cat([kept, torch.tensor([k])])
        assert relerr(short[rows_i], ref_short[i, pos_i]) < 1e-5
        assert relerr(a[rows_i].float(), ref_ln[i, pos_i]) < (2e-5 if dt == lib.F32 else 5e-3)
    # the split merge (4 workgroups per window, partials through device memory, last arriver adds them in the single-workgroup kernel's order): the
    # same bits, launch after launch on one scratch buffer (the kernel re-arms its arrival counters), with and without the f32 copy of the kept rows
    nbytes = int(lib.load().toc3d_gather_merge_ln_scratch_bytes(nW, C))
    assert nbytes >= nW * 16 * C * 4 + nW * 4 and nbytes % 256 == 0
    scratch = torch.zeros(nbytes // 4, device=DEV)
    for kept_copy in (1, 0, 1):
        one_s, one_a = torch.full((ms, C), 7.0, device=DEV), torch.zeros(ms, C, dtype=tdt, device=DEV)
        lib.call("toc3d_gather_merge_ln_ex", dt, xd, C, b["tok"], b["wgt"], b["crow_tok"], b["rep_row"], nW, N, k, ms, gw.to(DEV), gb.to(DEV), 1e-6,
                 one_s, one_a, C, kept_copy, S())
        for rep_i in range(3):
            sp_s, sp_a = torch.full((ms, C), 7.0, device=DEV), torch.zeros(ms, C, dtype=tdt, device=DEV)
            lib.call("toc3d_gather_merge_ln_split", dt, xd, C, b["tok"], b["wgt"], b["crow_tok"], b["rep_row"], nW, N, k, ms, gw.to(DEV), gb.to(DEV), 1e-6,
                     sp_s, sp_a, C, kept_copy, scratch, nbytes, (0, 8, 16)[rep_i], S())
            assert torch.equal(sp_s, one_s) and torch.equal(sp_a.view(torch.uint8), one_a.view(torch.uint8)), (kept_copy, rep_i)
        assert int(scratch[:nW].view(torch.int32).abs().sum().item()) == 0, "arrival counters re-armed"
        if kept_copy:
            assert torch.equal(one_s, short) and torch.equal(one_a, a)
    with pytest.raises(RuntimeError, match="scratch"):
        lib.call("toc3d_gather_merge_ln_split", dt, xd, C, b["tok"], b["wgt"], b["crow_tok"], b["rep_row"], nW, N, k, ms, gw.to(DEV), gb.to(DEV), 1e-6,
                 sp_s, sp_a, C, 1, scratch, nbytes - 256, 0, S())
    # scatter: kept rows replaced, dropped rows += r1 + r2, pads dropped (toc3d_eva_vit.py:449-467)
    slow_c = torch.randn(ms, C, generator=g)
    slow_out = torch.zeros(nW, k + 1, C)
    for i in range(nW):
        kept = (prow[i, :k] >= 0).nonzero()[:, 0]
        slow_out[i, kept] = slow_c[prow[i, kept]]
    r1, r2 = torch.randn(nW, C, generator=g), torch.randn(nW, C, generator=g)
    fast = O.gather_rows(xw, order[:, k:]) + r1[:, None] + r2[:, None]
    outw = torch.zeros_like(xw)
    outw.scatter_(1, order[:, :k, None].expand(-1, -1, C), slow_out[:, :k])
    outw.scatter_(1, order[:, k:, None].expand(-1, -1, C), fast)
    ref_x = O.window_unpartition(outw.reshape(nW, L, L, C), L, pad_hw, (h, w)).reshape(-1, C)
    lib.call("toc3d_scatter_update", xd, C, b["tok"], b["prow"], nW, N, k, slow_c.to(DEV), r1.to(DEV), r2.to(DEV), None, None, S())
    assert relerr(xd, ref_x) < 1e-6


@pytest.mark.parametrize("name,dt,tdt", DTYPES)
def test_attention_virtual_pad_keys_equal_explicit_pad_rows(name, dt, tdt):
    """toc3d_eva_vit.py:414,421,372: kept padded slots are LN(0)=beta rows.  Feeding them as virtual keys (rows=-1 +
    pad_qkv) must give the real rows exactly the output they get when the pads are explicit rows."""
    cfg = configs.get("toc3d_tiny")
    sd = synth.make_state_dict(cfg)
    C, heads, nW, n_real, n_pad = cfg["embed_dim"], cfg["num_heads"], 3, 37, 60
    pre = "blocks.3.attn."
    cosT, sinT = sd[pre + "rope.freqs_cos"].to(DEV), sd[pre + "rope.freqs_sin"].to(DEV)
    beta_row = (0.1 * rnd(1, C, seed=21)).to(tdt).float()                     # stands for LN1(0) = beta
    y = torch.cat([rnd(nW, n_real, C, seed=22), beta_row.expand(nW, n_pad, C)], 1)
    n = n_real + n_pad
    gsl = torch.Generator().manual_seed(23)
    slots = torch.stack([torch.randperm(256, generator=gsl)[:n] for _ in range(nW)]).int()
    wqkv = pack(torch.cat([sd[pre + "q_proj.weight"], sd[pre + "k_proj.weight"], sd[pre + "v_proj.weight"]]), dt, tdt)
    bqkv = torch.cat([sd[pre + "q_bias"], torch.zeros(C), sd[pre + "v_bias"]]).to(DEV)
    M = nW * n
    qkv = torch.empty(M, 3 * C, dtype=tdt, device=DEV)
    lib.call("toc3d_linear", dt, lib.EPI_BIAS, as_act(y.reshape(M, C), tdt), C, wqkv, C, bqkv, qkv, 3 * C, None, 0, 0, None, None, M, 3 * C, C, 0, S())
    rows = torch.arange(M, dtype=torch.int32).reshape(nW, n).to(DEV)
    cnt = torch.full((nW,), n, dtype=torch.int32, device=DEV)
    full = torch.zeros(M, C, dtype=tdt, device=DEV)
    lib.call("toc3d_window_attention", dt, qkv, 3 * C, full, C, rows, slots.to(DEV), cnt, None, None, None, n, nW, n, heads, cosT, sinT, 16, None, 64 ** -0.5, S())
    # virtual: only the real rows are queries; pads are keys taken from pad_qkv
    pad_qkv = qkv[n_real:n_real + 1].clone()
    rows_v = rows.clone()
    rows_v[:, n_real:] = -1
    cq = torch.full((nW,), n_real, dtype=torch.int32, device=DEV)
    virt = torch.zeros(M, C, dtype=tdt, device=DEV)
    lib.call("toc3d_window_attention", dt, qkv, 3 * C, virt, C, rows_v, slots.to(DEV), cq, cnt, None, pad_qkv, n, nW, n_real, heads, cosT, sinT, 16, None,
             64 ** -0.5, S())
    fr = full.view(nW, n, C)[:, :n_real].float()
    vr = virt.view(nW, n, C)[:, :n_real].float()
    assert torch.equal(fr, vr)
    assert (virt.view(nW, n, C)[:, n_real:] == 0).all(), "pad rows must not be written"


# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epoch", [False, True])
def test_query_scorer_against_reference_fixture(golden_dir, epoch):
    """Motion-aware queries + collapsed cross-attention scorer + Gumbel mask vs the REAL reference's outputs."""
    g = np.load(os.path.join(golden_dir, "scorer_toc3d_tiny.npz"))
    fl = "epoch" if epoch else "u01"
    cfg = configs.get("toc3d_tiny")
    sd = synth.make_state_dict(cfg)
    pre = "score_predictor.1."
    C = cfg["embed_dim"]
    inp = synth.make_inputs(cfg, views_per_frame=2, epoch_timestamps=epoch)
    mw = _pack_scorer(sd, pre)
    B, Q = 1, 64
    d = lambda t: t.to(DEV).contiguous()
    mq = torch.empty(B, Q, 256, device=DEV)
    lib.call("toc3d_motion_queries", mw, 1, 0, d(inp["temp_queries"]), d(inp["temp_ref_points"]), d(inp["temp_vel"]), d(inp["temp_timestamp"]), 1,
             d(inp["temp_ego_pose"]), d(inp["ego_pose_inv"]), B, Q, mq, S())
    ref_mq = torch.from_numpy(g[f"{fl}.mq"])
    # measured bound (tests/scorer_cases.py): the f32 oracle's own distance E_cpu from the f64 evaluation of the same inputs; the kernel gets 4 x that against
    # f64, and against the fixture's f32 values the fixture's own share on top (the real reference is an f32 evaluation like the oracle: one more E_cpu)
    import scorer_cases as SC
    case = dict(queries=inp["temp_queries"], ref_points=inp["temp_ref_points"], vel=inp["temp_vel"], timestamp=inp["temp_timestamp"],
                ego_pose=inp["temp_ego_pose"], ego_pose_inv=inp["ego_pose_inv"])
    with torch.no_grad():
        ref64 = SC.motion_ref64(sd, case, pre=pre)
        e_cpu = (O.motion_aware_queries(sd, pre, *SC.motion_args(case)).double() - ref64).abs().max().item()
    assert e_cpu <= SC.MOTION_CONDITION * ref64.abs().max().item()
    err64 = (mq.cpu().double() - ref64).abs().max().item()
    err = (mq.cpu() - ref_mq).abs().max().item()
    print(f"[scorer fixture] {fl}: E_cpu {e_cpu:.3e}  device vs f64 {err64:.3e}  device vs fixture {err:.3e}")
    assert err64 <= SC.MOTION_FACTOR * e_cpu, f"motion-aware queries: {err64} vs f64, 4 x E_cpu = {4 * e_cpu}"
    assert err <= (SC.MOTION_FACTOR + 1) * e_cpu, f"motion-aware queries max abs err {err} vs the fixture"
    # f32 timestamps take the other branch; must agree with the oracle run on f32 timestamps
    if not epoch:
        mq32 = torch.empty_like(mq)
        lib.call("toc3d_motion_queries", mw, 1, 0, d(inp["temp_queries"]), d(inp["temp_ref_points"]), d(inp["temp_vel"]), d(inp["temp_timestamp"].float()), 0,
                 d(inp["temp_ego_pose"]), d(inp["ego_pose_inv"]), B, Q, mq32, S())
        r32 = O.motion_aware_queries(sd, pre, inp["temp_queries"], inp["temp_ref_points"], inp["temp_vel"], inp["temp_timestamp"].float(),
                                     inp["temp_ego_pose"], inp["ego_pose_inv"])
        with torch.no_grad():
            ref64_32 = SC.motion_ref64(sd, dict(case, timestamp=inp["temp_timestamp"].float()), pre=pre)
        e32 = (r32.double() - ref64_32).abs().max().item()
        assert e32 <= SC.MOTION_CONDITION * ref64_32.abs().max().item()
        err64_32, err32 = (mq32.cpu().double() - ref64_32).abs().max().item(), (mq32.cpu() - r32).abs().max().item()
        print(f"[scorer fixture] f32 timestamps: E_cpu {e32:.3e}  device vs f64 {err64_32:.3e}  device vs f32 oracle {err32:.3e}")
        assert err64_32 <= SC.MOTION_FACTOR * e32 and err32 <= (SC.MOTION_FACTOR + 1) * e32
    x = torch.from_numpy(synth._rng("scorer/x").standard_normal((2, 20, 50, C), dtype=np.float32))
    m = torch.from_numpy(synth._rng("scorer/m").random((2, 20, 50, 1), dtype=np.float32))
    wc, bc = torch.empty(B, C, 2, device=DEV), torch.empty(B, 2, device=DEV)
    lib.call("toc3d_collapse_query_scorer", d(ref_mq), d(sd[pre + "input_proj.0.weight"]), d(sd[pre + "input_proj.0.bias"]),
             d(sd[pre + "aggregate.0.weight"]), d(sd[pre + "aggregate.0.bias"]), B, Q, C, 256 ** -0.5, wc, bc, S())
    M, T = 2000, 1000
    pred, score, mask = torch.empty(M, 2, device=DEV), torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    lib.call("toc3d_score_tokens", d(x.reshape(M, C)), C, d(m.reshape(M)), wc, bc, d(inp["gumbel"][1].reshape(M, 2)), 2, T, 2, pred, score, mask, S())
    ref_pred = torch.from_numpy(g[f"{fl}.pred_query"]).reshape(M, 2)
    assert (pred.cpu() - ref_pred).abs().max().item() < 5e-5
    assert torch.equal(score.cpu(), pred.cpu()[:, 0])
    assert (mask.cpu() - torch.from_numpy(g[f"{fl}.mask"]).reshape(M)).abs().max().item() < 5e-5
    order = torch.empty(2, T, dtype=torch.int64, device=DEV)
    lib.call("toc3d_rank_desc", d(ref_pred[:, 0].contiguous()), 2, T, order, S())
    k = int(T * cfg["token_ratio"][1])
    assert np.array_equal(order[:, :k].cpu().numpy(), g[f"{fl}.keep_idx"]) and np.array_equal(order[:, k:].cpu().numpy(), g[f"{fl}.drop_idx"])


@pytest.mark.parametrize("name,dt,tdt", DTYPES)
def test_first_frame_scorer(name, dt, tdt, golden_dir):
    """ScoreBasedTokenSelector.score (toc3d_utils.py:114-129) through the C ABI vs the reference fixture."""
    g = np.load(os.path.join(golden_dir, "scorer_toc3d_tiny.npz"))
    cfg = configs.get("toc3d_tiny")
    sd = synth.make_state_dict(cfg)
    pre = "score_predictor.1."
    C, V, T = cfg["embed_dim"], 2, 1000
    M = V * T
    x = torch.from_numpy(synth._rng("scorer/x").standard_normal((V, 20, 50, C), dtype=np.float32)).reshape(M, C).to(DEV)
    m = torch.from_numpy(synth._rng("scorer/m").random((V, 20, 50, 1), dtype=np.float32)).reshape(M).to(DEV)
    f = lambda k: sd[pre + k].to(DEV)
    a = torch.empty(M, C, dtype=tdt, device=DEV)
    t_act = torch.empty(M, C, dtype=tdt, device=DEV)
    u1 = torch.zeros(M, 64, dtype=tdt, device=DEV)
    u2 = torch.zeros(M, 64, dtype=tdt, device=DEV)
    lib.call("toc3d_layernorm_rows", dt, x, C, None, m, f("in_conv.0.weight"), f("in_conv.0.bias"), 1e-5, a, C, M, C, S())
    w_ic, w_o0, w_o2 = pack(sd[pre + "in_conv.1.weight"], dt, tdt), pack(sd[pre + "out_conv.0.weight"], dt, tdt), pack(sd[pre + "out_conv.2.weight"], dt, tdt)
    lib.call("toc3d_linear", dt, lib.EPI_GELU, a, C, w_ic, C, f("in_conv.1.bias"), t_act, C, None, 0, 0, None, None, M, C, C, 0, S())
    lib.call("toc3d_global_mean_half", dt, t_act, C, V, T, C, S())
    lib.call("toc3d_linear", dt, lib.EPI_GELU, t_act, C, w_o0, C, f("out_conv.0.bias"), u1, 64, None, 0, 0, None, None, M, C // 2, C, 0, S())
    lib.call("toc3d_linear", dt, lib.EPI_GELU, u1, 64, w_o2, 64, f("out_conv.2.bias"), u2, 64, None, 0, 0, None, None, M, C // 4, 64, 0, S())
    pred, score, mask = torch.empty(M, 2, device=DEV), torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    lib.call("toc3d_score_head", dt, u2, 64, C // 4, f("out_conv.4.weight"), f("out_conv.4.bias"), None, M, pred, score, mask, S())
    ref = torch.from_numpy(g["u01.pred_score"]).reshape(M, 2)
    err = (pred.cpu() - ref).abs().max().item()
    assert err < (5e-5 if dt == lib.F32 else 3e-2), err
    assert (mask.cpu() - torch.softmax(pred.cpu(), -1)[:, 0]).abs().max().item() < 1e-6


@pytest.mark.parametrize("name,dt,tdt", DTYPES)
def test_nhwc_to_nchw_and_im2col3x3(name, dt, tdt):
    V, h, w, C = 2, 20, 50, 32
    x = rnd(V, h, w, C, seed=3)
    out = torch.empty(V, C, h * w, device=DEV)
    lib.call("toc3d_nhwc_to_nchw", x.to(DEV), out, V, h * w, C, S())
    assert torch.equal(out.cpu().view(V, C, h, w), x.permute(0, 3, 1, 2))
    col = torch.zeros(V * h * w, 320, dtype=tdt, device=DEV)
    lib.call("toc3d_im2col_3x3", dt, x.to(DEV), col, 320, V, h, w, C, S())
    ref = torch.nn.functional.unfold(x.permute(0, 3, 1, 2), 3, padding=1)              # (V, C*9, T) ordered (c, ky, kx)
    ref = ref.view(V, C, 9, h * w).permute(0, 3, 2, 1).reshape(V * h * w, 9 * C)       # -> (ky,kx,c)
    assert relerr(col[:, : 9 * C].float(), ref.to(tdt).float()) == 0


@pytest.mark.parametrize("name,dt,tdt", DTYPES)
def test_linear_variants_are_bit_identical(name, dt, tdt):
    """Every tile / pipeline variant of toc3d_linear_ex accumulates K in the same order: outputs must be bit-equal."""
    M, N, K = 777, 640, 512
    A, W, b = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5), rnd(N, seed=3)
    a_d, w_d = as_act(A, tdt), pack(W, dt, tdt)
    ref = None
    every = list(range(1, 11)) + list(range(13, 30)) + [32, 33, 43, 44, 45, 46, 47, 48, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58, 154, 157, 110, 116, 126, 145, 147, 149, 151, 152, 214, 216, 217, 219, 226, 249, 314, 316, 317, 319, 326, 349]
    for v in [v for v in every + ([30, 60, 61, 62, 63, 64, 65, 66, 160, 163, 164] if dt == lib.BF16 else []) if lib.has_variant(v)]:
        out = torch.zeros(M, N, dtype=tdt, device=DEV)
        lib.call("toc3d_linear_ex", dt, lib.EPI_BIAS, v, a_d, K, w_d, K, b.to(DEV), out, N, None, 0, 0, None, None, M, N, K, 0, S())
        if ref is None:
            ref = out.clone()
            assert relerr(ref.float(), A.to(tdt).double() @ W.to(tdt).double().T + b.double()) < (1e-5 if dt == lib.F32 else 6e-3)
        else:
            assert torch.equal(out, ref), f"variant {v} differs"
    with pytest.raises(RuntimeError, match="variant"):
        lib.call("toc3d_linear_ex", dt, lib.EPI_BIAS, 99, a_d, K, w_d, K, b.to(DEV), out, N, None, 0, 0, None, None, M, N, K, 0, S())
    # the other epilogues across all variants: residual (+ modular residual rows) and SwiGLU
    res = rnd(M, N, seed=4).to(DEV)
    Hd, Hp = 300, 320
    w12 = torch.empty(2 * Hp, K, dtype=tdt, device=DEV)
    b12 = torch.empty(2 * Hp, device=DEV)
    lib.call("toc3d_pack_swiglu", dt, rnd(Hd, K, seed=5, scale=K ** -0.5).to(DEV), rnd(Hd, K, seed=6, scale=K ** -0.5).to(DEV), rnd(Hd, seed=7).to(DEV),
             rnd(Hd, seed=8).to(DEV), Hd, K, w12, b12, Hp, K, S())
    ref_r = ref_s = None
    for v in [v for v in every + ([60, 61, 62, 63, 64, 65, 66] if dt == lib.BF16 else []) if lib.has_variant(v)]:
        o32 = torch.zeros(M, N, device=DEV)
        lib.call("toc3d_linear_ex", dt, lib.EPI_RESIDUAL, v, a_d, K, w_d, K, b.to(DEV), o32, N, res, N, 0, None, None, M, N, K, 0, S())
        ref_r = o32.clone() if ref_r is None else ref_r
        assert torch.equal(o32, ref_r), f"residual epilogue: variant {v} differs"
        hid = torch.full((M, Hp), 9.0, dtype=tdt, device=DEV)
        if v in (33, 43, 44, 45, 46, 48, 145, 52, 53, 152):        # per-wave column slabs that are not whole (w1, w2) 32-column groups
            with pytest.raises(RuntimeError, match="cannot serve"):
                lib.call("toc3d_linear_ex", dt, lib.EPI_SWIGLU, v, a_d, K, w12, K, b12, hid, Hp, None, 0, 0, None, None, M, 2 * Hp, K, Hd, S())
            continue
        lib.call("toc3d_linear_ex", dt, lib.EPI_SWIGLU, v, a_d, K, w12, K, b12, hid, Hp, None, 0, 0, None, None, M, 2 * Hp, K, Hd, S())
        ref_s = hid.clone() if ref_s is None else ref_s
        assert torch.equal(hid, ref_s), f"swiglu epilogue: variant {v} differs"


@pytest.mark.parametrize("K", [64, 128, 192, 256, 1024, 2752])
def test_phased_tiles_every_ktile_count_and_bit_stable_under_load(K):
    """The phased big tiles (variants 60-63, 160) run a two-K-tile LDS ring whose B fragments are read one phase ahead into alternating register sets
    (gemm_kernels.h, `ktile`), the register-pipelined rings (64-66) read every K step's fragments half a K-tile ahead (gemm_tile, PIPE):
    1, 2, 3, 4 K-tiles exercise the prologue / tail guards, 16 and 43 (odd) the steady state.  Bit-equal to the 128x128 single-buffer
    variant, on every one of 60 launches with the copy kernel and another GEMM keeping the CUs' LDS and memory paths busy on a second stream."""
    dt, tdt = lib.BF16, torch.bfloat16
    M, N = 1111, 640
    A, W, b = rnd(M, K, seed=21), rnd(N, K, seed=22, scale=K ** -0.5), rnd(N, seed=23)
    a_d, w_d = as_act(A, tdt), pack(W, dt, tdt)
    ref = torch.zeros(M, N, dtype=tdt, device=DEV)
    lib.call("toc3d_linear_ex", dt, lib.EPI_BIAS, 16, a_d, K, w_d, K, b.to(DEV), ref, N, None, 0, 0, None, None, M, N, K, 0, S())
    assert relerr(ref.float(), A.to(tdt).double() @ W.to(tdt).double().T + b.double()) < 6e-3
    big_a, big_w = as_act(rnd(4096, 1024, seed=24), tdt), pack(rnd(2048, 1024, seed=25, scale=1 / 32), dt, tdt)
    big_o, big_b = torch.zeros(4096, 2048, dtype=tdt, device=DEV), torch.zeros(2048, device=DEV)
    src, dst = torch.zeros(1 << 24, dtype=torch.uint8, device=DEV), torch.zeros(1 << 24, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    for v in [v for v in (60, 160, 61, 62, 63, 64, 65, 66) if lib.has_variant(v)]:
        outs = []
        for i in range(60):
            if i % 6 == 0:
                with torch.cuda.stream(side):
                    for _ in range(3):
                        lib.call("toc3d_linear_ex", dt, lib.EPI_BIAS, 17, big_a, 1024, big_w, 1024, big_b, big_o, 2048, None, 0, 0, None, None, 4096, 2048, 1024, 0, S())
                        lib.call("toc3d_copy_bytes", src, dst, 1 << 24, S())
            out = torch.full((M, N), 7.0, dtype=tdt, device=DEV)
            lib.call("toc3d_linear_ex", dt, lib.EPI_BIAS, v, a_d, K, w_d, K, b.to(DEV), out, N, None, 0, 0, None, None, M, N, K, 0, S())
            outs.append(out)
        torch.cuda.synchronize()
        bad = [i for i, o in enumerate(outs) if not torch.equal(o, ref)]
        assert not bad, f"variant {v}, K = {K}: launches {bad[:8]} differ from the 128x128 tile"


@pytest.mark.parametrize("name,dt,tdt", DTYPES)
def test_linear_is_bit_stable_under_load(name, dt, tdt):
    """The GEMM keeps packed-FP32 instructions in its epilogues (csrc/Makefile); the erratum seen in the attention kernel
    (LABNOTES.md) must not touch it: every epilogue, at ViT-L sizes with several workgroups per CU and the attention kernel
    running beside it on a second stream, gives the same bits on every launch."""
    M, C, Hd = 6000, 1024, 2730
    Hp = ru(Hd, 64)
    a_d = as_act(rnd(M, C, seed=1), tdt)
    wq, bq = pack(rnd(3 * C, C, seed=2, scale=C ** -0.5), dt, tdt), rnd(3 * C, seed=3).to(DEV)
    w12 = torch.empty(2 * Hp, C, dtype=tdt, device=DEV)
    b12 = torch.empty(2 * Hp, device=DEV)
    lib.call("toc3d_pack_swiglu", dt, rnd(Hd, C, seed=4, scale=C ** -0.5).to(DEV), rnd(Hd, C, seed=5, scale=C ** -0.5).to(DEV),
             (rnd(Hd, seed=6) * 0.3).to(DEV), (rnd(Hd, seed=7) * 0.3 + 0.5).to(DEV), Hd, C, w12, b12, Hp, C, S())
    w3p = pack(rnd(C, Hd, seed=8, scale=Hd ** -0.5), dt, tdt)
    b3 = rnd(C, seed=9).to(DEV)
    lg, lb = (1 + 0.1 * rnd(Hd, seed=14)).to(DEV), (0.1 * rnd(Hd, seed=15)).to(DEV)
    res = rnd(M, C, seed=10).to(DEV)
    # a co-runner: the flash attention kernel on its own stream, many launches deep
    V, h, w, L, heads = 6, 20, 50, 16, 16
    qkv = torch.zeros(M, 3 * C, dtype=tdt, device=DEV)
    lib.call("toc3d_linear_ex", dt, lib.EPI_BIAS, 0, a_d, C, wq, C, bq, qkv, 3 * C, None, 0, 0, None, None, M, 3 * C, C, 0, S())
    nW, N = V * 2 * 4, L * L
    rows = torch.empty(nW, N, dtype=torch.int32, device=DEV)
    wslots, count, npad = torch.empty_like(rows), torch.empty(nW, dtype=torch.int32, device=DEV), torch.empty(nW, dtype=torch.int32, device=DEV)
    lib.call("toc3d_window_map_dense", V, h, w, L, rows, wslots, count, npad, S())
    cosT, sinT, vb = rnd(N, 64, seed=11).to(DEV), rnd(N, 64, seed=12).to(DEV), rnd(C, seed=13).to(DEV)
    att = torch.zeros(M, C, dtype=tdt, device=DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    R = 10
    runs = []
    for i in range(R):
        with torch.cuda.stream(side):
            for _ in range(4):
                lib.call("toc3d_window_attention", dt, qkv, 3 * C, att, C, rows, wslots, count, None, npad, None, N, nW, int(count.max()), heads,
                         cosT, sinT, L, vb, 0.125, S())
        o_qkv = torch.zeros(M, 3 * C, dtype=tdt, device=DEV)
        hid = torch.zeros(M, Hp, dtype=tdt, device=DEV)
        hln = torch.zeros(M, Hp, dtype=tdt, device=DEV)
        out = res.clone()
        gel = torch.zeros(M, C, dtype=tdt, device=DEV)
        lib.call("toc3d_linear_ex", dt, lib.EPI_BIAS, 0, a_d, C, wq, C, bq, o_qkv, 3 * C, None, 0, 0, None, None, M, 3 * C, C, 0, S())
        lib.call("toc3d_linear_ex", dt, lib.EPI_SWIGLU, 16, a_d, C, w12, C, b12, hid, Hp, None, 0, 0, None, None, M, 2 * Hp, C, Hd, S())
        lib.call("toc3d_layernorm_act", dt, hid, Hp, lg, lb, 1e-6, hln, Hp, M, Hd, S())
        lib.call("toc3d_linear_ex", dt, lib.EPI_RESIDUAL, 0, hln, Hp, w3p, Hp, b3, out, C, out, C, 0, None, None, M, C, Hp, 0, S())
        lib.call("toc3d_linear_ex", dt, lib.EPI_GELU, 0, a_d, C, wq, C, bq, gel, C, None, 0, 0, None, None, M, C, C, 0, S())
        runs.append((o_qkv, hid, hln, out, gel))
    torch.cuda.synchronize()
    for r in runs[1:]:
        for got, ref, what in zip(r, runs[0], ("bias", "swiglu hidden", "ffn_ln", "residual", "gelu")):
            assert torch.equal(got.view(torch.uint8), ref.view(torch.uint8)), f"{what} epilogue differs between launches"


# ---------------------------------------------------------------------------------------------------
# uint8 camera images
IMG_NORM = dict(mean=[103.530, 116.280, 123.675], std=[57.375, 57.120, 58.395])       # projects/configs/ToC3D/ToC3D_faster.py:13-14


@pytest.mark.parametrize("to_rgb", [False, True])
@pytest.mark.parametrize("V,H,W", [(2, 320, 800), (1, 300, 790), (3, 33, 47)])
def test_normalize_images_matches_oracle_bit_exact(to_rgb, V, H, W):
    """NormalizeMultiviewImage + PadMultiViewImage + HWC->CHW (transform_3d.py:87-100,38-50) on the device."""
    from oracle import image_oracle as I
    from toc3d_amd.preprocess import prepare_images
    rng = np.random.default_rng(V * 1000 + H)
    img = rng.integers(0, 256, (V, H, W, 3), dtype=np.uint8)
    ref = I.prepare_images(img, IMG_NORM["mean"], IMG_NORM["std"], to_rgb, 32)
    out = prepare_images(torch.from_numpy(img).to(DEV), IMG_NORM["mean"], IMG_NORM["std"], to_rgb, 32)
    assert tuple(out.shape) == ref.shape
    assert torch.equal(out.cpu(), torch.from_numpy(ref))
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        prepare_images(torch.from_numpy(img), IMG_NORM["mean"], IMG_NORM["std"], to_rgb, 32)


def test_normalize_images_matches_the_reference_pipeline_golden(golden_dir):
    """toc3d_normalize_images against tests/golden/image_norm.npz -- the reference's own NormalizeMultiviewImage / PadMultiViewImage classes executed on the
    configs' arguments (oracle/gen_golden_image.py; mmcv's two functions stood in for from their published definitions): bit-exact."""
    from toc3d_amd.preprocess import prepare_images
    g = np.load(os.path.join(golden_dir, "image_norm.npz"))
    for tag in "abcd":
        u8, to_rgb, exp = g[f"{tag}_u8"], bool(g[f"{tag}_to_rgb"]), g[f"{tag}_expected"]
        out = prepare_images(torch.from_numpy(u8).to(DEV), g["mean"].tolist(), g["std"].tolist(), to_rgb, int(g["size_divisor"]))
        assert torch.equal(out.cpu(), torch.from_numpy(exp)), f"case {tag}"


@pytest.mark.parametrize("name,dt,tdt", DTYPES)
@pytest.mark.parametrize("H,W", [(320, 800), (300, 790)])
def test_im2col_u8_equals_im2col_of_normalized_images(name, dt, tdt, H, W):
    """The fused uint8 im2col writes exactly what toc3d_im2col_patches writes for the normalised, padded float image."""
    from toc3d_amd.preprocess import prepare_images
    V, p = 2, 16
    rng = np.random.default_rng(5)
    img = torch.from_numpy(rng.integers(0, 256, (V, H, W, 3), dtype=np.uint8)).to(DEV)
    x = prepare_images(img, IMG_NORM["mean"], IMG_NORM["std"], False, 32)
    Hp, Wp = x.shape[2], x.shape[3]
    M, Kp = V * (Hp // p) * (Wp // p), 768
    a = torch.zeros(M, Kp, dtype=tdt, device=DEV)
    b = torch.zeros(M, Kp, dtype=tdt, device=DEV)
    lib.call("toc3d_im2col_patches", dt, x, a, Kp, V, 3, Hp, Wp, p, S())
    lib.call("toc3d_im2col_patches_u8", dt, img, V, H, W, torch.tensor(IMG_NORM["mean"]), torch.tensor(IMG_NORM["std"]), 0, b, Kp, Hp, Wp, p, S())
    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    with pytest.raises(RuntimeError, match="multiple of the patch"):
        lib.call("toc3d_im2col_patches_u8", dt, img, V, H, W, torch.tensor(IMG_NORM["mean"]), torch.tensor(IMG_NORM["std"]), 0, b, Kp, Hp + 1, Wp, p, S())


@pytest.mark.parametrize("name,dt,tdt", DTYPES)
def test_linear_unaligned_outputs_take_the_scalar_epilogue(name, dt, tdt):
    """The epilogue stores 4 columns per lane as one 8 / 16-byte access when leading dims and base pointers allow it; ragged
    N, odd leading dimensions and offset views fall back to per-element accesses with the same values."""
    M, N, K = 333, 130, 128
    A, W, b = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5), rnd(N, seed=3)
    a_d, w_d = as_act(A, tdt), pack(W, dt, tdt)
    res = rnd(M, N, seed=4)
    ref = A.to(tdt).double() @ W.to(tdt).double().T + b.double()
    tol = 1e-5 if dt == lib.F32 else 6e-3
    for ldo, off in ((N, 0), (N + 1, 0), (N + 2, 1), (136, 4)):
        buf = torch.zeros(M * ldo + 8, dtype=tdt, device=DEV)
        out = buf[off:off + M * ldo].view(M, ldo)
        lib.call("toc3d_linear_ex", dt, lib.EPI_BIAS, 16, a_d, K, w_d, K, b.to(DEV), out, ldo, None, 0, 0, None, None, M, N, K, 0, S())
        assert relerr(out[:, :N].float(), ref) < tol, (ldo, off)
        assert float(out[:, N:].abs().sum()) == 0 and float(buf[:off].abs().sum()) == 0 and float(buf[off + M * ldo:].abs().sum()) == 0
        b32 = torch.zeros(M * ldo + 8, device=DEV)
        o32 = b32[off:off + M * ldo].view(M, ldo)
        r32 = torch.zeros(M * ldo + 8, device=DEV)
        rv = r32[off:off + M * ldo].view(M, ldo)
        rv[:, :N] = res.to(DEV)
        rep = torch.zeros(M // 5 + 1, N, device=DEV)
        rep_index = torch.full((M,), -1, dtype=torch.int32)
        rep_index[4::5] = torch.arange(len(rep_index[4::5]), dtype=torch.int32)
        lib.call("toc3d_linear_ex", dt, lib.EPI_RESIDUAL, 8, a_d, K, w_d, K, b.to(DEV), o32, ldo, rv, ldo, 0, rep, rep_index.to(DEV), M, N, K, 0, S())
        assert relerr(o32[:, :N], ref + res.double()) < tol, (ldo, off)
        assert relerr(rep[: len(rep_index[4::5])], ref[4::5]) < tol
        assert float(o32[:, N:].abs().sum()) == 0


@pytest.mark.parametrize("variant", [1, 8, 10, 13, 14, 15, 16, 17, 22, 24, 26, 28, 29, 30, 45, 47, 49, 116, 117, 126, 145, 147, 149])
def test_every_tuned_gemm_pipeline_is_bit_stable_beside_attention(variant):
    """Each K-loop flavour the autotuner may pick (single buffer, rings of 2-4 stages, K-tiles of 32 / 64 / 128 / 256, 4 and 8
    wavefronts, banded order) launched repeatedly while the flash-attention kernel of another stream shares the CUs: regression
    for the raw-barrier scheduling race of the single-buffer loop (LABNOTES.md), which only showed under that kind of co-residency."""
    dt, tdt = lib.BF16, torch.bfloat16
    M, C, N = 6000, 1024, 3072
    a_d = as_act(rnd(M, C, seed=1), tdt)
    wq, bq = pack(rnd(N, C, seed=2, scale=C ** -0.5), dt, tdt), rnd(N, seed=3).to(DEV)
    V, h, w, L, heads = 6, 20, 50, 16, 16
    qkv = torch.zeros(M, 3 * C, dtype=tdt, device=DEV)
    lib.call("toc3d_linear_ex", dt, lib.EPI_BIAS, 0, a_d, C, wq, C, bq, qkv, 3 * C, None, 0, 0, None, None, M, N, C, 0, S())
    nW, NN = V * 2 * 4, L * L
    rows = torch.empty(nW, NN, dtype=torch.int32, device=DEV)
    wslots, count, npad = torch.empty_like(rows), torch.empty(nW, dtype=torch.int32, device=DEV), torch.empty(nW, dtype=torch.int32, device=DEV)
    lib.call("toc3d_window_map_dense", V, h, w, L, rows, wslots, count, npad, S())
    cosT, sinT, vb = rnd(NN, 64, seed=11).to(DEV), rnd(NN, 64, seed=12).to(DEV), rnd(C, seed=13).to(DEV)
    att = torch.zeros(M, C, dtype=tdt, device=DEV)
    outs = [torch.zeros(M, N, dtype=tdt, device=DEV) for _ in range(24)]
    torch.cuda.synchronize()
    side, mc = torch.cuda.Stream(), int(count.max())
    for o in outs:
        with torch.cuda.stream(side):
            for _ in range(3):
                lib.call("toc3d_window_attention", dt, qkv, 3 * C, att, C, rows, wslots, count, None, npad, None, NN, nW, mc, heads,
                         cosT, sinT, L, vb, 0.125, S())
        lib.call("toc3d_linear_ex", dt, lib.EPI_BIAS, variant, a_d, C, wq, C, bq, o, N, None, 0, 0, None, None, M, N, C, 0, S())
    torch.cuda.synchronize()
    for i, o in enumerate(outs[1:]):
        assert torch.equal(o.view(torch.uint8), outs[0].view(torch.uint8)), f"variant {variant}: launch {i + 1} differs from launch 0"
    assert torch.equal(outs[0], qkv), "and equals the heuristic variant's result"


@pytest.mark.gpu
def test_copy_segments_one_launch_many_ragged_copies():
    """toc3d_copy_segments: per-frame input staging in one launch -- unaligned pointers, odd byte counts, an empty segment."""
    import torch
    from toc3d_amd import lib
    dev = "cuda:0"
    torch.manual_seed(3)
    sizes = [4096, 48000, 7, 0, 1234, 16, 100001, 33]
    srcs = [torch.randint(0, 255, (n + 5,), dtype=torch.uint8, device=dev) for n in sizes]
    dsts = [torch.zeros(n + 9, dtype=torch.uint8, device=dev) for n in sizes]
    pairs = [(d[3:3 + n] if i % 2 else d[:n], s[1:1 + n] if i % 3 == 0 else s[:n]) for i, (d, s, n) in enumerate(zip(dsts, srcs, sizes))]
    lib.copy_segments([(d, s) for d, s in pairs], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for (d, s), full, n in zip(pairs, dsts, sizes):
        assert torch.equal(d, s)
        assert int(full.sum()) == int(s.sum())          # nothing written outside the segment
    with pytest.raises(RuntimeError):
        lib.copy_segments([(dsts[0][:4], srcs[0][:4])] * 17, torch.cuda.current_stream().cuda_stream) if False else lib.call(
            "toc3d_copy_segments", 17, None, None, None, torch.cuda.current_stream().cuda_stream)


def test_ffn_ln_folded_across_the_gemm_boundary():
    """SwiGLU.ffn_ln folded (EPI_SWIGLU_STATS -> EPI_RESIDUAL_LN, eva_vit.py:47-49) against the explicit sequence
    (EPI_SWIGLU -> toc3d_layernorm_act -> EPI_RESIDUAL) and an f64 reference on the same rounded hidden units; the row
    statistics and both outputs must not depend on the tile variant."""
    dt, tdt = lib.BF16, torch.bfloat16
    M, K, Hd, Hp, C = 777, 512, 300, 320, 384
    eps = 1e-6
    A = rnd(M, K, seed=1)
    a_d = as_act(A, tdt)
    w12 = torch.empty(2 * Hp, K, dtype=tdt, device=DEV)
    b12 = torch.empty(2 * Hp, device=DEV)
    lib.call("toc3d_pack_swiglu", dt, rnd(Hd, K, seed=5, scale=K ** -0.5).to(DEV), rnd(Hd, K, seed=6, scale=K ** -0.5).to(DEV), rnd(Hd, seed=7).to(DEV),
             rnd(Hd, seed=8).to(DEV), Hd, K, w12, b12, Hp, K, S())
    gamma, beta = (1.0 + 0.3 * rnd(Hd, seed=9)).to(DEV), (0.2 * rnd(Hd, seed=10)).to(DEV)
    W3, b3 = rnd(C, Hd, seed=11, scale=Hd ** -0.5).to(DEV), rnd(C, seed=12).to(DEV)
    res = rnd(M, C, seed=13).to(DEV)
    rep_index = torch.full((M,), -1, dtype=torch.int32, device=DEV)
    rep_index[::50] = torch.arange(len(range(0, M, 50)), dtype=torch.int32, device=DEV)
    nrep = int((rep_index >= 0).sum())
    # explicit sequence
    hid0 = torch.zeros(M, Hp, dtype=tdt, device=DEV)
    lib.call("toc3d_linear_ex", dt, lib.EPI_SWIGLU, 16, a_d, K, w12, K, b12, hid0, Hp, None, 0, 0, None, None, M, 2 * Hp, K, Hd, S())
    hln = torch.zeros(M, Hp, dtype=tdt, device=DEV)
    lib.call("toc3d_layernorm_act", dt, hid0, Hp, gamma, beta, eps, hln, Hp, M, Hd, S())
    out0 = res.clone()
    lib.call("toc3d_linear_ex", dt, lib.EPI_RESIDUAL, 16, hln, Hp, pack(W3.cpu(), dt, tdt), Hp, b3, out0, C, out0, C, 0, None, None, M, C, Hp, 0, S())
    # f64 reference on the rounded hidden units
    h = hid0[:, :Hd].double()
    ln = (h - h.mean(1, keepdim=True)) / torch.sqrt(h.var(1, unbiased=False, keepdim=True) + eps) * gamma.double() + beta.double()
    delta_ref = ln @ W3.double().T + b3.double()
    ref = res.double() + delta_ref
    # folded
    w3f = torch.empty(ru(C, 128), Hp, dtype=tdt, device=DEV)
    c1, c2 = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    lib.call("toc3d_pack_weight_lnfold", dt, W3.contiguous(), gamma, beta, b3, C, Hd, w3f, w3f.shape[0], Hp, c1, c2, S())
    assert relerr(c1, (gamma * W3).to(tdt).double().sum(1)) < 1e-5 and relerr(c2, (W3.double() * beta.double()).sum(1) + b3.double()) < 1e-5
    cap = 6
    ref_stats = ref_out = ref_rep = None
    for v in (1, 8, 10, 15, 16, 17, 19, 22, 24, 26, 28, 29, 49, 51, 54, 55, 56, 57, 58, 60, 61, 62, 63, 64, 65, 66, 116, 117, 119, 126, 149, 151, 154, 160, 163, 216, 219, 249, 316, 317, 349):      # incl. every variant a shipped table names for this epilogue
        stats = torch.zeros(4 + M * cap * 2, device=DEV)
        hid = torch.full((M, Hp), 9.0, dtype=tdt, device=DEV)
        lib.call("toc3d_linear_fused", dt, lib.EPI_SWIGLU_STATS, v, a_d, K, w12, K, b12, hid, Hp, None, 0, 0, None, None, M, 2 * Hp, K, Hd,
                 stats, cap, None, 0, None, 0, 0.0, None, 0, None, S())
        assert torch.equal(hid, hid0), f"variant {v}: hidden units differ from EPI_SWIGLU"
        nslots = int(stats[:1].view(torch.int32).item())
        assert nslots == (2 * Hp + 127) // 128
        st = stats[4:].view(M, cap, 2)[:, :nslots]
        if ref_stats is None:
            ref_stats = st.clone()
            assert relerr(st[..., 0].sum(1), hid0.double().sum(1)) < 1e-5 and relerr(st[..., 1].sum(1), (hid0.double() ** 2).sum(1)) < 1e-5
        assert torch.equal(st, ref_stats), f"variant {v}: row statistics depend on the tile variant"
    for v in (1, 8, 9, 10, 13, 14, 16, 17, 19, 22, 26, 28, 29, 33, 45, 47, 49, 51, 52, 53, 54, 55, 56, 57, 58, 60, 61, 62, 63, 64, 65, 66, 110, 114, 116, 117, 126, 145, 149, 151, 152, 156, 160, 161, 214, 217, 226, 314, 317, 326):
        out = res.clone()
        rep = torch.zeros(nrep, C, device=DEV)
        lib.call("toc3d_linear_fused", dt, lib.EPI_RESIDUAL_LN, v, hid0, Hp, w3f, Hp, c2, out, C, out, C, 0, rep, rep_index, M, C, Hp, 0,
                 None, 0, stats, cap, c1, Hd, eps, None, 0, None, S())
        if ref_out is None:
            ref_out, ref_rep = out.clone(), rep.clone()
            e_fold, e_seq = relerr(out, ref), relerr(out0, ref)
            print(f"[ffn_ln fold] rel err vs f64: folded {e_fold:.3e}, explicit LayerNorm pass {e_seq:.3e}")
            assert e_fold < 4e-3 and e_fold < 1.5 * e_seq + 1e-4
            assert relerr(rep, delta_ref[rep_index.cpu() >= 0]) < 6e-3            # representative rows capture the raw branch output
        assert torch.equal(out, ref_out) and torch.equal(rep, ref_rep), f"variant {v}: folded epilogue depends on the tile variant"
    # the host may pass the slot count (upper half of stats_in_cap) instead of letting the kernel read it from the buffer's header: same bits
    out = res.clone()
    rep = torch.zeros(nrep, C, device=DEV)
    lib.call("toc3d_linear_fused", dt, lib.EPI_RESIDUAL_LN, 16, hid0, Hp, w3f, Hp, c2, out, C, out, C, 0, rep, rep_index, M, C, Hp, 0,
             None, 0, stats, cap | ((2 * Hp + 127) // 128) << 32, c1, Hd, eps, None, 0, None, S())
    assert torch.equal(out, ref_out) and torch.equal(rep, ref_rep)
    for v, epi in ((47, lib.EPI_SWIGLU_STATS), (9, lib.EPI_SWIGLU_STATS)):       # (the phased tiles 60-63 serve the folded epilogues since round 5: in the loops above)
        with pytest.raises(RuntimeError, match="cannot serve"):
            if epi == lib.EPI_SWIGLU_STATS:
                lib.call("toc3d_linear_fused", dt, epi, v, a_d, K, w12, K, b12, hid, Hp, None, 0, 0, None, None, M, 2 * Hp, K, Hd, stats, cap, None, 0, None, 0, 0.0, None, 0, None, S())
            else:
                lib.call("toc3d_linear_fused", dt, epi, v, hid0, Hp, w3f, Hp, c2, out, C, out, C, 0, None, None, M, C, Hp, 0, None, 0, stats, cap, c1, Hd, eps, None, 0, None, S())
    with pytest.raises(RuntimeError, match="bf16 only"):
        lib.call("toc3d_linear_fused", lib.F32, lib.EPI_SWIGLU_STATS, 16, a_d, K, w12, K, b12, hid, Hp, None, 0, 0, None, None, M, 2 * Hp, K, Hd, stats, cap, None, 0, None, 0, 0.0, None, 0, None, S())


def test_ffn_ln_fold_on_the_bf16x3_path():
    """EPI_SWIGLU_STATS -> EPI_RESIDUAL_LN on f32 operands with bf16 x 3 products (precision fp32x3, round 3): against an f64 reference of
    w3(ffn_ln(silu(w1 x) * w2 x)) + residual (eva_vit.py:47-49,263) and across tile variants."""
    dt, tdt = lib.F32, torch.float32
    M, K, Hd, Hp, C = 777, 512, 300, 320, 384
    eps = 1e-6
    A = rnd(M, K, seed=1).to(DEV)
    w1, w2 = rnd(Hd, K, seed=5, scale=K ** -0.5).to(DEV), rnd(Hd, K, seed=6, scale=K ** -0.5).to(DEV)
    b1, b2 = rnd(Hd, seed=7).to(DEV), rnd(Hd, seed=8).to(DEV)
    w12 = torch.empty(2 * Hp, K, dtype=tdt, device=DEV)
    b12 = torch.empty(2 * Hp, device=DEV)
    lib.call("toc3d_pack_swiglu", dt, w1, w2, b1, b2, Hd, K, w12, b12, Hp, K, S())
    gamma, beta = (1.0 + 0.3 * rnd(Hd, seed=9)).to(DEV), (0.2 * rnd(Hd, seed=10)).to(DEV)
    W3, b3 = rnd(C, Hd, seed=11, scale=Hd ** -0.5).to(DEV), rnd(C, seed=12).to(DEV)
    res = rnd(M, C, seed=13).to(DEV)
    Ad = A.double()
    h = torch.nn.functional.silu(Ad @ w1.double().T + b1.double()) * (Ad @ w2.double().T + b2.double())
    ln = (h - h.mean(1, keepdim=True)) / torch.sqrt(h.var(1, unbiased=False, keepdim=True) + eps) * gamma.double() + beta.double()
    ref = res.double() + ln @ W3.double().T + b3.double()
    w3f = torch.zeros(ru(C, 128), Hp, dtype=tdt, device=DEV)
    c1, c2 = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    lib.call("toc3d_pack_weight_lnfold", dt, W3.contiguous(), gamma, beta, b3, C, Hd, w3f, w3f.shape[0], Hp, c1, c2, S())
    cap = 6
    first = None
    for v in (1, 8, 10, 16, 17, 19, 22, 26, 28, 29, 47, 49, 52, 116, 117, 126, 129, 149):
        stats = torch.zeros(4 + M * cap * 2, device=DEV)
        hid = torch.full((M, Hp), 9.0, dtype=tdt, device=DEV)
        try:
            lib.call("toc3d_linear_fused", lib.F32X3, lib.EPI_SWIGLU_STATS, v, A, K, w12, K, b12, hid, Hp, None, 0, 0, None, None, M, 2 * Hp, K, Hd,
                     stats, cap, None, 0, None, 0, 0.0, None, 0, None, S())
        except RuntimeError as e:                     # N-tiles that are not whole statistics slots
            assert "cannot serve" in str(e)
            continue
        out = res.clone()
        lib.call("toc3d_linear_fused", lib.F32X3, lib.EPI_RESIDUAL_LN, v, hid, Hp, w3f, Hp, c2, out, C, out, C, 0, None, None, M, C, Hp, 0,
                 None, 0, stats, cap, c1, Hd, eps, None, 0, None, S())
        if first is None:
            first = (hid.clone(), out.clone())
            e = relerr(out, ref)
            print(f"[ffn_ln fold, bf16 x 3] rel err vs f64 {e:.3e}")
            assert relerr(hid[:, :Hd], h) < 3e-5 and e < 3e-5 and torch.count_nonzero(hid[:, Hd:]) == 0
        assert torch.equal(hid, first[0]) and torch.equal(out, first[1]), f"variant {v} differs"
    assert first is not None


def test_norm2_fold_on_the_bf16x3_path():
    """EPI_RESIDUAL_STATS -> EPI_SWIGLU_STATS_LN on f32 buffers with bf16 x 3 products (precision fp32x3, round 4): the projection's f32 output, its f32
    copy and statistics, and the hidden units against f64 (eva_vit.py:262-263, 44-47); parity grade (<= 1e-4), independent of the tile variant."""
    dt, tdt = lib.F32, torch.float32
    M, C, Hd, Hp = 777, 384, 300, 320
    eps = 1e-6
    att = rnd(M, C, seed=1).to(DEV)
    Wp, bp = rnd(C, C, seed=2, scale=C ** -0.5), rnd(C, seed=3).to(DEV)
    wproj = pack(Wp, dt, tdt)
    x0 = (3.0 * rnd(M, C, seed=4) + 0.7).to(DEV)                      # residual stream with a non-zero mean
    g2, b2 = (1.0 + 0.3 * rnd(C, seed=5)).to(DEV), (0.2 * rnd(C, seed=6)).to(DEV)
    w1, w2 = rnd(Hd, C, seed=7, scale=C ** -0.5).to(DEV), rnd(Hd, C, seed=8, scale=C ** -0.5).to(DEV)
    bb1, bb2 = rnd(Hd, seed=9).to(DEV), rnd(Hd, seed=10).to(DEV)
    xd = x0.double() + att.double() @ Wp.double().T.to(DEV) + bp.double()
    ln = (xd - xd.mean(1, keepdim=True)) / torch.sqrt(xd.var(1, unbiased=False, keepdim=True) + eps) * g2.double() + b2.double()
    h_ref = torch.nn.functional.silu(ln @ w1.double().T + bb1.double()) * (ln @ w2.double().T + bb2.double())
    w12f = torch.empty(2 * Hp, C, dtype=tdt, device=DEV)
    c1, c2 = torch.empty(2 * Hp, device=DEV), torch.empty(2 * Hp, device=DEV)
    lib.call("toc3d_pack_swiglu_lnfold", dt, w1, w2, bb1, bb2, g2, b2, Hd, C, w12f, c1, c2, Hp, C, S())
    cap2, cap = C // 64, 6
    first = None
    for v in (1, 8, 10, 16, 17, 19, 22, 26, 28, 29, 47, 49, 52, 116, 117, 126, 129, 149):
        x = x0.clone()
        a_raw = torch.full((M, C), 9.0, dtype=tdt, device=DEV)
        st2 = torch.zeros(4 + M * cap2 * 2, device=DEV)
        hid = torch.full((M, Hp), 9.0, dtype=tdt, device=DEV)
        st = torch.zeros(4 + M * cap * 2, device=DEV)
        try:
            lib.call("toc3d_linear_fused", lib.F32X3, lib.EPI_RESIDUAL_STATS, v, att, C, wproj, C, bp, x, C, x, C, 0, None, None, M, C, C, 0,
                     st2, cap2, None, 0, None, 0, 0.0, a_raw, C, None, S())
            lib.call("toc3d_linear_fused", lib.F32X3, lib.EPI_SWIGLU_STATS_LN, v, a_raw, C, w12f, C, c2, hid, Hp, None, 0, 0, None, None, M, 2 * Hp, C, Hd,
                     st, cap, st2, cap2 | (C // 64) << 32, c1, C, eps, None, 0, None, S())
        except RuntimeError as e:                     # N-tiles that are not whole statistics slots
            assert "cannot serve" in str(e)
            continue
        assert torch.equal(a_raw, x), "the f32 copy IS the f32 output"
        if first is None:
            first = (x.clone(), st2.clone(), hid.clone(), st.clone())
            e_x, e_h = relerr(x, xd), relerr(hid[:, :Hd], h_ref)
            print(f"[norm2 fold, bf16 x 3] rel err vs f64: projection + residual {e_x:.3e}, hidden units {e_h:.3e}")
            assert e_x < 3e-5 and e_h < 1e-4 and torch.count_nonzero(hid[:, Hd:]) == 0
            s2 = st2[4:].view(M, cap2, 2)
            assert relerr(s2[..., 0].sum(1), x.double().sum(1)) < 1e-5 and relerr(s2[..., 1].sum(1), (x.double() ** 2).sum(1)) < 1e-5
        for got, want, what in zip((x, st2, hid, st), first, ("projection", "norm2 statistics", "hidden units", "ffn_ln statistics")):
            assert torch.equal(got, want), f"variant {v}: {what} depends on the tile variant"
    assert first is not None


def test_norm2_folded_across_the_projection_boundary():
    """norm2 folded (EPI_RESIDUAL_STATS -> EPI_SWIGLU_STATS_LN, eva_vit.py:263) against the explicit sequence (EPI_RESIDUAL ->
    toc3d_layernorm_rows -> EPI_SWIGLU_STATS) and an f64 reference; bf16 copy, statistics and hidden units independent of the tile variant."""
    dt, tdt = lib.BF16, torch.bfloat16
    M, C, Hd, Hp = 777, 384, 300, 320
    eps = 1e-6
    att = as_act(rnd(M, C, seed=1), tdt)
    Wp, bp = rnd(C, C, seed=2, scale=C ** -0.5), rnd(C, seed=3).to(DEV)
    wproj = pack(Wp, dt, tdt)
    x0 = (3.0 * rnd(M, C, seed=4) + 0.7).to(DEV)                      # residual stream with a non-zero mean
    g2, b2 = (1.0 + 0.3 * rnd(C, seed=5)).to(DEV), (0.2 * rnd(C, seed=6)).to(DEV)
    w1, w2 = rnd(Hd, C, seed=7, scale=C ** -0.5).to(DEV), rnd(Hd, C, seed=8, scale=C ** -0.5).to(DEV)
    bb1, bb2 = rnd(Hd, seed=9).to(DEV), rnd(Hd, seed=10).to(DEV)
    rep_index = torch.full((M,), -1, dtype=torch.int32, device=DEV)
    rep_index[::40] = torch.arange(len(range(0, M, 40)), dtype=torch.int32, device=DEV)
    nrep = int((rep_index >= 0).sum())
    # explicit sequence
    x_ref = x0.clone()
    rep0 = torch.zeros(nrep, C, device=DEV)
    lib.call("toc3d_linear_ex", dt, lib.EPI_RESIDUAL, 16, att, C, wproj, C, bp, x_ref, C, x_ref, C, 0, rep0, rep_index, M, C, C, 0, S())
    a_ln = torch.zeros(M, C, dtype=tdt, device=DEV)
    lib.call("toc3d_layernorm_rows", dt, x_ref, C, None, None, g2, b2, eps, a_ln, C, M, C, S())
    w12 = torch.empty(2 * Hp, C, dtype=tdt, device=DEV)
    b12 = torch.empty(2 * Hp, device=DEV)
    lib.call("toc3d_pack_swiglu", dt, w1, w2, bb1, bb2, Hd, C, w12, b12, Hp, C, S())
    hid_seq = torch.zeros(M, Hp, dtype=tdt, device=DEV)
    lib.call("toc3d_linear_ex", dt, lib.EPI_SWIGLU, 16, a_ln, C, w12, C, b12, hid_seq, Hp, None, 0, 0, None, None, M, 2 * Hp, C, Hd, S())
    # f64 reference from the updated f32 stream
    xd = x_ref.double()
    ln = (xd - xd.mean(1, keepdim=True)) / torch.sqrt(xd.var(1, unbiased=False, keepdim=True) + eps) * g2.double() + b2.double()
    h_ref = torch.nn.functional.silu(ln @ w1.double().T + bb1.double()) * (ln @ w2.double().T + bb2.double())
    # folded
    w12f = torch.empty(2 * Hp, C, dtype=tdt, device=DEV)
    c1, c2 = torch.empty(2 * Hp, device=DEV), torch.empty(2 * Hp, device=DEV)
    lib.call("toc3d_pack_swiglu_lnfold", dt, w1, w2, bb1, bb2, g2, b2, Hd, C, w12f, c1, c2, Hp, C, S())
    cap2, cap = C // 64, 6
    ref_a = ref_st = ref_h = None
    for v in (1, 8, 9, 10, 13, 14, 16, 17, 19, 22, 26, 28, 29, 33, 45, 47, 49, 51, 54, 55, 56, 57, 58, 60, 61, 62, 63, 64, 65, 66, 114, 116, 117, 126, 145, 156, 160, 162):
        x = x0.clone()
        a_raw = torch.full((M, C), 9.0, dtype=tdt, device=DEV)
        st2 = torch.zeros(4 + M * cap2 * 2, device=DEV)
        rep = torch.zeros(nrep, C, device=DEV)
        lib.call("toc3d_linear_fused", dt, lib.EPI_RESIDUAL_STATS, v, att, C, wproj, C, bp, x, C, x, C, 0, rep, rep_index, M, C, C, 0,
                 st2, cap2, None, 0, None, 0, 0.0, a_raw, C, None, S())
        assert torch.equal(x, x_ref) and torch.equal(rep, rep0), f"variant {v}: f32 output differs from EPI_RESIDUAL"
        assert torch.equal(a_raw, x_ref.to(tdt)), f"variant {v}: act-dtype copy is not the rounded output"
        assert int(st2[:1].view(torch.int32).item()) == cap2
        s2 = st2[4:].view(M, cap2, 2)
        if ref_st is None:
            ref_a, ref_st = a_raw.clone(), s2.clone()
            assert relerr(s2[..., 0].sum(1), a_raw.double().sum(1)) < 1e-5 and relerr(s2[..., 1].sum(1), (a_raw.double() ** 2).sum(1)) < 1e-5
        assert torch.equal(s2, ref_st), f"variant {v}: row statistics depend on the tile variant"
    for v in (1, 8, 10, 15, 16, 17, 19, 22, 24, 26, 28, 29, 49, 51, 54, 55, 56, 57, 58, 60, 61, 62, 63, 64, 65, 66, 116, 117, 126, 149, 154, 160, 163):
        hid = torch.full((M, Hp), 9.0, dtype=tdt, device=DEV)
        st = torch.zeros(4 + M * cap * 2, device=DEV)
        lib.call("toc3d_linear_fused", dt, lib.EPI_SWIGLU_STATS_LN, v, ref_a, C, w12f, C, c2, hid, Hp, None, 0, 0, None, None, M, 2 * Hp, C, Hd,
                 st, cap, st2, cap2, c1, C, eps, None, 0, None, S())
        if ref_h is None:
            ref_h, ref_hs = hid.clone(), st.clone()
            e_fold, e_seq = relerr(hid[:, :Hd], h_ref), relerr(hid_seq[:, :Hd], h_ref)
            print(f"[norm2 fold] hidden units rel err vs f64: folded {e_fold:.3e}, explicit LayerNorm launch {e_seq:.3e}")
            assert e_fold < 1.5e-2 and e_fold < 1.5 * e_seq + 1e-3
            assert torch.count_nonzero(hid[:, Hd:]) == 0
            sl = st[4:].view(M, cap, 2)[:, : (2 * Hp + 127) // 128]
            assert relerr(sl[..., 0].sum(1), hid.double().sum(1)) < 1e-5
        assert torch.equal(hid, ref_h) and torch.equal(st, ref_hs), f"variant {v}: folded w1|w2 epilogue depends on the tile variant"
    # with the slot count passed by the host (what the backbone does: no read of the buffer's header): the same table, the same bits
    for v in (16, 116, 15, 51, 17, 28, 29, 49, 54, 55, 56):
        hid = torch.full((M, Hp), 9.0, dtype=tdt, device=DEV)
        st = torch.zeros(4 + M * cap * 2, device=DEV)
        lib.call("toc3d_linear_fused", dt, lib.EPI_SWIGLU_STATS_LN, v, ref_a, C, w12f, C, c2, hid, Hp, None, 0, 0, None, None, M, 2 * Hp, C, Hd,
                 st, cap, st2, cap2 | (C // 64) << 32, c1, C, eps, None, 0, None, S())
        assert torch.equal(hid, ref_h) and torch.equal(st, ref_hs), f"variant {v}: the host-passed slot count changes the result"
    with pytest.raises(RuntimeError, match="different buffers"):
        lib.call("toc3d_linear_fused", dt, lib.EPI_SWIGLU_STATS_LN, 16, ref_a, C, w12f, C, c2, hid, Hp, None, 0, 0, None, None, M, 2 * Hp, C, Hd,
                 st2, cap2, st2, cap2, c1, C, eps, None, 0, None, S())


@pytest.mark.parametrize("name,dt,tdt", DTYPES)
def test_conv3x3_implicit_gemm_equals_im2col_gemm(name, dt, tdt):
    """toc3d_conv3x3_nhwc (CPFPN's 3x3 conv, necks/cp_fpn.py:124-133, as an implicit GEMM) == toc3d_im2col_3x3 + toc3d_linear bit for bit
    (same K order), for every tile variant, and == F.conv2d on the same rounded operands; ragged M (tiles past the last pixel)."""
    V, h, w, C, Co = 3, 20, 50, 256, 256
    x = rnd(V, h, w, C, seed=3)
    Wc, b = rnd(Co, C, 3, 3, seed=4, scale=(9 * C) ** -0.5), rnd(Co, seed=5).to(DEV)
    M = V * h * w
    x_act = x.to(DEV).to(tdt).contiguous()
    wp = pack(Wc.permute(0, 2, 3, 1).reshape(Co, 9 * C), dt, tdt)          # (Cout, ky, kx, Cin): toc3d_im2col_3x3's column order
    col = torch.zeros(M, 9 * C, dtype=tdt, device=DEV)
    lib.call("toc3d_im2col_3x3", dt, x_act.float(), col, 9 * C, V, h, w, C, S())
    ref = torch.zeros(M, Co, device=DEV)
    lib.call("toc3d_linear_ex", dt, lib.EPI_RESIDUAL, 16, col, 9 * C, wp, 9 * C, b, ref, Co, None, 0, 0, None, None, M, Co, 9 * C, 0, S())
    conv = torch.nn.functional.conv2d(x_act.double().permute(0, 3, 1, 2), Wc.to(DEV).to(tdt).double(), b.double(), padding=1)
    assert relerr(ref, conv.permute(0, 2, 3, 1).reshape(M, Co)) < (1e-5 if dt == lib.F32 else 1e-5)      # f32 accumulation of exact products
    zeros = torch.zeros(256, dtype=torch.uint8, device=DEV)
    zeros = torch.zeros(16, dtype=torch.uint8, device=DEV)               # 16 zero bytes are enough, whatever the K-tile width
    for v in (1, 8, 9, 10, 13, 14, 16, 17, 19, 22, 26, 28, 33, 45, 49, 51, 110, 114, 126) + ((24, 27, 30) if dt == lib.BF16 else ()):
        out = torch.full((M, Co), 7.0, device=DEV)
        lib.call("toc3d_conv3x3_nhwc", dt, v, x_act, C, wp, 9 * C, b, out, Co, V, h, w, Co, zeros, S())
        assert torch.equal(out, ref), f"variant {v}"
    if dt == lib.BF16:
        with pytest.raises(RuntimeError, match="cannot serve"):
            lib.call("toc3d_conv3x3_nhwc", dt, 60, x_act, C, wp, 9 * C, b, out, Co, V, h, w, Co, zeros, S())
    with pytest.raises(RuntimeError, match="multiple of 64"):
        lib.call("toc3d_conv3x3_nhwc", dt, 16, x_act, 96, wp, 9 * 96, b, out, Co, V, h, w, Co, zeros, S())


def test_gathered_residual_equals_the_shortcut_copy():
    """toc3d_gather_merge_ln_ex(kept_copy=0) + toc3d_linear_fused(residual_index=crow_tok): the projection GEMM reads the residual of a kept
    row from x, of a representative row in place -- the same bits as reading the f32 shortcut copy the gather kernel used to write."""
    dt, tdt = lib.BF16, torch.bfloat16
    V, h, w, C, L, ratio = 2, 20, 50, 128, 16, 0.4
    g = torch.Generator().manual_seed(9)
    x = torch.randn(V, h, w, C, generator=g)
    scores = -torch.rand(V, h, w, generator=g) * 3 - 0.1
    gw, gb = (1 + 0.1 * rnd(C, seed=2)).to(DEV), (0.1 * rnd(C, seed=3)).to(DEV)
    N = L * L
    k = int(N * ratio)
    b = _run_topk(scores, V, h, w, L, k)
    ms, nW = b["ms"], b["tok"].shape[0]
    xd = x.reshape(-1, C).to(DEV).contiguous()
    outs = {}
    for kept_copy in (1, 0):
        short = torch.full((ms, C), float("nan"), device=DEV)             # rows the kernel does not write stay NaN
        a = torch.empty(ms, C, dtype=tdt, device=DEV)
        lib.call("toc3d_gather_merge_ln_ex", dt, xd, C, b["tok"], b["wgt"], b["crow_tok"], b["rep_row"], nW, N, k, ms, gw, gb, 1e-6, short, a, C, kept_copy, S())
        att = as_act(rnd(ms, C, seed=4), tdt)
        wp, bp = pack(rnd(C, C, seed=5, scale=C ** -0.5), dt, tdt), rnd(C, seed=6).to(DEV)
        rep = torch.zeros(nW, C, device=DEV)
        if kept_copy:
            lib.call("toc3d_linear_ex", dt, lib.EPI_RESIDUAL, 16, att, C, wp, C, bp, short, C, short, C, 0, rep, b["rep_index"], ms, C, C, 0, S())
        else:
            kept = b["crow_tok"] >= 0
            assert bool(torch.isnan(short[kept]).all()) and bool(torch.isfinite(short[~kept]).all())
            lib.call("toc3d_linear_fused", dt, lib.EPI_RESIDUAL, 16, att, C, wp, C, bp, short, C, xd, C, 0, rep, b["rep_index"], ms, C, C, 0,
                     *lib.NO_FUSED[:9], b["crow_tok"], S())
        outs[kept_copy] = (short.clone(), rep.clone(), a.clone())
    for t0, t1 in zip(outs[1], outs[0]):
        assert bool(torch.isfinite(t1.float()).all()) and torch.equal(t0, t1)


@pytest.mark.parametrize("M,N,K", [(300, 200, 128), (1000, 384, 192), (6000, 1024, 768), (37, 3072, 1024), (3276, 1024, 2752)])
def test_linear_bf16x3_products_on_f32_operands(M, N, K):
    """TOC3D_DTYPE_F32X3: f32 buffers, every product formed as hi.hi + hi.lo + lo.hi on the bf16 matrix cores.  Against an f64 reference the
    error must sit at the 2^-16 class (1e-5 relative to the output scale), 100x below plain bf16 and within ~10x of the exact-f32 MFMA path;
    all epilogues it serves, all its tile variants bit-identical."""
    A, W, b = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5), rnd(N, seed=3)
    ref = A.double() @ W.double().T + b.double()
    a_d, w_d = as_act(A, torch.float32), pack(W, lib.F32, torch.float32)
    Kp = a_d.shape[1]
    outs = {}
    for dt in (lib.F32, lib.F32X3, lib.F32X6):
        out = torch.empty(M, N, device=DEV)
        lib.call("toc3d_linear", dt, lib.EPI_BIAS, a_d, Kp, w_d, Kp, b.to(DEV), out, N, None, 0, 0, None, None, M, N, Kp, 0, S())
        outs[dt] = out
    e32, ex3, ex6 = relerr(outs[lib.F32], ref), relerr(outs[lib.F32X3], ref), relerr(outs[lib.F32X6], ref)
    print(f"[bf16x3 {M}x{N}x{K}] rel max err: exact f32 MFMA {e32:.2e}   bf16 x 3 {ex3:.2e}   bf16 x 6 {ex6:.2e}")
    assert ex3 < 2e-5 and e32 < 1e-5 and ex6 < 2 * e32 + 1e-7      # the three-way split is f32-grade
    for v in (1, 8, 16, 17, 22, 26, 49, 117, 122):
        o6 = torch.empty(M, N, device=DEV)
        lib.call("toc3d_linear_ex", lib.F32X6, lib.EPI_BIAS, v, a_d, Kp, w_d, Kp, b.to(DEV), o6, N, None, 0, 0, None, None, M, N, Kp, 0, S())
        assert torch.equal(o6, outs[lib.F32X6]), f"x6 variant {v} differs"
    res = rnd(M, N, seed=4).to(DEV)
    base = None
    for v in (1, 8, 9, 10, 14, 16, 17, 19, 22, 26, 28, 29, 33, 45, 47, 49, 52, 53, 110, 116, 117, 122, 126, 129, 145, 152):
        out = torch.empty(M, N, device=DEV)
        lib.call("toc3d_linear_ex", lib.F32X3, lib.EPI_BIAS, v, a_d, Kp, w_d, Kp, b.to(DEV), out, N, None, 0, 0, None, None, M, N, Kp, 0, S())
        assert torch.equal(out, outs[lib.F32X3]), f"variant {v} differs"
        o32 = res.clone()
        lib.call("toc3d_linear_ex", lib.F32X3, lib.EPI_RESIDUAL, v, a_d, Kp, w_d, Kp, b.to(DEV), o32, N, o32, N, 0, None, None, M, N, Kp, 0, S())
        base = o32.clone() if base is None else base
        assert torch.equal(o32, base)
    assert relerr(base, ref + res.cpu().double()) < 2e-5
    lib.call("toc3d_linear", lib.F32X3, lib.EPI_GELU, a_d, Kp, w_d, Kp, b.to(DEV), out, N, None, 0, 0, None, None, M, N, Kp, 0, S())
    assert relerr(out, torch.nn.functional.gelu(ref)) < 2e-5
    with pytest.raises(RuntimeError, match="bf16 x 3"):
        lib.call("toc3d_linear_fused", lib.F32X6, lib.EPI_RESIDUAL_STATS, 0, a_d, Kp, w_d, Kp, b.to(DEV), out, N, None, 0, 0, None, None, M, N, Kp, 0, *lib.NO_FUSED, S())   # (x 3 serves the folded-LayerNorm epilogues 4-7 since rounds 3 / 4; x 6 does not)


def test_x3_planes_layout_and_in_place():
    x = (rnd(300, 256, seed=1) * 37.0).to(DEV)
    p = to_planes(x)
    hi, lo = planes_decode(p)
    assert torch.equal(hi, x.to(torch.bfloat16).float()), "hi plane = bf16(x)"
    assert torch.equal(lo, (x - hi).to(torch.bfloat16).float()), "lo plane = bf16(x - hi)"
    assert ((hi + lo) - x).abs().max() <= 2.0 ** -16 * x.abs().max()
    q = x.clone()
    lib.call("toc3d_x3_planes", q, 256, q, 256, 300, 256, S())       # in place
    assert torch.equal(q.view(torch.int32), p.view(torch.int32))
    wide = torch.zeros(300, 320, device=DEV)                           # leading dimension > K: the tail of the row is not touched
    lib.call("toc3d_x3_planes", x, 256, wide, 320, 300, 256, S())
    assert torch.equal(wide[:, :256].contiguous().view(torch.int32), p.view(torch.int32)) and torch.count_nonzero(wide[:, 256:]) == 0


def test_bf16x3_on_planes_is_bit_identical_to_the_in_kernel_split():
    """TOC3D_DTYPE_F32X3W / F32X3P (round 4): the same products on operands that arrive as (hi, lo) planes -- W packed once, A written as planes by its
    producer -- return the bits of TOC3D_DTYPE_F32X3, for the plain epilogues and through the whole folded block half (eva_vit.py:44-51,262-263):
    proj (+ residual, f32 copy as planes, statistics) -> w1|w2 (norm2 folded; hidden units as planes, statistics) -> w3 (ffn_ln folded, + residual)."""
    dt, tdt = lib.F32, torch.float32
    M, C, Hd, Hp = 777, 384, 300, 320
    eps = 1e-6
    att = rnd(M, C, seed=1).to(DEV)
    Wp, bp = rnd(C, C, seed=2, scale=C ** -0.5), rnd(C, seed=3).to(DEV)
    wproj = pack(Wp, dt, tdt)
    x0 = (3.0 * rnd(M, C, seed=4) + 0.7).to(DEV)
    g2, b2 = (1.0 + 0.3 * rnd(C, seed=5)).to(DEV), (0.2 * rnd(C, seed=6)).to(DEV)
    w1, w2 = rnd(Hd, C, seed=7, scale=C ** -0.5).to(DEV), rnd(Hd, C, seed=8, scale=C ** -0.5).to(DEV)
    bb1, bb2 = rnd(Hd, seed=9).to(DEV), rnd(Hd, seed=10).to(DEV)
    w12f = torch.empty(2 * Hp, C, dtype=tdt, device=DEV)
    c1, c2 = torch.empty(2 * Hp, device=DEV), torch.empty(2 * Hp, device=DEV)
    lib.call("toc3d_pack_swiglu_lnfold", dt, w1, w2, bb1, bb2, g2, b2, Hd, C, w12f, c1, c2, Hp, C, S())
    gf, bf = (1.0 + 0.3 * rnd(Hd, seed=11)).to(DEV), (0.2 * rnd(Hd, seed=12)).to(DEV)
    W3, b3 = rnd(C, Hd, seed=13, scale=Hd ** -0.5).to(DEV), rnd(C, seed=14).to(DEV)
    w3f = torch.zeros(ru(C, 128), Hp, dtype=tdt, device=DEV)
    c1_3, c2_3 = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    lib.call("toc3d_pack_weight_lnfold", dt, W3.contiguous(), gf, bf, b3, C, Hd, w3f, w3f.shape[0], Hp, c1_3, c2_3, S())
    cap2, cap = C // 64, 6

    def half(mode, v):
        """mode 0: F32X3 on f32 buffers; 1: F32X3W (weights as planes); 2: F32X3P (weights, A operands and the GEMM-to-GEMM activations as planes);
        3: the mixed forms, as a block whose attention output is still f32 launches them: proj F32X3WO, w1|w2 F32X3P, w3 F32X3WA."""
        d = (lib.F32X3, lib.F32X3W, lib.F32X3P, lib.F32X3WO)[mode]
        d12, d3 = (d, d) if mode < 3 else (lib.F32X3P, lib.F32X3WA)
        wp, w12, w3 = (wproj, w12f, w3f) if mode == 0 else (to_planes(wproj), to_planes(w12f), to_planes(w3f))
        a_in = to_planes(att) if mode == 2 else att
        x = x0.clone()
        a_raw = torch.full((M, C), 9.0, dtype=tdt, device=DEV)
        st2 = torch.zeros(4 + M * cap2 * 2, device=DEV)
        hid = torch.full((M, Hp), 9.0, dtype=tdt, device=DEV)
        st = torch.zeros(4 + M * cap * 2, device=DEV)
        q = torch.zeros(M, C, device=DEV)
        lib.call("toc3d_linear_ex", d, lib.EPI_BIAS, v, a_in, C, wp, C, bp, q, C, None, 0, 0, None, None, M, C, C, 0, S())        # a plain epilogue: f32 output in every mode
        lib.call("toc3d_linear_fused", d, lib.EPI_RESIDUAL_STATS, v, a_in, C, wp, C, bp, x, C, x, C, 0, None, None, M, C, C, 0,
                 st2, cap2, None, 0, None, 0, 0.0, a_raw, C, None, S())
        x1 = x.clone()
        lib.call("toc3d_linear_fused", d12, lib.EPI_SWIGLU_STATS_LN, v, a_raw, C, w12, C, c2, hid, Hp, None, 0, 0, None, None, M, 2 * Hp, C, Hd,
                 st, cap, st2, cap2 | (C // 64) << 32, c1, C, eps, None, 0, None, S())
        lib.call("toc3d_linear_fused", d3, lib.EPI_RESIDUAL_LN, v, hid, Hp, w3, Hp, c2_3, x, C, x, C, 0, None, None, M, C, Hp, 0,
                 None, 0, st, cap | 5 << 32, c1_3, Hd, eps, None, 0, None, S())
        return q, x1, a_raw, st2, hid, st, x

    ref = half(0, 16)
    names = ("bias epilogue", "proj + residual", "f32 copy", "norm2 statistics", "hidden units", "ffn_ln statistics", "w3 + residual")
    for v in (16, 17, 49, 126, 1):
        got_w = half(1, v)
        for n, g_, r_ in zip(names, got_w, ref):
            assert torch.equal(g_, r_), f"F32X3W variant {v}: {n} differs from F32X3"
        for mode, tag in ((2, "F32X3P"), (3, "F32X3WO / P / WA")):
            got_p = half(mode, v)
            for k, (n, g_, r_) in enumerate(zip(names, got_p, ref)):
                if k in (2, 4):      # the GEMM-to-GEMM activations left as planes: the planes of the f32 values F32X3 wrote
                    assert torch.equal(g_.view(torch.int32), to_planes(r_).view(torch.int32)), f"{tag} variant {v}: {n} is not the planes image of the F32X3 output"
                else:
                    assert torch.equal(g_, r_), f"{tag} variant {v}: {n} differs from F32X3"
    # round 6: the phased big tiles on planes (gemm_phased_kernel, X3 -- both operands must be planes): the same bits again, every epilogue of the block half
    for v in (60, 61, 62, 63, 160, 163, 54, 55, 56, 57, 58, 59, 155):      # (54-59: the 96- / 160-row tiles, whose partial DMA rounds the x3 form only takes on planes)
        got_p = half(2, v)
        for k, (n, g_, r_) in enumerate(zip(names, got_p, ref)):
            if k in (2, 4):
                assert torch.equal(g_.view(torch.int32), to_planes(r_).view(torch.int32)), f"F32X3P phased variant {v}: {n} is not the planes image of the F32X3 output"
            else:
                assert torch.equal(g_, r_), f"F32X3P phased variant {v}: {n} differs from F32X3"
    with pytest.raises(RuntimeError):      # the phased x3 form stages planes as they lie: an f32 A operand is refused
        half(1, 60)
    with pytest.raises(RuntimeError):      # ... and so are the 96-row tiles (their in-LDS split would need whole DMA rounds)
        half(1, 55)
    with pytest.raises(RuntimeError):      # rows of planes are whole 32-element groups
        bad = torch.zeros(M, C + 8, device=DEV)
        lib.call("toc3d_linear_ex", lib.F32X3P, lib.EPI_BIAS, 16, bad, C + 8, to_planes(wproj), C, bp, torch.zeros(M, C, device=DEV), C, None, 0, 0, None, None, M, C, C, 0, S())


def test_layernorm_rows_writes_planes():
    """toc3d_layernorm_rows with TOC3D_DTYPE_F32X3P: the f32 result written as (hi, lo) planes (the q|k|v GEMM's A operand on the fp32x3 path) is the planes
    image of the f32 kernel's output; misaligned rows are refused."""
    M, C = 333, 384
    x = (rnd(M, C, seed=1) * 3.0 + 0.5).to(DEV)
    g, b = (1.0 + 0.3 * rnd(C, seed=2)).to(DEV), (0.2 * rnd(C, seed=3)).to(DEV)
    o32, opl = torch.zeros(M, C, device=DEV), torch.zeros(M, C, device=DEV)
    lib.call("toc3d_layernorm_rows", lib.F32, x, C, None, None, g, b, 1e-6, o32, C, M, C, S())
    lib.call("toc3d_layernorm_rows", lib.F32X3P, x, C, None, None, g, b, 1e-6, opl, C, M, C, S())
    assert torch.equal(opl.view(torch.int32), to_planes(o32).view(torch.int32))
    with pytest.raises(RuntimeError, match="128-byte"):
        bad = torch.zeros(M, C + 8, device=DEV)
        lib.call("toc3d_layernorm_rows", lib.F32X3P, x, C, None, None, g, b, 1e-6, bad, C + 8, M, C, S())


@pytest.mark.parametrize("n", [77, 129, 201, 256, 400])
def test_window_attention_with_bf16x3_products(n):
    """toc3d_window_attention on f32 q|k|v with TOC3D_DTYPE_F32X3 / F32X3P / F32X3WO (the attention of precision "fp32x3"): both contractions as bf16 x 3
    products (hi.hi + hi.lo + lo.hi), RoPE / softmax / accumulation in f32 -- parity grade against the oracle (toc3d_eva_vit.py:484-518), close to the
    exact-f32 kernel; the planes forms return the planes image of the f32 forms (small-window and flash kernels: n <= 208 / larger)."""
    cfg = configs.get("toc3d_tiny")
    sd = synth.make_state_dict(cfg)
    C, heads, nW = cfg["embed_dim"], cfg["num_heads"], 5
    pre = "blocks.5.attn."
    cosT, sinT = sd[pre + "rope.freqs_cos"], sd[pre + "rope.freqs_sin"]        # 400-row table
    y = rnd(nW, n, C, seed=11)
    g = torch.Generator().manual_seed(12)
    slots = torch.stack([torch.randperm(400, generator=g)[:n] for _ in range(nW)])
    sd2 = dict(sd)
    sd2[pre + "proj.weight"], sd2[pre + "proj.bias"] = torch.eye(C), torch.zeros(C)
    ref = O.attention(y, sd2, pre, heads, cosT[slots], sinT[slots]).reshape(-1, C)
    wqkv = torch.cat([sd[pre + "q_proj.weight"], sd[pre + "k_proj.weight"], sd[pre + "v_proj.weight"]])
    bqkv = torch.cat([sd[pre + "q_bias"], torch.zeros(C), sd[pre + "v_bias"]])
    M = nW * n
    qkv = torch.empty(M, 3 * C, dtype=torch.float32, device=DEV)
    lib.call("toc3d_linear", lib.F32, lib.EPI_BIAS, as_act(y.reshape(M, C), torch.float32), C, pack(wqkv, lib.F32, torch.float32), C, bqkv.to(DEV), qkv, 3 * C, None, 0, 0,
             None, None, M, 3 * C, C, 0, S())
    rows = torch.arange(M, dtype=torch.int32).reshape(nW, n).to(DEV)
    count = torch.full((nW,), n, dtype=torch.int32, device=DEV)
    outs = {}
    for dt in (lib.F32, lib.F32X3, lib.F32X3P, lib.F32X3WO):
        out = torch.zeros(M, C, dtype=torch.float32, device=DEV)
        lib.call("toc3d_window_attention", dt, qkv, 3 * C, out, C, rows, slots.int().to(DEV), count, None, None, None, n, nW, n, heads,
                 cosT.to(DEV), sinT.to(DEV), 20, None, 64 ** -0.5, S())
        outs[dt] = out
    e32, ex3 = relerr(outs[lib.F32], ref), relerr(outs[lib.F32X3], ref)
    print(f"[attention n={n}] rel err vs oracle: exact f32 {e32:.3e}, bf16 x 3 products {ex3:.3e}; x3 vs exact {relerr(outs[lib.F32X3], outs[lib.F32].cpu()):.3e}")
    assert e32 < 5e-5 and ex3 < 1e-4
    assert torch.equal(outs[lib.F32X3P].view(torch.int32), to_planes(outs[lib.F32X3]).view(torch.int32))
    assert torch.equal(outs[lib.F32X3WO].view(torch.int32), to_planes(outs[lib.F32]).view(torch.int32))
