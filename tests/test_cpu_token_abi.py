"""CPU: every refusal of the token kernels' entry points (toc3d_window_topk, toc3d_gather_merge_ln_ex, toc3d_gather_merge_ln_split, toc3d_scatter_update,
toc3d_rebase_layernorm_rows, toc3d_layernorm_rows) is reached once and names its reason in toc3d_last_error().  The checks run before any launch, so the
pointers are made-up aligned addresses that are never dereferenced; only refusing calls and the empty ones that return before the launch are made.

Second half: the references tests/test_gpu_token_kernels.py holds the kernels to (tests/token_cases.py) are checked here for their own invariants."""
import pytest
import torch

import token_cases as T
from support import _call, _refused
from toc3d_amd import lib

A = 0x10000                                  # 256-byte aligned stand-in for a device buffer
BIG = (1 << 31) - 1024                       # first count the token kernels refuse (they count rows in 32 bits)


# ---- toc3d_layernorm_rows ---------------------------------------------------------------------------
def _ln(dtype=lib.F32, **o):
    a = dict(x=A, ldx=64, row_index=None, row_scale=None, gamma=A, beta=A, out=A, ldo=64, M=5, C=64)
    a.update(o)
    return (dtype, a["x"], a["ldx"], a["row_index"], a["row_scale"], a["gamma"], a["beta"], 1e-6, a["out"], a["ldo"], a["M"], a["C"], None)


@pytest.mark.parametrize("dtype,over,reason", [
    *[(lib.F32, {p: None}, "null buffer") for p in ("x", "gamma", "beta", "out")],
    (lib.F32, dict(C=0), "multiple of 4 and <= 2048"), (lib.F32, dict(C=62), "multiple of 4 and <= 2048"),
    (lib.BF16, dict(C=2052, ldx=2052, ldo=2052), "multiple of 4 and <= 2048"),
    (lib.F32, dict(ldx=60), "bad leading dims"), (lib.F32, dict(ldo=60), "bad leading dims"), (lib.F32, dict(ldx=66), "bad leading dims"), (lib.BF16, dict(ldo=66), "bad leading dims"),
    (lib.F32, dict(M=BIG + 1), "too many rows"), (lib.BF16, dict(M=1 << 40), "too many rows"),
    (lib.F32X3P, dict(out=A + 64), "128-byte"), (lib.F32X3P, dict(ldo=80), "128-byte"), (lib.F32X3P, dict(C=36, ldx=36, ldo=36), "128-byte"),
    (99, {}, "bad dtype"), (lib.F32X3, {}, "bad dtype"),
])
def test_layernorm_rows_refusals(dtype, over, reason):
    _refused("toc3d_layernorm_rows", _ln(dtype, **over), reason)


# ---- toc3d_window_topk ------------------------------------------------------------------------------
TOPK_PTRS = ("scores", "order", "tok", "wgt", "prow", "crow_tok", "rep_index", "rep_row", "arows", "aslots", "acount_q", "acount_k")


def _topk(**o):
    a = dict({p: A for p in TOPK_PTRS}, crow_rc=A, V=2, h=5, w=9, L=4, k=3)
    a.update(o)
    return (a["scores"], a["V"], a["h"], a["w"], a["L"], a["k"], *[a[p] for p in TOPK_PTRS[1:]], a["crow_rc"], None)


@pytest.mark.parametrize("over,reason", [
    *[({p: None}, "null buffer") for p in TOPK_PTRS],
    (dict(V=0), "bad dims"), (dict(h=0), "bad dims"), (dict(w=-1), "bad dims"), (dict(L=0), "bad dims"), (dict(L=65, k=1), "bad dims"),
    (dict(k=-1), "outside [0, 16)"), (dict(k=16), "outside [0, 16)"), (dict(L=64, k=4096), "outside [0, 4096)"),
    (dict(crow_rc=None, k=16), "outside [0, 16)"),                    # crow_rc is optional: refused for the reason that follows
    (dict(h=1 << 31), "too many tokens"), (dict(h=1 << 16, w=1 << 16), "too many tokens"), (dict(V=1 << 26), "too many tokens"), (dict(V=1 << 62, h=4, w=4), "too many tokens"),
])
def test_window_topk_refusals(over, reason):
    _refused("toc3d_window_topk", _topk(**over), reason)


def test_window_topk_rows_matches_the_reference_count_and_refuses():
    l = lib.load()
    for (V, h, w, L, k) in [(2, 4, 7, 3, 0), (2, 8, 15, 7, 20), (1, 9, 17, 8, 63), (3, 20, 50, 16, 128), (1, 33, 40, 32, 0)]:
        assert int(l.toc3d_window_topk_rows(V, h, w, L, k)) == T.topk_rows(V, h, w, L, k)
    for bad in [(0, 4, 4, 2, 1), (1, 0, 4, 2, 1), (1, 4, 0, 2, 1), (1, 4, 4, 0, 1), (1, 4, 4, 2, -1)]:
        assert int(l.toc3d_window_topk_rows(*bad)) == -1


# ---- toc3d_gather_merge_ln_ex / _split ----------------------------------------------------------------
GATHER_PTRS = ("x", "tok", "wgt", "crow_tok", "rep_row", "gamma", "beta", "shortcut", "a_out")


def _gather(dtype=lib.F32, split=None, **o):
    a = dict({p: A for p in GATHER_PTRS}, C=64, nW=3, N=16, k=5, rows=18, lda=64, kept_copy=1, scratch=A, scratch_bytes=1 << 40, split=0 if split is None else split)
    a.update(o)
    head = (dtype, a["x"], a["C"], a["tok"], a["wgt"], a["crow_tok"], a["rep_row"], a["nW"], a["N"], a["k"], a["rows"], a["gamma"], a["beta"], 1e-6,
            a["shortcut"], a["a_out"], a["lda"], a["kept_copy"])
    return head + ((None,) if split is None else (a["scratch"], a["scratch_bytes"], a["split"], None))


GATHER_COMMON = [
    *[(lib.F32, {p: None}, "null buffer") for p in GATHER_PTRS],
    (lib.F32, dict(C=0), "multiple of 4 and <= 1024"), (lib.F32, dict(C=66, lda=68), "multiple of 4 and <= 1024"), (lib.BF16, dict(C=1028, lda=1028), "multiple of 4 and <= 1024"),
    (lib.F32, dict(k=-1), "bad k / lda / rows"), (lib.F32, dict(k=16), "bad k / lda / rows"), (lib.F32, dict(lda=60), "bad k / lda / rows"),
    (lib.BF16, dict(lda=66), "bad k / lda / rows"), (lib.F32, dict(rows=2), "bad k / lda / rows"),
    (lib.F32, dict(N=1 << 40, k=(1 << 40) - 1), "too many rows"), (lib.F32, dict(rows=BIG + 1), "too many rows"),
    (lib.F32X3P, dict(a_out=A + 64), "128-byte"), (lib.F32X3P, dict(lda=80), "128-byte"), (lib.F32X3P, dict(C=36, lda=36), "128-byte"),
    (99, {}, "bad dtype"), (lib.F32X6, {}, "bad dtype"),
]


@pytest.mark.parametrize("dtype,over,reason", GATHER_COMMON + [(lib.F32, dict(N=1089, k=64), "N - k = 1025 dropped tokens per window exceed the kernel's 1024")])
def test_gather_merge_ln_ex_refusals(dtype, over, reason):
    _refused("toc3d_gather_merge_ln_ex", _gather(dtype, **over), reason, fn="toc3d_gather_merge_ln")


@pytest.mark.parametrize("dtype,over,reason", GATHER_COMMON + [
    (lib.F32, dict(N=1089, k=64), "bad k / lda / rows"),              # N - k = 1025
    *[(lib.F32, dict(split=s), "split = 2, 4, 8, 16") for s in (1, 3, 32, -2)],
    (lib.F32, dict(scratch=None), "256-byte aligned, zeroed once"), (lib.F32, dict(scratch=A + 128), "256-byte aligned, zeroed once"),
    (lib.F32, dict(scratch_bytes=16384 + 3 * 16 * 64 * 4 - 1), "256-byte aligned, zeroed once"),
    (lib.F32, dict(nW=4097, rows=5000), "at most 4096 windows per launch"),
])
def test_gather_merge_ln_split_refusals(dtype, over, reason):
    _refused("toc3d_gather_merge_ln_split", _gather(dtype, **dict(dict(split=0), **over)), reason)


def test_gather_merge_ln_empty_calls_and_scratch_size():
    l = lib.load()
    assert _call("toc3d_gather_merge_ln_ex", *_gather(nW=0))[0] == 0
    assert _call("toc3d_gather_merge_ln_split", *_gather(split=8, nW=0))[0] == 0
    assert _call("toc3d_gather_merge_ln_split", *_gather(split=0, nW=-3, scratch_bytes=0))[0] == 0
    assert int(l.toc3d_gather_merge_ln_scratch_bytes(3, 64)) == 16384 + 3 * 16 * 64 * 4
    assert int(l.toc3d_gather_merge_ln_scratch_bytes(0, 64)) == 0 and int(l.toc3d_gather_merge_ln_scratch_bytes(3, 0)) == 0


# ---- toc3d_scatter_update ---------------------------------------------------------------------------
def _scatter(**o):
    a = dict(x=A, C=64, tok=A, prow=A, nW=3, N=16, k=5, slow=A, r1=A, r2=A, r3=None, r4=None)
    a.update(o)
    return (a["x"], a["C"], a["tok"], a["prow"], a["nW"], a["N"], a["k"], a["slow"], a["r1"], a["r2"], a["r3"], a["r4"], None)


@pytest.mark.parametrize("over,reason", [
    *[({p: None}, "null buffer") for p in ("x", "tok", "prow", "slow", "r1", "r2")],
    (dict(r3=A), "come as a pair"), (dict(r4=A), "come as a pair"),
    (dict(C=0), "bad dims"), (dict(C=66), "bad dims"), (dict(C=1 << 32), "bad dims"), (dict(k=-1), "bad dims"), (dict(k=16), "bad dims"), (dict(N=0, k=0), "bad dims"),
    # one wavefront per slot: nW * N beyond 32 bits would wrap the grid size and the kernel's own int counts (nW * N itself beyond int64 too)
    (dict(nW=1 << 28, r3=A, r4=A), "too many slots"), (dict(nW=1 << 62), "too many slots"), (dict(N=1 << 33, k=1, nW=1), "too many slots"),
])
def test_scatter_update_refusals(over, reason):
    _refused("toc3d_scatter_update", _scatter(**over), reason)


def test_scatter_update_empty_call():
    assert _call("toc3d_scatter_update", *_scatter(nW=0))[0] == 0
    assert _call("toc3d_scatter_update", *_scatter(nW=-1, r3=A, r4=A))[0] == 0


# ---- toc3d_rebase_layernorm_rows ----------------------------------------------------------------------
REBASE_PTRS = ("slow", "rep_index", "tok", "wgt", "r1", "r2", "gamma", "beta", "out")


def _rebase(dtype=lib.F32, **o):
    a = dict({p: A for p in REBASE_PTRS}, C=64, N=16, k=5, ldo=64, rows=18)
    a.update(o)
    return (dtype, a["slow"], a["C"], a["rep_index"], a["tok"], a["wgt"], a["N"], a["k"], a["r1"], a["r2"], a["gamma"], a["beta"], 1e-6, a["out"], a["ldo"], a["rows"], None)


@pytest.mark.parametrize("dtype,over,reason", [
    *[(lib.F32, {p: None}, "null buffer") for p in REBASE_PTRS],
    (lib.F32, dict(C=0), "bad dims"), (lib.F32, dict(C=66, ldo=68), "bad dims"), (lib.BF16, dict(C=2052, ldo=2052), "bad dims"), (lib.F32, dict(ldo=60), "bad dims"),
    (lib.BF16, dict(ldo=66), "bad dims"), (lib.F32, dict(k=-1), "bad dims"), (lib.F32, dict(k=16), "bad dims"),
    (lib.F32, dict(rows=BIG + 1), "too many rows"), (lib.F32, dict(N=1 << 40), "too many rows"),
    (lib.F32X3P, dict(out=A + 64), "128-byte"), (lib.F32X3P, dict(ldo=80), "128-byte"), (lib.F32X3P, dict(C=36, ldo=36), "128-byte"),
    (99, {}, "bad dtype"), (lib.F32X3W, {}, "bad dtype"),
])
def test_rebase_layernorm_rows_refusals(dtype, over, reason):
    _refused("toc3d_rebase_layernorm_rows", _rebase(dtype, **over), reason)


def test_row_kernels_empty_calls():
    assert _call("toc3d_rebase_layernorm_rows", *_rebase(rows=0))[0] == 0
    assert _call("toc3d_rebase_layernorm_rows", *_rebase(lib.BF16, rows=-4))[0] == 0
    assert _call("toc3d_layernorm_rows", *_ln(M=0))[0] == 0
    assert _call("toc3d_layernorm_rows", *_ln(lib.BF16, M=-1, row_index=A, row_scale=A))[0] == 0


# ---- the references of tests/test_gpu_token_kernels.py ----------------------------------------------------
SWEEP = [(V, h, w, L, k, planted) for L in (3, 7, 8) for (V, h, w) in (T.GRIDS[L], (1, L, 2 * L), (3, L + 1, L - 1)) for k in T.KS[L] for planted in (False, True)]


def test_layout_reference_invariants():
    """Rows per window sum to toc3d_window_topk_rows; every real token appears exactly once, kept (one compact row of its own) or dropped; cap + virtual keys =
    k + 1; explicit zero rows exist exactly where a real token lost against a pad; the planted cases reach e_w > 0 with k below and above the real count."""
    l = lib.load()
    seen_below = seen_above = seen_tie = False
    for (V, h, w, L, k, planted) in SWEEP:
        N = L * L
        sc = T.make_scores(V, h, w, L, seed=L + k, planted=planted)
        assert float(sc.max()) < 0
        r = T.layout_reference(sc, V, h, w, L, k)
        nW = r["tok"].shape[0]
        assert sum(r["cap"]) == r["ms"] == int(l.toc3d_window_topk_rows(V, h, w, L, k))
        assert not (r["crow_tok"] == -9).any() and not (r["arows"] == -9).any() and not (r["aslots"] == -9).any() and not (r["crow_rc"] == -9).any()
        kept = r["crow_tok"][r["crow_tok"] >= 0]
        dropped = r["tok"][:, k:][r["tok"][:, k:] >= 0]
        assert sorted(kept.tolist() + dropped.tolist()) == list(range(V * h * w))
        assert int((r["crow_tok"] == -2).sum()) == nW and int((r["crow_tok"] == -1).sum()) == sum(r["e_w"])
        for i in range(nW):
            virtual = int((r["arows"][i] == -1).sum())
            assert r["cap"][i] + virtual == k + 1 and r["acount_q"][i] == r["cap"][i] and r["acount_k"][i] == k + 1
            assert r["arows"][i, :r["cap"][i]].tolist() == list(range(int(r["rep_row"][i]) - r["cap"][i] + 1, int(r["rep_row"][i]) + 1))
            assert sorted(r["aslots"][i].tolist()) == sorted(r["order"][i, :k].tolist() + [k])          # RoPE slots: the k kept slots and slot k for the representative
            lost = int((r["tok"][i, k:] >= 0).sum())                       # real tokens that were dropped
            assert r["e_w"][i] == min(k, r["real"][i]) - (r["real"][i] - lost) >= 0
            assert (r["e_w"][i] > 0) <= (r["real"][i] < N), "a full window has no pad to lose against"
            if not planted:
                assert r["e_w"][i] == 0
            seen_below |= r["e_w"][i] > 0 and k <= r["real"][i]
            seen_above |= r["e_w"][i] > 0 and k > r["real"][i]
        assert abs(float(r["wgt"][:, k:].sum(1).sub(1).abs().max())) < 1e-12 and float(r["wgt"].min()) >= 0
        seen_tie |= planted and bool((sc == -1e6).any())
    assert seen_below and seen_above and seen_tie


def test_layout_reference_on_a_window_worked_by_hand():
    """L = 2, one ragged window (one real column), k = 2: slots 0, 2 real (scores -2e6, -1), slots 1, 3 pads.  Rank: slot 2 (-1), pads 1, 3 (-1e6), slot 0.
    k best = {2, 1}: r_w = 1, cap = min(2, 2) + 1 = 3, e_w = 1: rows = [token of slot 2, zero row (pad slot 1), representative]; no virtual key."""
    sc = torch.tensor([[[-2e6], [-1.0]]])
    r = T.layout_reference(sc, 1, 2, 1, 2, 2)
    assert r["order"].tolist() == [[2, 1, 3, 0]] and r["tok"].tolist() == [[1, -1, -1, 0]]
    assert r["crow_tok"].tolist() == [1, -1, -2] and r["prow"].tolist() == [[0, 1, -1, -1]] and r["rep_index"].tolist() == [-1, -1, 0]
    assert r["arows"].tolist() == [[0, 1, 2]] and r["aslots"].tolist() == [[2, 1, 2]] and r["crow_rc"].tolist() == [1 << 16, 1, 1 << 16]
    assert r["e_w"] == [1] and r["cap"] == [3]
    r = T.layout_reference(sc, 1, 2, 1, 2, 3)                          # k = 3 > real = 2: cap = 3, k best = {2, 1, 3}: e_w = 1, one virtual key (slot 3)
    assert r["crow_tok"].tolist() == [1, -1, -2] and r["arows"].tolist() == [[0, 1, 2, -1]] and r["aslots"].tolist() == [[2, 1, 3, 3]]


def test_remap_sweep_covers_every_residue_pair():
    cases, need = T.remap_sweep_cases()
    assert all(v is not None for v in need.values())
    ex = {(key[1], key[2]) for key in need if key[0] is None and not key[3]}
    assert ex == {(a, b) for a in range(8) for b in range(8)}, "_ex: every (nW mod 8, kept-row blocks mod 8)"
    assert any(key[0] is None and key[3] for key in need) and ("nW<8", True) in need and ("nW<8", False) in need
    for s in T.SPLITS:
        assert {key[2] for key in need if key[0] == s} == set(range(8)) and any(key[0] == s and key[3] for key in need), s
    assert len(cases) < 200
