"""GPU: the token kernels of csrc/tokens.hip alone -- toc3d_window_topk, toc3d_gather_merge_ln[_ex|_split], toc3d_scatter_update, toc3d_rebase_layernorm_rows and
toc3d_layernorm_rows at C > 1024 -- against f64 references of the same seeded f32 inputs, at the column tails, row-block counts, k extremes and explicit
zero rows tests/test_gpu_ops.py never reaches.  Index outputs and everything that is only copied or added in a fixed order are compared BIT FOR BIT;
everything else per element, against a bound derived from the kernel's own operation count (u = 2^-24), never against a global ratio: a ragged window's
representative row is ~1e-6 of its neighbours and would vanish in one.

Inputs.  Scores are < 0 like log-probabilities (the merge denominator then has no cancellation).  Rows are 0.5 randn + 3 and the block outputs r1..r4 are
0.25 randn - 0.5, so that EVERY row a LayerNorm sees here has sigma <= |mean| (asserted in `ln_reference`); the LayerNorm bound below needs it.

Merge (representative row), per element c, weights w_j >= 0 computed in f64 from the f32 scores:
    |dev - ref| <= (2 (N - k) + 4) u sum_j |w_j| |x_jc|
    (the f32 denominator: (N - k) u; the division and the product: 2 u; the sum of N - k products in any order: (N - k) u; slack 2 u).

LayerNorm (wave_ln_stats / wave_ln_write: two-pass statistics), against f64 LayerNorm of the DEVICE's own f32 input row v, so that no rounding of an earlier
step can hide an error here or excuse one.  D = 4 MAXV + 6 is the number of additions an element passes through in either reduction (4 MAXV in the lane:
3 inside a float4 and 1 onto the running sum per float4; 6 butterfly levels across the wavefront); MAXV = 4 for C <= 1024, 8 above.
    mean:  |dm| <= (D + 2) u mean|v|                       (summation D u sum|v|, division by C; one u of slack)
           mean|v| <= sqrt(sigma^2 + mean^2) <= sqrt(2) |mean|            for sigma <= |mean|
    rstd:  the centred sum of squares sees dm only in second order (sum d = 0); relative error <= (D / 2 + 6.5) u
           (3 u per square incl. the subtraction, D u summation, division by C, + eps, square root and reciprocal at 2 u each; halved by the root)
    y_c = (v_c - mean) rstd gamma_c + beta_c:   subtraction, two products, one addition:
           |dy_c| <= u [ (D / 2 + 10.5) |gamma_c| |v_c - mean| rstd + sqrt(2) (D + 2) |gamma_c| |mean| rstd + |beta_c| ]
                  <= kappa u ( |gamma_c| (|v_c - mean| + |mean|) rstd + |beta_c| ),   kappa = ceil(sqrt(2) (D + 2)) = 34 (MAXV = 4), 57 (MAXV = 8).
    Output rounding: bf16 adds 2^-8 |y|, (hi, lo) planes 2^-16 |y| (applied to the value actually rounded: |y| + the bound above).  bf16 keeps 8 significant
    bits, so round-to-nearest errs by up to half an ulp = 2^-8 of a value just above a power of two (as f32's 24 bits give u = 2^-24); a first draft of this
    suite had 2^-9 here, which a CORRECTLY rounded conversion exceeds by up to 2 x.  Planes: lo = bf16(y - bf16(y)) leaves (2^-8)^2 = 2^-16.

Rebase (representative rows, in place), reference in f64 from the device's wgt / tok:  v - (1 - W)(r1 + r2), W = sum of wgt over the real dropped slots:
    |err_c| <= ((N - k) + 4) u |delta_c| + 3 u (|v_c| + |delta_c|)
    (W: (N - k) u; 1 - W, r1 + r2, the product: 3 u |delta|; the subtraction u (|v| + |delta|); slack.)

Selection weights: wgt = s / sum(s) with a same-sign f32 sum of N - k terms and one division: |dev - ref| <= ((N - k) + 2) u |ref|.

toc3d_scatter_update only copies and adds f32 in a fixed order ((x + r1) + r2, then (. + r3) + r4): the reference is f32 torch on the CPU, bit for bit.
"""
import math

import pytest
import torch

import token_cases as T
from oracle import toc3d_oracle as O
from support import DEV, S, _run_topk, bits, is_sent, planes_halves, rnd, sent, worst_report
from toc3d_amd import lib

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
EPS = 1e-6
G = 3                                                    # guard rows on both sides of every output
KAPPA = {4: 34, 8: 57}
COLS = [4, 60, 252, 256, 260, 508, 516, 1020, 1024]
KINDS = ["f32", "bf16", "planes"]
DT = {"f32": lib.F32, "bf16": lib.BF16, "planes": lib.F32X3P}
OUT_ROUND = {"f32": 0.0, "bf16": 2.0 ** -8, "planes": 2.0 ** -16}
note, _report = worst_report("token kernels", 58)


# ---- buffers with sentinels (support.sent / is_sent) ----------------------------------------------------
def decode(a, kind, C):
    """Output rows [R, ld] (CPU) -> (values f64 [R, C], True if nothing of the columns [C, ld) was written)."""
    R, ld = a.shape
    if kind != "planes":
        return a[:, :C].double(), is_sent(a[:, C:]) if ld > C else True
    hi, lo = planes_halves(a)
    clean = bool((hi[:, C:] == 0x7FC1).all() and (lo[:, C:] == 0x7FC1).all())
    hv, lv = hi[:, :C].contiguous().view(torch.bfloat16).double(), lo[:, :C].contiguous().view(torch.bfloat16).double()
    assert bool((lv.abs() <= 2.0 ** -8 * hv.abs()).all()), "lo plane is the bf16 remainder of the hi plane"
    return hv + lv, clean


def ld_pair(C, kind):
    """[(ld, padded)]: ld = C and ld > C; rows of planes have leading dimensions that are multiples of 32 (include/toc3d.h), so there C % 32 != 0 only runs padded."""
    if kind == "planes":
        return ([(C, False)] if C % 32 == 0 else []) + [((C + 32) // 32 * 32 + (32 if C % 32 == 0 else 0), True)]
    return [(C, False), (C + 12, True)]


def ln_reference(v, gw, gb, maxv):
    """v f64 [R, C] -> (f64 LayerNorm, the derived per-element bound before output rounding)."""
    mean = v.mean(1, keepdim=True)
    d = v - mean
    var = (d * d).mean(1, keepdim=True)
    zero = v.abs().amax(1, keepdim=True) == 0
    assert bool(((var <= mean * mean) | zero).all()), "the LayerNorm bound is derived for rows with sigma <= |mean|"
    rstd = 1.0 / torch.sqrt(var + EPS)
    y = O.layer_norm(v, gw, gb, EPS)
    assert float((y - (d * rstd * gw + gb)).abs().max()) < 1e-12
    return y, KAPPA[maxv] * U * (gw.abs() * (d.abs() + mean.abs()) * rstd + gb.abs())


def check_ln(tag, a_rows, kind, C, v, gw, gb, maxv):
    y, b = ln_reference(v, gw, gb, maxv)
    vals, clean = decode(a_rows, kind, C)
    assert clean, f"{tag}: columns [C, ld) of the output were written"
    tol = b + OUT_ROUND[kind] * (y.abs() + b)
    err = (vals - y).abs()
    assert bool((err <= tol).all()), f"{tag}: LayerNorm off by {float((err / tol.clamp_min(1e-300)).nan_to_num(nan=math.inf).max()):.3f} x its bound"
    note(tag, (err / tol.clamp_min(1e-300)).max())


def params(C):
    return (1 + 0.1 * rnd(C, seed=2)).double(), (0.1 * rnd(C, seed=3)).double()


def rows_like_x(n, C, seed):
    return 0.5 * rnd(n, C, seed=seed) + 3.0


def raw_like(n, C, seed):
    return 0.25 * rnd(n, C, seed=seed) - 0.5


# ---- selections (device buffers of toc3d_window_topk + the CPU reference of the layout) ---------------------
_SEL = {}
INT_OUTS = ("order", "tok", "prow", "crow_tok", "rep_index", "rep_row", "arows", "aslots", "acount_q", "acount_k", "crow_rc")


def selection(L, k, planted=True, grid=None, seed=None):
    V, h, w = grid or T.GRIDS[L]
    key = (V, h, w, L, k, planted, seed)
    if key not in _SEL:
        sc = T.make_scores(V, h, w, L, seed=L + k if seed is None else seed, planted=planted)
        b = _run_topk(sc, V, h, w, L, k)
        ref = T.layout_reference(sc, V, h, w, L, k)
        assert b["ms"] == ref["ms"]
        _SEL[key] = dict(b, ref=ref, scores=sc, V=V, h=h, w=w, L=L, k=k)
    return _SEL[key]


def check_selection(sel):
    b, ref, k, N = sel, sel["ref"], sel["k"], sel["N"]
    for name in INT_OUTS:
        assert torch.equal(b[name].cpu().long(), ref[name]), f"{name} differs from the layout reference (L={sel['L']} k={k} grid={sel['V'], sel['h'], sel['w']})"
    wg = b["wgt"].cpu().double()
    assert bool((wg[:, :k] == 0).all())
    err, tol = (wg - ref["wgt"]).abs()[:, k:], ((N - k) + 2) * U * ref["wgt"][:, k:]
    assert bool((err <= tol).all())
    note("window_topk wgt", (err / tol.clamp_min(1e-300)).max())


# ---- A. the selection layout in general ---------------------------------------------------------------------
@pytest.mark.parametrize("L", [3, 7, 8])
def test_window_topk_layout_with_zero_rows_and_k_extremes(L):
    """Every output of toc3d_window_topk against tests/token_cases.layout_reference (which does not assume e_w == 0), bit for bit (wgt: to its bound): grids
    whose edge windows have one real token / row / column, k in {0, 1, N - 1, above a ragged window's real count}, real scores of -2e6 (explicit zero rows,
    with k below and above the window's real count) and of exactly -1e6 (tie with the pads, the slot decides), ties among real tokens.  (A FULL window cannot
    have e_w > 0: it has no pad to lose against; -2e6 is planted there too and only reorders it.)"""
    n_zero = 0
    for grid in (T.GRIDS[L], (1, L, 2 * L), (3, L + 1, L - 1)):
        for k in T.KS[L]:
            for planted in (False, True):
                sel = selection(L, k, planted, grid)
                check_selection(sel)
                n_zero += sum(sel["ref"]["e_w"])
    assert n_zero > 0


# ---- B. gather + merge + LayerNorm ----------------------------------------------------------------------------
def gather_inputs(sel, C, seed=11):
    """x f32 [V*h*w, C] and, in f64, the reference representative rows [nW, C] with the sum_j |w_j| |x_jc| of their bound (oracle helpers on double tensors)."""
    V, h, w, L, k = (sel[n] for n in ("V", "h", "w", "L", "k"))
    N = L * L
    x = rows_like_x(V * h * w, C, seed)
    xw = O.window_partition(x.double().reshape(V, h, w, C), L)[0].reshape(-1, N, C)
    s_sorted, order = O.sort_desc_stable(T.window_scores(sel["scores"], L))
    assert torch.equal(order, sel["ref"]["order"])
    xd = O.gather_rows(xw, order[:, k:])
    rep = O.merge_tokens(xd, s_sorted[:, k:].double())[:, 0]
    mag = O.merge_tokens(xd.abs(), s_sorted[:, k:].double())[:, 0]
    return x, rep, mag


def launch_gather(sel, xd, C, kind, lda, kept_copy, gw, gb, split=None, scratch=None):
    ms = sel["ms"]
    short, a = sent(ms + 2 * G, C, False), sent(ms + 2 * G, lda, kind == "bf16")
    head = (DT[kind], xd, C, sel["tok"], sel["wgt"], sel["crow_tok"], sel["rep_row"], sel["nW"], sel["N"], sel["k"], ms, gw, gb, EPS, short[G:], a[G:], lda, kept_copy)
    if split is None:
        lib.call("toc3d_gather_merge_ln_ex", *head, S())
    else:
        lib.call("toc3d_gather_merge_ln_split", *head, scratch, scratch.numel() * 4, split, S())
    return short, a


def check_gather(tag, sel, x, rep, mag, C, kind, lda, kept_copy, short_full, a_full, gw, gb):
    ms, N, k, ref = sel["ms"], sel["N"], sel["k"], sel["ref"]
    short_full, a_full = short_full.cpu(), a_full.cpu()
    for buf in (short_full, a_full):
        assert is_sent(buf[:G]) and is_sent(buf[G + ms:]), f"{tag}: rows outside the compact set were written"
    short, crow = short_full[G:G + ms], ref["crow_tok"]
    kept, zero, reps = crow >= 0, crow == -1, ref["rep_row"]
    if kept_copy:
        assert torch.equal(short[kept].view(torch.int32), x[crow[kept]].view(torch.int32)), f"{tag}: kept rows are copies of their tokens"
    else:
        assert is_sent(short[kept]), f"{tag}: kept_copy = 0 leaves the f32 kept rows alone"
    assert bool((short[zero].view(torch.int32) == 0).all()), f"{tag}: explicit zero rows are +0"
    err, tol = (short[reps].double() - rep).abs(), (2 * (N - k) + 4) * U * mag
    assert bool((err <= tol).all()), f"{tag}: representative rows off by {float((err / tol).nan_to_num(nan=math.inf).max()):.3f} x the merge bound"
    note("gather merge (representative rows)", (err / tol).max())
    v = short.double()
    if not kept_copy:
        v[kept] = x[crow[kept]].double()
    check_ln(f"gather LayerNorm {kind}", a_full[G:G + ms], kind, C, v, gw, gb, 4)
    if bool(zero.any()):
        zr = decode(a_full[G:G + ms][zero], kind, C)[0]
        want = gb.float() if kind == "f32" else gb.float().bfloat16().double() if kind == "bf16" else None
        if want is not None:
            assert bool((zr == want.double()).all()), f"{tag}: LayerNorm of a zero row is beta in the output type"


def gather_case(tag, sel, C, kinds=KINDS, copies=(1, 0), pads=(False, True), splits=T.SPLITS):
    """_ex at every (kind, lda, kept_copy) against f64, then every split against _ex bit for bit; the arrival counters are zero afterwards."""
    x, rep, mag = gather_inputs(sel, C)
    gw, gb = params(C)
    xd, gwd, gbd = x.to(DEV), gw.float().to(DEV), gb.float().to(DEV)
    nbytes = int(lib.load().toc3d_gather_merge_ln_scratch_bytes(sel["nW"], C))
    scratch = torch.zeros(nbytes // 4, device=DEV)
    for kind in kinds:
        for lda in [ld for ld, padded in ld_pair(C, kind) if padded in pads]:
            for kept_copy in copies:
                t = f"{tag} C={C} {kind} lda={lda} kept_copy={kept_copy}"
                short, a = launch_gather(sel, xd, C, kind, lda, kept_copy, gwd, gbd)
                check_gather(t, sel, x, rep, mag, C, kind, lda, kept_copy, short, a, gw, gb)
                for sp in splits:
                    s2, a2 = launch_gather(sel, xd, C, kind, lda, kept_copy, gwd, gbd, split=sp, scratch=scratch)
                    assert torch.equal(bits(s2), bits(short)) and torch.equal(bits(a2), bits(a)), f"{t}: split={sp} differs from _ex"
    assert int(scratch[:sel["nW"]].view(torch.int32).abs().sum().item()) == 0, "arrival counters re-armed"


@pytest.mark.parametrize("C", COLS)
def test_gather_merge_ln_column_classes(C):
    """Every column class (one float4, partial first / second / third / fourth wavefront pass, the exact multiples) x {f32, bf16, planes} x {lda = C, lda > C}
    x kept_copy, on a selection with ragged windows, k above their real count and explicit zero rows."""
    sel = selection(7, 20)
    assert sum(sel["ref"]["e_w"]) > 0
    gather_case("columns", sel, C)


@pytest.mark.parametrize("L,k", [(32, 0), (8, 63), (8, 49), (8, 48), (8, 47), (3, 0), (7, 6)])
def test_gather_merge_ln_k_classes(L, k):
    """k = 0 with N - k = 1024 (the limit: every lane of every wave owns a dropped slot), k = N - 1 (one dropped slot: 15 waves own nothing), N - k in
    {15, 16, 17} (the edges of the k + wave + 16 j ownership), k = 0 on small windows, and explicit zero rows with k below the ragged windows' real count."""
    sel = selection(L, k)
    gather_case(f"L={L} k={k}", sel, 60, kinds=["f32", "bf16"], pads=(False,))


def test_gather_merge_ln_row_block_remap_sweep():
    """L = 4, C = 64: (V, h, w, k) chosen (tests/token_cases.remap_sweep_cases; coverage asserted in tests/test_cpu_token_abi.py) so that _ex sees every
    (nW mod 8, kept-row blocks mod 8) and each split's own block count (64 * 16 / split threads per block) every residue, with fewer than 8 windows and fewer
    than 8 kept-row blocks among them.  A remap that is not a bijection at one of them leaves rows unwritten (sentinel) or written twice."""
    cases, _ = T.remap_sweep_cases()
    for (V, h, w, k) in cases:
        sel = selection(4, k, planted=(V + h + w) % 3 == 0, grid=(V, h, w), seed=V + h + w + k)
        gather_case(f"remap V={V} h={h} w={w} k={k}", sel, 64, kinds=["f32"], copies=(1,), pads=(False,))


# ---- C. scatter, bit-exact --------------------------------------------------------------------------------------
def scatter_case(sel, C, four, seed=21):
    ref, nW, N, k, ms = sel["ref"], sel["nW"], sel["N"], sel["k"], sel["ms"]
    n_tok = sel["V"] * sel["h"] * sel["w"]
    g = torch.Generator().manual_seed(seed)
    x_full = torch.randn(n_tok + 2 * G, C, generator=g)
    slow = torch.randn(ms, C, generator=g)
    r = [torch.randn(nW, C, generator=g) for _ in range(4)]
    want = x_full.clone()
    tok, prow = ref["tok"], ref["prow"]
    pos = torch.arange(N)[None, :].expand(nW, N)
    win = torch.arange(nW)[:, None].expand(nW, N)
    mk, md = (tok >= 0) & (pos < k), (tok >= 0) & (pos >= k)
    assert bool((prow[mk] >= 0).all())
    want[G + tok[mk]] = slow[prow[mk]]
    upd = (x_full[G + tok[md]] + r[0][win[md]]) + r[1][win[md]]
    if four:
        upd = (upd + r[2][win[md]]) + r[3][win[md]]
    want[G + tok[md]] = upd
    xd = x_full.to(DEV)
    rd = [t.to(DEV) for t in r]
    lib.call("toc3d_scatter_update", xd[G:], C, sel["tok"], sel["prow"], nW, N, k, slow.to(DEV), rd[0], rd[1], rd[2] if four else None, rd[3] if four else None, S())
    assert torch.equal(xd.cpu().view(torch.int32), want.view(torch.int32)), f"scatter C={C} L={sel['L']} k={k} four={four}"


@pytest.mark.parametrize("C", COLS)
def test_scatter_update_bit_exact(C):
    """Both forms (two and four updates) over the whole of x plus guard rows, on selections with k = 0, explicit zero rows, ragged windows and kept pads:
    pad slots, virtual pads (prow = -1) and zero rows (tok = -1) write nothing."""
    for (L, k, planted) in [(7, 0, True), (7, 20, True), (3, 8, True), (8, 1, False), (7, 48, True)]:
        for four in (False, True):
            scatter_case(selection(L, k, planted), C, four)


def test_scatter_update_row_block_counts():
    """ceil(nW * N / 4) workgroups through xcd_remap: every residue mod 8, and fewer than 8 (the early-out)."""
    seen = set()
    for n in range(1, 9):
        sel = selection(3, 4, True, grid=(1, 3, 3 * n))
        blocks = -(-sel["nW"] * 9 // 4)
        seen.add((blocks % 8, blocks < 8))
        for C in (4, 64):
            scatter_case(sel, C, n % 2 == 0)
    assert {m for m, _ in seen} == set(range(8)) and any(small for _, small in seen) and not all(small for _, small in seen)


# ---- D. rebase + LayerNorm ---------------------------------------------------------------------------------------
def rebase_case(tag, sel, C, kind, ldo, seed=31):
    ms, nW, N, k, ref = sel["ms"], sel["nW"], sel["N"], sel["k"], sel["ref"]
    maxv = 4 if C <= 1024 else 8
    slow_full = rows_like_x(ms + 2 * G, C, seed)
    r1, r2 = raw_like(nW, C, seed + 1), raw_like(nW, C, seed + 2)
    gw, gb = params(C)
    sd, out = slow_full.to(DEV), sent(ms + 2 * G, ldo, kind == "bf16")
    lib.call("toc3d_rebase_layernorm_rows", DT[kind], sd[G:], C, sel["rep_index"], sel["tok"], sel["wgt"], N, k, r1.to(DEV), r2.to(DEV),
             gw.float().to(DEV), gb.float().to(DEV), EPS, out[G:], ldo, ms, S())
    got, out = sd.cpu(), out.cpu()
    assert is_sent(out[:G]) and is_sent(out[G + ms:]), f"{tag}: output rows outside [0, rows) were written"
    reps = ref["rep_row"]
    other = torch.ones(ms + 2 * G, dtype=torch.bool)
    other[G + reps] = False
    assert torch.equal(got[other].view(torch.int32), slow_full[other].view(torch.int32)), f"{tag}: non-representative rows (and the guard rows) are unchanged"
    tok_d, wgt_d = sel["tok"].cpu(), sel["wgt"].cpu().double()
    W = (wgt_d[:, k:] * (tok_d[:, k:] >= 0)).sum(1, keepdim=True)
    v, delta = slow_full[G + reps].double(), r1.double() + r2.double()
    want = v - (1 - W) * delta
    err = (got[G + reps].double() - want).abs()
    tol = ((N - k) + 4) * U * delta.abs() + 3 * U * (v.abs() + delta.abs())
    assert bool((err <= tol).all()), f"{tag}: rebased rows off by {float((err / tol).max()):.3f} x the bound"
    note("rebase (representative rows)", (err / tol).max())
    check_ln(f"rebase LayerNorm {kind} MAXV={maxv}", out[G:G + ms], kind, C, got[G:G + ms].double(), gw, gb, maxv)
    return W


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C", [4, 252, 260, 1024, 1028, 2044, 2048])
def test_rebase_layernorm_rows(C, kind):
    """Both MAXV instantiations and their tails, every output type, ldo = C and ldo > C; full windows (W = 1 to rounding), ragged windows that drop a real
    token among their pads (W ~ 1e-7), windows whose dropped set is all pads (W = 0 exactly) and windows that dropped a real token below the pads (-2e6)."""
    kinds_w = []
    for sel in (selection(7, 20, True), selection(7, 20, False), selection(7, 6, False)):
        for ldo, _ in ld_pair(C, kind):
            kinds_w.append(rebase_case(f"rebase C={C} {kind} ldo={ldo} L={sel['L']}", sel, C, kind, ldo))
    W = torch.cat(kinds_w)
    assert bool((W == 0).any()) and bool(((W - 1).abs() < 1e-5).any()) and bool(((W > 0) & (W < 1e-3)).any())


def test_rebase_layernorm_rows_row_block_counts():
    seen = set()
    for n in range(1, 13):
        sel = selection(3, 4, True, grid=(1, 3, 3 * n))
        blocks = -(-sel["ms"] // 4)
        seen.add((blocks % 8, blocks < 8))
        rebase_case(f"rebase blocks={blocks}", sel, 64, "f32", 64)
    assert {m for m, _ in seen} == set(range(8)) and any(small for _, small in seen)


@pytest.mark.parametrize("C,L,k", [(60, 7, 20), (256, 8, 47), (1020, 3, 4)])
def test_rebase_equals_scatter_and_regather(C, L, k):
    """The algebraic claim on the device.  Path 1: gather -> scatter_update(slow, r1, r2) -> gather (the block-by-block form: the representative row is
    re-merged from the updated dropped tokens).  Path 2: gather -> the block leaves rep_in + (r1 + r2) in its compact row -> rebase.  Representative rows agree
    within the sum of the two paths' bounds (path 1: the scatter's two additions, 2 u (|x| + |r1| + |r2|) per dropped token, carried through the weights, and
    the merge bound on the updated tokens; path 2: the merge bound, the block's two additions and the rebase bound); their LayerNorms within both LN bounds plus
    the first-order response of LayerNorm to that difference E: |gamma_c| rstd (E_c + mean E + |d_c| rstd rms E).  Kept rows are bit-equal in both outputs."""
    sel = selection(L, k)
    ms, nW, N, ref = sel["ms"], sel["nW"], sel["N"], sel["ref"]
    x, rep, mag = gather_inputs(sel, C)
    r1, r2 = raw_like(nW, C, 41), raw_like(nW, C, 42)
    gw, gb = params(C)
    gwd, gbd, r1d, r2d = gw.float().to(DEV), gb.float().to(DEV), r1.to(DEV), r2.to(DEV)
    reps = ref["rep_row"]
    xd = x.to(DEV)
    s1, _ = launch_gather(sel, xd, C, "f32", C, 1, gwd, gbd)
    x2 = xd.clone()
    lib.call("toc3d_scatter_update", x2, C, sel["tok"], sel["prow"], nW, N, k, s1[G:], r1d, r2d, None, None, S())
    s1b, a1b = launch_gather(sel, x2, C, "f32", C, 1, gwd, gbd)
    s2, _ = launch_gather(sel, xd, C, "f32", C, 1, gwd, gbd)
    rows = s2[G:G + ms]
    rows[reps.to(DEV)] = (rows[reps.to(DEV)] + r1d) + r2d
    a2 = sent(ms, C, False)
    lib.call("toc3d_rebase_layernorm_rows", lib.F32, rows, C, sel["rep_index"], sel["tok"], sel["wgt"], N, k, r1d, r2d, gwd, gbd, EPS, a2, C, ms, S())
    p1, p2, o1, o2 = s1b[G:G + ms].cpu(), rows.cpu(), a1b[G:G + ms].cpu(), a2.cpu()
    keptm = ref["crow_tok"] != -2
    assert torch.equal(p1[keptm].view(torch.int32), p2[keptm].view(torch.int32)) and torch.equal(o1[keptm].view(torch.int32), o2[keptm].view(torch.int32))
    # bounds, in f64: W and the weighted magnitudes of the updated dropped tokens
    wgt = ref["wgt"]
    real = (ref["tok"] >= 0) & (wgt > 0)
    W = (wgt * real).sum(1, keepdim=True)
    dabs, delta = r1.abs().double() + r2.abs().double(), r1.double() + r2.double()
    mag2 = mag + W * dabs                                            # sum_j w_j |x_j + delta| <= sum_j w_j |x_j| + W |delta|
    merge = lambda m: (2 * (N - k) + 4) * U * m
    path1 = 2 * U * mag2 + merge(mag2)
    rep_in = rep                                                     # (magnitudes only: the f64 reference row stands for the device's)
    path2 = merge(mag) + 2 * U * (rep_in.abs() + dabs) + ((N - k) + 4) * U * delta.abs() + 3 * U * (rep_in.abs() + 2 * dabs)
    E = path1 + path2
    err = (p1[reps].double() - p2[reps].double()).abs()
    assert bool((err <= E).all()), float((err / E).max())
    note("rebase vs scatter + re-gather (representative rows)", (err / E).max())
    v = p2[reps].double()
    y, b = ln_reference(v, gw, gb, 4)
    mean = v.mean(1, keepdim=True)
    d = v - mean
    rstd = 1.0 / torch.sqrt((d * d).mean(1, keepdim=True) + EPS)
    resp = gw.abs() * rstd * (E + E.mean(1, keepdim=True) + d.abs() * rstd * (E * E).mean(1, keepdim=True).sqrt())
    tol = 2 * b + resp
    lerr = (o1[reps].double() - o2[reps].double()).abs()
    assert bool((lerr <= tol).all()), float((lerr / tol).max())
    note("rebase vs scatter + re-gather (LayerNorm)", (lerr / tol).max())


# ---- E. toc3d_layernorm_rows above 1024 columns ---------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C", [1028, 2048])
def test_layernorm_rows_wide(C, kind):
    """The MAXV = 8 form of ln_rows_kernel (1024 < C <= 2048; nothing else launches it), plain and with row_index (-1 = zero row -> beta) and row_scale, with
    fewer than 8 row blocks and more, ldx > C."""
    gw, gb = params(C)
    gwd, gbd = gw.float().to(DEV), gb.float().to(DEV)
    for M, n_src in ((37, 50), (9, 9)):
        ldx = C + 8
        x = rows_like_x(n_src, ldx, 51)
        xd = x.to(DEV)
        g = torch.Generator().manual_seed(M)
        idx = torch.randint(0, n_src, (M,), generator=g, dtype=torch.int32)
        idx[::5] = -1
        scale = 0.5 + torch.rand(n_src, generator=g)
        for use_idx, use_scale in ((False, False), (True, False), (True, True), (False, True)):
            for ldo, _ in ld_pair(C, kind):
                out = sent(M + 2 * G, ldo, kind == "bf16")
                lib.call("toc3d_layernorm_rows", DT[kind], xd, ldx, idx.to(DEV) if use_idx else None, scale.to(DEV) if use_scale else None, gwd, gbd, EPS,
                         out[G:], ldo, M, C, S())
                out = out.cpu()
                assert is_sent(out[:G]) and is_sent(out[G + M:])
                src = idx.long() if use_idx else torch.arange(M)
                v = x[src.clamp_min(0), :C].clone()
                if use_scale:
                    v = v * scale[src.clamp_min(0), None]            # f32 product, as the kernel forms it: the LayerNorm input proper
                v[src < 0] = 0
                check_ln(f"layernorm_rows {kind} MAXV=8", out[G:G + M], kind, C, v.double(), gw, gb, 8)


# ---- F. explicit zero rows through a whole model ------------------------------------------------------------------------
def test_zero_rows_through_the_tiny_model():
    """toc3d_tiny in fp32 with the scorer's log-probs forced and -2e6 planted on a handful of real tokens of a full and of a ragged window (of both window
    sides): the explicit zero rows go through q|k|v, attention (as queries), the projection's gathered residual (res_index = -1) or the shortcut copy, the MLP
    and the scatter.  Same bar as the other tiny fp32 tests: rel_max < 1e-3 against the oracle fed the same scores."""
    import toc3d_amd
    from toc3d_amd import configs, synth
    from toc3d_amd.testing import instrument
    cfg = configs.get("toc3d_tiny")
    sd = synth.make_state_dict(cfg)
    inp = synth.make_inputs(cfg, views_per_frame=2)
    args = (inp["x"], inp["temp_queries"], inp["temp_ref_points"], inp["temp_vel"], inp["temp_timestamp"], inp["temp_ego_pose"], inp["ego_pose_inv"], True, inp["gumbel"])
    cap = {}
    with torch.no_grad():
        o = O.forward_toc3d(sd, cfg, *args, capture=cap)
    B = inp["x"].shape[0]
    h, w = inp["x"].shape[-2] // cfg["patch_size"], inp["x"].shape[-1] // cfg["patch_size"]
    forced, zero_rows = [], {}
    for s in range(3):
        sc = cap[f"stage{s}.pred"][:, :, 0].clone().reshape(B, h, w)
        assert float(sc.max()) <= 0
        sc[0, 2, 2:5] = -2e6                                         # a full window of both sides
        sc[0, h - 2:, 3:6] = -2e6                                    # ragged for side 16 (h = 20), full for side 20
        sc[1, 2:4, w - 4:w - 1] = -2e6                               # ragged for side 20 (w = 50), ragged for side 16 too
        forced.append((sc.reshape(B, h * w), o["token_masks"][s].flatten(1)))
        for L in (cfg["window_size"], cfg["global_window_size"]):
            zero_rows[L] = zero_rows.get(L, []) + [sum(T.layout_reference(sc, B, h, w, L, int(L * L * cfg["token_ratio"][s]))["e_w"])]
    # side 16: the ragged windows hold fewer real tokens than any stage keeps, so every stage has explicit zero rows; side 20: only the first stage keeps
    # as many slots (200) as its ragged window has real tokens
    assert min(zero_rows[cfg["window_size"]]) > 0 and zero_rows[cfg["global_window_size"]][0] > 0, zero_rows
    with torch.no_grad():
        ref = O.forward_toc3d(sd, cfg, *args, forced=forced)["last_feat"]
    d = lambda t: t.to(DEV)
    for gathered in (True, False):
        m = toc3d_amd.build_backbone(dict(cfg, precision="fp32"))
        m.load_state_dict(sd)
        m = instrument(m.to(DEV).eval())
        m.gathered_residual, m.autotune = gathered, False
        out = m(d(inp["x"]), temp_queries=d(inp["temp_queries"]), prev_exists=True, temp_ref_points=d(inp["temp_ref_points"]), temp_vel=d(inp["temp_vel"]),
                temp_timestamp=d(inp["temp_timestamp"]), temp_ego_pose=d(inp["temp_ego_pose"]), ego_pose_inv=d(inp["ego_pose_inv"]), gumbel_noise=inp["gumbel"],
                forced_scores=forced)
        feat = out.img_feats["last_feat"].double().cpu()
        assert bool(torch.isfinite(feat).all())
        rel = float((feat - ref.double()).abs().max() / ref.double().abs().max())
        print(f"[token kernels] zero rows through toc3d_tiny fp32, gathered_residual={gathered}: rel max err {rel:.3e}")
        assert rel < 1e-3, (gathered, rel)
