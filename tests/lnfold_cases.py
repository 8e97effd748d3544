"""Cases, f64 reference, per-element bounds, an f32 emulation and wrong references for the LayerNorm-consuming GEMM epilogues (EPI_SWIGLU_STATS_LN, EPI_RESIDUAL_LN of
toc3d_linear_fused, fed by the statistics of EPI_RESIDUAL_STATS / EPI_SWIGLU_STATS).  Shared by test_gpu_lnfold_kernels.py and test_cpu_lnfold_cases.py; no GPU needed here.

What the kernels evaluate (include/toc3d.h, csrc/gemm_kernels.h ln_rows_prepare_fn, gemm_epilogue):   z[i, n] = rstd_i * (a_i . W'_n - mean_i * c1_n) + c2_n
with (mean, rstd) from ONE-PASS sums  mean = S1 / n,  var = S2 / n - mean^2  -- the accuracy depends on the row: cond_i = (mean_i^2 + var_i) / (var_i + eps), which is the
1 + mean^2 / sigma^2 of a row whose variance is far above eps.  The GEMM multiplies the RAW row; the mean term is subtracted afterwards.

ROW FAMILIES (FAMILIES; row i of a launch belongs to family i mod 23 -- 23 is odd and above 16, so no family fills a 16-row tile, and M = 176 rows = two 64-row slabs and
a partial one give every family 7 or 8 rows; rows M - 2 and M - 1 belong to different families): centred; mean = +-{1, 3, 10, 30, 100, 1000} sigma; one outlier channel at
100 / 1000 sigma in slot 0 (column 1) or in the last, partly valid slot (column n - 1), and one row with both; sigma = 1e-2 / 1e-4 around a mean of 1 (var of the order of
eps and below); exactly constant rows 0 and 3; and a row that is zero on [0, ln_n) and 5.0 on the padding columns [ln_n, K) the kernel must ignore.  The values are what
the PRODUCING launch writes (the test reads them back), so the family names are nominal after a bf16 rounding: the reference takes the rounded values.

SHAPES.  M = 176, N <= 256.  W12_WIDTHS: C per slot count ceil(C / 64) in front of w1|w2 (1, 3, 4, 5, 6, 16, 17, 20; PRE = 4: the prefetch covers slots part + 4 j, j < 4, so
counts 4 .. 16 sit on the prefetch (16 = its last slot), 17 and 20 run the remainder loop `sl >= 4 * PRE`, 1 and 3 leave parts without a slot).  W3_WIDTHS: (Hd, Hp) per slot
count ceil(Hp / 64) in front of w3 (1, 5, 43, 48, 49, 52; PRE = 12: 48 = the last prefetched slot, 49 and 52 the remainder loop).  C = 40, 200, 332, 1028, 1252 and
Hd < Hp have ln_n % 64 != 0: a partly valid last slot and ln_n < K.  No width of these lists is refused by the argument checks (K = ceil(ln_n / 64) * 64 by construction); the
one refusal of the matrix is the split-K launch at K = 64 ("too short for a split of 2"), asserted as such.

PATHS of the preparation (path_of): "plain" = behind the first operand request (variant 19 in bf16, 16 in the bf16 x 3 forms), "early" = before the accumulators exist
(PREP_EARLY: OCC > 1 in the tile table -- variant 16 in bf16; the bf16 x 3 rows of the table all have OCC = 1 outside the RoPE epilogue, so those forms HAVE no early path),
"phased" = gemm_phased_kernel (variant 63; the bf16 x 3 forms are served there on planes only -- a form whose A is plain f32 is refused, and asserted as refused).

REFERENCE.  Two-pass f64 LayerNorm over the first ln_n columns of the values the kernel reads, then the f64 matmul with the packed weights read back, + c2 as packed
(epilogue_cases.explicit_ln_matmul); never the folded formula, and c1 is no input of it.

BOUND per element, u = 2^-24, every constant from a rounding point of the kernels:
  statistics   a 64-column slot is summed in a fixed tree (gemm_epilogue / tile_finish): 4 values in sequence in a lane, the 4 lanes of a group, the 4 groups of a slot:
               3 + 2 + 2 = 7 additions above any value, and for the squares one more rounding of the fma that forms the square: |dS1| <= 7 u sum|x|, |dS2| <= 8 u sum x^2.
               Where every value of a slot is a multiple of 2^q and sum|x| < 2^(q + 24) every partial sum is representable and the slot is EXACT (bf16 rows around a mean: the
               squares are exact and so are their sums); that test is made on the data, slot by slot.  Where the consumer reads A as (hi, lo) planes the producer summed the f32
               values it then split, |x - hi - lo| <= 2^-18 |x|: dS1 += 2^-18 sum|x|, dS2 += 2^-17 sum x^2.  The f64 combine adds < 1e-14.  ln_inv_n is float(1 / n): one u on
               mean and on S2 / n.  dvar = dS2 / n + u m2 + 2 |mean| dmean + dmean^2 + u var (the cast of var to f32); the computed rstd then lies in the BRACKET
               [(var + dvar + eps)^-1/2, (max(var - dvar, 0) + eps)^-1/2] (the clamp at 0 is the kernel's), widened by 5 u (the sum with eps, sqrtf and the division at <= 1 ulp
               = 2 u each).  Term: drstd_i / rstd_i * |ref - c2|; to first order it is kappa_s u cond_i |ref - c2| with kappa_s = (8 + 1 + 2 (7 + 1) + 1) / 2 = 13 for f32 rows.
  cancellation rstd^_i * (e_kind(K) * sum_j |a_ij| |W'_nj| + (dmean + 2 u |mean|) |c1_n| + |mean_i| e_c1 sum_j |W'_nj|): e_kind(K) = 2 u K for bf16 operands (products exact
               in f32; every addition of the accumulation chain is charged one ulp = 2 u, which holds for rounding and for truncation inside the matrix core) and
               2^-16 + 2 u 3 K for the bf16 x 3 forms (three products per element; dropped lo.lo term and the roundings of lo: 3 * 2^-18 plus cross terms < 2^-16); split-K adds
               2 u per slice.  2 u |mean|: its rounding to f32 and the product mean * c1.  e_c1 = (ceil(K / 256) + 8) u: the pack kernels sum c1 in f32, K / 256 values in sequence
               per thread and an 8-level tree -- c1 is no input of the reference, so its own error is the kernels' to carry.
  final        u (2 |ref - c2| + |ref|): the subtraction, the product with rstd and the sum with c2.
  outputs      f32 output = residual + z: + u |out|.  Hidden units h = silu(z1) * z2 of two packed pre-activations with bounds b1, b2: by DERIVATIVES at the reference point plus
               a second-order slack,  |dh| <= (|silu'(z1)| b1 + b1^2 / 4) (|z2| + b2) + |silu(z1)| b2   (max |silu''| = 1 / 2), + ((|z1| + 8) u) |h| for the SiLU itself (exp2 of a
               scaled argument: |z1| u; exp2, the sum with 1, the reciprocal and two products: 8 u) + the output rounding of the form, 2^-8 (bf16) or 2^-16 (planes).  The padding
               units [Hd, Hp) are exactly 0 and bounded by 0.  No element is excluded.

EMULATION (emulate): the kernels' sequence in f32 -- slot sums in the tree above, f64 combine in the order of ln_rows_prepare_fn (part p = slots p, p + 4, ..; (p0 + p1) +
(p2 + p3)), f32 mean / rstd, products in the form's arithmetic (bf16 exact; (hi, lo) split and hi.hi + hi.lo + lo.hi), one f32 rounding per 32-deep K step, the epilogue
expression in f32.  `mut` plants the wrong references of test_cpu_lnfold_cases.py."""
import functools
import math

import torch

import epilogue_cases as E

U = 2.0 ** -24
EPS = 1e-6
M = 176
N3 = 200                                              # output columns of the w3 stage (N % 64 != 0)
HD12, HP12 = 100, 128                                 # hidden units of the w1|w2 stage: N = 256 packed columns, 28 padding units
W12_WIDTHS = {1: 40, 3: 192, 4: 200, 5: 320, 6: 332, 16: 1024, 17: 1028, 20: 1252}
W3_WIDTHS = {1: (50, 64), 5: (290, 304), 43: (2730, 2752), 48: (3072, 3072), 49: (3100, 3136), 52: (3300, 3328)}
PRE = {"w12": 4, "w3": 12}
STAGES = ("w12", "w3")
FORMS = {"bf16": ("BF16", "BF16", "BF16"), "f32x3": ("F32X3", "F32X3", "F32X3"), "f32x3w": ("F32X3W", "F32X3W", "F32X3W"), "f32x3p": ("F32X3P", "F32X3P", "F32X3P"),
         "f32x3wo": ("F32X3WO", "F32X3P", "F32X3WA"), "f32x3wa": ("F32X3WA", "F32X3WO", "F32X3WA")}      # dtype of (proj, w1|w2, w3), as test_gpu_epilogue_tails.py
A_PLANES, O_PLANES = ("F32X3P", "F32X3WA"), ("F32X3P", "F32X3WO")
VSET = (16, 19, 63)
SPLIT_VARIANT = 2016
RATIOS = (1, 3, 10, 30, 100, 1000)
# family -> (mean, sigma, outlier in column 1, outlier in column n - 1, nominal |mean| / sigma of the envelope table or None)
FAMILIES = {"centred": (0.0, 1.0, 0.0, 0.0, 0)}
for _r in RATIOS:
    FAMILIES[f"mean+{_r}"] = (float(_r), 1.0, 0.0, 0.0, _r)
    FAMILIES[f"mean-{_r}"] = (-float(_r), 1.0, 0.0, 0.0, _r)
FAMILIES.update({"out100_first": (0.0, 1.0, 100.0, 0.0, None), "out1000_first": (0.0, 1.0, -1000.0, 0.0, None), "out100_last": (0.0, 1.0, 0.0, -100.0, None),
                 "out1000_last": (0.0, 1.0, 0.0, 1000.0, None), "out_both": (0.0, 1.0, 1000.0, -100.0, None), "small1e-2": (1.0, 1e-2, 0.0, 0.0, None),
                 "small1e-4": (1.0, 1e-4, 0.0, 0.0, None), "const0": (0.0, 0.0, 0.0, 0.0, None), "const3": (3.0, 0.0, 0.0, 0.0, None), "padonly": (0.0, 0.0, 0.0, 0.0, None)})
FAMILY_NAMES = tuple(FAMILIES)
OLD_FAMILIES = ("centred",)                           # what the inputs of the older tests held: |mean| / sigma <= 0.25
PAD_VALUE = 5.0
assert len(FAMILY_NAMES) == 23


def family_of(i):
    return FAMILY_NAMES[i % len(FAMILY_NAMES)]


def family_rows(name, m=M):
    return [i for i in range(m) if family_of(i) == name]


def slot_class(stage, slots):
    return "lt4" if slots < 4 else ("prefetch" if slots <= 4 * PRE[stage] else "remainder")


def widths(stage):
    return W12_WIDTHS if stage == "w12" else W3_WIDTHS


def shape_of(stage, slots):
    """-> dict(ln_n, K, N (GEMM columns), Hd, Hp (w12 only)) of a case."""
    if stage == "w12":
        C = W12_WIDTHS[slots]
        return dict(ln_n=C, K=E.ru(C, 64), N=2 * HP12, Hd=HD12, Hp=HP12, n_stat=C)
    Hd, Hp = W3_WIDTHS[slots]
    return dict(ln_n=Hd, K=E.ru(Hp, 64), N=N3, Hd=Hd, Hp=Hp, n_stat=Hp)


def dt_name(form, stage):
    return FORMS[form][1 if stage == "w12" else 2]


def kind_of(form):
    return "bf16" if form == "bf16" else "x3"


def path_of(form, stage, variant):
    """Which code path forms the row table for this launch: 'plain' | 'early' | 'phased' | 'refused' (module docstring)."""
    if variant == 63:
        return "phased" if form == "bf16" or dt_name(form, stage) in A_PLANES else "refused"
    if variant == 16:
        return "early" if form == "bf16" else "plain"
    return "plain"


def paths_of(form, stage):
    """The paths that exist for a form's launch of this stage."""
    return tuple(p for p in ("plain", "early", "phased") if any(path_of(form, stage, v) == p for v in VSET))


# ---- the designed rows --------------------------------------------------------------------------------------------------------------------------
def row_params(m=M):
    """[m, 4] f32: (mean, sigma, outlier of column 1, outlier of column n - 1) per row."""
    return torch.tensor([FAMILIES[family_of(i)][:4] for i in range(m)], dtype=torch.float32)


def designed_rows(n, seed, m=M):
    """[m, n] f32 rows of the families over n valid columns (one seeded randn pattern per row)."""
    p = row_params(m).double()
    g = torch.randn(m, n, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    x = p[:, 0:1] + p[:, 1:2] * g
    x[:, min(1, n - 1)] += p[:, 2]
    x[:, n - 1] += p[:, 3]
    return x.float()


def producer_operands(Hd, seed):
    """The hidden-unit rows of the families THROUGH the producing SwiGLU launch (K = 64): w1 = 0 and b1 = 4 make silu(z1) one constant, A row i = (mean, sigma, o_first,
    o_last, 0 ..) and w2 row u = (1, g_u, [u == 1], [u == Hd - 1], 0 ..), b2 = 0: h[i, u] = silu(4) (mean_i + sigma_i g_u + outliers).  -> (A [M, 64], w1, w2 [Hd, 64], b1, b2)."""
    A = torch.zeros(M, 64)
    A[:, :4] = row_params()
    w2 = torch.zeros(Hd, 64)
    w2[:, 0] = 1.0
    w2[:, 1] = torch.randn(Hd, generator=torch.Generator().manual_seed(seed))
    w2[min(1, Hd - 1), 2] = 1.0
    w2[Hd - 1, 3] = 1.0
    return A, torch.zeros(Hd, 64), w2, torch.full((Hd,), 4.0), torch.zeros(Hd)


def pad_rows():
    return family_rows("padonly")


# ---- the kernel's fixed trees ------------------------------------------------------------------------------------------------------------------------
def _f32(x):
    return x.to(torch.float32)


def slot_sums_tree(vals, width):
    """(sum, sum of squares) per 64-column slot of f32 vals[:, :width] in the producing epilogue's tree, in f32 arithmetic -> f32 [rows, slots, 2]."""
    rows = vals.shape[0]
    n = (width + 63) // 64
    v = torch.zeros(rows, n * 64, dtype=torch.float32)
    v[:, :width] = vals[:, :width].float()
    v = v.view(rows, n, 4, 4, 4)                       # slot, group of 16, lane of 4, value
    s, q = v[..., 0], _f32(v[..., 0].double() ** 2)
    for r in range(1, 4):
        s = s + v[..., r]
        q = _f32(v[..., r].double() ** 2 + q.double())      # fma: one rounding
    tree = lambda t: (t[..., 0] + t[..., 1]) + (t[..., 2] + t[..., 3])
    return torch.stack([tree(tree(s)), tree(tree(q))], -1)


def combine_f64(st, take=None):
    """ln_rows_prepare_fn's f64 combine of f32 slots st [rows, slots, 2]: part p adds slots p, p + 4, .. in sequence, (p0 + p1) + (p2 + p3).  take(p, sl) -> weight of a slot
    (the planted errors drop or repeat one)."""
    rows, n, _ = st.shape
    parts = []
    for p in range(4):
        acc = torch.zeros(rows, 2, dtype=torch.float64)
        for sl in range(p, n, 4):
            acc = acc + st[:, sl].double() * (1.0 if take is None else take(p, sl))
        parts.append(acc)
    return (parts[0] + parts[1]) + (parts[2] + parts[3])


# ---- host-side operands (the CPU tests; the GPU test reads the same fields back from the device) -------------------------------------------------------
def act_round(x32, form, planes):
    """f32 values -> (what the producer summed [f32], the values the consumer reads [f64], (hi, lo) of the bf16 x 3 products or None)."""
    if form == "bf16":
        r = x32.to(torch.bfloat16).float()
        return r, r.double(), None
    hi, lo = E.planes_split(x32)
    return x32, ((hi.double() + lo.double()) if planes else x32.double()), (hi, lo)


def pack_host(w, gamma, beta, b, K, form):
    """toc3d_pack_weight_lnfold / _swiglu_lnfold on the host: W' = round(gamma * w) [N, K] zero padded, c1 = f32 row sums of the ROUNDED W', c2 = beta . w + b; and the sums of the
    unrounded W' (a planted error)."""
    N, n = w.shape
    wp = torch.zeros(N, K)
    wp[:, :n] = gamma.float() * w.float()
    unrounded = wp.double().sum(1).float()
    if form == "bf16":
        wp = wp.to(torch.bfloat16).float()
    return wp, wp.double().sum(1).float(), (w.double() @ beta.double() + b.double()).float(), unrounded


def swiglu_pack_rows(w1, w2):
    """Interleave [Hp, *] w1 / w2 rows as toc3d_pack_swiglu: packed row 32 b + i = w1 row 16 b + i, 32 b + 16 + i = w2 row 16 b + i."""
    Hp = w1.shape[0]
    return torch.stack([w1.view(Hp // 16, 16, -1), w2.view(Hp // 16, 16, -1)], 1).reshape(2 * Hp, -1)


def stage_weights(stage, slots, seed=0):
    """Seeded state-dict weights of a case: (w [N, ln_n] in GEMM row order for w3; (w1, w2) [Hd, C] for w12), gamma, beta, biases, residual."""
    sh = shape_of(stage, slots)
    n = sh["ln_n"]
    rn = lambda *s, k: torch.randn(*s, generator=torch.Generator().manual_seed(1000 * slots + 10 * seed + k))
    gamma, beta = 1.0 + 0.3 * rn(n, k=1), 0.2 * rn(n, k=2)
    if stage == "w12":
        return dict(w1=rn(HD12, n, k=3) * n ** -0.5, w2=rn(HD12, n, k=4) * n ** -0.5, b1=rn(HD12, k=5), b2=rn(HD12, k=6), gamma=gamma, beta=beta)
    return dict(w=rn(N3, n, k=3) * n ** -0.5, b=rn(N3, k=5), gamma=gamma, beta=beta, res=rn(M, N3, k=7))


@functools.lru_cache(maxsize=4)
def host_case(form, stage, slots):
    """Every operand of a case as the kernels would hold it, built on the host -> the dict `analyse` and `emulate` take."""
    sh = shape_of(stage, slots)
    n, K = sh["ln_n"], sh["K"]
    planes = dt_name(form, stage) in A_PLANES
    x32 = designed_rows(n, seed=slots)
    if stage == "w3":
        x32 = (x32.double() * 3.928055160151634).float()       # silu(4): the scale the producing launch gives the hidden units
    summed, vals, split = act_round(x32, form, planes)
    a = torch.zeros(M, K, dtype=torch.float64)
    a[:, :n] = vals
    a[pad_rows(), n:] = PAD_VALUE
    sw = stage_weights(stage, slots)
    if stage == "w12":
        pad = lambda t: torch.cat([t, torch.zeros(HP12 - HD12, *t.shape[1:])])
        wp, c1, c2, c1u = pack_host(swiglu_pack_rows(pad(sw["w1"]), pad(sw["w2"])), sw["gamma"], sw["beta"], swiglu_pack_rows(pad(sw["b1"])[:, None], pad(sw["b2"])[:, None])[:, 0], K, form)
        res = None
    else:
        wp, c1, c2, c1u = pack_host(sw["w"], sw["gamma"], sw["beta"], sw["b"], K, form)
        res = sw["res"]
    return dict(form=form, stage=stage, slots=slots, a=a, a_planes=planes, stats=slot_sums_tree(summed, sh["n_stat"] if stage == "w12" else n), summed=summed,
                w=wp.double(), c1=c1, c2=c2, c1_unrounded=c1u, res=res, split=1, **sh)


# ---- reference and bound ---------------------------------------------------------------------------------------------------------------------------
def _grid_exponent(x):
    """q per element with x a multiple of 2^q (f64 tensor of f32-representable values; zeros: a large q)."""
    m, e = torch.frexp(x)
    mi = (m.abs() * 2.0 ** 24).to(torch.int64)
    low = torch.frexp((mi & -mi).double())[1] - 1
    return torch.where(x == 0, torch.full_like(e, 4096), e - 24 + low)


def _slot_errors(x, n, a_planes):
    """Per row: bounds on |dS1|, |dS2| of the producer's f32 slot sums of x [rows, n] (module docstring: 7 u / 8 u per slot, 0 where the slot is exact on its grid,
    + the (hi, lo) split of a planes consumer)."""
    rows = x.shape[0]
    ns = (n + 63) // 64
    v = torch.zeros(rows, ns * 64, dtype=torch.float64)
    v[:, :n] = x
    v = v.view(rows, ns, 64)
    sa, sq = v.abs().sum(2), (v * v).sum(2)
    if a_planes:
        return (sa * (7 * U + 2.0 ** -18)).sum(1), (sq * (8 * U + 2.0 ** -17 + 2.0 ** -36)).sum(1)
    q = _grid_exponent(v).min(2).values.double()
    exact1, exact2 = sa < 2.0 ** (q + 24).clamp(max=1000), sq < 2.0 ** (2 * q + 24).clamp(max=1000)
    return torch.where(exact1, 0.0, 7 * U * sa).sum(1), torch.where(exact2, 0.0, 8 * U * sq).sum(1)


def e_kind(kind, K, split=1):
    return (2 * U * K if kind == "bf16" else 2.0 ** -16 + 2 * U * 3 * K) + (2 * U * split if split > 1 else 0.0)


def silu64(z):
    return z * torch.sigmoid(z)


def analyse(c, eps=EPS):
    """A case dict -> dict(ref, bound, ...) of every output of the stage: 'hid' [M, Hp] (w12) or 'out', 'raw' [M, N] (w3), all f64; plus per-row cond / rstd."""
    a, w, n, K = c["a"], c["w"], c["ln_n"], c["K"]
    kind = kind_of(c["form"])
    x = a[:, :n]
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    c1, c2 = c["c1"].double(), c["c2"].double()
    z = E.explicit_ln_matmul(a, w, c2, n, eps)
    # statistics
    d1, d2 = _slot_errors(x, n, c["a_planes"])
    m2 = (x * x).mean(1, keepdim=True)
    dmean = d1[:, None] / n + (U + 1e-14) * mean.abs()
    dvar = d2[:, None] / n + (U + 1e-14) * m2 + 2 * mean.abs() * dmean + dmean ** 2 + U * var
    r_hi, r_lo = (1 + 5 * U) / torch.sqrt((var - dvar).clamp_min(0.0) + eps), (1 - 5 * U) / torch.sqrt(var + dvar + eps)
    drstd = torch.maximum(r_hi - rstd, rstd - r_lo)
    t_stat = drstd / rstd * (z - c2).abs()
    # cancellation
    absdot = a.abs() @ w.abs().T
    e_c1 = (math.ceil(K / 256) + 8) * U
    t_cancel = (rstd + drstd) * (e_kind(kind, K, c["split"]) * absdot + (dmean + 2 * U * mean.abs()) * c1.abs() + mean.abs() * e_c1 * w.abs().sum(1))
    bz = t_stat + t_cancel + U * (2 * (z - c2).abs() + z.abs())
    out = dict(mean=mean[:, 0], var=var[:, 0], rstd=rstd[:, 0], cond=((mean ** 2 + var) / (var + eps))[:, 0], z=z, bz=bz, t_stat=t_stat, t_cancel=t_cancel)
    if c["stage"] == "w3":
        res = c["res"].double()
        out.update(raw=z, b_raw=bz, out=res + z, b_out=bz + U * ((res + z).abs() + bz))
        return out
    Hd, Hp = c["Hd"], c["Hp"]
    zz, bb = z.view(M, Hp // 16, 2, 16), bz.view(M, Hp // 16, 2, 16)
    z1, z2, b1, b2 = (t.reshape(M, Hp) for t in (zz[:, :, 0], zz[:, :, 1], bb[:, :, 0], bb[:, :, 1]))
    sg = torch.sigmoid(z1)
    s, ds = z1 * sg, sg * (1 + z1 * (1 - sg))
    h = s * z2
    bh = (ds.abs() * b1 + 0.25 * b1 * b1) * (z2.abs() + b2) + s.abs() * b2
    bh = bh + (z1.abs() + 8) * U * (h.abs() + bh)
    r_out = 2.0 ** -8 if kind == "bf16" else (2.0 ** -16 if dt_name(c["form"], "w12") in O_PLANES else U)
    bh = bh + r_out * (h.abs() + bh)
    h[:, Hd:], bh[:, Hd:] = 0.0, 0.0
    out.update(hid=h, b_hid=bh)
    return out


def outputs_of(stage):
    return ("hid",) if stage == "w12" else ("out", "raw")


def ratios(got, an, key):
    """|got - ref| / bound per element (0 / 0 = 0: an element bounded by 0 must be met exactly, else inf)."""
    err, b = (got.double() - an[key]).abs(), an["b_" + key]
    r = err / b
    r[(err == 0) & (b == 0)] = 0.0
    r[torch.isnan(got.double())] = float("inf")
    return r


def bar_of(form, key):
    """The bar the suite already holds this output class to (epilogue_cases): of the ROW's own largest |ref| in the envelope table."""
    return E.TOL_BF16 if (form == "bf16" and key == "hid") else E.TOL_F32


def worst_by_family(r):
    """ratio tensor [M, *] -> {family: worst}."""
    return {f: float(r[family_rows(f)].max()) for f in FAMILY_NAMES}


def envelope(pass_by_ratio):
    """{nominal ratio: all elements met the bar} -> the largest ratio up to which every family passes (None: not even the centred rows)."""
    best = None
    for r in (0,) + RATIOS:
        if not pass_by_ratio.get(r, False):
            break
        best = r
    return best


# ---- emulation of the kernels' sequence in f32 (and the planted errors) ---------------------------------------------------------------------------------------
MUTANTS = ("ln_n_is_K", "var_n_minus_1", "eps_1e-5", "mean_bf16", "c1_unrounded", "last_slot_dropped", "slot_4PRE_dropped", "slot0_twice", "no_clamp", "row_M-1_for_M-2")


def _products(c):
    """a . w^T in the form's arithmetic, one f32 rounding per 32-deep K step (bf16: exact products; bf16 x 3: hi.hi, hi.lo, lo.hi as three steps)."""
    a, w, K = c["a"], c["w"], c["K"]
    if kind_of(c["form"]) == "bf16":
        terms = [(a, w)]
    else:
        ah, al = E.planes_split(a.float())
        wh, wl = E.planes_split(w.float())
        terms = [(ah.double(), wh.double()), (ah.double(), wl.double()), (al.double(), wh.double())]
    acc = torch.zeros(a.shape[0], w.shape[0], dtype=torch.float32)
    for k in range(0, K, 32):
        for ta, tw in terms:
            acc = _f32(acc.double() + ta[:, k:k + 32] @ tw[:, k:k + 32].T)
    return acc


def emulate(c, mut=None, eps=EPS, acc=None):
    """The outputs of the stage as the kernels form them, in f32 -> dict like `analyse` ('hid' | 'out', 'raw').  mut: one of MUTANTS.  acc: the products, when the caller has
    them already (they do not depend on mut)."""
    n, K, st = c["ln_n"], c["K"], c["stats"]
    ns = st.shape[1]
    pre4 = 4 * PRE[c["stage"]]
    take = None
    if mut == "last_slot_dropped":
        take = lambda p, sl: 0.0 if sl == ns - 1 else 1.0
    elif mut == "slot_4PRE_dropped":
        take = lambda p, sl: 0.0 if sl == pre4 else 1.0
    elif mut == "slot0_twice":                          # a part that lies past the row adds the clamped slot 0
        take = lambda p, sl: 1.0
    S = combine_f64(st, take)
    if mut == "slot0_twice" and ns < 4:
        S = S + st[:, 0].double() * (4 - ns)
    inv = float(torch.tensor(1.0 / (K if mut == "ln_n_is_K" else n), dtype=torch.float32))
    mean = S[:, 0] * inv
    var = S[:, 1] * (1.0 / (n - 1) if mut == "var_n_minus_1" else inv) - mean * mean * (n / (n - 1) if mut == "var_n_minus_1" else 1.0)
    if mut != "no_clamp":
        var = var.clamp_min(0.0)
    mu = mean.float()
    if mut == "mean_bf16":
        mu = mu.to(torch.bfloat16).float()
    rs = 1.0 / torch.sqrt(var.float() + torch.tensor(1e-5 if mut == "eps_1e-5" else eps, dtype=torch.float32))
    if mut == "row_M-1_for_M-2":
        mu, rs = mu.clone(), rs.clone()
        mu[M - 2], rs[M - 2] = mu[M - 1], rs[M - 1]
    c1 = c["c1_unrounded"] if mut == "c1_unrounded" else c["c1"]
    acc = _products(c) if acc is None else acc
    z = rs[:, None] * (acc - mu[:, None] * c1.float()) + c["c2"].float()
    if c["stage"] == "w3":
        return dict(raw=z, out=c["res"].float() + z)
    Hd, Hp = c["Hd"], c["Hp"]
    zz = z.view(M, Hp // 16, 2, 16)
    h = (torch.nn.functional.silu(zz[:, :, 0]) * zz[:, :, 1]).reshape(M, Hp)
    h[:, Hd:] = 0.0
    if kind_of(c["form"]) == "bf16":
        h = h.to(torch.bfloat16).float()
    elif dt_name(c["form"], "w12") in O_PLANES:
        hi, lo = E.planes_split(h)
        h = hi + lo
    return dict(hid=h)


def folded_f64(c, eps=EPS):
    """The folded formula in f64 on exact f64 sums, with c1 = the exact row sums of the packed W': the wrong reference that must be indistinguishable from the two-pass one."""
    z = E.folded_ln_matmul(c["a"], c["w"], c["w"][:, :c["ln_n"]].sum(1), c["c2"], c["ln_n"], eps)
    if c["stage"] == "w3":
        return dict(raw=z, out=c["res"].double() + z)
    h = E.swiglu_units(z, c["Hd"], c["Hp"])
    return dict(hid=h)
