"""The row kernels of the head's token side and of the memory bank -- toc3d_head_frustum_inputs (csrc/frustum_point.h), toc3d_mln_apply, toc3d_se_gate
(csrc/head_tokens.hip), toc3d_memory_scores, toc3d_memory_pre_update, toc3d_memory_post_update (csrc/memory.hip) -- as f64 references with per-element bounds,
the case lists, and f32 emulations that spell each kernel's operation sequence with one numpy / torch f32 operation per rounding.  Shared by
test_cpu_head_rows_cases.py (emulations through the bounds, planted errors; no GPU) and test_gpu_head_row_kernels.py (the kernels through the C ABI).
Importing this needs no GPU, and nothing here imports from a ``test_*`` module.  u = 2^-24; every bound is per element.

Frustum.  The f64 value comes from the f32 img2lidar, coords_d and position_range the kernel is handed and the integers.  The pixel centre is x stride +
stride / 2 exactly (an integer); the kernel's (c / pad) pad is two roundings of it.  For coordinate i the terms are t = (M_i0 cx sc, M_i1 cy sc, M_i2 dep, M_i3), sc =
max(dep, 1e-5f), s = sum t, p = (s - lo_i) / (hi_i - lo_i).  In f32 the first two terms carry four roundings (the two of the centre, centre x sc, M x that), the
third one, the fourth none; the three additions put at most three more on each: 7 u sum |t| to first order, 8 u with the second order.  The subtraction is one
rounding of s - lo; the span, the division and the second order give 3 u |p|:

    dp = (8 u sum |t| + u |s - lo|) / |hi - lo| + 3 u |p|.

pos_in is mmdet's inverse_sigmoid of p, which has four kinks (the clamps to [0, 1] and the two 1e-5 floors) and is monotone non-decreasing, so it is not
linearised: inv64(p - dp) - e <= got <= inv64(p + dp) + e with e = 4 u (1 + |value|) for 1 - x, the division and logf.  Where the whole interval [p - dp, p + dp]
lies at or below 0 (at or above 1) the output is one constant, logf(1e-5f / 1.f) (logf(1.f / 1e-5f)): every such element carries the same bits, and those lie
within e of the f64 logarithm of the f32 quotient (they are part of the band check like every other element).  WHICH f32 a libm returns there is its own business --
the true values lie 0.36 and 0.33 of an ulp from the nearest f32; numpy returns that one at both arguments, the MI355X's logf returns -11.512927055 at 1e-5f, two
f32 steps below it (1.64 ulp off, 0.525 of e), and the nearest at 1.f / 1e-5f --, so the tests do not spell the constant: they take it from a launch of the same case under a position range a million
metres away (FAR_BELOW, FAR_ABOVE: every p near -1 or near 2), whose whole pos_in must be that one pattern, and require the clamped elements of the narrow ranges
to carry it.

How small an error of p the frustum bound catches (test_cpu_head_rows_cases.py::test_frustum_smallest_shift_caught measures it on the f32 emulation, over every
frustum case, on the 5393 interior elements 0.01 < p < 0.99 of cone's columns 2..7): dp is between 2.0 and 254.5 ulps of p (the large ones where p is small against
sum |t| / span).  Shifting EVERY such p by 1 ulp, up or down, leaves all of them inside dp; at 2 ulps the first is outside; at 289 ulps every single one is.  The
unshifted emulation sits at <= 0.44 of dp (0.33 of the pos_in band), the device at <= 0.43 of dp on cone and 0.35 of the band on the unclamped pos_in.

MLN (toc3d_mln_apply).  Two-pass statistics over the E columns of a row: focal_head_cases.stats_bounds with n = E gives dm = E u mean|x| on the mean and (E + 10) u
+ dm^2 / (var + eps) on rstd^-2, so rho = half of that on rstd.  a = (x - m) rstd: da = (dm + u |x - m|) rstd + |a| (rho + u); out = gamma a + beta: do = |gamma| da
+ 2 u (|gamma a| + |beta|).  The bound holds for any order of the additions; the CPU file runs the kernel's (lane-strided partial sums, then the butterfly) and a
plain sequential one.

Sigmoids (toc3d_se_gate, toc3d_memory_scores).  s = 1 / (1 + expf(-z)): 8 u s + 2^-126; the floor covers results that are f32 subnormals or flushed to zero (expf
overflows to inf beyond 88.72 and the quotient is 0).  The gate pos s adds the product's own rounding, u |out|, which gets the same floor for the same reason.  The
maximum over the classes is 1-Lipschitz: the score's bound is the largest class bound of its row.

Memory.  emb, vel and ts are copies, products with 0 or 1 and one f64 add or subtract: exact against the same operation on the host.  A 4x4 product or a transformed
point is a dot4 (four products, three additions, in k order): 5 u sum |a| |b|.  The propagated slots of pre_update add nx (pseudo (hi - lo) + lo) with nx = 1 - x in
{0, 1}: 4 u (|ref| + |ps|) for the addition and the affine map's last addition, and 2 u |pseudo (hi - lo)| for the span and the product, whose roundings scale with
the product and not with ps = product + lo, which cancels where the pseudo point sits mid-range (the f32 emulation exceeds 4 u (|ref| + |ps|) alone there: see
test_cpu_head_rows_cases.py::test_memory_emulations_inside_the_bounds)."""
import math

import numpy as np
import torch

import focal_head_cases as FC
from toc3d_amd import synth

U = FC.U
F = np.float32
FLOOR = 2.0 ** -126
IS_EPS = float(F(1e-5))                                    # the kernel's 1e-5f, as the f64 it is
MLN_EPS = float(F(1e-5))
SHIPPED_RANGE = (-61.2, -61.2, -10.0, 61.2, 61.2, 10.0)
NARROW_A = (-20.0, -20.0, -2.0, 20.0, 20.0, 2.0)
NARROW_B = (-15.5, -30.0, -1.5, 25.0, 30.0, 1.0)
FAR_BELOW = (1e6, 1e6, 1e6, 2e6, 2e6, 2e6)                 # every p near -1: all of pos_in is logf(1e-5f / 1.f)
FAR_ABOVE = (-2e6, -2e6, -2e6, -1e6, -1e6, -1e6)           # every p near 2: all of pos_in is logf(1.f / 1e-5f)


# ---- frustum ------------------------------------------------------------------------------------------------------------------------------------------------------
# (name, (B, N, h, w), D, position_range, seed, options).  20 plain cases; then pad_h > 16 h, a non-LID coords_d, bin 0 = 0.0 at D = 30 (where bin 0 is also bin
# D - 30, so the floored depth reaches cone), and the two narrow ranges on which the clamps of inverse_sigmoid run.
FRUSTUM_SHAPES = ((1, 1, 1, 1), (1, 1, 1, 5), (2, 2, 2, 3), (1, 3, 3, 7), (1, 2, 5, 9))
FRUSTUM_D = (30, 33, 64, 65)
FRUSTUM_CASES = [(f"{'x'.join(map(str, s))} D={D}", s, D, SHIPPED_RANGE, sum(s) + D, {}) for s in FRUSTUM_SHAPES for D in FRUSTUM_D] + [
    ("1x2x5x9 D=64 pad_h+32", (1, 2, 5, 9), 64, SHIPPED_RANGE, 11, dict(pad_h_extra=32)),
    ("2x2x2x3 D=33 uniform bins", (2, 2, 2, 3), 33, SHIPPED_RANGE, 12, dict(lid=False)),
    ("1x3x3x7 D=30 bin0=0", (1, 3, 3, 7), 30, SHIPPED_RANGE, 13, dict(zero_bin=True)),
    ("2x2x2x3 D=64 narrow A", (2, 2, 2, 3), 64, NARROW_A, 24, {}),
    ("1x3x3x7 D=33 narrow B bin0=0", (1, 3, 3, 7), 33, NARROW_B, 3, dict(zero_bin=True)),
]
FRUSTUM_CLAMP_CASES = ("2x2x2x3 D=64 narrow A", "1x3x3x7 D=33 narrow B bin0=0")
FRUSTUM_BY_NAME = {c[0]: c for c in FRUSTUM_CASES}


def coords_d(D, far, lid=True, depth_start=1.0):
    """HeadTokenEmbedding's depth bins (streampetr_head.py:221-232), f32."""
    index = torch.arange(0, D, 1).float()
    if lid:
        return depth_start + (far - depth_start) / (D * (1 + D)) * index * (index + 1)
    return depth_start + (far - depth_start) / D * index


def frustum_inputs(shape, D, prange, seed, lid=True, zero_bin=False, pad_h_extra=0, stride=16):
    B, N, h, w = shape
    inp = synth.head_tokens_inputs(dict(in_channels=1, stride=stride), B, N, h, w, seed=seed)
    pr = torch.tensor([float(v) for v in prange], dtype=torch.float32)
    cd = coords_d(D, SHIPPED_RANGE[3], lid).float().contiguous()        # the bins stay the shipped ones: a narrow range then leaves points outside it
    if zero_bin:
        cd[0] = 0.0
    return dict(i2l=torch.linalg.inv(inp["lidar2img"].reshape(B * N, 4, 4)).contiguous(), intr=inp["intrinsics"].reshape(B * N, 4, 4).contiguous(), cd=cd, pr=pr,
                B=B, N=N, h=h, w=w, D=D, stride=stride, pad_h=h * stride + pad_h_extra, pad_w=w * stride)


def frustum_case(name):
    _, shape, D, prange, seed, opt = FRUSTUM_BY_NAME[name]
    return frustum_inputs(shape, D, prange, seed, **opt)


def with_range(a, prange):
    """The same case under another position_range."""
    return dict(a, pr=torch.tensor([float(v) for v in prange], dtype=torch.float32))


def distinct_bits(t):
    """The distinct f32 bit patterns of a numpy / torch f32 array, sorted."""
    return sorted(set(torch.as_tensor(t).contiguous().view(torch.int32).flatten().tolist()))


def _token_index(a):
    hw = a["h"] * a["w"]
    tok = torch.arange(a["B"] * a["N"] * hw)
    pix, view = tok % hw, tok // hw
    tok_in_b = tok - (view // a["N"]) * a["N"] * hw
    return tok, pix % a["w"], pix // a["w"], view, tok_in_b


def inv_sigmoid64(p):
    x = p.clamp(0.0, 1.0)
    return torch.log(x.clamp_min(IS_EPS) / (1.0 - x).clamp_min(IS_EPS))


def frustum_reference(a):
    """-> dict: p, dp f64 [M, D, 3]; cone, dcone f64 [M, 8]."""
    D, st = a["D"], a["stride"]
    _, x, y, view, tok_in_b = _token_index(a)
    cx, cy = (x * st + st // 2).double()[:, None, None], (y * st + st // 2).double()[:, None, None]
    dep = a["cd"].double()[None, None, :]
    sc = dep.clamp_min(IS_EPS)
    Mv = a["i2l"].double()[view][:, :3]                                          # [M, 3, 4]
    t = torch.stack([Mv[:, :, 0:1] * cx * sc, Mv[:, :, 1:2] * cy * sc, Mv[:, :, 2:3] * dep, Mv[:, :, 3:4].expand(-1, -1, D)], -1)         # [M, 3, D, 4]
    s = t.sum(-1)
    pr = a["pr"].double()
    lo, span = pr[:3][None, :, None], (pr[3:] - pr[:3])[None, :, None]
    p = (s - lo) / span
    dp = (8 * U * t.abs().sum(-1) + U * (s - lo).abs()) / span.abs() + 3 * U * p.abs()
    p, dp = p.permute(0, 2, 1).contiguous(), dp.permute(0, 2, 1).contiguous()     # [M, D, 3]
    cam = (view // a["N"]) * a["N"] + tok_in_b % a["N"]                          # the reference's repeat order (streampetr_head.py:384-386)
    K = a["intr"].double()[cam]
    f = torch.stack([K[:, 0, 0].abs() / 1e3, K[:, 1, 1].abs() / 1e3], 1)
    cone = torch.cat([f, p[:, D - 1], p[:, D - 30]], 1)
    dcone = torch.cat([U * f, dp[:, D - 1], dp[:, D - 30]], 1)
    return dict(p=p, dp=dp, cone=cone, dcone=dcone)


def pos_in_band(p, dp):
    """-> (centre, lower, upper, mask of the elements pinned to logf(1e-5f / 1.f), mask of those pinned to logf(1.f / 1e-5f)), each [M, 3 D]."""
    e = lambda v: 4 * U * (1.0 + v.abs())
    c, lo, hi = inv_sigmoid64(p), inv_sigmoid64(p - dp), inv_sigmoid64(p + dp)
    f = lambda t: t.flatten(1)
    return f(c), f(lo - e(lo)), f(hi + e(hi)), f(p + dp <= 0.0), f(p - dp >= 1.0)


def band_ratio(got, c, lo, hi):
    """Distance from the centre over the half-width on that side; <= 1 exactly where lo <= got <= hi."""
    got = got.double()
    return torch.where(got >= c, (got - c) / (hi - c), (c - got) / (c - lo))


def clamp_shares(p):
    n = p.numel()
    return float((p <= 0.0).sum()) / n, float((p >= 1.0).sum()) / n, float(((p > 0.0) & (p < 1.0)).sum()) / n


def inverse_sigmoid_f32(p):
    """act_rows.h inverse_sigmoid on a numpy f32 array, one operation per rounding."""
    x = np.minimum(np.maximum(p, F(0)), F(1))
    return np.log(np.maximum(x, F(1e-5)) / np.maximum(F(1) - x, F(1e-5)))


def emulate_frustum(a, drop_half=False, cone_bin=30, camera_is_view=False):
    """frustum_point's f32 operation sequence -> (p [M, D, 3], pos_in [M, 3 D], cone [M, 8]) as numpy f32.  The keywords plant errors: the pixel corner for its
    centre, bin D - cone_bin for bin D - 30, the view's own intrinsics for camera (token % N)."""
    D, st, N = a["D"], a["stride"], a["N"]
    _, x, y, view, tok_in_b = _token_index(a)
    half = 0 if drop_half else st // 2
    pw, ph = F(a["pad_w"]), F(a["pad_h"])
    cx = ((x.numpy() * st + half).astype(F) / pw) * pw
    cy = ((y.numpy() * st + half).astype(F) / ph) * ph
    dep = a["cd"].numpy().astype(F)
    sc = np.maximum(dep, F(1e-5))
    c0, c1 = cx[:, None] * sc[None, :], cy[:, None] * sc[None, :]                # [M, D]
    Mv = a["i2l"].numpy().astype(F)[view.numpy()]                                # [M, 4, 4]
    pr = a["pr"].numpy().astype(F)
    p = np.empty((len(cx), D, 3), dtype=F)
    for i in range(3):
        s = Mv[:, i, 0:1] * c0
        s = s + Mv[:, i, 1:2] * c1
        s = s + Mv[:, i, 2:3] * dep[None, :]
        s = s + Mv[:, i, 3:4]
        p[:, :, i] = (s - pr[i]) / (pr[3 + i] - pr[i])
    assert p.dtype == F and c0.dtype == F
    cam = view if camera_is_view else (view // N) * N + tok_in_b % N
    K = a["intr"].numpy().astype(F)[cam.numpy()]
    cone = np.concatenate([(np.abs(K[:, 0, 0]) / F(1e3))[:, None], (np.abs(K[:, 1, 1]) / F(1e3))[:, None], p[:, D - 1], p[:, D - cone_bin]], 1)
    return p, inverse_sigmoid_f32(p).reshape(len(cx), 3 * D), cone


def frustum_ratios(ref, pos_in, cone):
    """numpy / torch f32 outputs -> (worst pos_in ratio, worst cone ratio of columns 0..1, of 2..4, of 5..7, the distinct values among the elements pinned to
    logf(1e-5f / 1.f), those among the elements pinned to logf(1.f / 1e-5f)): each of the last two must hold one value (none where nothing is pinned)."""
    c, lo, hi, pin_lo, pin_hi = pos_in_band(ref["p"], ref["dp"])
    got = torch.as_tensor(pos_in)
    r_pos = float(band_ratio(got, c, lo, hi).max())
    rc = (torch.as_tensor(cone).double() - ref["cone"]).abs() / ref["dcone"]
    return r_pos, float(rc[:, :2].max()), float(rc[:, 2:5].max()), float(rc[:, 5:].max()), distinct_bits(got[pin_lo]), distinct_bits(got[pin_hi])


def bits_to_f32(b):
    return float(np.array([b], dtype=np.int32).view(F)[0])


def shift_ulps(v, k):
    """A numpy f32 array moved k ulps away from zero (k >= 0) or towards it (k < 0): the ordering of positive floats is that of their bit patterns."""
    return (v.view(np.int32) + np.int32(k)).view(F)


# ---- MLN ----------------------------------------------------------------------------------------------------------------------------------------------------------
MLN_E = (1, 63, 64, 65, 100, 1000, 1024)       # below, at and past one wavefront; a lane tail; 1024 = all 16 registers of every lane
MLN_M = (1, 5, 7)                              # four rows per workgroup: a partly filled last one
MLN_PROFILES = ("ordinary", "shift 100", "shift 1e4", "spread 1e-3")
MLN_CONSTANT_E = (64, 1024)


def mln_inputs(M, E, profile, seed=0):
    """-> (x, gamma, beta) f32 [M, E].  "constant": every row one value of at most 13 significant bits, so every partial sum of its E copies is exact."""
    g = torch.Generator().manual_seed(23000 + 97 * seed + 7 * E + M)
    r = torch.randn(M, E, generator=g)
    spread = 0.5 + 1.5 * torch.rand(M, 1, generator=g)
    if profile == "ordinary":
        x = 3.0 * r + 0.5
    elif profile == "shift 100":
        x = (r + 100.0) * spread
    elif profile == "shift 1e4":
        x = (r + 1.0e4) * spread
    elif profile == "spread 1e-3":
        x = 1.0e-3 * r
    elif profile == "constant":
        x = (torch.round(r[:, :1] * 8.0 * 256.0) / 256.0 + 0.5).expand(M, E)
    else:
        raise KeyError(profile)
    gamma, beta = 1.0 + 0.3 * torch.randn(M, E, generator=g), torch.randn(M, E, generator=g)
    return x.float().contiguous(), gamma.float().contiguous(), beta.float().contiguous()


def mln_reference(x, gamma, beta):
    """f64 out [M, E] and its bound, from the f32 inputs."""
    M, E = x.shape
    x64, g64, b64 = x.double(), gamma.double(), beta.double()
    mean, var, dm, b_var = FC.stats_bounds(x64.view(M, 1, 1, E), E, 1, eps=MLN_EPS)      # one group of E terms per row: [M, 1]
    rho = 0.5 * b_var
    rstd = (var + MLN_EPS) ** -0.5
    a = (x64 - mean) * rstd
    da = (dm + U * (x64 - mean).abs()) * rstd + a.abs() * (rho + U)
    return g64 * a + b64, g64.abs() * da + 2 * U * ((g64 * a).abs() + b64.abs())


def _wave_sum_f32(v):
    """[M, 16, 64] f32 (register i, lane l holds column l + 64 i; zeros past E) -> [M]: each lane adds its registers in order from 0.f, then wave_sum's butterfly
    (lanes l and l ^ 32, ^ 16, ^ 8, ^ 4, ^ 2, ^ 1)."""
    s = np.zeros((v.shape[0], 64), dtype=F)
    for i in range(16):
        s = s + v[:, i]
    for half in (32, 16, 8, 4, 2, 1):
        s = s[:, :half] + s[:, half:2 * half]
    return s[:, 0]


def _seq_sum_f32(v):
    s = np.zeros(v.shape[0], dtype=F)
    for c in range(v.shape[1]):
        s = s + v[:, c]
    return s


def emulate_mln(x, gamma, beta, order="lanes", var_div=None, eps=1e-5, drop_col=None):
    """mln_kernel in numpy f32.  order: "lanes" (the kernel's) or "sequential".  Planted errors: var_div (divisor of the squares' sum, E by default), eps, drop_col
    (a column left out of the first sum)."""
    x, gamma, beta = (t.numpy().astype(F) for t in (x, gamma, beta))
    M, E = x.shape

    def total(v):
        if order == "sequential":
            return _seq_sum_f32(v)
        pad = np.zeros((M, 1024), dtype=F)
        pad[:, :E] = v
        return _wave_sum_f32(pad.reshape(M, 16, 64))
    first = x.copy()
    if drop_col is not None:
        first[:, drop_col] = 0
    mean = (total(first) / F(E))[:, None]
    dlt = x - mean
    rstd = (F(1) / np.sqrt(total(dlt * dlt) / F(E if var_div is None else var_div) + F(eps)))[:, None]
    out = gamma * ((x - mean) * rstd) + beta
    assert out.dtype == F
    return out


# ---- sigmoids ------------------------------------------------------------------------------------------------------------------------------------------------------
SPECIAL_LOGITS = (0.0, 1e-3, -1e-3, 88.7, -88.7, 89.0, -89.0, 104.0, -104.0, 120.0, -120.0)
SIGMOID_N = (1, 255, 256, 257)
GATE_N = SIGMOID_N + (4099,)
SCORE_CLASSES = (1, 3, 10)


def logits(n, seed=0, special=None):
    """f32 [n]: random logits up to about +-12 with SPECIAL_LOGITS planted from the last element backwards (``special``: that one value in the last element)."""
    z = 4.0 * torch.randn(n, generator=torch.Generator().manual_seed(29000 + seed))
    plant = SPECIAL_LOGITS if special is None else (special,)
    for i, v in enumerate(plant[:n]):
        z[n - 1 - i] = v
    return z.float().contiguous()


def sigmoid_reference(z):
    s = torch.sigmoid(z.double())
    return s, 8 * U * s + FLOOR


def gate_reference(pos, se):
    s, ds = sigmoid_reference(se)
    out = pos.double() * s
    return out, pos.double().abs() * ds + U * out.abs() + FLOOR


def score_reference(cls):
    """cls f32 [rows, classes] -> (score, bound)."""
    s, ds = sigmoid_reference(cls)
    return s.max(1).values, ds.max(1).values


def emulate_sigmoid(z):
    z = z.numpy().astype(F)
    with np.errstate(over="ignore"):
        return F(1) / (F(1) + np.exp(-z))


# ---- memory --------------------------------------------------------------------------------------------------------------------------------------------------------
MEM_B, MEM_PREV = 3, (1.0, 0.0, 1.0)
MEM_LEN = (1, 5, 48)
MEM_D = (1, 32, 100, 256)
MEM_TOPK_Q = {1: (1, 2, 70), 16: (16, 17, 70)}
MEM_LD_BBOX = (5, 8, 10)
PC_RANGE = (-51.2, -51.2, -5.0, 51.2, 51.2, 3.0)


def rigid_poses(n, seed):
    """f32 [n, 4, 4]: a rotation about all three axes, every angle in [-pi, pi), and a translation of up to 40 m per axis."""
    g = torch.Generator().manual_seed(31000 + seed)
    ang = (torch.rand(n, 3, generator=g, dtype=torch.float64) * 2 - 1) * math.pi
    c, s = ang.cos(), ang.sin()
    one, zero = torch.ones(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    m = lambda *v: torch.stack(v, 1).view(n, 3, 3)
    Rz = m(c[:, 0], -s[:, 0], zero, s[:, 0], c[:, 0], zero, zero, zero, one)
    Ry = m(c[:, 1], zero, s[:, 1], zero, one, zero, -s[:, 1], zero, c[:, 1])
    Rx = m(one, zero, zero, zero, c[:, 2], -s[:, 2], zero, s[:, 2], c[:, 2])
    T = torch.eye(4, dtype=torch.float64).repeat(n, 1, 1)
    T[:, :3, :3] = Rz @ Ry @ Rx
    T[:, :3, 3] = (torch.rand(n, 3, generator=g, dtype=torch.float64) * 2 - 1) * 40.0
    return T


def memory_bank(B, cap, L, D, seed, zero=False):
    """A bank [B, cap, ...] whose slots [0, L) hold data (zeros: a fresh bank); the caller fills the others with its guard."""
    g = torch.Generator().manual_seed(33000 + seed)
    bank = dict(emb=torch.zeros(B, cap, D), ref=torch.zeros(B, cap, 3), ts=torch.zeros(B, cap, dtype=torch.float64), pose=torch.zeros(B, cap, 16), vel=torch.zeros(B, cap, 2))
    if not zero:
        bank["emb"][:, :L] = torch.randn(B, L, D, generator=g)
        bank["ref"][:, :L] = torch.randn(B, L, 3, generator=g) * torch.tensor([25.0, 25.0, 2.0])
        bank["ts"][:, :L] = -1.5e9 - 3.0 * torch.rand(B, L, generator=g, dtype=torch.float64)
        bank["pose"][:, :L] = rigid_poses(B * L, seed + 1).float().view(B, L, 16)
        bank["vel"][:, :L] = torch.randn(B, L, 2, generator=g) * 3.0
    return bank


def frame_data(B, seed):
    """prev_exists, f64 epoch timestamps, ego pose and its inverse (the inverse formed in f64), and the f32 pc_range."""
    pose = rigid_poses(B, 500 + seed)
    ts = torch.tensor([1.5e9 + 0.5 * seed + 7.0 * b + 0.123456789 for b in range(B)], dtype=torch.float64)
    return dict(prev=torch.tensor(MEM_PREV[:B]), ts=ts, ego=pose.float().contiguous(), ego_inv=torch.linalg.inv(pose).float().contiguous(),
                pc=torch.tensor(PC_RANGE, dtype=torch.float32))


def _dot4_ref(A, Bm):
    """f64 [.., 4, 4] x [.., 4, n] -> (product, 5 u sum |a| |b|)."""
    return A @ Bm, 5 * U * (A.abs() @ Bm.abs())


def _homog(r):
    return torch.cat([r, torch.ones_like(r[..., :1])], -1)[..., None]


def pre_update_reference(bank, data, pseudo, L, num_propagated, fresh):
    """-> (exact: dict of emb / vel / ts as the host computes them; approx: dict of pose / ref -> (f64 value, bound)), all on slots [0, L)."""
    x = data["prev"]
    x64 = x.double()
    emb, vel, ts = bank["emb"][:, :L].clone(), bank["vel"][:, :L].clone(), bank["ts"][:, :L].clone()
    B = emb.shape[0]
    pose, ref = bank["pose"][:, :L].double().view(B, L, 4, 4), bank["ref"][:, :L].double()
    bp, br = torch.zeros_like(pose), torch.zeros_like(ref)
    if not fresh:
        emb, vel = emb * x[:, None, None], vel * x[:, None, None]
        ts = (ts + data["ts"][:, None]) * x64[:, None]
        P = data["ego_inv"].double()[:, None]
        pose, bp = _dot4_ref(P, pose)
        ref, br = _dot4_ref(P[:, :, :3], _homog(ref))
        ref, br = ref[..., 0], br[..., 0]
        pose, bp, ref, br = (t * x64.view(B, *([1] * (t.dim() - 1))) for t in (pose, bp, ref, br))
    if num_propagated:
        n = num_propagated
        nx = (1.0 - x64)[:, None, None]
        pc = data["pc"].double()
        prod = pseudo.double()[:n] * (pc[3:] - pc[:3])
        ps = (prod + pc[:3])[None]
        br = br.clone()
        br[:, :n] += (4 * U * (ref[:, :n].abs() + ps.abs()) + 2 * U * prod.abs()[None]) * nx
        ref = ref.clone()
        ref[:, :n] += nx * ps
        pose = pose.clone()
        for i in range(4):
            pose[:, :n, i, i] += nx[:, :, 0]
    return dict(emb=emb, vel=vel, ts=ts), dict(pose=(pose.reshape(B, L, 16), bp.reshape(B, L, 16)), ref=(ref, br))


def _dot4_f32(a, b):
    """numpy f32 [..., 4] rows against [..., 4] columns, the kernel's dot4: products and additions in k order."""
    s = a[..., 0] * b[..., 0]
    for k in (1, 2, 3):
        s = s + a[..., k] * b[..., k]
    return s


def emulate_pre_update(bank, data, pseudo, L, num_propagated, fresh):
    """pre_update_kernel's pose and ref in numpy f32 -> (pose [B, L, 16], ref [B, L, 3])."""
    x = data["prev"].numpy().astype(F)
    B = len(x)
    pose, ref = bank["pose"][:, :L].numpy().astype(F).reshape(B, L, 4, 4), bank["ref"][:, :L].numpy().astype(F)
    if not fresh:
        P = data["ego_inv"].numpy().astype(F)
        pose = _dot4_f32(P[:, None, :, None, :], pose.transpose(0, 1, 3, 2)[:, :, None, :, :]) * x[:, None, None, None]
        r4 = np.concatenate([ref, np.ones((B, L, 1), dtype=F)], -1)
        ref = _dot4_f32(P[:, None, :3, :], r4[:, :, None, :]) * x[:, None, None]
    if num_propagated:
        n = num_propagated
        nx = (F(1) - x)[:, None, None]
        pc = data["pc"].numpy().astype(F)
        ps = pseudo.numpy().astype(F)[:n] * (pc[3:] - pc[:3]) + pc[:3]
        ref, pose = ref.copy(), pose.copy()
        ref[:, :n] = ref[:, :n] + nx * ps[None]
        for i in range(4):
            pose[:, :n, i, i] = pose[:, :n, i, i] + nx[:, :, 0]
    assert pose.dtype == F and ref.dtype == F
    return pose.reshape(B, L, 16), ref


def post_update_inputs(B, Q, D, ld_bbox, seed):
    """Decoder outputs of one frame: outs_dec [B, Q, D], bbox [B, Q, ld_bbox], a rec_ego_pose of its own for every query, and ``order``: an arbitrary permutation
    of the queries per sample (the kernel takes its first topk entries; the ranking is not part of these tests)."""
    g = torch.Generator().manual_seed(35000 + seed)
    order = torch.stack([torch.randperm(Q, generator=g) for _ in range(B)]).long()
    rec = rigid_poses(B * Q, 900 + seed).float().view(B, Q, 16)
    assert not bool((rec.view(-1, 4, 4) == torch.eye(4)).all(-1).all(-1).any()), "no rec_ego_pose is the identity"
    return dict(order=order, rec=rec.contiguous(), bbox=(torch.randn(B, Q, ld_bbox, generator=g) * 12.0).contiguous(), dec=torch.randn(B, Q, D, generator=g).contiguous())


def _post_sources(bank, dec, L, topk):
    """What slot l of the out bank is built from: query order[b, l] for l < topk, slot l - topk of the in bank behind them."""
    B, Q = dec["order"].shape
    top = dec["order"][:, :topk]
    take = lambda t: torch.gather(t, 1, top[..., None].expand(B, topk, t.shape[2]))
    bbox = dec["bbox"]
    return dict(emb=torch.cat([take(dec["dec"]), bank["emb"][:, :L]], 1), vel=torch.cat([take(bbox[:, :, -2:]), bank["vel"][:, :L]], 1),
                ts=torch.cat([torch.zeros(B, topk, dtype=torch.float64), bank["ts"][:, :L]], 1),
                pose=torch.cat([take(dec["rec"]), bank["pose"][:, :L]], 1), ref=torch.cat([take(bbox[:, :, :3]), bank["ref"][:, :L]], 1))


def post_update_reference(bank, data, dec, L, topk):
    """-> (exact: emb / vel / ts; approx: pose / ref -> (f64 value, bound)) of the out bank [B, topk + L, ...]."""
    src = _post_sources(bank, dec, L, topk)
    B, cap = src["ts"].shape
    Eg = data["ego"].double()[:, None]
    pose, bp = _dot4_ref(Eg, src["pose"].double().view(B, cap, 4, 4))
    ref, br = _dot4_ref(Eg[:, :, :3], _homog(src["ref"].double()))
    return (dict(emb=src["emb"], vel=src["vel"], ts=src["ts"] - data["ts"][:, None]),
            dict(pose=(pose.reshape(B, cap, 16), bp.reshape(B, cap, 16)), ref=(ref[..., 0], br[..., 0])))


def emulate_post_update(bank, data, dec, L, topk):
    src = _post_sources(bank, dec, L, topk)
    B, cap = src["ts"].shape
    Eg = data["ego"].numpy().astype(F)
    pose = _dot4_f32(Eg[:, None, :, None, :], src["pose"].numpy().astype(F).reshape(B, cap, 4, 4).transpose(0, 1, 3, 2)[:, :, None, :, :])
    r4 = np.concatenate([src["ref"].numpy().astype(F), np.ones((B, cap, 1), dtype=F)], -1)
    ref = _dot4_f32(Eg[:, None, :3, :], r4[:, :, None, :])
    assert pose.dtype == F and ref.dtype == F
    return pose.reshape(B, cap, 16), ref


def worst(got, val, bound):
    """max |got - f64| / bound over all elements; an element with a zero bound must be met exactly (it then counts as 0, otherwise as inf)."""
    err = (torch.as_tensor(got).double() - val).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    return float(r.max()) if r.numel() else 0.0
