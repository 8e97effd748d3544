"""Cases and f64 references shared by tests/test_gpu_scorer_kernels.py (the kernels of csrc/scorer.hip on the GPU) and tests/test_cpu_scorer_abi.py (the
references' own invariants, without a GPU).  Everything here runs on the CPU; all inputs are seeded.

Every reference takes the SAME f32 (or bf16) numbers the kernel reads and evaluates the operation in f64.  Every bound is a function of those inputs and of
u = 2^-24 alone (operation counts are stated where the bound is formed); the two measured figures -- E_cpu of the motion-aware queries and the libm allowance of
the log-softmax / softmax tail -- are distances between torch's own f32 CPU evaluation and f64, never anything the device produced.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import toc3d_oracle as O

U = 2.0 ** -24
QD = 256
PC_RANGE = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]
PRE = "s."

# ---------------------------------------------------------------------------------------------------
# 1. motion-aware queries
# ---------------------------------------------------------------------------------------------------
MOTION_BQ = [(1, 1), (1, 7), (1, 8), (1, 9), (2, 5), (2, 27), (3, 64)]        # (2, 5): the group of 8 holds queries of both samples
MOTION_TS = ["f64_small", "f64_epoch", "f32_small"]
MOTION_STAGES = [1, 3]
MOTION_FACTOR = 4.0            # device <= 4 x E_cpu
MOTION_CONDITION = 2e-6        # E_cpu <= 2e-6 max|ref64|: the inputs are ones the f32 oracle itself evaluates to f32 accuracy

_LINEARS = [("query_embedding.0", 384), ("query_embedding.2", 256), ("ego_pose_pe.reduce.0", 180), ("ego_pose_pe.gamma", 256), ("ego_pose_pe.beta", 256),
            ("ego_pose_queries.reduce.0", 180), ("ego_pose_queries.gamma", 256), ("ego_pose_queries.beta", 256), ("time_embedding.0", 256)]


def motion_state_dict(stage):
    """One scorer's parameters (f32), different for every stage: weights randn * fan_in^-0.5, biases 0.1 randn, the time embedding's LayerNorm 1 + 0.1 randn."""
    g = torch.Generator().manual_seed(1000 + stage)
    sd = {}
    for name, fan_in in _LINEARS:
        sd[PRE + name + ".weight"] = torch.randn(QD, fan_in, generator=g) * fan_in ** -0.5
        sd[PRE + name + ".bias"] = 0.1 * torch.randn(QD, generator=g)
    sd[PRE + "time_embedding.1.weight"] = 1 + 0.1 * torch.randn(QD, generator=g)
    sd[PRE + "time_embedding.1.bias"] = 0.1 * torch.randn(QD, generator=g)
    sd[PRE + "pc_range"] = torch.tensor(PC_RANGE)
    return sd


def _se3(g, n):
    yaw, pitch = 0.2 * torch.randn(n, generator=g, dtype=torch.float64), 0.02 * torch.randn(n, generator=g, dtype=torch.float64)
    M = torch.zeros(n, 4, 4, dtype=torch.float64)
    cy, sy, cp, sp = yaw.cos(), yaw.sin(), pitch.cos(), pitch.sin()
    M[:, 0, 0], M[:, 0, 1], M[:, 0, 2] = cy * cp, -sy, cy * sp
    M[:, 1, 0], M[:, 1, 1], M[:, 1, 2] = sy * cp, cy, sy * sp
    M[:, 2, 0], M[:, 2, 2] = -sp, cp
    M[:, :3, 3] = torch.randn(n, 3, generator=g, dtype=torch.float64) * torch.tensor([3.0, 3.0, 0.1], dtype=torch.float64)
    M[:, 3, 3] = 1.0
    return M


def motion_inputs(B, Q, ts_kind, seed=0):
    """queries [B,Q,256], ref_points [B,Q,3] (global frame), vel [B,Q,2], timestamp [B,Q,1] (f64, or f32 for 'f32_small'), ego_pose [B,Q,4,4], ego_pose_inv
    [B,4,4].  Every sample has its own ego_pose_inv, its own ego poses and its own timestamp scale (1, 3, 10 for 'small': |t| <= 10; another epoch second per
    sample for 'f64_epoch')."""
    g = torch.Generator().manual_seed(77 + 131 * B + Q + seed)
    pc = torch.tensor(PC_RANGE)
    inp = dict(queries=torch.randn(B, Q, QD, generator=g), vel=torch.randn(B, Q, 2, generator=g),
               ref_points=pc[:3] + torch.rand(B, Q, 3, generator=g) * (pc[3:] - pc[:3]))
    if ts_kind == "f64_epoch":
        ts = -(1.5e9 + 0.5 * torch.arange(Q, dtype=torch.float64)[None, :] + 1000.0 * torch.arange(B, dtype=torch.float64)[:, None])
    else:
        scale = torch.tensor([1.0, 3.0, 10.0], dtype=torch.float64)[:B, None]
        ts = (2 * torch.rand(B, Q, generator=g, dtype=torch.float64) - 1) * scale
    inp["timestamp"] = ts[..., None].float() if ts_kind == "f32_small" else ts[..., None]
    inp["ego_pose"] = _se3(g, B * Q).reshape(B, Q, 4, 4).float()
    inp["ego_pose_inv"] = torch.linalg.inv(_se3(g, B)).float()
    if B > 1:
        assert not torch.equal(inp["ego_pose_inv"][0], inp["ego_pose_inv"][1])
    return inp


def motion_args(inp):
    return (inp["queries"], inp["ref_points"], inp["vel"], inp["timestamp"], inp["ego_pose"], inp["ego_pose_inv"])


def motion_ref64(sd, inp, pre=PRE):
    """oracle.toc3d_oracle.motion_aware_queries with weights and inputs in f64.  Two things belong to the operation's definition and are kept: the ego-motion
    vector is cast to f32 before the NeRF encoding (toc3d_utils.py:351), so the angles e * 2^k are exact f32 values here as in the kernel; dim_t is built in
    f32 (inside oracle.pos2posemb) and promoted."""
    sd = {k: v.double() for k, v in sd.items() if k.startswith(pre)}
    queries, ref_points, vel, timestamp, ego_pose, ego_pose_inv = motion_args(inp)
    lin = lambda x, name: F.linear(x, sd[pre + name + ".weight"], sd[pre + name + ".bias"])
    ref_points = ref_points.double()
    pts = (ego_pose_inv.double()[:, None] @ torch.cat([ref_points, torch.ones_like(ref_points[..., :1])], -1)[..., None])[..., :3, 0]
    pc = sd[pre + "pc_range"]
    pts = (pts - pc[:3]) / (pc[3:6] - pc[0:3])
    emb = O.pos2posemb3d(pts)
    assert emb.dtype == torch.float64
    pos = lin(F.relu(lin(emb, "query_embedding.0")), "query_embedding.2")
    motion = torch.cat([vel, timestamp, ego_pose[..., :3, :].flatten(-2)], dim=-1).float().double()
    motion = O.nerf_encoding(motion)
    pos = O.mln(pos, motion, sd, pre + "ego_pose_pe.")
    te = lin(O.pos2posemb1d(timestamp.double()), "time_embedding.0")
    pos = pos + F.layer_norm(te, (QD,), sd[pre + "time_embedding.1.weight"], sd[pre + "time_embedding.1.bias"], O.TORCH_LN_EPS)
    out = O.mln(queries.double(), motion, sd, pre + "ego_pose_queries.") + pos
    assert out.dtype == torch.float64
    return out


def motion_oracle32(sd, inp):
    return O.motion_aware_queries(sd, PRE, *motion_args(inp))


_MOTION = {}


def motion_case(B, Q, ts_kind, stage):
    """(inputs, ref64 [B,Q,256], E_cpu = max |f32 oracle on the CPU - ref64|), computed once per case."""
    key = (B, Q, ts_kind, stage)
    if key not in _MOTION:
        inp, sd = motion_inputs(B, Q, ts_kind), motion_state_dict(stage)
        with torch.no_grad():
            ref = motion_ref64(sd, inp)
            e_cpu = float((motion_oracle32(sd, inp).double() - ref).abs().max())
        _MOTION[key] = (inp, ref, e_cpu)
    return _MOTION[key]


# ---------------------------------------------------------------------------------------------------
# 2. collapsed scorer
# ---------------------------------------------------------------------------------------------------
# every Q of {1, 15, 16, 17, 64, 100}, every C of {1, 255, 256, 257, 1024}, both B
COLLAPSE_CASES = [(1, 1, 1), (3, 1, 257), (1, 15, 255), (3, 15, 1024), (1, 16, 256), (3, 16, 1), (1, 17, 257), (3, 17, 255), (1, 64, 1024), (3, 64, 256),
                  (1, 100, 257), (3, 100, 255), (3, 100, 1024)]
COLLAPSE_SCALE = 256 ** -0.5                 # = 2^-4, exact in f32
COLLAPSE_C0 = 2                              # the product with `scale`, and one u for the second-order terms


def collapse_inputs(B, Q, C, seed=0):
    g = torch.Generator().manual_seed(300 + 7 * B + 13 * Q + C + seed)
    return dict(mq=torch.randn(B, Q, QD, generator=g), w_in=torch.randn(QD, C, generator=g) * max(C, 1) ** -0.5, b_in=0.1 * torch.randn(QD, generator=g),
                w_agg=torch.randn(2, Q, generator=g) * Q ** -0.5, b_agg=0.1 * torch.randn(2, generator=g))


def collapse_ref64(i, scale=COLLAPSE_SCALE):
    """(wc [B,C,2], bc [B,2], their per-element bounds).  u[b,c,j] = sum_q mq[b,q,c] W_agg[j,q] is a chain of Q FMAs, wc a chain of 256 FMAs over c and one
    product with scale: (Q + 256 + c0) u scale sum_c |W_in[c,i]| sum_q |mq| |W_agg|.  bc: Q for u, one product with b_in, 8 additions deep in the 256-term
    block sum (6 butterfly levels in the wavefront, 2 across the four wavefronts), the product with scale, one u of slack: (Q + 12) u scale sum_c |b_in[c]|
    sum_q |mq| |W_agg|, and u |bc| for the final addition of b_agg."""
    mq, w_in, b_in, w_agg, b_agg = (i[k].double() for k in ("mq", "w_in", "b_in", "w_agg", "b_agg"))
    Q = mq.shape[1]
    u = torch.einsum("bqc,jq->bcj", mq, w_agg)
    ua = torch.einsum("bqc,jq->bcj", mq.abs(), w_agg.abs())
    wc = scale * torch.einsum("ci,bcj->bij", w_in, u)
    bc = scale * torch.einsum("c,bcj->bj", b_in, u) + b_agg
    wc_tol = (Q + 256 + COLLAPSE_C0) * U * scale * torch.einsum("ci,bcj->bij", w_in.abs(), ua)
    bc_tol = (Q + 12) * U * scale * torch.einsum("c,bcj->bj", b_in.abs(), ua) + U * bc.abs()
    return wc, bc, wc_tol, bc_tol


# ---------------------------------------------------------------------------------------------------
# 3. token scores: logits -> log-softmax -> Gumbel soft mask
# ---------------------------------------------------------------------------------------------------
TOKENS_C = [4, 128, 252, 256, 260, 1024, 1028]
TOKENS_VT = [(1, 1, 1), (2, 3, 1), (4, 5, 2), (6, 7, 3), (2, 1000, 2)]          # (V, T, views_per_frame)
HEAD_K = [8, 32, 256, 504, 512, 520, 1032]
HEAD_M = [1, 3, 4, 5, 1001]
G_MIN = float(-math.log(-math.log(2.0 ** -24)))           # the generator's extremes (include/toc3d.h, toc3d_gumbel_from_bits): ~ -2.81
G_MAX = float(-math.log(-math.log(1 - 2.0 ** -24)))       # ~ 16.64
LIBM_FACTOR = 4.0              # the device gets 4 x the worst CPU figure
LIBM_SANITY = 4.0              # ... and the CPU figure itself, in the units below, stays under this (measured: see test_gpu_scorer_kernels.py)


def gumbel_rows(M, seed):
    """[M, 2] f32 Gumbel(0, 1) noise; rows 0 and 1 (where they exist) hold the generator's extremes in both orders."""
    g = torch.Generator().manual_seed(seed)
    n = -torch.log(-torch.log(torch.rand(M, 2, generator=g).clamp(2.0 ** -24, 1 - 2.0 ** -24)))
    n[0] = torch.tensor([G_MIN, G_MAX])
    if M > 1:
        n[1] = torch.tensor([G_MAX, G_MIN])
    return n


def spread_rows(x, dd):
    """Scales rows of x (in place) so that |l0 - l1| ~ 20 on rows 2, 6, 10, ... and ~ 100 on rows 3 (mod 8) -- dd [M] is the rows' current l0 - l1 without
    the bias.  Rows with |dd| <= 0.25 are left alone: scaling them up would only scale the cancellation, and with it the bound."""
    M = x.shape[0]
    for start, step, target in ((2, 4, 20.0), (3, 8, 100.0)):
        rows = torch.arange(start, max(M, start), step)
        rows = rows[dd[rows].abs() > 0.25]
        x[rows] *= (target / dd[rows].abs()).float()[:, None]
    return x


def tail_ref64(logits, delta, gumbel):
    """logits f64 [M,2], delta f64 [M] (the logits' bound), gumbel f32 [M,2] or None -> dict(pred, mask, pred_tol, mask_tol, k_pred, k_mask).

    pred = log_softmax, mask = softmax(pred + g)[0], in f64.  A logit error of delta moves pred by at most 2 delta (dp0 = s1 (dl0 - dl1)) and a0 - a1 by
    2 delta, hence the mask by delta / 2 (logistic slope <= 1/4).  The libm allowance is MEASURED (no HIP math accuracy table ships with the toolchain): torch's
    f32 CPU log_softmax / softmax on the logits rounded to f32 against f64 on the same rounded rows, in units of u (1 + |l0 - l1|) for pred and
    u (1 + (|a0| + |a1|) / 4) for the mask (the size of one rounding of the quantities the tail forms: l - max, pred + g, and the outputs themselves); the
    worst row's figure k, times LIBM_FACTOR, is what every row of the device gets, in the same units."""
    g = torch.zeros_like(logits) if gumbel is None else gumbel.double()
    pred = torch.log_softmax(logits, -1)
    a = pred + g
    mask = torch.softmax(a, -1)[:, 0]
    l32 = logits.float()
    unit_p = U * (1 + (l32[:, 0] - l32[:, 1]).abs().double())
    p32 = torch.log_softmax(l32, -1)
    k_pred = float(((p32.double() - torch.log_softmax(l32.double(), -1)).abs().amax(1) / unit_p).max())
    a32 = p32 + g.float()
    unit_m = U * (1 + a32.abs().sum(1).double() / 4)
    k_mask = float(((torch.softmax(a32, -1)[:, 0].double() - torch.softmax(a32.double(), -1)[:, 0]).abs() / unit_m).max())
    k_pred, k_mask = max(k_pred, 1.0), max(k_mask, 1.0)              # never below one rounding of the output
    assert k_pred <= LIBM_SANITY and k_mask <= LIBM_SANITY, (k_pred, k_mask)
    unit_p = U * (1 + (logits[:, 0] - logits[:, 1]).abs())
    unit_m = U * (1 + a.abs().sum(1) / 4)
    pred_tol = (2 * delta + LIBM_FACTOR * k_pred * unit_p)[:, None].expand(-1, 2)
    # the mask sees pred's own rounding too: a0 - a1 carries 2 x pred's allowance, a quarter of which reaches the mask
    mask_tol = delta / 2 + LIBM_FACTOR * k_pred * unit_p / 2 + LIBM_FACTOR * k_mask * unit_m
    return dict(pred=pred, mask=mask, pred_tol=pred_tol, mask_tol=mask_tol, k_pred=k_pred, k_mask=k_mask)


def tokens_inputs(C, V, T, vpf, with_mask, seed=0):
    """x [V*T, C], mask [V*T] or None, wc [B, C, 2], bc [B, 2] with B = V / vpf: every sample has its own collapsed weights."""
    g = torch.Generator().manual_seed(500 + C + 17 * V + T + seed)
    M, B = V * T, V // vpf
    x = torch.randn(M, C, generator=g)
    mask = torch.rand(M, generator=g) if with_mask else None
    wc, bc = torch.randn(B, C, 2, generator=g) * C ** -0.5, torch.randn(B, 2, generator=g)
    b = (torch.arange(M) // T) // vpf
    mk = mask.double() if with_mask else torch.ones(M, dtype=torch.float64)
    dd = torch.einsum("mc,mc->m", x.double() * mk[:, None], (wc[b, :, 0] - wc[b, :, 1]).double())
    spread_rows(x, dd)
    return dict(x=x, mask=mask, wc=wc, bc=bc, b=b)


def tokens_logits64(i):
    """(logits f64 [M,2], delta [M]).  Per element the kernel rounds x * mask and the product with w, adds 2 deep inside a float4, once per trip onto the
    lane's running sum (trips = ceil(C / 256)), 6 butterfly levels, and adds bc: (11 + trips) u sum |x mask w| with one u of slack, + u |bc|."""
    x, wc, bc, b = i["x"].double(), i["wc"].double(), i["bc"].double(), i["b"]
    C = x.shape[1]
    mk = i["mask"].double()[:, None] if i["mask"] is not None else 1.0
    xm = x * mk
    logits = torch.einsum("mc,mcj->mj", xm, wc[b]) + bc[b]
    mag = torch.einsum("mc,mcj->mj", xm.abs(), wc[b].abs())
    delta = (11 + -(-C // 256)) * U * mag + U * bc[b].abs()
    return logits, delta.amax(1)


def head_inputs(kdim, ld, M, bf16, seed=0):
    """f [M, ld] (f32 or bf16; columns [kdim, ld) hold NaN: they must never be read), w [2, kdim], b [2]."""
    g = torch.Generator().manual_seed(700 + kdim + 3 * ld + M + seed)
    f = torch.randn(M, kdim, generator=g)
    w, b = torch.randn(2, kdim, generator=g) * kdim ** -0.5, torch.randn(2, generator=g)
    if bf16:
        f = f.bfloat16().float()
    spread_rows(f, f.double() @ (w[0] - w[1]).double())
    full = torch.full((M, ld), float("nan"))
    full[:, :kdim] = f
    return dict(f=full.bfloat16() if bf16 else full, w=w, b=b, kdim=kdim)


def head_logits64(i):
    """(logits, delta) from the values the kernel reads (the bf16-rounded ones for bf16 rows).  Each lane runs 8 * trips FMAs in a chain (trips =
    ceil(kdim / 512)), then 6 butterfly levels and the bias: (8 trips + 8) u sum |f w| with one u of slack, + u |b|."""
    k = i["kdim"]
    f, w, b = i["f"][:, :k].double(), i["w"].double(), i["b"].double()
    logits = f @ w.T + b
    delta = (8 * -(-k // 512) + 8) * U * (f.abs() @ w.abs().T) + U * b.abs()
    return logits, delta.amax(1)


# ---------------------------------------------------------------------------------------------------
# 4. global mean of the upper half of the columns
# ---------------------------------------------------------------------------------------------------
MEAN_C = [2, 64, 126, 128, 130, 258]
MEAN_T = [1, 3, 4, 5, 1000]
MEAN_V = [1, 3]


def mean_inputs(V, T, C, ld, bf16, seed=0):
    g = torch.Generator().manual_seed(900 + V + 5 * T + C + ld + seed)
    t = torch.randn(V * T, ld, generator=g) + 0.5
    return t.bfloat16() if bf16 else t


def mean_ref64(t, V, T, C, bf16):
    """(mean f64 [V, C/2] of the stored values, its bound (T/4 + 5) u mean|v| (+ 2^-8 |mean| when the result is rounded to bf16))."""
    v = t.double().reshape(V, T, -1)[:, :, C // 2:C]
    mean = v.mean(1)
    tol = (T / 4 + 5) * U * v.abs().mean(1) + (2.0 ** -8 * mean.abs() if bf16 else 0.0)
    return mean, tol


# ---------------------------------------------------------------------------------------------------
# 5. Philox4x32-10
# ---------------------------------------------------------------------------------------------------
PHILOX_KAT = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
              ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
              ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
GUMBEL_N = [1, 2, 3, 4, 5, 1023, 1024, 1025, 4099]
GUMBEL_SEEDS = [1234, (0xDEADBEEF << 32) | 0x12345678, 0xFFFFFFFF00000000]
GUMBEL_FRAMES = [0, 7, (1 << 32) + 5]


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., 'Parallel random numbers: as easy as 1, 2, 3', SC'11).  counter: uint32 array [..., 4], key: two uint32 -> uint32 [..., 4]."""
    c = [np.asarray(counter, dtype=np.uint64)[..., i] for i in range(4)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    mask = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & mask]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack(c, axis=-1).astype(np.uint32)


def gumbel_words(n, seed, frame):
    """The n 32-bit words behind toc3d_gumbel_noise(n, seed) at frame counter `frame`: block q = element / 4 has counter (q lo, q hi, frame lo, frame hi)
    and key (seed lo, seed hi); element 4 q + e is word e of the block."""
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    ctr = np.stack([q & np.uint64(0xFFFFFFFF), q >> np.uint64(32), np.full_like(q, frame & 0xFFFFFFFF), np.full_like(q, frame >> 32)], axis=-1)
    return philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32)).reshape(-1)[:n]


# ---------------------------------------------------------------------------------------------------
# 6. bicubic resize of the absolute position embedding
# ---------------------------------------------------------------------------------------------------
BICUBIC_CASES = [(4, 4, 4), (4, 1, 1), (4, 3, 7), (4, 9, 5), (16, 8, 8), (16, 20, 50)]      # (S, h, w); (4, 4, 4) is the copy path, the 16-grids downscale once
BICUBIC_C = [1, 255, 257]
BICUBIC_SUM = 12               # two 4-tap sums, each a product and an addition per tap plus the chain: <= 5 roundings deep each, 2 u for second order
BICUBIC_COEF = 40              # roundings of one cubic_coeffs polynomial in units of u (Horner with |A| = 0.75: intermediates <= 6, see below)


def _cubic(t):
    A = -0.75
    x0, x2, x3 = t + 1, 1 - t, 2 - t
    return torch.stack([((A * x0 - 5 * A) * x0 + 8 * A) * x0 - 4 * A, ((A + 2) * t - (A + 3)) * t * t + 1, ((A + 2) * x2 - (A + 3)) * x2 * x2 + 1,
                        ((A * x3 - 5 * A) * x3 + 8 * A) * x3 - 4 * A], -1)


def bicubic_ref64(pos, S, h, w):
    """pos f32 [S*S, C] -> (F.interpolate(bicubic, align_corners=False) in f64 as [h*w, C], the per-element bound, this module's own f64 cubic convolution).

    Bound.  out = sum_ij cy_i cx_j pos_ij.  The two 4-tap sums: BICUBIC_SUM u sum_ij |cy_i| |cx_j| |pos_ij|.  The coefficients themselves are NOT relatively
    accurate (the outer taps pass through zero), so their error is absolute: the source coordinate f = (S / n)(k + 0.5) - 0.5 is formed in f32 with three
    roundings, |df| <= 3 u (|f| + 1); t = f - floor(f) is exact; a coefficient moves by at most 1.5 |dt| (max |c'(t)| = 1.35 on [0, 1]; the convolution is
    continuous across floor's jump) and its Horner evaluation adds at most BICUBIC_COEF u (six roundings of intermediates that stay below 6 in magnitude,
    carried through at most two further products with x <= 2): |dc| <= e(f) = (BICUBIC_COEF + 4.5 (|f| + 1)) u, and
        |dev - ref| <= BICUBIC_SUM u sum_ij |cy_i| |cx_j| |pos_ij| + sum_ij (e(fy) |cx_j| + e(fx) |cy_i|) |pos_ij|."""
    C = pos.shape[1]
    p = pos.double().reshape(S, S, C)
    if S == h and S == w:
        ref = p.reshape(h * w, C)
        return ref, torch.zeros_like(ref), ref
    ref = F.interpolate(p.permute(2, 0, 1)[None], size=(h, w), mode="bicubic", align_corners=False)[0].permute(1, 2, 0).reshape(h * w, C)
    fy = (S / h) * (torch.arange(h, dtype=torch.float64) + 0.5) - 0.5
    fx = (S / w) * (torch.arange(w, dtype=torch.float64) + 0.5) - 0.5
    iy, ix = fy.floor(), fx.floor()
    cy, cx = _cubic(fy - iy), _cubic(fx - ix)                                      # [h, 4], [w, 4]
    ty = (iy.long()[:, None] - 1 + torch.arange(4)).clamp(0, S - 1)                # [h, 4]
    tx = (ix.long()[:, None] - 1 + torch.arange(4)).clamp(0, S - 1)
    taps = p[ty[:, None, :, None], tx[None, :, None, :]]                           # [h, w, 4, 4, C]
    wgt = cy[:, None, :, None] * cx[None, :, None, :]                              # [h, w, 4, 4]
    own = torch.einsum("hwij,hwijc->hwc", wgt, taps).reshape(h * w, C)
    ey = (BICUBIC_COEF + 4.5 * (fy.abs() + 1)) * U
    ex = (BICUBIC_COEF + 4.5 * (fx.abs() + 1)) * U
    wtol = BICUBIC_SUM * U * wgt.abs() + ey[:, None, None, None] * cx.abs()[None, :, None, :] + ex[None, :, None, None] * cy.abs()[:, None, :, None]
    tol = torch.einsum("hwij,hwijc->hwc", wtol, taps.abs()).reshape(h * w, C)
    return ref, tol, own
