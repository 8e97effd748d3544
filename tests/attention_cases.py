"""Cases, f64 reference, per-element bounds, kernel emulations and wrong references ("mutants") shared by tests/test_gpu_attention_kernels.py (the seven
attention kernel bodies on the GPU, through the C ABI) and tests/test_cpu_attention_cases.py (the same cases without a GPU: the bounds admit an emulation
of each kernel's rounding points and reject every mutant).  CPU and torch only.

Kernel bodies and how a launch reaches them (`body_of` mirrors launch_attn / launch_rot_x3, csrc/attention.hip:653-671, csrc/attention_rot.hip:547-560):
    toc3d_window_attention_rot  bf16            attn_rot_kernel                   (stride <= 416)
                                F32X3P          attn_rot_x3_kernel<false>         keys rounded up to 32 <= 288 (512 B of LDS per key, 144 KB)
                                                attn_rot_x3_kernel<true>          above: 128-key super-tiles
    toc3d_window_attention      five kinds      attn_small_kernel<9 | 11 | 13>    stride <= 144 / 176 / 208 AND the window's K and V^T fit 96 KB of LDS:
                                                                                  bf16 always; the f32 buffers (528 B per key) up to stride 160, so the
                                                                                  f32 forms run <9> to 144, <11> for 145..160 and never <13>
                                                attn_kernel (flash)               everything else

Reference.  `reference(b)` takes the operands the device is handed AFTER their rounding to the buffer type (bf16 values; (hi, lo) planes = hi + lo; f32) and
returns, in f64, out[w, i, head, d], A[w, i, head, d] = sum_k P_ik |v_kd| (P the f64 softmax over the window's real keys, its virtual kept-pad keys -- k and v of
pad_rot[slot] on the rot path, of the one pad_qkv row rotated by its slot on the other -- and the npad analytic zero-pad keys: score 0, value v_bias), and
    T[w, i, head]  = max_k sum_d |q_d k_d|                                       in nats, q rotated and scaled, k rotated;
    Tp[w, i, head] = max_k sum_t (|q_2t| + |q_2t+1|) (|k_2t| + |k_2t+1|) >= T    the same over RoPE pairs (toc3d_window_attention only, below).
Rot path: q and k arrive rotated, q scaled by head_dim^-0.5 log2(e), the kernel exponentiates with exp2: S = q.k ln 2.  toc3d_window_attention: f64 RoPE by
slot from the [L*L, 64] f32 tables (eva_utils.py:378-379), times `scale`.

Bound, per element:      |dev - ref| <= eps(kind, T_i, Tp_i) A + (n_keys + 8) u A,        u = 2^-24, n_keys = the window's keys (+ 1 for the npad term).
The second term is the f32 accumulation of numerator and denominator (MFMA steps of 32 products on bf16 operands, of 4 on f32 ones, lane partials, the
butterfly over the four lane groups), the rescales of the online forms (one per 64-key tile at most), the pad term, the reciprocal and the final product.

eps = first + 2 e / (1 - e),  e = expm1(delta) + 4 u.   delta bounds the absolute error of a score MINUS its reference point, in nats; 4 u is the exponential
itself (v_exp_f32 / expf: <= 2 ulp).  If every unnormalised P_k is off by a relative e_k, |e_k| <= e, in numerator AND denominator, the output moves by
|sum_k P_k e_k (v_k - out)| / sum_k P_k (1 + e_k) <= e (A + |out|) / (1 - e) <= 2 e A / (1 - e).  `first` collects what hits the numerator or the output
alone, each relative to A >= |out|.  Units: bf16 round-to-nearest 2^-8, (hi, lo) planes 2^-16, f32 2^-24.

  attn_rot_kernel (attention_rot.hip:100-257).  Operands reach the MFMAs untouched (DMA to LDS, :153-157).
      scores      f32 sums of 64 exact bf16 products (:197-200): 64 u T;  s - mx (:219): u |s - mx| <= (2 T + 6) u (the deferred reference point is at most
                  RESCALE_THR = 8 log2 units below the maximum, :209)                                              delta = (66 T + 6) u
      numerator   P rounded to bf16 as the MFMA operand (:220), V exact: 2^-8
      denominator the f32 pv (:221): nothing
      output      to_act<bf16_t> (:248): 2^-8 of the value rounded, <= A (1 + what precedes)
      third 2^-8  every second-order product of the above and of the u terms, generously                           first = 3 * 2^-8
  attn_rot_x3_kernel<false | true> (attention_rot.hip:321-545).  q = qh + ql, k = kh + kl, v = vh + vl exactly (planes).
      scores      ql.kh + qh.kl + qh.kh (x3_mma16, :314-318, :428-429): ql.kl is lost, |ql| <= 2^-8 |q|: 2^-16 T;  192 f32 additions: 192 u T;  s - mx: (2 T + 6) u
                                                                                                                   delta = 2^-16 T + (194 T + 6) u
      numerator   P = ph + pl + r, |r| <= 2^-16 P (:450-456); pl.vh + ph.vl + ph.vh (:470): r.v and pl.vl are lost: 2 * 2^-16
      output      (hi, lo) planes (:526-528): 2^-16                                                                first = 3 * 2^-16
  attn_small_kernel / attn_kernel, bf16 (attention.hip:178-405, :422-637).  RoPE in f32 on the loaded row (rope8_lds, :98-110): an element's error is
      relative to the NORM OF ITS PAIR, <= 2 u (|x'_a| + |x'_b|) -- hence Tp; the scale u (:239, :551).
      scores      rotated, scaled q and rotated k are rounded to bf16 (make_frag :241, :553; store8 :291, :516): (2 * 2^-8 + 2^-16) T;  the f32 RoPE of both,
                  the scale, 64 additions: 73 u Tp;  s - max and the product with log2(e) inside __expf (:119): (4 T + 12) u
                                                                                                                   delta = (2^-7 + 2^-16) T + (73 Tp + 4 T + 12) u
      numerator   P -> bf16 (make_frag :345, :600); the sum takes the f32 pv (:342, :602)
      output      to_act<bf16_t> (:394, :626)                                                                      first = 3 * 2^-8 (as attn_rot_kernel)
  the same two bodies on f32 buffers, exact products (F32, F32X3WO): f32 MFMAs (common.h mma_step), expf.
      scores      delta = (73 Tp + 4 T + 12) u
      numerator   P and V are f32: nothing beyond the accumulation term
      output      f32: u;  F32X3WO: planes (store4_planes :397, :629): 2^-16                                       first = 4 u | 2^-16 + 4 u
  the same on f32 buffers with bf16 x 3 products (F32X3, F32X3P; X3 = true).  Nothing arrives split: x3_split (:146-155) keeps hi + lo of an f32 value and
      DROPS the remainder r, |r| <= 2^-16 |x| -- a rounding point the planes kernels do not have.
      scores      q' = qh + ql + rq, k' likewise (:240, :552, x3_chunk_bits :286, :511); lo.hi + hi.lo + hi.hi (x3_mma :172-176): ql.kl, rq.k and q.rk are lost:
                  3 * 2^-16 T;  192 additions + RoPE + scale: 201 u Tp;  (4 T + 12) u                             delta = 3 * 2^-16 T + (201 Tp + 4 T + 12) u
      numerator   P split (:344, :599), V split when staged (x3_store_vt :166-171): pl.vl, rp.v, p.rv are lost: 3 * 2^-16
      output      F32X3: f32, u;  F32X3P: planes, 2^-16                                                            first = 3 * 2^-16 + 4 u | 4 * 2^-16 + 4 u
The formulas need e < 1; the cases keep delta <= DELTA_CAP = 0.25 (asserted on the CPU), which caps T of each kind.

Inputs, "flat" family.  Seeded by the case's name.  k, v ~ randn; q ~ std randn (`q_std`) in the units the kernel exponentiates (0.12 log2 units on the rot path;
the same std(q) * scale in nats for the f32 forms of toc3d_window_attention; 0.01 nats and 4 x the loudness for its bf16 form, where delta carries 2^-7 T; a quarter
of the std where a window has ONE query row, which is all or nothing for a mutant), so the softmax is nearly uniform and a single key weighs ~1 / n in EVERY row.  Edge keys -- {0, 15, 16, 31, 32, 63, 64, 127, 128, 255, 256} and, relative to the window's own
key count, {-33, -32, -17, -16, -2, -1}, where they exist -- carry v = +-loud with a random sign per (window, head, key, dim),
loud = max(4, 2^ceil(log2((keys + npad) / 16))): dropping one moves a row by ~loud / n of an A that is O(1).  Rows of the q|k|v buffer that no list names,
rows listed beyond a window's count, the guard columns and the unused q part of the pad rows hold +-2^100: a kernel may read a row it masks, it may not
let it weigh in.  Virtual kept-pad keys: on the rot path the pad_rot rows of slots 1..31 are loud and the virtual EDGE keys take their slots there, the others
above; on the other path the ONE pad row is loud where a window has a single pad and quiet otherwise (every virtual key has the same v: see `mutants` for what that leaves
visible).
npad cases named "npadneg": q' = 0.15 |q|, k' = -|k| after rotation and 2 x the loudness: every real score is negative (~ -0.5 nats), so the row's reference point is the
pads' 0 from start to end (no rescale in the first chunk of the attn_rot kernels, m < 0 in the flash epilogue).
"Spike" family: the construction of test_rot_attention_deferred_rescale_is_the_exact_softmax (tests/test_gpu_attn_rot.py) -- in window 0, key 70 far above
every earlier key for queries 0..39, key n - 5 above that for queries 20..59 -- at full precision on the f32 and planes forms, scaled down on the bf16 form of
toc3d_window_attention until delta <= DELTA_CAP.

Mutants (CPU only; `mutants(b, ref)` yields (name, wrong out, affected [window] mask, rows or None)):
    (a) key e dropped, for every edge key e          (b) key 0 read in place of the last key          (c) the npad term omitted
    (d) the npad keys counted once                    (e) v, and k, taken from the neighbouring head   (f) virtual pad keys from pad_rot[0] / rotated by slot 0
    (g) one query row computed with the previous row's q
A softmax that is peaked by construction hides a dropped key in every row whose weight sits elsewhere, at any loudness; so on the spike family only (e) and (g)
apply.  With virtual keys on toc3d_window_attention all pads share one v: dropping or mis-rotating one of SEVERAL is invisible in the output by construction,
so there (a) applies to real keys and to a window's only pad, (f) to windows with one pad -- and not on the bf16 form, whose flat inputs keep every score within
~0.1 nats so that 2^-7 T stays small: a mis-rotated pad moves its weight by ~10 %, under that bound; the f32 forms of the same template catch it.  For the same reason
(e) with k from the neighbouring head does not apply where several pads share v (the output is their v whatever the scores) nor, like (g), on the "npadneg" cases (q' = c |q| in every row and
k' = -|k| in every head: a neighbour's gives nearly the same scores).  On the bf16 form's spike cases T of EVERY row of window 0 is the spike key's, 2 x the bound is ~0.9 A there, and (e) is required of windows 1 and 2 only.
"""
import math
import zlib
from dataclasses import dataclass
from functools import lru_cache

import torch

from support import DEV
from toc3d_amd import synth

U = 2.0 ** -24
LN2 = math.log(2.0)
HD = 64
ROPE_SIDE = 21                                   # 441 slots: room for 401 distinct ones
PLAIN_SCALE = 0.125
DELTA_CAP = 0.25
T_CAP_FLAT = 8.0                                 # nats; the flat family stays below (asserted on the CPU)
EDGE_ABS = (0, 15, 16, 31, 32, 63, 64, 127, 128, 255, 256)
EDGE_REL = (-33, -32, -17, -16, -2, -1)
GUARD_ROWS = 5
BIG = 2.0 ** 100
TBF = torch.bfloat16
PLAIN_KINDS = ("f32", "bf16", "x3", "x3p", "x3wo")


@dataclass(frozen=True)
class Case:
    name: str
    path: str                  # "rot": toc3d_window_attention_rot, "plain": toc3d_window_attention
    kind: str                  # rot: "bf16" | "x3p";  plain: "f32" | "bf16" | "x3" | "x3p" | "x3wo"
    n: int                     # stride = the launch's largest key count
    counts: tuple = None       # query count per window (default: n everywhere); keys = the same unless virt_q
    nwin: int = 3
    heads: int = 2
    npad: int = 0
    virt_q: int = 0            # > 0: every window has virt_q queries and n keys, keys virt_q.. are virtual kept pads
    family: str = "flat"
    scattered: bool = False    # ldqkv > 3C, ldo > C, rows a permutation of the buffer
    neg: bool = False          # npad cases: every real score negative, so the reference point of every row stays at the pads' 0

    def __str__(self):
        return self.name


# ---- roundings ------------------------------------------------------------------------------------------------
def r_bf16(x):
    return x.float().to(TBF).double()


def split_bf16(x):
    """f32 value -> (hi, lo) as the kernels split it: hi = bf16(x), lo = bf16(x - hi)."""
    x = x.float()
    hi = x.to(TBF).float()
    return hi.double(), (x - hi).to(TBF).double()


def r_planes(x):
    hi, lo = split_bf16(x)
    return hi + lo


def r_f32(x):
    return x.float().double()


# ---- dispatch mirror -------------------------------------------------------------------------------------------
def body_of(case):
    if case.path == "rot":
        if case.kind == "bf16":
            return "attn_rot_kernel"
        return "attn_rot_x3_kernel<true>" if (case.n + 31) // 32 * 32 * 512 > 144 * 1024 else "attn_rot_x3_kernel<false>"
    s, esz = case.n, 2 if case.kind == "bf16" else 4
    if s <= 208:
        nsub, nk32 = (s + 15) // 16, (s + 31) // 32 * 32
        lds = (nsub * 16 * (HD + 16 // esz) + HD * (nk32 + 16 // esz)) * esz + (s + 3) // 4 * 4 * 8 + ROPE_SIDE * 256
        if lds <= 96 * 1024:
            return "attn_small_kernel<%d>" % (9 if s <= 144 else 11 if s <= 176 else 13)
    return "attn_kernel"


def edge_keys(nk):
    return sorted({e for e in EDGE_ABS if e < nk} | {nk + o for o in EDGE_REL if nk + o >= 0})


def loud_of(nk, npad, case=None):
    """The bf16 form of toc3d_window_attention gets 4 x: its bound carries 2 * 2^-7 T beside the 3 * 2^-8, and one of ~13 equally loud edge keys is ~1 / 13 of A at most."""
    f = (4.0 if (case.path, case.kind) == ("plain", "bf16") else 1.0) * (2.0 if case.neg else 1.0) if case is not None else 1.0      # neg: the real keys weigh e^-0.5 of a pad
    return max(4.0, 2.0 ** math.ceil(math.log2(max(nk + npad, 1) / 16.0))) * f


def q_std(case):
    """std of q in the buffer: log2 units on the rot path (its q carries log2(e)), nats / PLAIN_SCALE on the other."""
    if case.family == "spike" and case.path == "rot":
        return 0.6
    if case.family == "spike":
        return (0.09 if case.kind == "bf16" else 0.6 * LN2) / PLAIN_SCALE
    flat = 0.25 if case.virt_q == 1 else 1.0     # one query row per (window, head) is all or nothing for a mutant: flatter, so that no key's weight is far below 1 / n by chance
    if case.path == "rot":
        return 0.12 * flat
    return (0.01 if case.kind == "bf16" else 0.12 * LN2 * flat) / PLAIN_SCALE


def round_operand(case, x):
    if case.kind == "bf16":
        return r_bf16(x)
    if case.path == "rot":
        return r_planes(x)
    return r_f32(x)


# ---- inputs ----------------------------------------------------------------------------------------------------
@lru_cache(maxsize=4)
def build(case):
    g = torch.Generator().manual_seed(zlib.crc32(case.name.encode()))
    H, n, nW = case.heads, case.n, case.nwin
    C = H * HD
    counts = case.counts or (n,) * nW
    assert len(counts) == nW and max(counts) <= n
    nq = torch.tensor([case.virt_q if case.virt_q and c else c for c in counts])
    nk = torch.tensor([n if case.virt_q and c else c for c in counts])
    npd = torch.tensor([case.npad if c else 0 for c in counts])
    ldqkv, ldo = (3 * C + 32, C + 32) if case.scattered else (3 * C, C)
    R = nW * n + GUARD_ROWS
    ids = torch.randperm(R, generator=g) if case.scattered else torch.arange(R)
    own = ids[GUARD_ROWS:].view(nW, n)                                    # the buffer row every list position owns (row 0 is in no list unless scattered)
    j = torch.arange(n)[None, :]
    is_q, is_key = j < nq[:, None], j < nk[:, None]
    rows = torch.where(is_key & ~is_q, torch.full_like(own, -1), own)    # virtual pads: -1;  beyond the key count: a real row nobody may use

    std = q_std(case)
    q = torch.randn(nW, n, H, HD, generator=g) * std
    k = torch.randn(nW, n, H, HD, generator=g)
    v = torch.randn(nW, n, H, HD, generator=g)
    sign = torch.randint(0, 2, (nW, n, H, HD), generator=g) * 2.0 - 1.0
    L = ROPE_SIDE
    base = torch.stack([torch.randperm(L * L - 32, generator=g) + 32 for _ in range(nW)])
    slots = base.repeat(1, -(-n // base.shape[1]))[:, :n].contiguous()    # distinct while they last (toc3d_window_attention has at most 401 keys here)
    cos, sin = synth.rope_tables(L)
    if case.neg:
        # q' = 0.15 |q| (toc3d_window_attention on bf16: |q|, it is flat already), k' = -|k| in the ROTATED domain: scores around -0.5 nats, all below the pads' 0
        qn, kn = q.abs().double() * (1.0 if (case.path, case.kind) == ("plain", "bf16") else 0.15), -k.abs().double()
        if case.path == "plain":
            cs, sn = cos.double()[slots][:, :, None, :], sin.double()[slots][:, :, None, :]
            qn, kn = rope_f64(qn, cs, -sn), rope_f64(kn, cs, -sn)
        q, k = qn.float(), kn.float()
    if case.family == "spike":
        # k[key] = amp / 6 * (sum of the spiking queries, in the units of test_rot_attention_deferred_rescale_is_the_exact_softmax: std 0.6); toc3d_window_attention
        # rotates q and k by their own slots, so there the sum is taken over the ROTATED queries and the key is rotated back by its slot
        amps = (4.0, 8.0) if (case.path, case.kind) == ("plain", "bf16") else (6.0, 12.0)
        for key, qs, amp in ((70, range(0, 40), amps[0]), (n - 5, range(20, 60), amps[1])):
            qi = [i for i in qs if i < n]
            if case.path == "rot":
                k[0, key] = q[0, qi].sum(0) * (amp / 6.0) * (0.6 / std)
            else:
                cs, sn = cos.double()[slots[0]][:, None, :], sin.double()[slots[0]][:, None, :]
                tgt = rope_f64(q[0, qi].double(), cs[qi], sn[qi]).sum(0) * (amp / 6.0) * (0.6 / std)
                k[0, key] = rope_f64(tgt, cs[key], -sn[key]).float()
    else:
        for w in range(nW):
            for e in edge_keys(int(nk[w])):
                v[w, e] = sign[w, e] * loud_of(int(nk[w]), int(npd[w]), case)
    big = (torch.randint(0, 2, (R, ldqkv), generator=g) * 2.0 - 1.0) * BIG
    qkv = big.clone()
    lst = own[is_q]
    qkv[lst, :3 * C] = torch.cat([q[is_q].reshape(-1, C), k[is_q].reshape(-1, C), v[is_q].reshape(-1, C)], 1)
    qkv = round_operand(case, qkv)

    pad = None
    if case.virt_q:
        npr = L * L if case.path == "rot" else 1
        pad = (torch.randint(0, 2, (npr, ldqkv), generator=g) * 2.0 - 1.0) * BIG
        pad[:, C:2 * C] = torch.randn(npr, C, generator=g)
        pad[:, 2 * C:3 * C] = torch.randn(npr, C, generator=g)
        ld = loud_of(n, 0, case)
        psign = torch.randint(0, 2, (npr, C), generator=g) * 2.0 - 1.0
        if case.path == "rot":
            pad[1:32, 2 * C:3 * C] = psign[1:32] * ld
            for w in range(nW):
                for t, e in enumerate(e for e in edge_keys(int(nk[w])) if e >= int(nq[w])):
                    slots[w, e] = 1 + t
        elif n - case.virt_q == 1:                                        # a window's ONLY pad is an edge key like any other; several pads stay quiet so that the real keys stand out
            pad[:, 2 * C:3 * C] = psign * ld
        pad = round_operand(case, pad)
    return dict(case=case, H=H, C=C, n=n, nW=nW, R=R, ldqkv=ldqkv, ldo=ldo, nq=nq, nk=nk, npad=npd, rows=rows.int(), slots=slots.int(), own=own, qkv=qkv, pad=pad,
                v_bias=torch.randn(C, generator=g).float() if case.npad else None, cos=cos.float(), sin=sin.float(), L=L, is_q=is_q,
                written=own[is_q])


def rope_f64(x, cos, sin):
    """eva_utils.py:378-379 with rotate_half over pairs (2t, 2t+1); x [..., 64]."""
    x2 = torch.stack([-x[..., 1::2], x[..., 0::2]], -1).flatten(-2)
    return x * cos + x2 * sin


def operands(b, pad_slot0=False, windows=None):
    """q [W, n, H, 64] and k in the units the kernel multiplies (rotated, q scaled), v, the factor to nats; f64."""
    case, H, C, n = b["case"], b["H"], b["C"], b["n"]
    ws = torch.arange(b["nW"]) if windows is None else torch.tensor(windows)
    rows, slots = b["rows"][ws].long(), b["slots"][ws].long()
    x = b["qkv"][rows.clamp_min(0)]
    q, k, v = (x[..., i * C:(i + 1) * C].reshape(len(ws), n, H, HD) for i in range(3))
    virt = rows < 0
    if b["pad"] is not None:
        p = b["pad"][(slots * 0 if pad_slot0 else slots) if case.path == "rot" else slots * 0]
        pk, pv = (p[..., i * C:(i + 1) * C].reshape(len(ws), n, H, HD) for i in (1, 2))
        k, v = torch.where(virt[..., None, None], pk, k), torch.where(virt[..., None, None], pv, v)
    factor = LN2
    if case.path == "plain":
        ks = torch.where(virt, slots * 0, slots) if pad_slot0 else slots
        cq, sq = b["cos"].double()[slots][:, :, None, :], b["sin"].double()[slots][:, :, None, :]
        ck, sk = b["cos"].double()[ks][:, :, None, :], b["sin"].double()[ks][:, :, None, :]
        q, k, factor = rope_f64(q, cq, sq) * PLAIN_SCALE, rope_f64(k, ck, sk), 1.0
    return ws, q, k, v, factor


def attend(b, ws, q, k, v, factor):
    """The f64 softmax attention of the windows ws with the unnormalised pieces the mutants edit: P [W, H, Q, K + 1] (column K = the npad keys), V [W, K + 1, H, 64]."""
    H, n = b["H"], b["n"]
    nk, npd = b["nk"][ws], b["npad"][ws]
    S = torch.einsum("wqhd,wkhd->whqk", q, k) * factor
    S = S.masked_fill((torch.arange(n)[None, :] >= nk[:, None])[:, None, None, :], -math.inf)
    pad_col = torch.where(npd > 0, npd.double().clamp_min(1).log(), torch.full((len(ws),), -math.inf, dtype=torch.float64))
    S = torch.cat([S, pad_col[:, None, None, None].expand(-1, H, n, 1)], -1)
    m = S.amax(-1, keepdim=True)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    P = torch.exp(S - m)
    vb = b["v_bias"].double().view(1, 1, H, HD) if b["v_bias"] is not None else torch.zeros(1, 1, H, HD, dtype=torch.float64)
    V = torch.cat([torch.nan_to_num(v, posinf=0.0, neginf=0.0).clamp(-1e30, 1e30), vb.expand(len(ws), 1, H, HD)], 1)
    V = V * (torch.cat([torch.arange(n)[None, :] < nk[:, None], npd[:, None] > 0], 1))[:, :, None, None]      # masked keys hold +-2^100: 0 * that must not reach a sum as inf - inf
    num = torch.einsum("whqk,wkhd->wqhd", P, V)
    anum = torch.einsum("whqk,wkhd->wqhd", P, V.abs())
    den = P.sum(-1).permute(0, 2, 1)[..., None]
    return P, V, num, anum, den


def reference(b, windows=None):
    ws, q, k, v, factor = operands(b, windows=windows)
    P, V, num, anum, den = attend(b, ws, q, k, v, factor)
    n = b["n"]
    valid = b["is_q"][ws]                                                       # [W, n] query rows
    keym = (torch.arange(n)[None, :] < b["nk"][ws][:, None])[:, None, None, :]
    qa, ka = q.abs().clamp(max=1e30), k.abs().clamp(max=1e30) * (torch.arange(n)[None, :] < b["nk"][ws][:, None])[:, :, None, None]
    T = (torch.einsum("wqhd,wkhd->whqk", qa, ka) * factor).masked_fill(~keym, 0.0).amax(-1).permute(0, 2, 1)
    qp, kp = qa[..., 0::2] + qa[..., 1::2], ka[..., 0::2] + ka[..., 1::2]
    Tp = (torch.einsum("wqhd,wkhd->whqk", qp, kp) * factor).masked_fill(~keym, 0.0).amax(-1).permute(0, 2, 1)
    den_ok = den.clamp_min(1e-300)
    return dict(ws=ws, q=q, k=k, v=v, factor=factor, P=P, V=V, num=num, den=den, out=num / den_ok, A=anum / den_ok, T=T, Tp=Tp, valid=valid)


# ---- bounds ----------------------------------------------------------------------------------------------------
def eps_of(case, T, Tp):
    p, kd = case.path, case.kind
    if p == "rot" and kd == "bf16":
        first, delta = 3 * 2.0 ** -8, (66 * T + 6) * U
    elif p == "rot":
        first, delta = 3 * 2.0 ** -16, 2.0 ** -16 * T + (194 * T + 6) * U
    elif kd == "bf16":
        first, delta = 3 * 2.0 ** -8, (2.0 ** -7 + 2.0 ** -16) * T + (73 * Tp + 4 * T + 12) * U
    elif kd in ("f32", "x3wo"):
        first, delta = (4 * U if kd == "f32" else 2.0 ** -16 + 4 * U), (73 * Tp + 4 * T + 12) * U
    else:
        first, delta = (3 * 2.0 ** -16 + 4 * U if kd == "x3" else 4 * 2.0 ** -16 + 4 * U), 3 * 2.0 ** -16 * T + (201 * Tp + 4 * T + 12) * U
    e = torch.expm1(delta) + 4 * U
    return first + 2 * e / (1 - e), delta


def bound(b, ref):
    """[W, n, H, 64] per-element bound (meaningful on the valid query rows)."""
    eps, _ = eps_of(b["case"], ref["T"], ref["Tp"])
    nkeys = (b["nk"][ref["ws"]] + (b["npad"][ref["ws"]] > 0)).double()[:, None, None, None]
    return (eps[..., None] + (nkeys + 8) * U) * ref["A"]


# ---- emulation of the kernels' rounding points ------------------------------------------------------------------
def emulate(b, ref):
    """The rounding points of the kernel this case runs, applied to the reference's operands: f32 scores from the operands as the MFMAs see them, unnormalised f32 P,
    the numerator from P as the MFMA operand sees it with f32 accumulation, the denominator from the f32 P, the output rounded to its buffer type."""
    case, H, n = b["case"], b["H"], b["n"]
    ws, q, k, v, factor = ref["ws"], ref["q"], ref["k"], ref["v"], ref["factor"]
    nk, npd = b["nk"][ws], b["npad"][ws]
    keym = torch.arange(n)[None, :] < nk[:, None]
    q, k, v = (torch.where(keym[:, :, None, None], t, torch.zeros_like(t)) for t in (q.clamp(-1e30, 1e30), k, v))
    dot = lambda a, c: torch.einsum("wqhd,wkhd->whqk", a, c)
    bf, x3 = case.kind == "bf16", case.kind in ("x3", "x3p")
    if case.path == "plain":
        q, k = r_f32(q), r_f32(k)                                               # the f32 RoPE and scale
    if bf:
        S = dot(r_bf16(q), r_bf16(k))
    elif x3:
        (qh, ql), (kh, kl) = split_bf16(q), split_bf16(k)
        S = dot(ql, kh) + dot(qh, kl) + dot(qh, kh)
    else:
        S = dot(q, k)
    S = r_f32(S).masked_fill(~keym[:, None, None, :], -math.inf)               # in the kernel's own units (log2 on the rot path)
    m = S.amax(-1, keepdim=True)
    m = torch.where(npd[:, None, None, None] > 0, m.clamp_min(0.0), m)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    P = r_f32(torch.exp((S - m) * factor)).float()                              # [W, H, Q, K] f32
    vf = v.permute(0, 2, 1, 3).float()                                          # [W, H, K, 64]
    if bf:
        num = P.to(TBF).float() @ vf
    elif x3:
        ph = P.to(TBF).float()
        pl = (P - ph).to(TBF).float()
        vh = vf.to(TBF).float()
        vl = (vf - vh).to(TBF).float()
        num = pl @ vh + ph @ vl + ph @ vh
    else:
        num = P @ vf
    den = P.sum(-1, keepdim=True)
    if b["v_bias"] is not None:
        padw = (npd.double()[:, None, None, None] * torch.exp(-m * factor)).float()
        num, den = num + padw * b["v_bias"].view(1, H, 1, HD), den + padw
    out = (num / den.clamp_min(1e-30)).permute(0, 2, 1, 3)
    if bf:
        return r_bf16(out)
    if case.kind in ("x3p", "x3wo"):
        return r_planes(out)
    return out.double()


# ---- wrong references ------------------------------------------------------------------------------------------------
def _edit(ref, sub=(), add=()):
    """out with unnormalised columns taken out / put in: each item (p [W, H, Q], v [W, H, 64])."""
    num, den = ref["num"].clone(), ref["den"].clone()
    for sgn, items in ((-1.0, sub), (1.0, add)):
        for p, v in items:
            num += sgn * p.permute(0, 2, 1)[..., None] * v[:, None]
            den += sgn * p.permute(0, 2, 1)[..., None]
    return num / den.clamp_min(1e-300)


def _col(ref, idx):
    """Column idx[w] of P and V per window."""
    W = idx.shape[0]
    ar = torch.arange(W)
    return ref["P"][ar, :, :, idx], ref["V"][ar, idx]


def mutants(b, ref):
    """Yield (name, wrong out [W, n, H, 64], affected [W] bool, rows or None): rows = [(window, row)] when only those rows are affected."""
    case, n, nW, H = b["case"], b["n"], b["nW"], b["H"]
    nq, nk, npd = b["nq"], b["nk"], b["npad"]
    live = nq > 0
    zero = torch.zeros(nW, dtype=torch.long)
    padcol = torch.full((nW,), n, dtype=torch.long)
    nvirt = nk - nq
    if case.family == "flat":
        for kind, offs in (("abs", EDGE_ABS), ("rel", EDGE_REL)):
            for o in offs:
                e = torch.full((nW,), o, dtype=torch.long) if kind == "abs" else nk + o
                has = live & (e >= 0) & (e < nk) & ((nk + npd) >= 2)
                if kind == "rel":                                               # an absolute edge that coincides is the same mutant
                    has &= ~torch.isin(e, torch.tensor(EDGE_ABS))
                if case.path == "plain" and case.virt_q:
                    has &= (e < nq) | (nvirt == 1)
                if not bool(has.any()):
                    continue
                p, v = _col(ref, torch.where(has, e, zero))
                p = p * has[:, None, None]
                yield f"a:drop key {o}" + ("" if kind == "abs" else " from the end"), _edit(ref, sub=[(p, v)]), has, None
        has = live & (nk >= 2)
        if bool(has.any()):
            (p0, v0), (pl, vl) = _col(ref, zero), _col(ref, torch.where(has, nk - 1, zero))
            out = _edit(ref, sub=[(pl * has[:, None, None], vl)], add=[(p0 * has[:, None, None], v0)])
            yield "b:key 0 for the last key", out, has, None
        has = live & (npd > 0) & (nk > 0)
        if bool(has.any()):
            pp, vp = _col(ref, padcol)
            out = _edit(ref, sub=[(pp * has[:, None, None], vp)])
            yield "c:npad term omitted", out, has, None
        has = live & (npd > 1)
        if bool(has.any()):
            pp, vp = _col(ref, padcol)
            out = _edit(ref, sub=[(pp * (has * (1 - 1 / npd.double().clamp_min(1)))[:, None, None], vp)])
            yield "d:npad keys counted once", out, has, None
        if case.virt_q:
            has = live & (nvirt > 0) if case.path == "rot" else live & (nvirt == 1) & (case.kind != "bf16")
            if bool(has.any()):
                ws, q, k, v, f = operands(b, pad_slot0=True)
                _, _, num, _, den = attend(b, ws, q, k, v, f)
                yield "f:pad keys from slot 0", num / den.clamp_min(1e-300), has, None
    if H >= 2:
        for name, kk, vv in (("e:v of the neighbouring head", ref["k"], ref["v"].roll(1, 2)), ("e:k of the neighbouring head", ref["k"].roll(1, 2), ref["v"])):
            has = live & ((nk + npd) >= 2) & ((nvirt <= 1) | (case.path == "rot")) if name.startswith("e:k") else live
            if name.startswith("e:k") and case.neg:
                continue                                                        # k' = -|k| in every head: a neighbour's k gives nearly the same scores by construction
            if (case.path, case.kind, case.family) == ("plain", "bf16", "spike"):
                # T of EVERY row of window 0 is the spike key's (~25 nats: the key is a sum over 40 queries), so 2 x the bound of the bf16 form is ~0.9 A there and only
                # the 60 spiking rows of n can move that far; windows 1 and 2 carry the condition
                has = has & (torch.arange(nW) > 0)
            _, _, num, _, den = attend(b, ref["ws"], ref["q"], kk, vv, ref["factor"])
            yield name, num / den.clamp_min(1e-300), has, None
    cand = [w for w in range(nW) if int(nq[w]) >= 2 and int(nk[w] + npd[w]) >= 2]
    if cand and not case.neg:                                                   # (neg: q' = c |q| in every row, a neighbour's q gives nearly the same scores by construction)
        w0 = cand[0]
        i = 20 if case.family == "spike" else min(int(nq[w0]) - 1, 37)      # spike: row 19 follows key 70, row 20 key n - 5
        ws, q, k, v, f = operands(b, windows=[w0])
        q = q.clone()
        q[0, i] = q[0, i - 1]
        _, _, num, _, den = attend(b, ws, q, k, v, f)
        out = ref["out"].clone()
        out[w0, i] = (num / den.clamp_min(1e-300))[0, i]
        has = torch.zeros(nW, dtype=torch.bool)
        has[w0] = True
        yield "g:previous row's q", out, has, [(w0, i)]


# ---- the cases ---------------------------------------------------------------------------------------------------
KEY_COUNTS = {
    ("rot", "bf16"): (1, 9, 31, 32, 33, 64, 65, 129, 255, 256, 257, 401, 416),
    ("rot", "x3p"): (1, 17, 32, 33, 129, 257, 288, 289, 384, 385, 401, 640),
}
SMALL_N = (1, 15, 16, 17, 33, 143, 144, 145, 160, 161, 176, 177, 207, 208)      # 160 | 161: where the f32 buffers leave the small kernel (LDS)
FLASH_N = (209, 255, 256, 257, 320, 321, 401)
# F32X3 and F32X3WO: both ends of every body's range (for the f32 buffers <9> ends at 144, <11> is 145..160, the flash kernel starts at 161) and of the table's ranges
SUBSET_N = (1, 144, 145, 160, 161, 176, 177, 208, 209, 401)
NPADS = ((8, 248), (32, 224), (96, 160), (40, 360))
RAGGED_BIG = {("rot", "bf16"): (401,), ("rot", "x3p"): (257, 401), ("plain", None): (143, 160, 207, 321)}
VIRT_K = {("rot", "bf16"): (33, 97, 241), ("rot", "x3p"): (33, 97, 321), ("plain", None): (33, 97, 241)}


def _kinds():
    return [("rot", "bf16"), ("rot", "x3p")] + [("plain", kd) for kd in PLAIN_KINDS]


def _all_cases():
    out = []
    for path, kd in _kinds():
        tag = f"{path}-{kd}"
        ns = KEY_COUNTS.get((path, kd)) or (SUBSET_N if kd in ("x3", "x3wo") else SMALL_N + FLASH_N)
        scat = {33, 257, 401, 640, 144, 208}
        for n in ns:
            # (640 keys: the entry point takes 512 queries at most, so the last 128 keys are virtual pads)
            out.append(Case(f"{tag}-n{n}", path, kd, n, nwin=2 if n > 300 else 3, scattered=n in scat, virt_q=512 if n == 640 else 0))
        rag = RAGGED_BIG.get((path, kd)) or RAGGED_BIG[("plain", None)]
        for n in (33,) + rag:
            out.append(Case(f"{tag}-ragged-n{n}", path, kd, n, counts=(n, 1, n - 1, (n + 1) // 2, 0), nwin=5, scattered=n == 33))
        for nkk in VIRT_K.get((path, kd)) or VIRT_K[("plain", None)]:
            for cq in (1, nkk - 1):
                out.append(Case(f"{tag}-virt-k{nkk}-q{cq}", path, kd, nkk, virt_q=cq, nwin=3, scattered=nkk == 97))
        for n, npad in NPADS + (((300, 100),) if path == "plain" else ()):      # (300, 100): the flash kernel's own npad epilogue (the table's four all fit the small kernel)
            out.append(Case(f"{tag}-npad-n{n}-p{npad}", path, kd, n, npad=npad, nwin=3, counts=(n, max(n - 7, 1), n) if npad == 248 else None))
        # all scores below the pads' 0: the reference point never moves off its start (attn_rot kernels: no rescale even in the first chunk; flash: m < 0 in the epilogue)
        for n, npad in ((96, 160),) + (((300, 100),) if path == "plain" else ((33, 223),)):
            out.append(Case(f"{tag}-npadneg-n{n}-p{npad}", path, kd, n, npad=npad, nwin=3, neg=True))
        if path == "rot":
            for nwin in (4, 17, 49):
                for n in (40, 129):
                    out.append(Case(f"{tag}-grid-w{nwin}-n{n}", path, kd, n, nwin=nwin, heads=16))
        # once per body: rot 129 / 256 / 400 (<false>, <false>, <true> on planes); the other entry point <9> at 129, <11> at 160, <13> (bf16) at 201, flash at 400
        for n in (129, 256, 400) if path == "rot" else (129, 160, 400) if kd in ("x3", "x3wo") else (129, 160, 201, 400):
            out.append(Case(f"{tag}-spike-n{n}", path, kd, n, family="spike", nwin=3))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


CASES = _all_cases()


# ---- RoPE helpers of the pre-rotated path (test_gpu_attn_rot.py, test_gpu_epilogue_tails.py) -----------------------------------------------------------------
def compact_tables(cos, sin):
    """[L*L, 64] reference buffers -> the [2, L, 16] tables toc3d_linear_qkv_rope consumes (what backbone._pack_blocks builds)."""
    L = int(round(cos.shape[0] ** 0.5))
    out = []
    for t in (cos, sin):
        g = t.view(L, L, 64)
        out.append(torch.stack([g[:, 0, 0:32:2], g[0, :, 32:64:2]]))
    return torch.stack(out).contiguous().to(DEV), L


def rc_of(slots, L):
    return (((slots // L) << 16) | (slots % L)).to(torch.int32).contiguous().to(DEV)


def rope_ref(x, cos, sin):
    """eva_utils.py:378-379 with rotate_half over pairs (2t, 2t+1); x [..., 64], cos / sin broadcastable."""
    x2 = torch.stack([-x[..., 1::2], x[..., 0::2]], -1).flatten(-2)
    return x * cos + x2 * sin
