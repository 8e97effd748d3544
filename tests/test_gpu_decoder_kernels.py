"""GPU: the decoder's kernels (csrc/mha.hip, toc3d_relu_inplace) one by one against plain f64 references, at the layouts, logit profiles and row / lane tails
the module tests (tests/test_gpu_decoder.py) never reach, and the module itself at sizes with a tail in every dimension.

1. toc3d_mha_attention_ex on the operand layouts of decoder.py:_frame: q and k as column ranges of one fused [rows, 2W] buffer, keys / values as layer l's W
   columns of [rows, L * W] buffers, two key segments whose boundary and end fall anywhere against the 32-key chunk and the 8-wave split, `out` with ldo > W.
   Everything around the operands holds a sentinel (2^15: finite, and ruinous if read as data).
2. The streamed softmax on logit profiles a Gaussian never produces.  Operands are multiples of 2^-3 of magnitude <= 32: exact in bf16, every 32-term dot product
   exact in f32, so both precisions and the f64 reference see the same logits and what is left is exp2, the rescale, the rounding of P and the merge.
   Per element, with ref = softmax(q.k^T / sqrt(32)).v and A = softmax(...).|v| in f64:  |out - ref| <= bound * A + 1e-30, bound = 2 * 2^-8 (bf16: P and the
   output are each rounded once to bf16, unit roundoff 2^-8, each worth at most 2^-8 * A; f32 accumulation and the exp2 argument are two orders below) and 1e-4
   (fp32x3: the project's per-op budget, tests/test_gpu_decoder.py::test_mha_attention_against_f64).  The floor covers entries where every contributing v is 0
   up to terms below 2^-126, which f32 flushes and f64 keeps.
3. toc3d_add_layernorm_pos / toc3d_add_pos_rows / toc3d_relu_inplace: lane tails (E not a multiple of 64), the last workgroup of four rows partly filled, every
   combination of the optional outputs, leading dimensions all different and larger than E with sentinels in the padding, both act dtypes.  f32 outputs against the f64
   LayerNorm of tests/support.py at the project's 2e-5 (tests/test_gpu_ops.py::test_layernorm_rows), bf16 act outputs bit-equal to torch's RNE rounding of
   the kernel's own f32 result.  Offsets stop at 16 and are left out below E = 63: an f32 LayerNorm itself is outside 2e-5 at offset 1000 or at E = 2 with an offset.
4. PETRTemporalTransformer at E 128 / F 1024 (split-K FFN at a width that is not 256) and E 192 / F 320 with B 2, 45 queries, 19 memory rows, 333 tokens.

Worst figures measured on MI355X (profiles/decoder_parity.txt, section "kernels one by one"); the asserted bounds are the derived ones above, not these:
   softmax families, worst ratio to the bound over the key counts (fp32x3 / bf16): ramp 0.13 / 0.50, split_ramp 0.13 / 0.76, saw 0.07 / 0.63, late spike 0.001 / 0,
   early spike 0.001 / 0, uniform 0 / 0.13, all negative 0.07 / 0.49, wide 0.08 / 0.66; spikes in the second segment 0.001 / 0; through strided views: ramp 0.15 / 0.50,
   wide 0.07 / 0.49, late spike 0.001 / 0.  Gaussian operands on the decoder's layouts: 0.30 / 0.60 (global rel max err 2.0e-5 / 3.2e-3).
   toc3d_add_layernorm_pos, worst rel max err of out / out2 over all widths: gaussian 1.6e-7 / 1.9e-7, offset 16 6.3e-7 / 1.7e-7, scale 1e-3 1.2e-7 / 1.8e-7,
   scale 1e3 1.6e-7 / 1.8e-7, constant rows 0 / 1.4e-7; bf16 act_pos <= 3.5e-3 (one bf16 rounding).
   The module: fp32x3 <= 2.1e-5 on every layer and intermediate at both sizes; bf16 relative L2 8.3e-3 / 8.5e-3 / 8.0e-3 / 7.5e-3 next to the control's
   8.5e-3 / 8.4e-3 / 7.9e-3 / 7.5e-3 (E 128 with / without temp_memory, E 192 with / without).
Left out for run time: the full cross product of part 1's axes (every value of B, H, Nq and every listed (Nk, Nk2) pair appears at least once; see _LAYOUT_CASES)."""
import pytest
import torch

import toc3d_amd  # noqa: F401
from decoder_cases import _heads, build, restated_decoder, run
from support import DEV, layer_norm, rel_l2, rel_max
from toc3d_amd import lib, synth

pytestmark = pytest.mark.gpu
SENT = 32768.0                              # exact in bf16 and f32
PRECISIONS = [("fp32x3", lib.F32X3, torch.float32), ("bf16", lib.BF16, torch.bfloat16)]
ACT_DTYPES = [("f32", lib.F32, torch.float32), ("bf16", lib.BF16, torch.bfloat16)]
BOUND = {"fp32x3": 1e-4, "bf16": 2 * 2.0 ** -8}
FLOOR = 1e-30


def _ref_and_scale(q, k, v, H):
    """f64: softmax(q.k^T / sqrt(32)).v and softmax(...).|v|, both [B, Nq, W]."""
    qh, kh, vh = (_heads(t.double(), H) for t in (q, k, v))
    p = torch.softmax(qh @ kh.transpose(-1, -2) * 32 ** -0.5, -1)
    back = lambda t: t.transpose(1, 2).reshape(q.shape)
    return back(p @ vh), back(p @ vh.abs())


def _ratio(out, ref, A, bound):
    """max over elements of (|out - ref| - floor)+ / (bound * A): <= 1 is the assertion |out - ref| <= bound * A + floor (an excess over A = 0 counts as inf)."""
    excess = ((out.double() - ref).abs() - FLOOR).clamp_min(0)
    r = torch.where(excess > 0, excess / (bound * A), torch.zeros_like(excess))
    return r.max().item()


def _mha(dt, q, ldq, k, ldk, v, ldv, k2, ldk2, v2, ldv2, out, ldo, B, Nq, Nk, Nk2, H):
    lib.call("toc3d_mha_attention_ex", dt, q, ldq, k, ldk, v, ldv, k2, ldk2, v2, ldv2, out, ldo, B, Nq, Nk, Nk2, H, 32, 32 ** -0.5, lib.stream_ptr())


class _Cols:
    """`data` [rows, cols] as columns [col0, col0 + cols) of a [rows + 2, width] buffer filled with the sentinel: .ptr / .ld are what the kernel is given."""
    def __init__(self, data, width, col0, buf=None):
        rows, cols = data.shape
        self.buf = torch.full((rows + 2, width), SENT, dtype=data.dtype, device=DEV) if buf is None else buf
        self.buf[:rows, col0:col0 + cols] = data
        self.ptr, self.ld = self.buf.data_ptr() + col0 * self.buf.element_size(), width


class _Out:
    """[rows, W] at row 1, column 8 of a [rows + 2, W + 16] sentinel buffer (ldo = W + 16)."""
    def __init__(self, rows, W, tdt):
        self.buf = torch.full((rows + 2, W + 16), SENT, dtype=tdt, device=DEV)
        self.rows, self.W, self.ld = rows, W, W + 16
        self.ptr = self.buf.data_ptr() + (self.ld + 8) * self.buf.element_size()

    def result(self):
        torch.cuda.synchronize()
        inside = torch.zeros_like(self.buf, dtype=torch.bool)
        inside[1:1 + self.rows, 8:8 + self.W] = True
        assert bool((self.buf[~inside] == SENT).all()), "the kernel wrote outside [rows, W] of out"
        return self.buf[1:1 + self.rows, 8:8 + self.W].clone()


def _strided_attention(form, dt, q, k1, v1, k2, v2, H, l, L=3):
    """One launch on the decoder's layouts.  q [B, Nq, W]; k1 / v1 [B, Nk, W] or None; k2 / v2 [B, Nk2, W] or None.
    form "self": q | k1 fused in one [rows, 2W] buffer, v1 on its own with ld = W, (k2, v2) = layer l's columns of [B * Nk2, L * W] buffers.
    form "cross": q on its own, (k1, v1) = layer l's columns of [B * Nk, L * W] buffers, no second segment."""
    B, Nq, W = q.shape
    flat = lambda t: t.reshape(-1, W)
    Nk, Nk2 = (0 if k1 is None else k1.shape[1]), (0 if k2 is None else k2.shape[1])
    if form == "self":
        fused = torch.full((B * max(Nq, Nk) + 2, 2 * W), SENT, dtype=q.dtype, device=DEV)
        Q = _Cols(flat(q), 2 * W, 0, fused)
        K1 = _Cols(flat(k1), 2 * W, W, fused) if Nk else None
        V1 = _Cols(flat(v1), W, 0) if Nk else None
        K2 = _Cols(flat(k2), L * W, l * W) if Nk2 else None
        V2 = _Cols(flat(v2), L * W, l * W) if Nk2 else None
    else:
        assert Nk2 == 0
        Q = _Cols(flat(q), W, 0)
        K1, V1, K2, V2 = _Cols(flat(k1), L * W, l * W), _Cols(flat(v1), L * W, l * W), None, None
    p = lambda c: (None, 0) if c is None else (c.ptr, c.ld)
    out = _Out(B * Nq, W, q.dtype)
    _mha(dt, *p(Q), *p(K1), *p(V1), *p(K2), *p(V2), out.ptr, out.ld, B, Nq, Nk, Nk2, H)
    return out.result().view(B, Nq, W)


def _contiguous_attention(dt, q, k, v, H):
    B, Nq, W = q.shape
    out = torch.empty(B * Nq, W, dtype=q.dtype, device=DEV)
    _mha(dt, q.contiguous(), W, k.contiguous(), W, v.contiguous(), W, None, 0, None, 0, out, W, B, Nq, k.shape[1], 0, H)
    torch.cuda.synchronize()
    return out.view(B, Nq, W)


# ---- 1. layouts ---------------------------------------------------------------------------------------------------------------------
# (form, B, H, Nq, Nk, Nk2, layer): every B in {1, 3}, H in {1, 2, 8}, Nq in {1, 31, 32, 33, 45}; (Nk, Nk2) put the segment boundary and the end of the key list
# before, on and after a chunk boundary, and the last chunk on wave 0 (255, 256 keys: chunk 7 is wave 7's; 257: chunk 8 is wave 0's second) or another wave.
_LAYOUT_CASES = [
    ("self", 1, 1, 1, 1, 0, 0), ("self", 3, 2, 31, 0, 1, 2), ("self", 1, 8, 32, 0, 40, 0), ("self", 3, 1, 33, 31, 1, 2), ("self", 1, 2, 45, 32, 32, 0),
    ("self", 3, 8, 1, 33, 222, 2), ("self", 1, 1, 31, 45, 211, 0), ("self", 3, 2, 32, 45, 212, 2), ("self", 3, 8, 45, 45, 19, 0), ("self", 1, 2, 45, 45, 19, 2),
    ("self", 1, 8, 45, 900, 768, 2), ("self", 3, 1, 33, 900, 768, 0),
    ("cross", 1, 1, 45, 1, 0, 0), ("cross", 3, 8, 33, 333, 0, 2), ("cross", 1, 2, 31, 257, 0, 0), ("cross", 3, 1, 1, 6001, 0, 2), ("cross", 1, 8, 32, 255, 0, 2),
]


@pytest.mark.parametrize("precision,dt,tdt", PRECISIONS)
@pytest.mark.parametrize("form,B,H,Nq,Nk,Nk2,l", _LAYOUT_CASES)
def test_mha_on_the_decoder_layouts(form, B, H, Nq, Nk, Nk2, l, precision, dt, tdt):
    g = torch.Generator().manual_seed(1000 * Nq + 10 * Nk + Nk2 + B + H)
    W = H * 32
    mk = lambda n, s: (torch.randn(B, n, W, generator=g) * s).to(DEV).to(tdt) if n else None
    q, k1, k2, v1, v2 = mk(Nq, 1.5), mk(Nk, 1.5), mk(Nk2, 1.5), mk(Nk, 1.0), mk(Nk2, 1.0)
    k = torch.cat([t for t in (k1, k2) if t is not None], 1)
    v = torch.cat([t for t in (v1, v2) if t is not None], 1)
    ref, A = _ref_and_scale(q, k, v, H)
    out = _strided_attention(form, dt, q, k1, v1, k2, v2, H, l)
    again = _strided_attention(form, dt, q, k1, v1, k2, v2, H, l)
    assert torch.equal(out, again), "two launches differ"
    assert torch.equal(out, _contiguous_attention(dt, q, k, v, H)), "strided / two-segment operands and one contiguous key list differ"
    assert bool(torch.isfinite(out).all())
    ratio, err = _ratio(out, ref, A, BOUND[precision]), rel_max(out, ref)
    print(f"[mha layout {form} {precision} B={B} H={H} Nq={Nq} Nk={Nk}+{Nk2} l={l}] ratio to the bound {ratio:.3f}   rel max err {err:.2e}")
    assert ratio <= 1.0
    if precision == "fp32x3":
        assert err < 1e-4


# ---- 2. softmax profiles ------------------------------------------------------------------------------------------------------------
def _grid(g, shape, lo, hi, step=0.125):
    return torch.randint(int(lo / step), int(hi / step) + 1, shape, generator=g).float() * step


FAMILIES = ("ramp", "split_ramp", "saw", "late_spike", "early_spike", "uniform", "all_negative", "wide")


def _family(name, B, H, Nq, N, spike=None, seed=0):
    """q [B, Nq, W], k, v [B, N, W] f32 on the 2^-3 grid.  Per head q_i = [2 x 16 | +-1 x 16], k_j = [m_j x 16 | grid in +-2]: the logit of key j is
    32 m_j / sqrt(32) (4.08 log2 units per unit of m) for every query, plus a per-query part from the random halves.  `spike` = key index of the spike families."""
    g = torch.Generator().manual_seed(seed + N)
    j = torch.arange(N).float()
    if name in ("ramp", "split_ramp"):
        m = torch.floor(j * (64.0 / max(N - 1, 1)) * 8) / 8 - 32
    elif name == "saw":
        m = ((j % 32) - 16) * (1 + (j // 32) % 3) * 0.5
    elif name in ("late_spike", "early_spike"):
        m = torch.zeros(N)
        m[(N - 1 if name == "late_spike" else 0) if spike is None else spike] = 16.0          # 130.6 log2 units above the rest
    elif name == "uniform":
        m = torch.zeros(N)
    elif name == "all_negative":
        m = -24 + _grid(g, (N,), -1, 1)
    elif name == "wide":
        m = _grid(g, (N,), -24, 24)
    q = torch.cat([torch.full((B, Nq, H, 16), 2.0), torch.randint(0, 2, (B, Nq, H, 16), generator=g).float() * 2 - 1], -1)
    if name == "uniform":
        q = torch.zeros_like(q)
    if name == "split_ramp":                # every other query sees the ramp falling: in every chunk the maximum moves for half of a wavefront's queries only --
        q[:, 1::2, :, :16] *= -1            # the rescale has to happen when ANY lane's maximum moved (in the other families all queries' maxima move together)
    k = torch.cat([m[None, :, None, None].expand(B, N, H, 16), _grid(g, (B, N, H, 16), -2, 2)], -1)
    v = _grid(g, (B, N, H, 32), -4, 4)
    for t in (q, k, v):
        assert bool((t.abs() <= 32).all()) and torch.equal(t, (t * 8).round() / 8) and torch.equal(t, t.bfloat16().float())
    return tuple(t.reshape(B, -1, H * 32).to(DEV) for t in (q, k, v))


def _check_profile(tag, precision, out, q, k, v, H):
    ref, A = _ref_and_scale(q, k, v, H)
    finite = bool(torch.isfinite(out).all())
    ratio = _ratio(out, ref, A, BOUND[precision]) if finite else float("inf")
    print(f"[softmax {tag} {precision}] worst ratio to the bound {ratio:.3f}")
    assert finite, "non-finite output"
    assert ratio <= 1.0


@pytest.mark.parametrize("precision,dt,tdt", PRECISIONS)
@pytest.mark.parametrize("N", [1, 31, 257, 1668, 6001])
@pytest.mark.parametrize("name", FAMILIES)
def test_softmax_profiles(name, N, precision, dt, tdt):
    B, H, Nq = 2, 2, 33
    q, k, v = _family(name, B, H, Nq, N)
    out = _contiguous_attention(dt, q.to(tdt), k.to(tdt), v.to(tdt), H)
    assert torch.equal(out, _contiguous_attention(dt, q.to(tdt), k.to(tdt), v.to(tdt), H)), "two launches differ"
    if name == "uniform":                   # all logits equal: the plain mean of v (the per-element bound below says the same; this one is independent of A)
        mean = v.double().view(B, N, -1).mean(1, keepdim=True).expand(B, Nq, H * 32)
        assert (out.double() - mean).abs().max().item() <= BOUND[precision] * 4.0
    _check_profile(f"{name} Nk={N}", precision, out, q, k, v, H)


@pytest.mark.parametrize("precision,dt,tdt", PRECISIONS)
@pytest.mark.parametrize("Nk,Nk2", [(45, 212), (900, 768)])
@pytest.mark.parametrize("name", ["late_spike", "early_spike"])
def test_softmax_spike_in_the_second_segment(name, Nk, Nk2, precision, dt, tdt):
    """The dominant key is the last (late) or the first (early) row of the SECOND buffer."""
    B, H, Nq, N = 2, 2, 33, Nk + Nk2
    q, k, v = _family(name, B, H, Nq, N, spike=N - 1 if name == "late_spike" else Nk)
    c = lambda t: t.to(tdt).contiguous()
    W = H * 32
    out = torch.empty(B * Nq, W, dtype=tdt, device=DEV)
    k1, k2, v1, v2 = c(k[:, :Nk]), c(k[:, Nk:]), c(v[:, :Nk]), c(v[:, Nk:])
    _mha(dt, c(q), W, k1, W, v1, W, k2, W, v2, W, out, W, B, Nq, Nk, Nk2, H)
    torch.cuda.synchronize()
    out = out.view(B, Nq, W)
    assert torch.equal(out, _contiguous_attention(dt, c(q), c(k), c(v), H)), "two segments and one buffer differ"
    _check_profile(f"{name} in segment 2 Nk={Nk}+{Nk2}", precision, out, q, k, v, H)


@pytest.mark.parametrize("precision,dt,tdt", PRECISIONS)
@pytest.mark.parametrize("name,form,Nk,Nk2", [("ramp", "self", 45, 212), ("wide", "cross", 257, 0), ("late_spike", "self", 33, 222)])
def test_softmax_profiles_through_strided_views(name, form, Nk, Nk2, precision, dt, tdt):
    B, H, Nq = 3, 2, 45
    q, k, v = _family(name, B, H, Nq, Nk + Nk2)
    c = lambda t: t.to(tdt) if t.shape[1] else None
    out = _strided_attention(form, dt, q.to(tdt), c(k[:, :Nk]), c(v[:, :Nk]), c(k[:, Nk:]), c(v[:, Nk:]), H, l=1)
    assert torch.equal(out, _contiguous_attention(dt, q.to(tdt), k.to(tdt), v.to(tdt), H))
    _check_profile(f"{name} strided {form} Nk={Nk}+{Nk2}", precision, out, q, k, v, H)


# ---- 3. row kernels -----------------------------------------------------------------------------------------------------------------
class _Rows:
    """An [M, E] operand or result inside an [M + 2, ld] sentinel buffer."""
    def __init__(self, M, E, ld, tdt, data=None):
        self.buf = torch.full((M + 2, ld), SENT, dtype=tdt, device=DEV)
        self.M, self.E, self.ld = M, E, ld
        if data is not None:
            self.buf[:M, :E] = data
        self.before = self.buf.clone()

    def value(self):
        assert bool((self.buf[self.M:] == SENT).all()) and bool((self.buf[:, self.E:] == SENT).all()), "written past [M, E]"
        return self.buf[:self.M, :self.E]

    def unchanged(self):
        return torch.equal(self.buf, self.before)


def _ln_inputs(family, M, E, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    if family == "gaussian":
        x = r(M, E)
    elif family == "offset16":
        x = r(M, E) + 16.0
    elif family == "tiny":
        x = r(M, E) * 1e-3                     # variance 1e-6, below eps
    elif family == "large":
        x = r(M, E) * 1e3
    elif family == "constant":                 # multiples of 1/4 up to 8: the row sum (<= 8192) and the mean are exact in f32, so x - mean is exactly 0
        x = (torch.randint(-32, 33, (M, 1), generator=g).float() / 4).expand(M, E).clone()
    return x.to(DEV), (1 + 0.1 * r(E)).to(DEV), (0.1 * r(E)).to(DEV), (1 + 0.1 * r(E)).to(DEV), (0.1 * r(E)).to(DEV), r(M, E).to(DEV)


def _run_add_ln_pos(dt, tdt, x, g1, b1, g2, b2, pos, want_act, want_pos, want_out2, eps=1e-5):
    """One launch with all leading dimensions different and larger than E; returns (out, act, act_pos, out2) (absent: None) after the sentinel checks."""
    M, E = x.shape
    X, P = _Rows(M, E, E + 3, torch.float32, x), _Rows(M, E, E + 5, torch.float32, pos)
    O, O2 = _Rows(M, E, E + 1, torch.float32), _Rows(M, E, E + 9, torch.float32)
    Ac, Ap = _Rows(M, E, E + 7, tdt), _Rows(M, E, E + 2, tdt)
    opt = lambda on, r: (r.buf if on else None, r.ld)
    consts = [t.clone() for t in (g1, b1, g2, b2)]
    lib.call("toc3d_add_layernorm_pos", dt, X.buf, X.ld, g1, b1, eps, P.buf if want_pos else None, P.ld, O.buf, O.ld, *opt(want_act, Ac), *opt(want_pos, Ap),
             g2 if want_out2 else None, b2 if want_out2 else None, *opt(want_out2, O2), M, E, lib.stream_ptr())
    torch.cuda.synchronize()
    assert X.unchanged() and P.unchanged() and all(torch.equal(a, b) for a, b in zip(consts, (g1, b1, g2, b2))), "an input was written"
    for on, r in ((want_act, Ac), (want_pos, Ap), (want_out2, O2)):
        assert on or r.unchanged()
    return O.value(), Ac.value() if want_act else None, Ap.value() if want_pos else None, O2.value() if want_out2 else None


def _check_add_ln_pos(tag, tdt, x, g1, b1, g2, b2, pos, res, worst):
    out, act, act_pos, out2 = res
    ref = layer_norm(x.double(), g1.double(), b1.double())
    e1 = rel_max(out, ref)
    worst["out"] = max(worst.get("out", 0.0), e1)
    assert e1 < 2e-5, (tag, "out", e1)
    if out2 is not None:
        e2 = rel_max(out2, layer_norm(ref, g2.double(), b2.double()))
        worst["out2"] = max(worst.get("out2", 0.0), e2)
        assert e2 < 2e-5, (tag, "out2", e2)
    # act outputs: the rounding (bf16: RNE; f32: none) of the kernel's own f32 result, bit for bit -- and with it inside the project's 5e-3 / 2e-5 of f64
    if act is not None:
        assert torch.equal(act, out.to(tdt)), (tag, "act")
    if act_pos is not None:
        assert torch.equal(act_pos, (out + pos).to(tdt)), (tag, "act_pos")
        e3 = rel_max(act_pos, ref + pos.double())
        worst["act_pos"] = max(worst.get("act_pos", 0.0), e3)
        assert e3 < (2e-5 if tdt == torch.float32 else 5e-3), (tag, "act_pos", e3)


@pytest.mark.parametrize("name,dt,tdt", ACT_DTYPES)
@pytest.mark.parametrize("M", [1, 3, 4, 5, 203])
@pytest.mark.parametrize("E", [1, 63, 64, 65, 255, 256, 257, 1000, 1024])
def test_add_layernorm_pos_every_output_combination(E, M, name, dt, tdt):
    """All eight present / absent combinations of (act, act_pos, out2) -- the decoder issues four of them: act_pos only, act only, all three, out2 only."""
    x, g1, b1, g2, b2, pos = _ln_inputs("gaussian", M, E, seed=E * 7 + M)
    worst = {}
    for combo in range(8):
        wa, wp, w2 = bool(combo & 1), bool(combo & 2), bool(combo & 4)
        res = _run_add_ln_pos(dt, tdt, x, g1, b1, g2, b2, pos, wa, wp, w2)
        _check_add_ln_pos(f"E={E} M={M} {name} act={wa} act_pos={wp} out2={w2}", tdt, x, g1, b1, g2, b2, pos, res, worst)
    print(f"[add_layernorm_pos gaussian {name} E={E} M={M}] worst rel max err " + "  ".join(f"{k} {v:.2e}" for k, v in sorted(worst.items())))


@pytest.mark.parametrize("name,dt,tdt", ACT_DTYPES)
@pytest.mark.parametrize("E", [1, 63, 64, 65, 255, 256, 257, 1000, 1024])
@pytest.mark.parametrize("family", ["offset16", "tiny", "large", "constant"])
def test_add_layernorm_pos_input_families(family, E, name, dt, tdt):
    if family == "offset16" and E < 63:
        family = "gaussian"                    # an f32 LayerNorm of a few entries with a common offset is itself outside 2e-5 (module docstring)
    M = 5
    x, g1, b1, g2, b2, pos = _ln_inputs(family, M, E, seed=E + 100)
    worst = {}
    res = _run_add_ln_pos(dt, tdt, x, g1, b1, g2, b2, pos, True, True, True)
    _check_add_ln_pos(f"{family} E={E} {name}", tdt, x, g1, b1, g2, b2, pos, res, worst)
    if family == "constant" or E == 1:         # variance 0: the output is beta exactly
        assert torch.equal(res[0], b1[None].expand(M, E)), "LayerNorm of a constant row is not beta"
    print(f"[add_layernorm_pos {family} {name} E={E}] worst rel max err " + "  ".join(f"{k} {v:.2e}" for k, v in sorted(worst.items())))


@pytest.mark.parametrize("name,dt,tdt", ACT_DTYPES)
@pytest.mark.parametrize("mode", ["act", "act_pos", "both"])
@pytest.mark.parametrize("M,E", [(1, 1), (3, 65), (5, 257), (7, 64), (203, 1000), (4, 1025)])
def test_add_pos_rows_bit_exact(M, E, mode, name, dt, tdt):
    assert (M * E) % 256
    g = torch.Generator().manual_seed(M + E)
    x, pos = torch.randn(M, E, generator=g).to(DEV) * 3, torch.randn(M, E, generator=g).to(DEV)
    X, P, Ac, Ap = _Rows(M, E, E + 3, torch.float32, x), _Rows(M, E, E + 5, torch.float32, pos), _Rows(M, E, E + 7, tdt), _Rows(M, E, E + 2, tdt)
    wa, wp = mode != "act_pos", mode != "act"
    lib.call("toc3d_add_pos_rows", dt, X.buf, X.ld, P.buf if wp else None, P.ld, Ac.buf if wa else None, Ac.ld, Ap.buf if wp else None, Ap.ld, M, E, lib.stream_ptr())
    torch.cuda.synchronize()
    assert X.unchanged() and P.unchanged()
    assert torch.equal(Ac.value(), x.to(tdt)) if wa else Ac.unchanged()
    assert torch.equal(Ap.value(), (x + pos).to(tdt)) if wp else Ap.unchanged()


@pytest.mark.parametrize("name,dt,tdt", ACT_DTYPES)
@pytest.mark.parametrize("n", [1, 255, 257, 1000, 203 * 320 + 1])
def test_relu_inplace_bit_exact(n, name, dt, tdt):
    g = torch.Generator().manual_seed(n)
    x = (torch.randn(n + 7, generator=g) * 4).to(tdt)
    x[0], x[n - 1] = -0.0, -1.5
    if n > 4:
        x[1], x[2], x[3] = 0.0, -0.0, 2.5
    x[n:] = -3.0                                # past n: negative, must stay
    d = x.to(DEV)
    lib.call("toc3d_relu_inplace", dt, d, n, lib.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(d[:n], torch.relu(x[:n].to(DEV))) and bool((d[n:] == -3.0).all())     # == : +0 and -0 compare equal


# ---- 4. the module ------------------------------------------------------------------------------------------------------------------
_SIZES = {"e128": dict(embed_dims=128, num_heads=4, feedforward_channels=1024, num_layers=2),
          "e192": dict(embed_dims=192, num_heads=6, feedforward_channels=320, num_layers=2)}
_SHAPE = dict(B=2, num_query=32, num_propagated=13, Nm=19, Nk=333)


def _on_dev(inp):
    return {k: None if v is None else v.to(DEV) for k, v in inp.items()}


@pytest.mark.parametrize("with_temp", [True, False])
@pytest.mark.parametrize("tag", sorted(_SIZES))
def test_decoder_fp32x3_at_sizes_with_tails(tag, with_temp):
    sizes = _SIZES[tag]
    E, L = sizes["embed_dims"], sizes["num_layers"]
    inp = synth.decoder_inputs(sizes, _SHAPE, with_temp=with_temp)
    cap64 = {}
    with torch.no_grad():
        ref = restated_decoder(synth.decoder_state_dict(sizes), sizes, _on_dev(inp), dtype=torch.float64, capture=cap64)
    m = build(sizes)
    if tag == "e128":
        from toc3d_amd import decoder
        assert decoder._tile_variant(90, E, sizes["feedforward_channels"], True) == decoder.SPLITK_VARIANT      # the FFN's second GEMM is the split-K one
    for _ in range(3):                                  # eager, recorded, replayed
        outs, _, _ = run(m, inp)
    assert outs.shape == (L, 2, 45, E) and bool(torch.isfinite(outs).all())
    state = m._states[(2, 45, 333, 19 if with_temp else 0)]
    assert state.get("cplan") is not None
    errs = [rel_max(outs[l], ref[l]) for l in range(L)]
    m.capture = {}
    outs_e, _, _ = run(m, inp)
    assert torch.equal(outs_e, outs), "eager launches and the replayed plan differ"
    mids = {k: rel_max(v, cap64[k]) for k, v in m.capture.items()}
    print(f"[decoder {tag} {'temp' if with_temp else 'notemp'} fp32x3] rel max err per layer {[f'{e:.2e}' for e in errs]}   intermediates max {max(mids.values()):.2e}")
    assert len(mids) == 3 * L and max(errs) < 1e-3 and max(mids.values()) < 1e-3


@pytest.mark.parametrize("with_temp", [True, False])
@pytest.mark.parametrize("tag", sorted(_SIZES))
def test_decoder_bf16_at_sizes_with_tails(tag, with_temp):
    sizes = _SIZES[tag]
    inp = synth.decoder_inputs(sizes, _SHAPE, with_temp=with_temp)
    sd = synth.decoder_state_dict(sizes)
    with torch.no_grad():
        ref = restated_decoder(sd, sizes, _on_dev(inp), dtype=torch.float64)
        ctl = restated_decoder(sd, sizes, _on_dev(inp), contract=torch.bfloat16)
    eager, plan = build(sizes, "bf16", "eager"), build(sizes, "bf16", "plan")
    oe = run(eager, inp)[0]
    for _ in range(3):
        outs = run(plan, inp)[0]
    assert torch.equal(outs, oe), "eager launches and the replayed plan differ"
    e_hip, e_ctl = rel_l2(outs[-1], ref[-1]), rel_l2(ctl[-1], ref[-1])
    print(f"[decoder {tag} {'temp' if with_temp else 'notemp'} bf16] rel l2 of the last layer vs f64: hip {e_hip:.3e}   torch-bf16 control {e_ctl:.3e}")
    assert bool(torch.isfinite(outs).all())
    assert e_hip <= 1.2 * e_ctl
