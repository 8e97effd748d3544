"""GPU: toc3d_focal_sample_weight (csrc/focal_select.hip, include/toc3d_select.h) alone, through the C ABI.

1. Bit for bit against the ``sample_weight`` that toc3d_focal_heads writes from the same class-tower columns, statistics and weights: the two kernels share one
   spelling of the per-row operation sequence (csrc/focal_row.h).  The full kernel reads x [M, 2E] and statistics [V, 64, 2] (toc3d_focal_gn_stats with two
   branches); the selection kernel gets the class tower's half of exactly those statistics, [V, 32, 2], and either the class columns alone (ldx = E) or the
   two-tower buffer with NaN in every box-tower column (ldx = 2E): a finite result there shows that nothing from column E on is read.  toc3d_focal_gn_stats with
   one branch on the class columns alone gives the bits of the two-branch statistics' class half (what FocalHead.select_rows launches).
2. Per element against f64 from the f32 inputs the kernel read, with the dot-product-through-sigmoid bound of tests/focal_head_cases.py, as the sibling test of
   the full kernel (tests/test_gpu_focal_head_kernels.py, docstring item 2) derives it: |dh| <= 4 u H for the affine, a logit within (E + 6) u (sum H |w| + |b|)
   (dot_bound with extra = 6), the maximum over the classes 1-Lipschitz, a sigmoid s within dz / 4 + 8 u s, the product one more rounding.  The module prints
   its worst error as a fraction of the bound when it finishes.
3. The canary of tests/support.py on both sides of ``weight``: G elements in front of row 0 and behind row M - 1 come back untouched.

Shapes, V = 2 throughout: T in {1, 31, 33} (one row; a short chunk; one row past the 32-row chunk: a second workgroup per view), E in {32, 64, 256} (one channel
per group with 8 active lanes; 16 active lanes; all 64 lanes), num_classes in {1, 3, 64}.  E = 256 with num_classes = 64 is beyond both entry points' 64 KB of
LDS (65 * 256 floats for the selection kernel, 71 * 256 for the full one): that combination is asserted to be refused, before any launch, by both."""
import pytest
import torch

import focal_head_cases as FC
from support import CAN32, DEV, S, is_canary, same_bits, worst_report
from toc3d_amd import lib

pytestmark = pytest.mark.gpu
U = FC.U
G = 5                                                    # canary elements on each side of weight
note, _report = worst_report("focal select kernel", 44)
FITS = lambda E, NC: (NC + 7) * E * 4 + (128 + NC + 7) * 4 <= 64 * 1024          # toc3d_focal_heads' LDS budget (the larger of the two)
CASES = [(T, E, NC, wide) for T in (1, 31, 33) for E in (32, 64, 256) for NC in (1, 3, 64) for wide in (False, True) if FITS(E, NC)]
V = 2


def inputs(T, E, NC):
    """x f32 [V*T, 2E] as the conv leaves it (every channel with a spread of its own in [0.5, 2]) and the weights of both halves, seeded per case."""
    g = torch.Generator().manual_seed(18000 + 1000 * T + 10 * E + NC)
    r = lambda *s: torch.randn(*s, generator=g)
    spread = 0.5 + 1.5 * torch.rand(2 * E, generator=g)
    x = r(V * T, 2 * E) * spread
    P = dict(gamma=1.0 + 0.1 * r(2 * E), beta=0.1 * r(2 * E), wc=r(NC + 1, E) * 3.0 * E ** -0.5, bc=-1.0 + 0.3 * r(NC + 1), wr=r(6, E) * 2.0 * E ** -0.5, br=0.3 * r(6))
    return x.to(DEV).contiguous(), {k: v.to(DEV).contiguous() for k, v in P.items()}


def stats_of(x, ldx, T, E, branches):
    st = torch.zeros(V, branches * 32, 2, device=DEV)
    lib.call("toc3d_focal_gn_stats", lib.F32, x, ldx, V, T, E, branches, FC.GN_EPS, st, S())
    return st


def full_weight(x, stats2, P, T, E, NC):
    """sample_weight of toc3d_focal_heads on the two-tower buffer."""
    M = V * T
    z = lambda *s: torch.zeros(*s, device=DEV)
    wgt = z(M)
    loc = torch.full((M, 2), 0.5, device=DEV)
    lib.call("toc3d_focal_heads", lib.F32, x, 2 * E, stats2, P["gamma"], P["beta"], P["wc"], P["bc"], P["wr"], P["br"], loc, V, T, E, NC,
             z(M, NC), NC, z(M, 4), z(M, 2), z(M), wgt, S())
    return wgt


def select_weight(x, ldx, stats1, P, T, E, NC):
    M = V * T
    buf = torch.empty(M + 2 * G, device=DEV)
    buf.view(torch.int32).fill_(CAN32)
    lib.call("toc3d_focal_sample_weight", lib.F32, x, ldx, stats1, P["gamma"], P["beta"], P["wc"], P["bc"], V, T, E, NC, buf[G:], S())
    torch.cuda.synchronize()
    assert bool(is_canary(buf[:G]).all()), "the elements in front of weight were written"
    assert bool(is_canary(buf[G + M:]).all()), f"the elements behind row M = {M} were written"
    return buf[G:G + M].clone()


def reference(xc, stats1, P, T, E, NC):
    """f64 from the f32 inputs the kernel read -> (sample_weight, per-element bound)."""
    d = lambda t: t.double().cpu()
    cpg, M = E // 32, V * T
    st = d(stats1).view(V, 1, 32, 1, 2)
    a = ((d(xc).view(V, T, 32, cpg) - st[..., 0]) * st[..., 1]).reshape(M, E) * d(P["gamma"][:E])
    beta = d(P["beta"][:E])
    h, H = torch.relu(a + beta), a.abs() + beta.abs()
    wc, bc = d(P["wc"]), d(P["bc"])
    z, dz = h @ wc.T + bc, FC.dot_bound(H, wc.abs(), bc.abs(), E, extra=6)
    sig = lambda v, dv: (torch.sigmoid(v), dv / 4 + 8 * U * torch.sigmoid(v))
    sm, dsm = sig(z[:, :NC].max(1).values, dz[:, :NC].max(1).values)
    sc, dsc = sig(z[:, NC], dz[:, NC])
    wgt = sm * sc
    return wgt, sc * dsm + sm * dsc + U * wgt


@pytest.mark.parametrize("T,E,NC,wide", CASES)
def test_sample_weight_bits_and_f64(T, E, NC, wide):
    x, P = inputs(T, E, NC)
    M = V * T
    stats2 = stats_of(x, 2 * E, T, E, 2)
    stats1 = stats2.view(V, 2, 32, 2)[:, 0].contiguous()             # the class tower's half of the statistics the full kernel reads
    xc = x[:, :E].contiguous()
    assert same_bits(stats_of(xc, E, T, E, 1), stats1), "one-branch statistics of the class columns differ from the two-branch statistics' class half"
    want = full_weight(x, stats2, P, T, E, NC)
    if wide:
        xin, ldx = x.clone(), 2 * E
        xin[:, E:] = float("nan")                                    # the box tower: nothing from column E on may reach a result
    else:
        xin, ldx = xc, E
    got = select_weight(xin, ldx, stats1, P, T, E, NC)
    assert bool(torch.isfinite(got).all())
    assert same_bits(got, want), f"{int((got != want).sum())} of {M} weights differ from toc3d_focal_heads' bits"
    assert same_bits(got, select_weight(xin, ldx, stats1, P, T, E, NC)), "two runs, two results"
    val, bnd = reference(xc, stats1, P, T, E, NC)
    ratio = ((got.double().cpu() - val).abs() / bnd).max().item()
    tag = f"T={T} E={E} NC={NC} ldx={'2E' if wide else 'E'}"
    print(f"sample_weight {tag}: bits equal on {M} rows; f64 err / bound {ratio:.3f} (max bound {float(bnd.max()):.2e}, weights in "
          f"[{float(val.min()):.3g}, {float(val.max()):.3g}])")
    note(tag, ratio)
    assert ratio <= 1.0


def test_the_combination_beyond_lds_is_refused_by_both():
    T, E, NC = 1, 256, 64
    assert not FITS(E, NC)
    x, P = inputs(T, E, NC)
    stats2 = stats_of(x, 2 * E, T, E, 2)
    with pytest.raises(RuntimeError, match="toc3d_focal_heads: .*64 KB of LDS"):
        full_weight(x, stats2, P, T, E, NC)
    with pytest.raises(RuntimeError, match="toc3d_focal_sample_weight: .*64 KB of LDS"):
        select_weight(x, 2 * E, stats2.view(V, 2, 32, 2)[:, 0].contiguous(), P, T, E, NC)
