"""GPU: the kernels of csrc/focal_head.hip alone, through the C ABI -- toc3d_focal_gn_stats and toc3d_focal_heads -- and the ranking behind them, per element
against f64 references.  Each kernel is fed the device's OWN upstream buffer read back (the heads kernel gets the statistics the statistics kernel wrote), so a
bound covers that kernel's f32 arithmetic alone.  Outputs are pre-filled with the NaN sentinel of tests/support.py: rows past M and padding columns must come back
untouched.  The module prints its worst error as a fraction of each bound when it finishes.  u = 2^-24.

1. Statistics (focal_head_cases.stats_bounds).  n = (E / 32) T terms per group.  Any order of f32 additions of n terms errs by at most (n - 1) u sum |x|, the
   division by n adds one rounding: |mean' - mean| <= n u mean|x|.  The second pass sums (x - m)^2 about the COMPUTED mean m; exactly, sum (x - m)^2 / n = var +
   (m - mean)^2, and in f32 each term carries three roundings, the sum n - 1, the division and the add of eps one each, 1 / sqrt two more (each counted twice in
   rstd^-2) and two of slack: |rstd'^-2 - (var + eps)| <= ((n + 10) u + (n u mean|x|)^2 / (var + eps)) (var + eps).  The case with every channel shifted by 100 x its
   spread is the one a one-pass E[x^2] - E[x]^2 fails: there mean^2 / var = 10^4 and f32 keeps 7 digits.  Two runs give the same bits.

2. Heads and geometry.  a = (x - mean) rstd gamma is three roundings, a + beta one, ReLU is 1-Lipschitz: |dh| <= 4 u (|a| + |beta|) =: 4 u H with H >= |h|.  A
   logit is E FMAs in some order and the bias add: delta = (E + 6) u (sum H |w| + |bias|) covers both (dot_bound with extra = 6: the 4 of dh, the bias add, one of
   slack).  Behind the logits: a sigmoid s = 1 / (1 + expf(-z)) is given 8 u s for expf, the add and the division on top of its slope <= 1 / 4 times the error of z;
   inverse_sigmoid = logf(x / (1 - x)) is given 3 u (1 + |.|) (subtraction, division, logf); every further +, -, * one rounding of its result; the clamps and the
   maximum over the classes are 1-Lipschitz (the maximum's delta is the largest class delta of the row).
   Exact: with ltrb = +-30 both clamps act and the box is (0.5, y, 1, 0) bit for bit.

3. Ranking: topk_indexes of the module equals torch.sort(stable=True, descending=True) of the device's own sample_weight, integer for integer, with planted ties
   (views that repeat view 0 tie with it token for token).
"""
import pytest
import torch

import focal_head_cases as FC
from support import DEV, S, is_sent, same_bits, sent, worst_report
from toc3d_amd import FocalHead, lib, synth

pytestmark = pytest.mark.gpu
U = FC.U
G = 3                                                    # guard rows behind every output
note, _report = worst_report("focal head kernels", 44)
HW = {1: (1, 1), 5: (1, 5), 15: (3, 5), 33: (3, 11), 1000: (20, 50)}


def make_rows(V, T, E, offset=0.0, seed=0):
    """f32 rows [V*T, 2E + 4] as the conv leaves them (the 4 padding columns hold the sentinel: nothing may read them into a result): every channel with a
    spread of its own in [0.5, 2] and shifted by ``offset`` spreads."""
    g = torch.Generator().manual_seed(17000 + seed)
    spread = 0.5 + 1.5 * torch.rand(2 * E, generator=g)
    x = sent(V * T, 2 * E + 4, device="cpu")
    x[:, :2 * E] = (torch.randn(V * T, 2 * E, generator=g) + offset) * spread
    return x.to(DEV)


def run_stats(x, V, T, E):
    stats = sent(V * 64 + G, 2)
    lib.call("toc3d_focal_gn_stats", lib.F32, x, x.shape[1], V, T, E, 2, FC.GN_EPS, stats, S())
    torch.cuda.synchronize()
    assert is_sent(stats[V * 64:]), "rows past V * 64 groups were written"
    return stats


@pytest.mark.parametrize("T,E,V,offset", FC.STATS_CASES)
def test_gn_stats(T, E, V, offset):
    x = make_rows(V, T, E, offset, seed=T + E + V)
    stats = run_stats(x, V, T, E)
    assert same_bits(stats, run_stats(x, V, T, E)), "two runs, two results"
    cpg = E // 32
    x64 = x[:, :2 * E].double().cpu().view(V, T, 64, cpg)
    mean, var, b_mean, b_var = FC.stats_bounds(x64, cpg, T)
    got = stats[:V * 64].double().cpu().view(V, 64, 2)
    r_mean = ((got[..., 0] - mean).abs() / b_mean.clamp_min(1e-300)).max().item()
    r_var = ((got[..., 1] ** -2 - (var + FC.GN_EPS)).abs() / ((var + FC.GN_EPS) * b_var)).max().item()
    tag = f"stats T={T} E={E} V={V}" + (" offset" if offset else "")
    print(f"{tag}: mean err / bound {r_mean:.3f}, (var + eps) err / bound {r_var:.3f}; mean^2 / var up to {float((mean ** 2 / var.clamp_min(1e-30)).max()):.1e}")
    note(tag + " mean", r_mean)
    note(tag + " var+eps", r_var)
    assert r_mean <= 1.0 and r_var <= 1.0


def heads_weights(E, NC, seed, ltrb_saturated=False):
    g = torch.Generator().manual_seed(17500 + seed)
    r = lambda *s: torch.randn(*s, generator=g)
    P = dict(gamma=1.0 + 0.1 * r(2 * E), beta=0.1 * r(2 * E), wc=r(NC + 1, E) * 3.0 * E ** -0.5, bc=-1.0 + 0.3 * r(NC + 1), wr=r(6, E) * 2.0 * E ** -0.5, br=0.3 * r(6))
    if ltrb_saturated:
        P["wr"][:4] = 0.0
        P["br"][:4] = torch.tensor([30.0, -30.0, 30.0, -30.0])
    return {k: v.to(DEV).contiguous() for k, v in P.items()}


def run_heads(x, stats, P, loc, V, T, E, NC):
    M = V * T
    o = dict(cls=sent(M + G, NC + 3), box=sent(M + G, 4), ctr2d=sent(M + G, 2), ctrness=sent(M + G, 1), weight=sent(M + G, 1))
    lib.call("toc3d_focal_heads", lib.F32, x, x.shape[1], stats, P["gamma"], P["beta"], P["wc"], P["bc"], P["wr"], P["br"], loc, V, T, E, NC,
             o["cls"], NC + 3, o["box"], o["ctr2d"], o["ctrness"], o["weight"], S())
    torch.cuda.synchronize()
    for k, t in o.items():
        assert is_sent(t[M:]), f"{k}: rows past M = {M} were written"
    assert is_sent(o["cls"][:M, NC:]), "cls_out: the padding columns were written"
    return {k: (t[:M, :NC] if k == "cls" else t[:M]).cpu() for k, t in o.items()}


def heads_reference(x, stats, P, loc, V, T, E, NC):
    """f64 from the f32 inputs the kernel read -> values and per-element bounds of the five outputs."""
    d = lambda t: t.double().cpu()
    cpg, M = E // 32, V * T
    st = d(stats[:V * 64]).view(V, 1, 2, 32, 1, 2)
    xv = d(x[:, :2 * E]).view(V, T, 2, 32, cpg)
    a = ((xv - st[..., 0]) * st[..., 1]).reshape(M, 2 * E) * d(P["gamma"])
    beta = d(P["beta"])
    h, H = torch.relu(a + beta), a.abs() + beta.abs()
    wc, bc, wr, br = d(P["wc"]), d(P["bc"]), d(P["wr"]), d(P["br"])
    zc, dc = h[:, :E] @ wc.T + bc, FC.dot_bound(H[:, :E], wc.abs(), bc.abs(), E, extra=6)
    zr, dr = h[:, E:] @ wr.T + br, FC.dot_bound(H[:, E:], wr.abs(), br.abs(), E, extra=6)
    sig = lambda z, dz: (torch.sigmoid(z), dz / 4 + 8 * U * torch.sigmoid(z))
    l = d(loc).view(M, 2)
    s, ds = sig(zr[:, :4], dr[:, :4])
    raw = torch.stack([l[:, 0] - s[:, 0], l[:, 1] - s[:, 1], l[:, 0] + s[:, 2], l[:, 1] + s[:, 3]], 1)
    xy, dxy = raw.clamp(0, 1), ds + U * raw.abs()
    box = torch.stack([(xy[:, 0] + xy[:, 2]) / 2, (xy[:, 1] + xy[:, 3]) / 2, xy[:, 2] - xy[:, 0], xy[:, 3] - xy[:, 1]], 1)
    dbox = torch.stack([(dxy[:, 0] + dxy[:, 2]) / 2, (dxy[:, 1] + dxy[:, 3]) / 2, dxy[:, 0] + dxy[:, 2], dxy[:, 1] + dxy[:, 3]], 1) + U * box.abs()
    inv = FC.inverse_sigmoid(l)
    z = inv + zr[:, 4:]
    ctr, dctr = sig(z, 3 * U * (1 + inv.abs()) + dr[:, 4:] + U * z.abs())
    sm, dsm = sig(zc[:, :NC].max(1).values, dc[:, :NC].max(1).values)
    sc, dsc = sig(zc[:, NC], dc[:, NC])
    wgt = sm * sc
    val = dict(cls=zc[:, :NC], ctrness=zc[:, NC:], box=box, ctr2d=ctr, weight=wgt[:, None])
    bnd = dict(cls=dc[:, :NC], ctrness=dc[:, NC:], box=dbox, ctr2d=dctr, weight=(sc * dsm + sm * dsc + U * wgt)[:, None])
    return val, bnd


@pytest.mark.parametrize("NC,V,T,E", FC.HEADS_CASES)
def test_heads_and_geometry(NC, V, T, E):
    x = make_rows(V, T, E, seed=NC + T)
    stats = run_stats(x, V, T, E)                        # the device's own statistics, read back by the reference
    P = heads_weights(E, NC, seed=NC + T)
    h, w = HW[T]
    loc = synth.focal_head_inputs(dict(in_channels=1, stride=16), dict(B=1, N=V, h=h, w=w))["location"].to(DEV).contiguous()     # the reference's pixel centres
    out = run_heads(x, stats, P, loc, V, T, E, NC)
    val, bnd = heads_reference(x, stats, P, loc, V, T, E, NC)
    for k in val:
        ratio = ((out[k].double() - val[k]).abs() / bnd[k]).max().item()
        print(f"heads NC={NC} M={V * T} E={E} {k}: err / bound {ratio:.3f} (max bound {float(bnd[k].max()):.2e})")
        note(f"heads NC={NC} M={V * T} E={E} {k}", ratio)
        assert ratio <= 1.0, (k, ratio)
    box = out["box"]
    assert bool(((box >= 0) & (box <= 1)).all())
    assert same_bits(out["weight"], run_heads(x, stats, P, loc, V, T, E, NC)["weight"]), "two runs, two results"


def test_boxes_exactly_clamped():
    NC, V, T, E = 3, 2, 15, 64
    x = make_rows(V, T, E, seed=99)
    stats = run_stats(x, V, T, E)
    P = heads_weights(E, NC, seed=99, ltrb_saturated=True)
    loc = synth.focal_head_inputs(dict(in_channels=1, stride=16), dict(B=1, N=V, h=3, w=5))["location"].to(DEV).contiguous()
    box = run_heads(x, stats, P, loc, V, T, E, NC)["box"]
    ly = loc.view(-1, 2)[:, 1].cpu()
    want = torch.stack([torch.full_like(ly, 0.5), ly, torch.ones_like(ly), torch.zeros_like(ly)], 1)
    print("clamped boxes:", box[:3].tolist())
    assert same_bits(box, want), "x1 = lx - 1 -> 0 and x2 = lx + 1 -> 1 exactly; y1 = y2 = ly"


@pytest.mark.parametrize("B,n", FC.RANK_CASES)
def test_ranking_equals_a_stable_descending_sort(B, n):
    N, h, w = {15: (3, 1, 5), 2000: (2, 20, 50)}[n]
    sizes = synth.FOCAL_HEAD_TINY
    m = FocalHead(**sizes, precision="fp32x3")
    m.load_state_dict(synth.focal_head_state_dict(sizes))
    m = m.to(DEV)
    inp = synth.focal_head_inputs(sizes, dict(B=B, N=N, h=h, w=w), seed=n)
    feats = inp["img_feats"]
    feats[:, 1:] = feats[:, :1]                          # the planted block: every view repeats view 0, so token t of views 0 .. N-1 tie
    for K, ratio in ((0, 0.0), (1, 1.5 / n), (int(0.3 * n), 0.3), (n, 1.0)):
        m.infer_ratio = ratio
        out = m(inp["location"].to(DEV), img_feats=feats.to(DEV))
        wgt = out["sample_weight"]
        want = torch.sort(wgt.view(B, n), dim=1, descending=True, stable=True).indices[:, :K]
        ties = int((wgt.view(B, N, h * w)[:, 0] == wgt.view(B, N, h * w)[:, 1]).sum())
        print(f"B={B} n={n} K={K}: {ties} tied pairs between views 0 and 1")
        assert ties == B * h * w, "the planted ties are there"
        assert out["topk_indexes"].dtype == torch.int64 and tuple(out["topk_indexes"].shape) == (B, K, 1) == (B, int(n * ratio), 1)
        assert torch.equal(out["topk_indexes"].view(B, K), want)
