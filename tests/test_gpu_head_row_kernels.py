"""GPU: the row kernels of the head's token side and of the memory bank alone, through the C ABI, per element against the f64 references of
tests/head_rows_cases.py (derivations of every bound in its docstring; the same bounds are pinned on f32 emulations by tests/test_cpu_head_rows_cases.py).
Outputs are pre-filled with the NaN sentinel or the canary of tests/support.py: whatever lies behind the last row or the last valid column must come back untouched.
No element of any case is left out of a comparison.  The module prints its worst error as a fraction of each bound when it finishes.  u = 2^-24.

1. toc3d_head_frustum_inputs: pos_in inside [inv64(p - dp), inv64(p + dp)] widened by 4 u (1 + |.|), the elements whose whole interval is clamped all holding the bits of
   one constant, logf(1e-5f / 1.f) / logf(1.f / 1e-5f) as the device's libm returns it (read from a launch under a range far away, all of whose pos_in is that constant); cone's columns 2..4 / 5..7 within dp of bins D - 1 / D - 30 and its columns 0..1 within u of |K00|, |K11| / 1e3 of
   camera (token % N); cone_act carries cone's bits in F32; pos_in and cone_act in BF16 are RNE of the F32 launch's values.  Two position ranges narrow enough that
   the clamps run (the shares of clamped elements are asserted), one coords_d with bin 0 = 0.0, one uniform, one pad_h > 16 h.  On the two clamp cases the sampled
   kernel's rows are still the full kernel's, bit for bit (indices inside [0, LEN) only).
2. toc3d_mln_apply at E in {1, 63, 64, 65, 100, 1000, 1024}, M in {1, 5, 7}: ordinary rows, rows shifted by 100 and 10^4 spreads, rows of spread 1e-3, and a constant
   row at the two power-of-two E (out = beta bit for bit); ld_act > E with canaries in all three act dtypes; bf16 out_act = RNE of out, planes = (bf16(out),
   bf16(out - hi)), and the f32 out does not depend on the dtype.
3. toc3d_se_gate and toc3d_memory_scores at n / rows in {1, 255, 256, 257} (one element past a workgroup, one short of it), logits from -120 to 120 with the
   values where expf overflows or the quotient underflows planted in the last elements; scores lie in [0, 1] and are never the kernel's -1 start value.
4. toc3d_memory_pre_update / toc3d_memory_post_update called directly: rigid poses with rotations about all three axes, a rec_ego_pose of its own for every query,
   ``order`` an arbitrary permutation; emb, vel and ts bit-exact against the host, pose and ref within the dot4 bound; the in bank keeps its bits, slots past
   memory_len and rows past the bank keep their guards."""
import itertools

import pytest
import torch

import head_rows_cases as HC
from support import DEV, S, SENT32, canary, check_untouched, is_sent, planes_decode, same_bits, sent, worst_report
from toc3d_amd import lib

pytestmark = pytest.mark.gpu
G = 3                                                    # guard rows behind every output
note, _report = worst_report("head row kernels", 44)
dev = lambda t: t.to(DEV).contiguous()


# ---- 1. frustum ---------------------------------------------------------------------------------------------------------------------------------------------------
def run_frustum(a, dt, bf16, index=None):
    """-> (pos_in [R, 3 D], cone_act [R, 8], cone [R, 8]) on the host; R = every token, or the B * K an index list names (the sampled kernel)."""
    B, N, h, w, D = (a[k] for k in "BNhwD")
    R = B * N * h * w if index is None else index.numel()
    ld = (3 * D + 63) // 64 * 64
    i2l, intr, cd = dev(a["i2l"]), dev(a["intr"]), dev(a["cd"])
    pin, ca, cone = sent(R + G, ld, bf16), sent(R + G, 64, bf16), sent(R + G, 8)
    tail = (D, a["stride"], a["pad_h"], a["pad_w"], pin, ld, ca, 64, cone, S())
    if index is None:
        lib.call("toc3d_head_frustum_inputs", dt, i2l, intr, cd, a["pr"], B, N, h, w, *tail)
    else:
        idx = dev(index)
        lib.call("toc3d_head_frustum_inputs_sampled", dt, i2l, intr, cd, a["pr"], idx, B, N, h, w, index.shape[1], *tail)
    torch.cuda.synchronize()
    assert is_sent(pin[R:]) and is_sent(ca[R:]) and is_sent(cone[R:]), f"rows >= {R} were written"
    assert is_sent(pin[:R, 3 * D:]), f"pos_in: columns >= {3 * D} were written"
    assert is_sent(ca[:R, 8:]), "cone_act: columns >= 8 were written"
    return pin[:R, :3 * D].cpu(), ca[:R, :8].cpu(), cone[:R].cpu()


CLAMP_CONSTANTS = {}                                     # the two constants of the clamped elements, as the first clamp case saw them


@pytest.mark.parametrize("name", [c[0] for c in HC.FRUSTUM_CASES])
def test_frustum_inputs(name):
    a = HC.frustum_case(name)
    ref = HC.frustum_reference(a)
    family = name.split(" ", 2)[2] if name.count(" ") > 1 else "plain"
    if name in HC.FRUSTUM_CLAMP_CASES:
        low, high, inside = HC.clamp_shares(ref["p"])
        print(f"frustum {name}: {100 * low:.1f} % of p at or below 0, {100 * high:.1f} % at or above 1, {100 * inside:.1f} % inside")
        assert low >= 0.05 and high >= 0.05 and inside >= 0.50, "the clamps must run in this case"
    pin, ca, cone = run_frustum(a, lib.F32, False)
    r_pos, r_f, r_last, r_d30, c_lo, c_hi = HC.frustum_ratios(ref, pin, cone)
    print(f"frustum {name}: pos_in {r_pos:.3f} cone f {r_f:.3f} last bin {r_last:.3f} bin D-30 {r_d30:.3f}; clamped elements hold {[HC.bits_to_f32(b) for b in c_lo]} / {[HC.bits_to_f32(b) for b in c_hi]}")
    for key, r in (("pos_in", r_pos), ("cone |f| / 1e3", r_f), ("cone bin D-1", r_last), ("cone bin D-30", r_d30)):
        note(f"frustum {key} [{family}]", r)
    assert r_pos <= 1.0, "pos_in outside [inv64(p - dp) - e, inv64(p + dp) + e]"
    pinned = 1 if name in HC.FRUSTUM_CLAMP_CASES else 0
    assert len(c_lo) == pinned and len(c_hi) == pinned, "the elements whose whole interval is clamped do not all hold the one constant logf(1e-5f / 1.f) / logf(1.f / 1e-5f)"
    if pinned:
        assert CLAMP_CONSTANTS.setdefault("bits", (c_lo, c_hi)) == (c_lo, c_hi), "the clamp constants differ between two cases"
        for prange, want in ((HC.FAR_BELOW, c_lo), (HC.FAR_ABOVE, c_hi)):            # the same case a million metres outside the range: nothing but the constant
            assert HC.distinct_bits(run_frustum(HC.with_range(a, prange), lib.F32, False)[0]) == want, "a clamped element is not the constant of a range far away"
    assert r_f <= 1.0 and r_last <= 1.0 and r_d30 <= 1.0, (r_f, r_last, r_d30)
    assert same_bits(ca, cone), "cone_act in F32 carries cone's bits"
    pin_b, ca_b, cone_b = run_frustum(a, lib.BF16, True)
    assert same_bits(cone_b, cone), "the f32 cone depends on the dtype"
    assert same_bits(pin_b, pin.to(torch.bfloat16)), "pos_in in BF16 is not RNE of the F32 kernel's"
    assert same_bits(ca_b, cone.to(torch.bfloat16)), "cone_act in BF16 is not RNE of cone"
    if name in HC.FRUSTUM_CLAMP_CASES:
        B, LEN = a["B"], a["N"] * a["h"] * a["w"]
        g = torch.Generator().manual_seed(41)
        index = torch.stack([torch.randperm(LEN, generator=g) for _ in range(B)]).long()
        rows = (index + torch.arange(B)[:, None] * LEN).flatten()
        for got, full in zip(run_frustum(a, lib.F32, False, index=index), (pin, ca, cone)):
            assert same_bits(got, full[rows]), "a sampled row is not the full kernel's row"


# ---- 2. MLN -------------------------------------------------------------------------------------------------------------------------------------------------------
def run_mln(x, g, b, dt, tdt, planes, tag):
    M, E = x.shape
    ld = (E + 31) // 32 * 32 + 32
    xd, gd, bd = dev(x), dev(g), dev(b)
    out, act = sent(M + G, E), canary(M + G, ld, tdt)
    lib.call("toc3d_mln_apply", dt, xd, gd, bd, M, E, out, act, ld, S())
    torch.cuda.synchronize()
    assert is_sent(out[M:]), f"{tag}: out rows >= {M} were written"
    check_untouched(tag, act, M, E, planes)
    return out[:M].cpu(), act[:M].cpu()


@pytest.mark.parametrize("E", HC.MLN_E)
def test_mln_apply(E):
    for M in HC.MLN_M:
        for profile in HC.MLN_PROFILES + (("constant",) if E in HC.MLN_CONSTANT_E else ()):
            tag = f"mln E={E} M={M} {profile}"
            x, g, b = HC.mln_inputs(M, E, profile)
            val, bound = HC.mln_reference(x, g, b)
            out, act = run_mln(x, g, b, lib.F32, torch.float32, False, tag + " f32")
            r = HC.worst(out, val, bound)
            print(f"{tag}: err / bound {r:.3f} (mean^2 / var up to {float((x.double().mean(1) ** 2 / x.double().var(1, unbiased=False).clamp_min(1e-30)).max()) if E > 1 else 0.0:.1e})")
            note(f"mln_apply [{profile}]", r)
            assert r <= 1.0, (tag, r)
            assert same_bits(act[:, :E], out), f"{tag}: out_act in F32 is not out"
            if profile == "constant":
                assert same_bits(out, b), f"{tag}: a constant row at a power-of-two E gives beta bit for bit"
            out_b, act_b = run_mln(x, g, b, lib.BF16, torch.bfloat16, False, tag + " bf16")
            assert same_bits(out_b, out), f"{tag}: the f32 out depends on the dtype (bf16)"
            assert same_bits(act_b[:, :E], out.to(torch.bfloat16)), f"{tag}: out_act in BF16 is not RNE of out"
            out_p, act_p = run_mln(x, g, b, lib.F32X3P, torch.float32, True, tag + " planes")
            assert same_bits(out_p, out), f"{tag}: the f32 out depends on the dtype (planes)"
            hi, lo = planes_decode(act_p)
            want_hi = out.to(torch.bfloat16).float()
            assert torch.equal(hi[:, :E], want_hi) and torch.equal(lo[:, :E], (out - want_hi).to(torch.bfloat16).float()), f"{tag}: planes are not (bf16(out), bf16(out - hi))"


# ---- 3. sigmoids ----------------------------------------------------------------------------------------------------------------------------------------------------
def logit_sets(n, seed):
    """One seeded vector with the special logits in its last elements; a single element takes each special value in turn."""
    if n == 1:
        return [HC.logits(1, seed, special=v) for v in HC.SPECIAL_LOGITS]
    return [HC.logits(n, seed)]


@pytest.mark.parametrize("n", HC.GATE_N)
def test_se_gate(n):
    for se in logit_sets(n, seed=n):
        pos = 2.0 * torch.randn(n, generator=torch.Generator().manual_seed(n))
        pd, sd = dev(pos), dev(se)
        out = sent(n + G, 1)
        lib.call("toc3d_se_gate", pd, sd, out, n, S())
        torch.cuda.synchronize()
        assert is_sent(out[n:]), f"elements >= {n} were written"
        got = out[:n, 0].cpu()
        val, bound = HC.gate_reference(pos, se)
        r = HC.worst(got, val, bound)
        print(f"se_gate n={n} last logit {float(se[-1]):g}: err / bound {r:.3f}; out at the last element {float(got[-1]):.3e} (f64 {float(val[-1]):.3e})")
        note(f"se_gate n={n}", r)
        assert bool(torch.isfinite(got).all()) and r <= 1.0, (n, r)


@pytest.mark.parametrize("classes", HC.SCORE_CLASSES)
@pytest.mark.parametrize("rows", HC.SIGMOID_N)
def test_memory_scores(rows, classes):
    sets = logit_sets(rows * classes, seed=rows + classes) if rows > 1 else [HC.logits(classes, seed=classes, special=v) for v in HC.SPECIAL_LOGITS]
    for z in sets:
        cls = z.view(rows, classes)
        cd = dev(cls)
        score = sent(rows + G, 1)
        lib.call("toc3d_memory_scores", cd, rows, classes, score, S())
        torch.cuda.synchronize()
        assert is_sent(score[rows:]), f"rows >= {rows} were written"
        got = score[:rows, 0].cpu()
        val, bound = HC.score_reference(cls)
        r = HC.worst(got, val, bound)
        print(f"memory_scores rows={rows} classes={classes} last logit {float(z[-1]):g}: err / bound {r:.3f}; last score {float(got[-1]):.3e} (f64 {float(val[-1]):.3e})")
        note(f"memory_scores classes={classes}", r)
        assert bool(((got >= 0.0) & (got <= 1.0)).all()), "a score outside [0, 1] (the kernel's start value is -1)"
        assert r <= 1.0, (rows, classes, r)


# ---- 4. memory ------------------------------------------------------------------------------------------------------------------------------------------------------
GUARD64 = 0x7FF8_7FC1_7FC1_7FC1                          # an f64 NaN pattern for the timestamps' guard slots


def guarded_bank(bank, L):
    """The host bank on the device with the sentinel in every slot >= L -> (device bank, the bits it starts with)."""
    out = {}
    for k, t in bank.items():
        t = t.clone()
        if k == "ts":
            t.view(torch.int64)[:, L:] = GUARD64
        else:
            t.view(torch.int32)[:, L:] = SENT32
        out[k] = dev(t)
    return out, {k: (t.view(torch.int64) if k == "ts" else t.view(torch.int32)).clone() for k, t in out.items()}


def ints(t):
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t.contiguous().view(torch.int32)


def check_bank(tag, got, exact, approx, family):
    for k, want in exact.items():
        assert torch.equal(ints(got[k]), ints(want)), f"{tag}: {k} is not the host's, bit for bit"
    for k, (val, bound) in approx.items():
        r = HC.worst(got[k], val, bound)
        note(f"{family} {k}", r)
        assert r <= 1.0, (tag, k, r)
    return {k: HC.worst(got[k], *approx[k]) for k in approx}


@pytest.mark.parametrize("L", HC.MEM_LEN)
def test_memory_pre_update(L):
    B, cap = HC.MEM_B, L + G
    for npg, D, fresh in itertools.product(sorted({0, 1, L}), HC.MEM_D, (0, 1)):
        tag = f"pre_update memory_len={L} num_propagated={npg} D={D} fresh={fresh}"
        data = HC.frame_data(B, seed=L + npg)
        host = HC.memory_bank(B, cap, L, D, seed=L + 7 * npg + D, zero=bool(fresh))
        pseudo = torch.rand(max(npg, 1), 3, generator=torch.Generator().manual_seed(L + D))
        bank, before = guarded_bank(host, L)
        x, ts, inv, pc = dev(data["prev"]), dev(data["ts"]), dev(data["ego_inv"]), dev(data["pc"])
        ps = dev(pseudo) if npg else None                 # num_propagated = 0: a null pointer
        lib.call("toc3d_memory_pre_update", bank["emb"], bank["ref"], bank["ts"], bank["pose"], bank["vel"], x, ts, inv, ps, pc, B, cap, L, npg, D, fresh, S())
        torch.cuda.synchronize()
        for k, t in bank.items():
            assert torch.equal(ints(t)[:, L:], before[k][:, L:]), f"{tag}: {k}: slots >= memory_len were written"
        got = {k: t[:, :L].cpu() for k, t in bank.items()}
        exact, approx = HC.pre_update_reference(host, data, pseudo, L, npg, fresh)
        r = check_bank(tag, got, exact, approx, f"pre_update [num_propagated {'0' if npg == 0 else '1' if npg == 1 else 'memory_len'}]")
        print(f"{tag}: pose {r['pose']:.3f} ref {r['ref']:.3f}; emb, vel, ts exact")


@pytest.mark.parametrize("topk", list(HC.MEM_TOPK_Q))
def test_memory_post_update(topk):
    B = HC.MEM_B
    for Q, L, ld_bbox, D in itertools.product(HC.MEM_TOPK_Q[topk], HC.MEM_LEN, HC.MEM_LD_BBOX, HC.MEM_D):
        tag = f"post_update topk={topk} Q={Q} memory_len={L} ld_bbox={ld_bbox} D={D}"
        cap = L + topk
        data = HC.frame_data(B, seed=Q + ld_bbox)
        host = HC.memory_bank(B, cap, L, D, seed=Q + L + D)
        dec = HC.post_update_inputs(B, Q, D, ld_bbox, seed=Q + topk + ld_bbox)
        src, before = guarded_bank(host, L)                     # slots >= memory_len of the in bank hold NaNs: nothing may read them into a result
        rows = B * cap
        out = dict(emb=sent(rows + G, D), ref=sent(rows + G, 3), pose=sent(rows + G, 16), vel=sent(rows + G, 2),
                   ts=torch.full((rows + G,), GUARD64, dtype=torch.int64, device=DEV).view(torch.float64))
        order, rec, bbox, od, ego, ts = dev(dec["order"]), dev(dec["rec"]), dev(dec["bbox"]), dev(dec["dec"]), dev(data["ego"]), dev(data["ts"])
        lib.call("toc3d_memory_post_update", src["emb"], src["ref"], src["ts"], src["pose"], src["vel"], out["emb"], out["ref"], out["ts"], out["pose"], out["vel"],
                 order, rec, bbox, ld_bbox, od, ego, ts, B, Q, cap, L, topk, D, S())
        torch.cuda.synchronize()
        for k, t in src.items():
            assert torch.equal(ints(t), before[k]), f"{tag}: the in bank's {k} changed"
        for k, t in out.items():
            assert bool((ints(t)[rows:] == (GUARD64 if k == "ts" else SENT32)).all()), f"{tag}: {k}: rows behind the bank were written"
        got = {k: t[:rows].cpu().view(B, cap, *t.shape[1:]) for k, t in out.items()}
        exact, approx = HC.post_update_reference(host, data, dec, L, topk)
        r = check_bank(tag, got, exact, approx, f"post_update [topk {topk}]")
        if D == HC.MEM_D[0]:
            print(f"{tag}: pose {r['pose']:.3f} ref {r['ref']:.3f}; emb, vel, ts exact")
