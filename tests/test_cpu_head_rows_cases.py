"""CPU: the bounds of tests/head_rows_cases.py, pinned without a GPU.  The f32 emulations of the frustum body, the MLN row, the sigmoid and the memory kernels'
4x4 products (one numpy f32 operation per rounding, in the kernel's order) must sit inside the bounds on every case the GPU file runs; the narrow position ranges must
keep their shares of clamped elements; and planted errors -- the ones a kernel of this kind gets wrong -- must land outside.  Each test prints its worst ratios."""
import numpy as np
import pytest
import torch

import head_rows_cases as HC

U = HC.U


# ---- frustum -----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in HC.FRUSTUM_CASES])
def test_frustum_emulation_inside_the_bounds(name):
    a = HC.frustum_case(name)
    ref = HC.frustum_reference(a)
    p, pos_in, cone = HC.emulate_frustum(a)
    r_pos, r_f, r_last, r_d30, c_lo, c_hi = HC.frustum_ratios(ref, pos_in, cone)
    r_p = HC.worst(p, ref["p"], ref["dp"])
    print(f"frustum {name}: p {r_p:.3f} pos_in {r_pos:.3f} cone f {r_f:.3f} last bin {r_last:.3f} bin D-30 {r_d30:.3f}")
    assert max(r_p, r_pos, r_f, r_last, r_d30) <= 1.0
    clamps = name in HC.FRUSTUM_CLAMP_CASES
    assert len(c_lo) == len(c_hi) == (1 if clamps else 0), "every element whose whole interval is clamped holds the one constant"
    if clamps:         # the constants are those of a range far away, where nothing else is left; numpy's logf returns the f32 nearest to the true logarithm at both arguments
        for prange, want, share in ((HC.FAR_BELOW, c_lo, 0), (HC.FAR_ABOVE, c_hi, 1)):
            far = HC.with_range(a, prange)
            assert HC.clamp_shares(HC.frustum_reference(far)["p"])[share] == 1.0
            assert HC.distinct_bits(HC.emulate_frustum(far)[1]) == want
        assert HC.bits_to_f32(c_lo[0]) == float(np.float32(np.log(float(np.float32(1e-5))))) and HC.bits_to_f32(c_hi[0]) == float(np.float32(np.log(float(np.float32(1.0) / np.float32(1e-5)))))
    assert r_p <= 0.62, "the emulation sat at 0.44 of dp when the bound was derived: well past that, the emulation or the reference has changed"


def test_frustum_case_list_covers_what_it_must():
    by = HC.FRUSTUM_BY_NAME
    assert len(by) == len(HC.FRUSTUM_CASES) == 25
    assert {c[1] for c in HC.FRUSTUM_CASES} == set(HC.FRUSTUM_SHAPES) and {c[2] for c in HC.FRUSTUM_CASES} == set(HC.FRUSTUM_D)
    a = HC.frustum_case("1x2x5x9 D=64 pad_h+32")
    assert a["pad_h"] > 16 * a["h"] and a["pad_w"] == 16 * a["w"] and a["pad_w"] & (a["pad_w"] - 1)            # pad_w = 144: no power of two
    assert 2 * 5 * 9 * 64 > 256 and (2 * 5 * 9 * 64) % 256                                                    # several workgroups, a partial last one
    lid, flat = HC.frustum_case("2x2x2x3 D=33")["cd"].double(), HC.frustum_case("2x2x2x3 D=33 uniform bins")["cd"].double()
    assert float((lid.diff().diff()).abs().min()) > 1e-3 and float(flat.diff().diff().abs().max()) < 1e-4       # LID bins widen, the others do not
    for name in ("1x3x3x7 D=30 bin0=0", "1x3x3x7 D=33 narrow B bin0=0"):
        assert float(HC.frustum_case(name)["cd"][0]) == 0.0                                                    # the fmaxf(dep, 1e-5f) branch
    a = HC.frustum_case("1x3x3x7 D=33")
    tok, _, _, view, tok_in_b = HC._token_index(a)
    assert int(((view // 3) * 3 + tok_in_b % 3 != view).sum()) >= 12, "N = 3, hw = 21: the camera rule differs from the view on most tokens"
    assert len({float(a["intr"][n, 0, 0]) for n in range(3)}) == 3


@pytest.mark.parametrize("name", HC.FRUSTUM_CLAMP_CASES)
def test_clamp_shares(name):
    ref = HC.frustum_reference(HC.frustum_case(name))
    low, high, inside = HC.clamp_shares(ref["p"])
    _, _, _, pin_lo, pin_hi = HC.pos_in_band(ref["p"], ref["dp"])
    print(f"{name}: {100 * low:.1f} % at or below 0, {100 * high:.1f} % at or above 1, {100 * inside:.1f} % inside; pinned exactly: {int(pin_lo.sum())} / {int(pin_hi.sum())}")
    assert low >= 0.05 and high >= 0.05 and inside >= 0.50
    assert int(pin_lo.sum()) >= 0.05 * pin_lo.numel() - 3 and int(pin_hi.sum()) >= 0.05 * pin_hi.numel() - 3
    # the floors of inverse_sigmoid (0 < p < 1e-5 or 1 - 1e-5 < p < 1) need not hold an element; the bracket is right there whether they do or not


def test_frustum_planted_errors_exceed_the_bound():
    a = HC.frustum_case("1x3x3x7 D=33")
    ref = HC.frustum_reference(a)
    good = HC.frustum_ratios(ref, *HC.emulate_frustum(a)[1:])
    assert max(good[:4]) <= 1.0
    corner = HC.frustum_ratios(ref, *HC.emulate_frustum(a, drop_half=True)[1:])
    bin29 = HC.frustum_ratios(ref, *HC.emulate_frustum(a, cone_bin=29)[1:])
    cam = HC.frustum_ratios(ref, *HC.emulate_frustum(a, camera_is_view=True)[1:])
    print(f"planted: pixel corner pos_in {corner[0]:.3g} cone {corner[2]:.3g}; bin D-29 cone {bin29[3]:.3g}; camera = view cone {cam[1]:.3g}")
    assert corner[0] > 1.0 and corner[2] > 1.0 and corner[3] > 1.0
    assert bin29[3] > 1.0 and bin29[0] <= 1.0 and bin29[2] <= 1.0
    assert cam[1] > 1.0 and cam[0] <= 1.0 and cam[2] <= 1.0


def test_frustum_smallest_shift_caught():
    """Every interior p of cone (0.01 < p < 0.99, columns 2..7 of every case) moved k ulps, up or down: the smallest k at which one of them leaves dp, and the
    smallest at which each of them does.  The figures stand in head_rows_cases's docstring."""
    parts = []
    for c in HC.FRUSTUM_CASES:
        a = HC.frustum_case(c[0])
        ref = HC.frustum_reference(a)
        got = HC.emulate_frustum(a)[2][:, 2:]
        val, dp = ref["cone"][:, 2:].numpy(), ref["dcone"][:, 2:].numpy()
        keep = (val > 0.01) & (val < 0.99)
        parts.append((got[keep], val[keep], dp[keep]))
    got, val, dp = (np.concatenate(x) for x in zip(*parts))
    assert len(got) > 2000
    first = every = None
    for k in range(1, 400):
        r = np.minimum(np.abs(HC.shift_ulps(got, k).astype(np.float64) - val), np.abs(HC.shift_ulps(got, -k).astype(np.float64) - val)) / dp
        r_any = np.maximum(np.abs(HC.shift_ulps(got, k).astype(np.float64) - val), np.abs(HC.shift_ulps(got, -k).astype(np.float64) - val)) / dp
        if first is None and r_any.max() > 1.0:
            first = k
        if r.min() > 1.0:
            every = k
            break
    dp_ulps = dp / np.spacing(got.astype(np.float32)).astype(np.float64)
    print(f"frustum bound on {len(got)} interior p: dp = {dp_ulps.min():.1f} .. {dp_ulps.max():.1f} ulps of p; first element caught at a shift of {first} ulps, every element at {every}")
    assert first is not None and every is not None and first <= 4 and every <= 400


# ---- MLN ---------------------------------------------------------------------------------------------------------------------------------------------------------
def mln_cases():
    for E in HC.MLN_E:
        for M in HC.MLN_M:
            for profile in HC.MLN_PROFILES + (("constant",) if E in HC.MLN_CONSTANT_E else ()):
                yield E, M, profile


@pytest.mark.parametrize("E", HC.MLN_E)
def test_mln_emulation_inside_the_bound_in_both_orders(E):
    for E_, M, profile in mln_cases():
        if E_ != E:
            continue
        x, g, b = HC.mln_inputs(M, E, profile)
        val, bound = HC.mln_reference(x, g, b)
        ratios = {order: HC.worst(HC.emulate_mln(x, g, b, order=order), val, bound) for order in ("lanes", "sequential")}
        print(f"mln E={E} M={M} {profile}: lanes {ratios['lanes']:.3f} sequential {ratios['sequential']:.3f}")
        assert max(ratios.values()) <= 1.0, (M, profile, ratios)
        if profile == "constant":
            assert np.array_equal(HC.emulate_mln(x, g, b).view(np.int32), b.numpy().view(np.int32)), "a constant row at a power-of-two E gives beta bit for bit"


def test_mln_planted_errors_exceed_the_bound():
    for E in (63, 64, 65, 100, 1000, 1024):
        x, g, b = HC.mln_inputs(5, E, "ordinary")
        val, bound = HC.mln_reference(x, g, b)
        r = HC.worst(HC.emulate_mln(x, g, b, var_div=E - 1), val, bound)
        print(f"planted: variance over E - 1 at E={E}: {r:.3g}")
        assert r > 1.0
        x, g, b = HC.mln_inputs(5, E, "spread 1e-3")
        val, bound = HC.mln_reference(x, g, b)
        r = HC.worst(HC.emulate_mln(x, g, b, eps=1e-6), val, bound)
        print(f"planted: eps 1e-6 on rows of spread 1e-3 at E={E}: {r:.3g}")
        assert r > 1.0
    for profile in HC.MLN_PROFILES:
        x, g, b = HC.mln_inputs(5, 65, profile)
        val, bound = HC.mln_reference(x, g, b)
        r = HC.worst(HC.emulate_mln(x, g, b, drop_col=64), val, bound)          # column 64: lane 0's second register, the only one of the lane tail
        print(f"planted: column 64 left out of the sum at E=65, {profile}: {r:.3g}")
        assert r > 1.0


# ---- sigmoids ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_sigmoid_emulation_inside_the_bound():
    z = torch.cat([torch.linspace(-120.0, 120.0, 48001), torch.tensor(HC.SPECIAL_LOGITS)]).float()
    s, ds = HC.sigmoid_reference(z)
    got = HC.emulate_sigmoid(z)
    r = HC.worst(got, s, ds)
    print(f"sigmoid over [-120, 120]: {r:.3f}; at -89 -> {float(got[-5]):.3e} (f64 {float(s[-5]):.3e})")
    assert r <= 1.0 and bool(np.isfinite(got).all()) and got.min() >= 0.0 and got.max() <= 1.0
    assert HC.worst(got * np.float32(1.0 + 2.0 ** -20), s, ds) > 1.0, "a relative error of 16 u is caught"
    z = HC.logits(257, seed=1)
    assert all(float(np.float32(v)) in set(z[-len(HC.SPECIAL_LOGITS):].tolist()) for v in HC.SPECIAL_LOGITS) and float(z[-1]) == 0.0, "the special logits sit in the last elements"
    cls = HC.logits(30, seed=2).view(10, 3)
    sc, dsc = HC.score_reference(cls)
    assert HC.worst(HC.emulate_sigmoid(cls).max(1), sc, dsc) <= 1.0


# ---- memory ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_memory_emulations_inside_the_bounds():
    rows = []
    only_4u = 0.0
    for L in HC.MEM_LEN:
        for npg in sorted({0, 1, L}):
            for fresh in (0, 1):
                data = HC.frame_data(HC.MEM_B, seed=L + npg)
                bank = HC.memory_bank(HC.MEM_B, L + 3, L, 4, seed=L + 7 * npg, zero=bool(fresh))
                pseudo = torch.rand(max(npg, 1), 3, generator=torch.Generator().manual_seed(L))
                _, approx = HC.pre_update_reference(bank, data, pseudo, L, npg, fresh)
                pose, ref = HC.emulate_pre_update(bank, data, pseudo, L, npg, fresh)
                r = HC.worst(pose, *approx["pose"]), HC.worst(ref, *approx["ref"])
                rows.append(r)
                if npg:       # the same slots against 4 u (|ref| + |ps|) alone
                    pc = data["pc"].double()
                    prod = pseudo.double()[:npg] * (pc[3:] - pc[:3])
                    nx = (1.0 - data["prev"].double())[:, None, None]
                    val, b = approx["ref"]
                    b4 = b[:, :npg] - 2 * U * prod.abs()[None] * nx
                    e = (torch.as_tensor(ref[:, :npg]).double() - val[:, :npg]).abs()
                    only_4u = max(only_4u, float((e[b4 > 0] / b4[b4 > 0]).max()))
                assert max(r) <= 1.0, (L, npg, fresh, r)
    print(f"pre_update emulation: pose {max(r[0] for r in rows):.3f} ref {max(r[1] for r in rows):.3f}; propagated ref against 4 u (|ref| + |ps|) alone: {only_4u:.3f}")
    worst_post = [0.0, 0.0]
    for topk, Qs in HC.MEM_TOPK_Q.items():
        for Q in Qs:
            for L in HC.MEM_LEN:
                data, bank = HC.frame_data(HC.MEM_B, seed=Q), HC.memory_bank(HC.MEM_B, L + topk, L, 4, seed=Q + L)
                dec = HC.post_update_inputs(HC.MEM_B, Q, 4, 8, seed=Q + topk)
                _, approx = HC.post_update_reference(bank, data, dec, L, topk)
                pose, ref = HC.emulate_post_update(bank, data, dec, L, topk)
                worst_post = [max(worst_post[0], HC.worst(pose, *approx["pose"])), max(worst_post[1], HC.worst(ref, *approx["ref"]))]
    print(f"post_update emulation: pose {worst_post[0]:.3f} ref {worst_post[1]:.3f}")
    assert max(worst_post) <= 1.0


def test_memory_planted_errors_exceed_the_bound():
    """A transposed read of a fresh row's pose, velocity from the wrong columns, the reference point of another query."""
    L, topk, Q = 5, 16, 17
    data, bank = HC.frame_data(HC.MEM_B, seed=1), HC.memory_bank(HC.MEM_B, L + topk, L, 4, seed=2)
    dec = HC.post_update_inputs(HC.MEM_B, Q, 4, 8, seed=3)
    exact, approx = HC.post_update_reference(bank, data, dec, L, topk)
    tr = dict(dec, rec=dec["rec"].view(HC.MEM_B, Q, 4, 4).transpose(2, 3).reshape(HC.MEM_B, Q, 16).contiguous())
    pose_t, _ = HC.emulate_post_update(bank, data, tr, L, topk)
    assert HC.worst(pose_t[:, :topk], approx["pose"][0][:, :topk], approx["pose"][1][:, :topk]) > 1.0
    assert HC.worst(pose_t[:, topk:], approx["pose"][0][:, topk:], approx["pose"][1][:, topk:]) <= 1.0
    assert torch.equal(exact["vel"][:, :topk], torch.gather(dec["bbox"][:, :, 6:8], 1, dec["order"][:, :topk, None].expand(-1, -1, 2)))
    ident = dict(dec, rec=torch.eye(4).flatten().repeat(HC.MEM_B, Q, 1))
    a, b = HC.emulate_post_update(bank, data, ident, L, topk)[0], HC.emulate_post_update(bank, data, dict(ident, rec=ident["rec"].view(HC.MEM_B, Q, 4, 4).transpose(2, 3).reshape(HC.MEM_B, Q, 16)), L, topk)[0]
    assert np.array_equal(a, b), "with the identity the transposed read shows nothing: why rec_ego_pose differs per query here"
