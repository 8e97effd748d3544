"""CPU: the cases, bounds and emulation of tests/lnfold_cases.py are sound (no GPU): the case matrix covers every path of ln_rows_prepare_fn at every slot-count class,
the f32 emulation of the documented formula stays inside the derived bound on every case and family, every planted error lands outside it on a family the older inputs
did not have, and the one wrong reference that must not matter -- the folded formula in f64 -- is indistinguishable from the two-pass one."""
import pytest
import torch

import lnfold_cases as L
from support import report_lines

CASES = [(stage, slots) for stage in L.STAGES for slots in L.widths(stage)]
NEW = [f for f in L.FAMILY_NAMES if f not in L.OLD_FAMILIES]


def test_every_path_has_a_case_for_every_slot_count_class():
    """plain / early / phased (where the form has the path) x below 4 slots / on the prefetch / in the remainder loop, for both stages; the slot counts are the issue's."""
    assert sorted(L.W12_WIDTHS) == [1, 3, 4, 5, 6, 16, 17, 20] and sorted(L.W3_WIDTHS) == [1, 5, 43, 48, 49, 52]
    for slots, C in L.W12_WIDTHS.items():
        assert -(-C // 64) == slots
    for slots, (Hd, Hp) in L.W3_WIDTHS.items():
        assert -(-Hp // 64) == slots and Hd > 64 * (slots - 1) and Hp % 16 == 0 and Hp <= 3328       # the last slot holds valid units (the outlier column Hd - 1)
    for form in L.FORMS:
        for stage in L.STAGES:
            paths = L.paths_of(form, stage)
            assert "plain" in paths and (form != "bf16" or paths == ("plain", "early", "phased"))
            assert ("phased" in paths) == (form == "bf16" or L.dt_name(form, stage) in L.A_PLANES)
            for cls in ("lt4", "prefetch", "remainder"):
                for path in paths:
                    assert any(L.slot_class(stage, s) == cls and L.path_of(form, stage, v) == path for s in L.widths(stage) for v in L.VSET), (form, stage, cls, path)
    # the boundaries themselves: the last prefetched slot and the first of the remainder loop
    assert L.slot_class("w12", 16) == "prefetch" and L.slot_class("w12", 17) == "remainder" and L.slot_class("w3", 48) == "prefetch" and L.slot_class("w3", 49) == "remainder"
    # partly valid last slots and ln_n < K, and ln_n == K
    for stage in L.STAGES:
        shapes = [L.shape_of(stage, s) for s in L.widths(stage)]
        assert any(sh["ln_n"] % 64 and sh["ln_n"] < sh["K"] for sh in shapes) and any(sh["ln_n"] == sh["K"] for sh in shapes)
        assert all(sh["N"] <= 256 for sh in shapes)
    assert L.M <= 192 and L.M % 64 and L.M > 128


def test_families_interleave_and_cover_the_last_rows():
    for t0 in range(0, L.M, 16):
        assert len({L.family_of(i) for i in range(t0, min(t0 + 16, L.M))}) == min(16, L.M - t0)
    assert L.family_of(L.M - 1) != L.family_of(L.M - 2)
    assert all(len(L.family_rows(f)) >= 7 for f in L.FAMILY_NAMES)
    x = L.designed_rows(300, seed=1).double()
    for f, (mean, sigma, o1, o2, _) in L.FAMILIES.items():
        rows = x[L.family_rows(f)]
        if sigma == 0:
            assert bool((rows == mean).all()), f
        elif o1 == 0 and o2 == 0:
            assert abs(float(rows.mean()) - mean) < 0.2 * sigma and abs(float(rows.std()) / sigma - 1) < 0.1, f
        else:
            assert (o1 == 0 or abs(float(rows[:, 1].mean()) - o1) < 3) and (o2 == 0 or abs(float(rows[:, -1].mean()) - o2) < 3), f


@pytest.mark.parametrize("form", list(L.FORMS))
def test_emulation_stays_within_the_bound(form):
    """The f32 emulation of the documented formula against the two-pass f64 reference: every element of every case and family inside its bound; no element excluded; the
    padding hidden units exactly 0 with a bound of 0; the constant rows finite."""
    worst = {}
    for stage, slots in CASES:
        c = L.host_case(form, stage, slots)
        an, em = L.analyse(c), L.emulate(c)
        for key in L.outputs_of(stage):
            b = an["b_" + key]
            assert bool(torch.isfinite(b).all()) and bool(torch.isfinite(em[key]).all()), (form, stage, slots, key)
            if key == "hid":
                assert bool((b[:, :c["Hd"]] > 0).all()) and not b[:, c["Hd"]:].any() and not em[key][:, c["Hd"]:].any()
            else:
                assert bool((b > 0).all())                 # share of excluded elements: zero
            r = L.ratios(em[key], an, key)
            if key == "out":                               # constant rows: the two-pass reference is c2 (+ residual) exactly, rstd = eps^-1/2
                const = L.family_rows("const0") + L.family_rows("const3")
                assert torch.equal(an["out"][const], c["res"].double()[const] + c["c2"].double()) and bool((an["rstd"][const] == L.EPS ** -0.5).all())
            for f, v in L.worst_by_family(r).items():
                k = f"{form} {stage} {key} {f}"
                worst[k] = max(worst.get(k, 0.0), v)
            assert float(r.max()) <= 1.0, (form, stage, slots, key, float(r.max()))
    for line in report_lines("lnfold emulation", 36, worst):
        print(line)


# planted error -> the cases it is planted in (those where it changes anything: ln_n < K; < 4 slots; the remainder loop; bf16 for the rounding of W')
MUTANT_CASES = {
    "ln_n_is_K": [("f32x3", "w12", 1), ("bf16", "w3", 5)], "var_n_minus_1": [("f32x3", "w12", 1), ("bf16", "w12", 1)], "eps_1e-5": [("f32x3", "w12", 1), ("bf16", "w12", 3), ("bf16", "w3", 1)],
    "mean_bf16": [("f32x3p", "w12", 6), ("bf16", "w12", 3)], "c1_unrounded": [("bf16", "w12", 16), ("bf16", "w12", 3)],
    "last_slot_dropped": [("f32x3", "w12", 6), ("bf16", "w3", 49)], "slot_4PRE_dropped": [("f32x3p", "w12", 17), ("bf16", "w12", 20), ("f32x3wo", "w3", 49), ("bf16", "w3", 52)],
    "slot0_twice": [("f32x3", "w12", 1), ("bf16", "w12", 3), ("f32x3wa", "w3", 1)], "row_M-1_for_M-2": [("f32x3w", "w12", 4), ("bf16", "w3", 48)],
}


@pytest.mark.parametrize("mut", list(MUTANT_CASES))
def test_planted_errors_land_outside_the_bound(mut):
    """Each wrong reference, planted in the emulation, leaves the bound on at least one element of a family the older inputs (|mean| / sigma <= 0.25) did not have."""
    lines = []
    for form, stage, slots in MUTANT_CASES[mut]:
        c = L.host_case(form, stage, slots)
        an, em = L.analyse(c), L.emulate(c, mut)
        key = L.outputs_of(stage)[-1]
        wf = L.worst_by_family(L.ratios(em[key], an, key))
        out = {f: v for f, v in wf.items() if f in NEW and v > 1.0}
        lines.append(f"[lnfold mutant] {mut:<18s} {form} {stage} slots {slots}: worst ratio {max(wf.values()):.3g} ({len(out)} new families outside)")
        assert out, (mut, form, stage, slots, wf)
        if mut == "row_M-1_for_M-2":
            assert float(L.ratios(em[key], an, key)[L.M - 2].max()) > 1.0
    print("\n" + "\n".join(lines))


def test_an_unclamped_variance_yields_nan_exactly_where_it_falls_below_minus_eps():
    """`var` not clamped at 0 yields NaN -- sqrtf of a negative number, never inf -- on exactly the rows whose computed S2 / n - mean^2 lies below -eps (asserted row by row).
    Which rows those are: in front of w3 the constant row is silu(4) * 3, an f32 value with a full mantissa, so its squares round and the one-pass variance errs by
    ~ u mean^2 = 8e-6 > eps: every such row is NaN without the clamp (asserted: the constant rows are among them).  In front of w1|w2 the constant rows are exactly 0 and 3:
    the slot sums are exact, S2 / n - mean^2 = -9 d (1 + d) with d the error of float(1 / n), |d| <= 2^-25, above -eps: finite and inside the bound even without the clamp
    (asserted).  Rows with a variance far above eps are never touched by the clamp."""
    for form, stage, slots in (("f32x3", "w3", 5), ("f32x3p", "w3", 43), ("f32x3", "w3", 52), ("f32x3w", "w12", 20), ("bf16", "w12", 5)):
        c = L.host_case(form, stage, slots)
        an, em = L.analyse(c), L.emulate(c, "no_clamp")
        key = L.outputs_of(stage)[-1]
        S = L.combine_f64(c["stats"])
        inv = float(torch.tensor(1.0 / c["ln_n"], dtype=torch.float32))
        var = (S[:, 1] * inv - (S[:, 0] * inv) ** 2).float() + torch.tensor(L.EPS, dtype=torch.float32)
        bad = var < 0
        assert torch.equal(torch.isnan(em[key]).any(1), bad) and not torch.isinf(em[key]).any()
        assert all(float(an["var"][i]) < 10 * L.EPS for i in torch.nonzero(bad)[:, 0].tolist())
        const3 = L.family_rows("const3")
        if stage == "w3":
            assert bool(bad[const3].all())
        else:
            assert not bad.any() and float(L.ratios(em[key], an, key)[const3 + L.family_rows("const0")].max()) <= 1.0
        assert bool(torch.isfinite(L.emulate(c)[key]).all())       # ... and with the clamp every row is finite


@pytest.mark.parametrize("form", ["bf16", "f32x3", "f32x3p"])
def test_the_folded_formula_in_f64_is_indistinguishable(form):
    """The reference does not limit the test: the folded formula evaluated in f64 differs from the two-pass reference by less than 1e-3 of any element's bound."""
    worst = 0.0
    for stage, slots in CASES:
        c = L.host_case(form, stage, slots)
        an, wrong = L.analyse(c), L.folded_f64(c)
        for key in L.outputs_of(stage):
            worst = max(worst, float(L.ratios(wrong[key], an, key).max()))
    print(f"\n[lnfold] {form}: folded formula in f64 against two-pass f64: worst {worst:.2e} of the bound")
    assert worst < 1e-3
