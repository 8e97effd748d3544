"""CPU: what tests/test_gpu_attention_kernels.py holds the attention kernels to (tests/attention_cases.py), checked without a GPU, for every case the GPU file
runs: an emulation of the kernel's own rounding points stays inside the derived bound with no slack factor; every applicable wrong reference ("mutant") pushes at
least 25 % of the query rows of every (window, head) it touches beyond TWICE the bound in some element (the one-row mutant: that row); and the input
conditions the derivation relies on hold (delta <= DELTA_CAP so that e < 1, T below the flat family's cap, the spikes where the construction wants them)."""
import pytest
import torch

import attention_cases as AC

SHARE, FACTOR = 0.25, 2.0


@pytest.fixture(scope="module")
def emu_worst():
    worst = {}
    yield worst
    print("\n[attention cases] emulation: worst error as a fraction of the derived bound")
    for key in sorted(worst):
        print(f"[attention cases] {key:<44s} {worst[key]:.3f}")


def test_the_case_list_covers_every_body_and_boundary():
    bodies = {}
    for c in AC.CASES:
        bodies.setdefault((AC.body_of(c), c.kind), set()).add(c.family)
    want = [("attn_rot_kernel", "bf16"), ("attn_rot_x3_kernel<false>", "x3p"), ("attn_rot_x3_kernel<true>", "x3p")]
    want += [(f"attn_small_kernel<{m}>", "bf16") for m in (9, 11, 13)] + [("attn_kernel", kd) for kd in AC.PLAIN_KINDS]
    want += [(f"attn_small_kernel<{m}>", kd) for m in (9, 11) for kd in AC.PLAIN_KINDS]
    for key in want:
        assert bodies.get(key) == {"flat", "spike"}, key
    assert not any(b == "attn_small_kernel<13>" and kd != "bf16" for b, kd in bodies), "f32 buffers of more than 160 keys do not fit the small kernel's 96 KB"
    by = {c.name: c for c in AC.CASES}
    assert AC.body_of(by["rot-x3p-n288"]) == "attn_rot_x3_kernel<false>" and AC.body_of(by["rot-x3p-n289"]) == "attn_rot_x3_kernel<true>"
    assert AC.body_of(by["plain-bf16-n208"]) == "attn_small_kernel<13>" and AC.body_of(by["plain-bf16-n209"]) == "attn_kernel"
    assert AC.body_of(by["plain-f32-n144"]) == "attn_small_kernel<9>" and AC.body_of(by["plain-f32-n145"]) == "attn_small_kernel<11>"
    assert AC.body_of(by["plain-f32-n176"]) == "attn_kernel"


def test_edge_keys_and_loudness():
    assert AC.edge_keys(1) == [0] and AC.edge_keys(9) == [0, 7, 8]
    assert AC.edge_keys(401) == [0, 15, 16, 31, 32, 63, 64, 127, 128, 255, 256, 368, 369, 384, 385, 399, 400]
    assert AC.loud_of(1, 0) == 4 and AC.loud_of(64, 0) == 4 and AC.loud_of(65, 0) == 8 and AC.loud_of(401, 0) == 32 and AC.loud_of(8, 248) == 16 and AC.loud_of(401, 0, AC.Case("x", "plain", "bf16", 401)) == 128


@pytest.mark.parametrize("case", AC.CASES, ids=str)
def test_bound_admits_the_emulation_and_rejects_the_mutants(case, emu_worst):
    b = AC.build(case)
    ref = AC.reference(b)
    valid = ref["valid"]                                                        # [W, n]
    bnd = AC.bound(b, ref)
    out = ref["out"]
    assert bool(torch.isfinite(out[valid]).all()) and bool(torch.isfinite(bnd[valid]).all()) and bool((bnd[valid] > 0).all())
    # ---- input conditions ----
    _, delta = AC.eps_of(case, ref["T"], ref["Tp"])
    assert float(delta[valid].max()) <= AC.DELTA_CAP, f"delta {float(delta[valid].max()):.3f}"
    if case.family == "flat":
        assert float(ref["T"][valid].max()) <= AC.T_CAP_FLAT, float(ref["T"][valid].max())
        if case.neg:
            Sn = torch.einsum("wqhd,wkhd->whqk", ref["q"], ref["k"]) * ref["factor"]
            assert float(Sn.max()) < 0 and float(Sn.min()) > -2.0, "every real score below the pads' 0, none far below"
    else:
        S0 = torch.einsum("qhd,khd->hqk", ref["q"][0], ref["k"][0]) * ref["factor"]
        first = 32 if case.path == "rot" else 64
        assert float(S0.max() - S0[:, :, :first].max()) > (8 * AC.LN2 if case.path == "rot" else 2.0), "the planted spikes must move the reference point after the first chunk"
    # ---- the emulation of the kernel's rounding points is inside the bound, no slack ----
    emu = AC.emulate(b, ref)
    ratio = ((emu - out).abs() / bnd)[valid]
    assert float(ratio.max()) <= 1.0, f"emulation at {float(ratio.max()):.3f} x the bound"
    key = f"{AC.body_of(case)} {case.kind} {case.family}"
    emu_worst[key] = max(emu_worst.get(key, 0.0), float(ratio.max()))
    # ---- every applicable mutant is caught ----
    seen = set()
    for name, wrong, has, rows in AC.mutants(b, ref):
        seen.add(name[0])
        beyond = (((wrong - out).abs() > FACTOR * bnd).any(-1))                 # [W, n, H]
        if rows is not None:
            for w, i in rows:
                assert bool(beyond[w, i].any()), f"{name}: row {i} of window {w} stays within {FACTOR} x the bound"
            continue
        for w in torch.nonzero(has).flatten().tolist():
            share = beyond[w][valid[w]].double().mean(0)                        # per head
            assert float(share.min()) >= SHARE, f"{name}: window {w} moves only {float(share.min()):.2f} of its rows beyond {FACTOR} x the bound"
    if case.family == "flat":
        assert "a" in seen or case.n == 1 and not case.npad
        assert ("c" in seen and "d" in seen) == bool(case.npad) and ("f" in seen) == bool(case.virt_q and (case.path == "rot" or case.n - case.virt_q == 1 and case.kind != "bf16"))
    assert "e" in seen and ("g" in seen or case.n == 1 or case.virt_q == 1 or case.neg)
