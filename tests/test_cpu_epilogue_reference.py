"""CPU: the f64 references and the case enumerator of tests/test_gpu_epilogue_tails.py are themselves checked here -- a reference that is wrong, or a class that
silently has no case, would make the GPU matrix prove nothing."""
import pytest
import torch

import epilogue_cases as E
from support import rnd


@pytest.mark.parametrize("ln_n,K", E.ln_shapes())
@pytest.mark.parametrize("tdt", [torch.float32, torch.bfloat16])
def test_folded_identity_equals_the_explicit_layernorm_in_f64(ln_n, K, tdt):
    """rstd * (a . W' - mean * c1) + c2 == LN(a) . W' + c2 when c1 holds the row sums of the SAME rounded W': to 1e-12 in f64 at every (ln_n, K) of the matrix.
    The rows carry a mean and padding columns [ln_n, K) that must not count."""
    M, N, eps = 37, 72, 1e-6
    a = (3.0 * rnd(M, K, seed=1) + 0.7).to(tdt).float()
    a[:, ln_n:] = 9.0                                        # padding: read by neither form
    gamma, beta = 1.0 + 0.3 * rnd(ln_n, seed=2), 0.2 * rnd(ln_n, seed=3)
    w, b = rnd(N, ln_n, seed=4, scale=ln_n ** -0.5), rnd(N, seed=5)
    wp = torch.zeros(N, K)
    wp[:, :ln_n] = (gamma * w).to(tdt).float()               # the packed, rounded, gamma-scaled weights
    c1 = wp.double().sum(1)
    c2 = (w.double() * beta.double()).sum(1) + b.double()
    ref = E.explicit_ln_matmul(a, wp, c2, ln_n, eps)
    got = E.folded_ln_matmul(a, wp, c1, c2, ln_n, eps, torch.float64)
    err = ((got - ref).abs().max() / ref.abs().max()).item()
    assert err < 1e-12, err
    # ... and the explicit form is the LayerNorm torch computes (f64), with the affine folded into (W', c2) only up to the rounding of W'
    ln = torch.nn.functional.layer_norm(a[:, :ln_n].double(), (ln_n,), None, None, eps)
    assert torch.allclose(E.layernorm_rows_f64(a, ln_n, eps), ln, rtol=0, atol=1e-12)
    # the f32 evaluation of the folded form (the control of the GPU tests) stays far below the 2e-5 the kernels are held to
    ctl = E.folded_ln_matmul(a, wp, c1.float(), c2.float(), ln_n, eps, torch.float32)
    assert ((ctl - ref).abs().max() / ref.abs().max()).item() < 2e-6


def test_planes_helpers_round_trip():
    x = rnd(19, 96, seed=1) * 37.0
    x[0, :4] = torch.tensor([0.0, -0.0, 1.0, -3.5])
    img = E.planes_encode(x)
    assert img.shape == x.shape and img.dtype == torch.float32
    hi, lo = E.planes_planes(img)
    eh, el = E.planes_split(x)
    assert torch.equal(hi, eh) and torch.equal(lo, el)
    assert torch.equal(hi, x.to(torch.bfloat16).float()) and ((hi + lo) - x).abs().max() <= 2.0 ** -16 * x.abs().max()
    # the layout of include/toc3d.h: element c -> group c / 32, hi at bf16 index c % 32, lo at 32 + c % 32 of the group's 64
    raw = img.view(torch.bfloat16).view(19, 3, 64)
    assert raw[5, 1, 7].float() == hi[5, 39] and raw[5, 1, 32 + 7].float() == lo[5, 39]
    assert torch.equal(E.planes_encode(x).view(torch.int32), img.view(torch.int32))      # deterministic
    y = rnd(4, 64, seed=2).to(torch.bfloat16).float()        # values that are bf16 already: hi = the value, lo = 0
    hy, ly = E.planes_planes(E.planes_encode(y))
    assert torch.equal(hy, y) and torch.count_nonzero(ly) == 0


def test_swiglu_unit_order_and_slot_sums():
    Hd, Hp = 20, 32
    z = rnd(3, 2 * Hp, seed=2).double()
    h = E.swiglu_units(z, Hd, Hp)
    for u in (0, 15, 16, 19):
        b, i = divmod(u, 16)
        assert h[1, u] == torch.nn.functional.silu(z[1, 32 * b + i]) * z[1, 32 * b + 16 + i]
    assert torch.count_nonzero(h[:, Hd:]) == 0
    v = rnd(4, 200, seed=3)
    s = E.slot_sums(v, 132, 64)
    assert s.shape == (4, 3, 2)
    assert torch.allclose(s[:, 2, 0], v[:, 128:132].double().sum(1)) and torch.allclose(s[:, 0, 1], (v[:, :64].double() ** 2).sum(1))


@pytest.mark.parametrize("variant", sorted(E.VARIANTS))
@pytest.mark.parametrize("cls", E.ROW_CLASSES)
def test_every_row_class_has_a_case_for_every_variant(cls, variant):
    cases = E.row_cases(cls, variant)
    assert cases, f"no M of ROWS exercises {cls} on variant {variant}"
    assert all(0 < M < E.M_ALIGNED + 64 for M in cases)
    if cls in ("pair_then_past", "block_plus_one"):          # ... and not only through the short list's first-block cases
        assert any(M > E.VARIANTS[variant][1] for M in cases)


@pytest.mark.parametrize("cls", E.COL_CLASSES)
def test_every_column_class_has_a_configuration(cls):
    assert [n for n, c in E.COLS.items() if cls in E.col_classes(c)], f"no column configuration exercises {cls}"


def test_matrix_invariants():
    assert E.M_ALIGNED % 32 == 0 and all(M < E.M_ALIGNED for M in E.ROWS) and set(E.ROWS_SHORT) <= set(E.ROWS)
    assert {"m1", "m16", "even_partial", "even_alone", "odd_partial"} <= set().union(*(E.row_classes(M, 128, 64) for M in E.ROWS))
    assert set().union(*(E.row_classes(M, 128, 64) for M in E.ROWS_SHORT)) >= {"odd_partial", "block_plus_one", "below_slab"}
    for cfg in E.COLS.values():
        assert cfg["C"] <= E.C_FULL and cfg["K1"] % 64 == 0 and cfg["Hp"] % 16 == 0 and cfg["Hd"] <= cfg["Hp"]
    # slab heights of the launch table: 48, 64, 80, 96 and 128 rows; workgroup tiles of 96 .. 256 rows
    assert {v[1] for v in E.VARIANTS.values()} == {48, 64, 80, 96, 128} and {v[0] for v in E.VARIANTS.values()} == {96, 128, 160, 192, 256}
