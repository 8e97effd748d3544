"""GPU: TOC3D_EPI_BIAS_RELU -- relu(A.W^T + bias) in the GEMM epilogue -- against the two-launch sequence it replaces and against f64.

For every dtype EPI_BIAS is served in (BF16, F32, F32X3, F32X6, and the planes family F32X3W / WA / WO / P: all of them leave `out` plain in the act dtype, so there is
no planes image of the output to recombine -- the planes forms are held to the bits of F32X3 instead), M in {1, 63, 64, 65, 129} x N in {8, 64, 72, 130} x K in
{64, 192}, and the tile variants gemm.small_m_variant can return for a GEMM without a residual (0 = the library's default tile through toc3d_linear, 14 through
toc3d_linear_ex and toc3d_linear_fused; its third value, the split-K variant, serves residual epilogues only and is asserted refused by name):

  * the output is BIT-EQUAL to EPI_BIAS followed by toc3d_relu_inplace on the same variant -- inputs centred (about half the pre-activations negative), one column
    NaN (a NaN bias: relu gives 0), one column a tiny negative and one a negative f32 denormal (zero weights: relu gives +0);
  * it lies within the bars tests/test_gpu_epilogue_tails.py holds these output classes to (TOL_* of tests/epilogue_cases.py:
    bf16-rounded 6e-3, f32 and the bf16 x 3 / x 6 forms 2e-5 of the output's max) against f64 relu(A.W^T + b) on the operands the kernel reads;
  * canaries around the written region (spare rows and columns) are untouched."""
import functools

import pytest
import torch

from toc3d_amd import gemm, lib

from epilogue_cases import TOL_BF16, TOL_F32
from support import DEV, S, a_planes, bits, canary, check_untouched, pack, relerr, rnd, ru, to_planes

pytestmark = pytest.mark.gpu
MS, NS, KS = (1, 63, 64, 65, 129), (8, 64, 72, 130), (64, 192)
DTYPES = {"bf16": lib.BF16, "f32": lib.F32, "f32x3": lib.F32X3, "f32x6": lib.F32X6, "f32x3w": lib.F32X3W, "f32x3wa": lib.F32X3WA, "f32x3wo": lib.F32X3WO,
          "f32x3p": lib.F32X3P}
NAN_COL, TINY_COL, DENORM_COL = 1, 2, 5


def variants():
    """Every variant small_m_variant returns over the shapes of this file (and the head's), split by whether a residual-free GEMM can take it."""
    seen = {gemm.small_m_variant(M, N, K, r) for M in MS + (900, 6000) for N in NS + (256, 1024) for K in KS + (2048,) for r in (False, True)}
    assert seen == {0, 14, gemm.SPLITK_VARIANT}
    return (0, 14), gemm.SPLITK_VARIANT


@functools.lru_cache(maxsize=None)
def operands(N, K):
    """W [N, K], bias [N] with the special columns; f32, on the device."""
    W = rnd(N, K, seed=100 + N + K, scale=K ** -0.5)
    b = 0.3 * rnd(N, seed=200 + N)
    W[[NAN_COL, TINY_COL, DENORM_COL]] = 0.0
    b[NAN_COL], b[TINY_COL], b[DENORM_COL] = float("nan"), -1e-30, -1e-40
    return W, b.to(DEV)


@functools.lru_cache(maxsize=None)
def rows(K):
    return rnd(max(MS), K, seed=300 + K)


def launch(dt, epi, v, a_in, w_in, b, M, N, K, tdt):
    out = canary(M + 8, ru(N, 32) + 32, tdt)
    ldo = out.shape[1]
    head = (a_in, K, w_in, w_in.shape[1], b, out, ldo, None, 0, 0, None, None, M, N, K, 0)
    if v == 0:
        lib.call("toc3d_linear", dt, epi, *head, S())
    elif M % 2:
        lib.call("toc3d_linear_ex", dt, epi, v, *head, S())
    else:
        lib.call("toc3d_linear_fused", dt, epi, v, *head, *lib.NO_FUSED, S())
    return out


@pytest.mark.parametrize("form", list(DTYPES))
def test_relu_epilogue_equals_bias_then_relu_and_f64(form):
    dt = DTYPES[form]
    bf = dt == lib.BF16
    pdt, tdt = (lib.BF16, torch.bfloat16) if bf else (lib.F32, torch.float32)
    tol = TOL_BF16 if bf else TOL_F32
    served, splitk = variants()
    worst = 0.0
    ws = torch.zeros(1 << 20, dtype=torch.int32, device=DEV)
    for K in KS:
        A = rows(K).to(DEV).to(tdt).contiguous()
        a_in = to_planes(A) if a_planes(dt) else A
        for N in NS:
            W, b = operands(N, K)
            Wp = pack(W, pdt, tdt)
            w_in = to_planes(Wp) if dt in (lib.F32X3W, lib.F32X3WA, lib.F32X3WO, lib.F32X3P) else Wp
            lin = A.double() @ Wp[:N].double().T + b.double()
            ref = torch.where(lin > 0, lin, torch.zeros_like(lin))              # relu(v) = v > 0 ? v : 0: NaN -> 0
            assert 0.3 < float((lin[:, 6:] < 0).double().mean()) < 0.7 or N == 8, "about half the pre-activations are negative"
            for M in MS:
                for v in served:
                    tag = f"{form} M={M} N={N} K={K} v{v}"
                    fused = launch(dt, lib.EPI_BIAS_RELU, v, a_in, w_in, b, M, N, K, tdt)
                    two = launch(dt, lib.EPI_BIAS, v, a_in, w_in, b, M, N, K, tdt)
                    assert bool(torch.isnan(two[:M, NAN_COL].float()).all()) and bool((two[:M, TINY_COL].float() < 0).all()), f"{tag}: the inputs do not reach the edge cases"
                    lib.call("toc3d_relu_inplace", pdt, two, two.numel(), S())     # (the canary is positive: ReLU leaves it as it is)
                    assert torch.equal(bits(fused), bits(two)), f"{tag}: not the bits of EPI_BIAS + toc3d_relu_inplace"
                    for c in (NAN_COL, TINY_COL, DENORM_COL):
                        assert bool((bits(fused[:M, c]) == 0).all()), f"{tag}: column {c} must be +0"
                    e = relerr(fused[:M, :N], ref[:M])
                    worst = max(worst, e)
                    assert e < tol, f"{tag}: rel err vs f64 {e:.3e} (bar {tol:.0e})"
                    check_untouched(tag, fused, M, N, False)
                    if v == served[0] and dt not in (lib.BF16, lib.F32, lib.F32X3, lib.F32X6):
                        # the planes forms leave `out` plain and return the bits of the form that splits in LDS
                        base = launch(lib.F32X3, lib.EPI_BIAS_RELU, v, A, Wp, b, M, N, K, tdt)
                        assert torch.equal(bits(fused), bits(base)), f"{tag}: not the bits of F32X3"
            with pytest.raises(RuntimeError, match=r"split-K serves the residual epilogues \(1, 5, 6\), not 10"):
                out = canary(MS[-1] + 8, ru(N, 32) + 32, tdt)
                lib.call("toc3d_linear_fused_ws", dt, lib.EPI_BIAS_RELU, splitk, a_in, K, w_in, w_in.shape[1], b, out, out.shape[1], None, 0, 0, None, None,
                         MS[-1], N, K, 0, *lib.NO_FUSED, ws, ws.numel() * 4, S())
    print(f"[relu epilogue {form}] worst rel err vs f64 over {len(MS) * len(NS) * len(KS) * len(served)} launches: {worst:.3e} (bar {tol:.0e})")


@pytest.mark.parametrize("form", ["f32x3wa", "bf16"])
@pytest.mark.parametrize("N,K", [(1024, 192), (256, 256), (256, 64)])
def test_relu_epilogue_at_the_token_sides_shapes(form, N, K):
    """M = 6000 (47 row tiles, a tail of 112 rows) at the widths of the head's four Linear + ReLU, on the tile the host picks for them (the default tile at
    N = 1024, 64x64 at N = 256) and in the dtypes the token side launches: bit-equal to the two-launch form, within the bar of f64, canaries untouched."""
    dt = DTYPES[form]
    bf = dt == lib.BF16
    pdt, tdt = (lib.BF16, torch.bfloat16) if bf else (lib.F32, torch.float32)
    M = 6000
    A = rnd(M, K, seed=400 + K).to(DEV).to(tdt).contiguous()
    W, b = operands(N, K)
    Wp = pack(W, pdt, tdt)
    a_in, w_in = (A, Wp) if bf else (to_planes(A), to_planes(Wp))
    v = gemm.small_m_variant(M, N, K, False)
    assert v == (0 if N == 1024 else 14)
    lin = A.double() @ Wp[:N].double().T + b.double()
    ref = torch.where(lin > 0, lin, torch.zeros_like(lin))
    fused = launch(dt, lib.EPI_BIAS_RELU, v, a_in, w_in, b, M, N, K, tdt)
    two = launch(dt, lib.EPI_BIAS, v, a_in, w_in, b, M, N, K, tdt)
    lib.call("toc3d_relu_inplace", pdt, two, two.numel(), S())
    assert torch.equal(bits(fused), bits(two)), "not the bits of EPI_BIAS + toc3d_relu_inplace"
    e = relerr(fused[:M, :N], ref)
    print(f"[relu epilogue {form} M={M} N={N} K={K} v{v}] rel err vs f64 {e:.3e}")
    assert e < (TOL_BF16 if bf else TOL_F32)
    check_untouched(f"{form} M={M} N={N}", fused, M, N, False)
