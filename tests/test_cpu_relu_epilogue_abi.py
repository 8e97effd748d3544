"""CPU: the ABI surface of the ReLU epilogue (TOC3D_EPI_BIAS_RELU = 10) and of the token-side row kernels' planes output (TOC3D_DTYPE_F32X3P).

Both are new VALUES of existing arguments: no entry point is added or re-signed, the ABI version stays where tests/test_cpu_head_queries_abi.py pins it.  The
argument checks run before any launch, so the device pointers here are made-up aligned addresses that are never dereferenced; only refusing calls and calls that
return before a launch (M = 0; a dtype no kernel serves) are made -- as in test_cpu_head_queries_abi.py.

Deliberate gap: of the three row kernels only toc3d_mln_apply has a call that returns before its launch (M = 0), so only its ACCEPTANCE of F32X3P is asserted
here.  toc3d_head_frustum_inputs and toc3d_nchw_to_rows launch on every accepted call; here they get their refusals (which show that the dtype is recognised as
planes: only F32X3P reaches the planes message), and their accepted launches are checked on the GPU in tests/test_gpu_head_tokens_x3.py."""
import ctypes
import os
import re

import pytest

from toc3d_amd import lib

A = 0x10000                                  # 128-byte aligned stand-in for device buffers
ERR_ARG = -1
CSRC = os.path.join(os.path.dirname(lib.LIB_PATH), "csrc")
PLANES_FAMILY = (lib.F32X3W, lib.F32X3WA, lib.F32X3WO, lib.F32X3P)
ALL_DTYPES = (lib.BF16, lib.F32, lib.F32X3, lib.F32X6) + PLANES_FAMILY
RELU, BIAS = lib.EPI_BIAS_RELU, lib.EPI_BIAS


def err():
    return lib.load().toc3d_last_error().decode()


def linear(dtype, epi, entry="toc3d_linear", **over):
    """One call of toc3d_linear / _ex / _fused with M = 0 unless overridden: passes the argument checks and returns before the launch, or is refused."""
    a = dict(A=A, lda=128, W=A, ldw=128, bias=A, out=A, ldo=160, res=None, ldr=0, rrm=0, rep=None, rep_i=None, M=0, N=130, K=128, nv=0, res_i=None, variant=0)
    a.update(over)
    l = lib.load()
    head = (a["A"], a["lda"], a["W"], a["ldw"], a["bias"], a["out"], a["ldo"], a["res"], a["ldr"], a["rrm"], a["rep"], a["rep_i"], a["M"], a["N"], a["K"], a["nv"])
    if entry == "toc3d_linear":
        rc = l.toc3d_linear(dtype, epi, *head, None)
    elif entry == "toc3d_linear_ex":
        rc = l.toc3d_linear_ex(dtype, epi, a["variant"], *head, None)
    else:
        rc = l.toc3d_linear_fused(dtype, epi, a["variant"], *head, None, 0, None, 0, None, 0, 0.0, None, 0, a["res_i"], None)
    return rc, err()


def test_header_binding_and_sources_agree_on_the_code():
    raw = open(lib.HEADER_PATH).read()
    assert int(re.search(r"#define\s+TOC3D_EPI_BIAS_RELU\s+(\d+)", raw).group(1)) == lib.EPI_BIAS_RELU == 10
    codes = {n: int(v) for n, v in re.findall(r"#define\s+TOC3D_EPI_(\w+)\s+(\d+)", lib.header_text())}
    assert sorted(codes.values()) == list(range(11)), "epilogue codes are 0..10, each once"
    assert all(getattr(lib, "EPI_" + n) == v for n, v in codes.items())
    # the comment next to the define says what kind of ABI change this is
    note = raw[raw.index("#define TOC3D_EPI_QKV_ROPE"):raw.index("#define TOC3D_EPI_BIAS_RELU")]
    assert "TOC3D_ABI_VERSION stays 11" in note and "no entry point is added" in note
    # the sources take the codes from the header (capi.h includes it; common.h and the kernels define none of their own)
    assert '#include "../../include/toc3d.h"' in open(os.path.join(CSRC, "capi.h")).read()
    for f in os.listdir(CSRC):
        if f.endswith((".h", ".hip", ".cpp")):
            assert not re.search(r"#define\s+TOC3D_EPI_", open(os.path.join(CSRC, f)).read()), f
    # no entry point came or went with it: the binding's table still names exactly the header's int-returning functions it named before
    assert set(lib._SIGS) <= set(lib.header_functions()) and lib.ABI_VERSION == 11


@pytest.mark.parametrize("entry", ["toc3d_linear", "toc3d_linear_ex", "toc3d_linear_fused"])
@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_epilogue_10_passes_the_argument_checks_wherever_bias_does(entry, dtype):
    lda = 128
    for epi in (BIAS, RELU):
        rc, msg = linear(dtype, epi, entry, lda=lda)
        assert rc == 0, (epi, msg)


@pytest.mark.parametrize("over,reason", [
    (dict(K=100), "multiple of 64"), (dict(ldo=128), "ldo < N"), (dict(lda=64), "leading dims smaller than K"), (dict(A=A + 4), "16-byte aligned"),
    (dict(N=0), "bad dims"), (dict(out=None), "null buffer"), (dict(lda=130), "rows must be 16-byte aligned"),
])
@pytest.mark.parametrize("dtype", [lib.BF16, lib.F32, lib.F32X3, lib.F32X6, lib.F32X3P])
def test_epilogue_10_is_refused_exactly_where_bias_is(dtype, over, reason):
    want = linear(dtype, BIAS, **over)
    got = linear(dtype, RELU, **over)
    assert want[0] == ERR_ARG and reason in want[1] and "toc3d_linear" in want[1], want
    assert got == want


def test_epilogue_10_named_refusals():
    # A rows in planes are whole 32-element groups, as for EPI_BIAS
    for dt in (lib.F32X3P, lib.F32X3WA):
        rc, msg = linear(dt, RELU, "toc3d_linear_fused", lda=144, K=128)
        assert rc == ERR_ARG and "whole 32-element groups" in msg, msg
        assert linear(dt, BIAS, "toc3d_linear_fused", lda=144, K=128) == (rc, msg)
    # a residual_index belongs to the residual epilogues
    rc, msg = linear(lib.F32, RELU, "toc3d_linear_fused", res_i=A)
    assert rc == ERR_ARG and "residual_index needs a residual epilogue" in msg
    # split-K serves the residual epilogues only: the workspace entry point names the epilogue it refuses
    l = lib.load()
    for epi in (BIAS, RELU):
        rc = l.toc3d_linear_fused_ws(lib.BF16, epi, 4014, A, 1024, A, 1024, A, A, 256, None, 0, 0, None, None, 0, 256, 1024, 0, None, 0, None, 0, None, 0, 0.0,
                                     None, 0, None, A, 1 << 20, None)
        assert rc == ERR_ARG and f"split-K serves the residual epilogues (1, 5, 6), not {epi}" in err()
    # the codes on either side of it stay what they were
    rc, msg = linear(lib.F32, 11)
    assert rc == ERR_ARG and "epilogue 11" in msg
    rc, msg = linear(lib.F32, lib.EPI_QKV_ROPE)
    assert rc == ERR_ARG and "epilogue 9" in msg
    rc, msg = linear(lib.BF16, lib.EPI_SWIGLU_STATS, "toc3d_linear_ex")
    assert rc == ERR_ARG and "takes the extra arguments of toc3d_linear_fused" in msg
    rc, msg = linear(lib.F32X3, lib.EPI_QKV_ROPE, "toc3d_linear_fused")
    assert rc == ERR_ARG and "serve epilogues 0-3, 10" in msg


# ---- token-side row kernels: TOC3D_DTYPE_F32X3P ------------------------------------------------------------------------------------------------------------
I2L = INTR = CD = A
PR = (ctypes.c_float * 6)(-61.2, -61.2, -10.0, 61.2, 61.2, 10.0)


def frustum(dtype, pos=A, ld_pos=192, cone_act=A, ld_cone=64):
    rc = lib.load().toc3d_head_frustum_inputs(dtype, I2L, INTR, CD, PR, 1, 2, 3, 4, 64, 16, 48, 64, pos, ld_pos, cone_act, ld_cone, A, None)
    return rc, err()


def nchw(dtype, out=A, ldo=64):
    rc = lib.load().toc3d_nchw_to_rows(dtype, A, out, ldo, 2, 40, 12, None)
    return rc, err()


def mln(dtype, out_act=A, ld_act=64, M=0):
    rc = lib.load().toc3d_mln_apply(dtype, A, A, A, M, 64, A, out_act, ld_act, None)
    return rc, err()


@pytest.mark.parametrize("call,name,bad", [
    (frustum, "toc3d_head_frustum_inputs: pos_in", [dict(ld_pos=200), dict(pos=A + 64), dict(pos=A + 16)]),
    (frustum, "toc3d_head_frustum_inputs: cone_act", [dict(ld_cone=40), dict(ld_cone=8), dict(cone_act=A + 32)]),
    (nchw, "toc3d_nchw_to_rows: out", [dict(ldo=40), dict(ldo=72), dict(out=A + 64)]),
    (mln, "toc3d_mln_apply: out_act", [dict(ld_act=72), dict(out_act=A + 8), dict(out_act=A + 64, M=5)]),
])
def test_row_kernels_refuse_bad_planes_rows_by_name(call, name, bad):
    for over in bad:
        rc, msg = call(lib.F32X3P, **over)
        assert rc == ERR_ARG and name in msg and "128-byte boundaries" in msg and "multiple of 32" in msg, (over, msg)


def test_row_kernels_accept_planes_and_keep_their_other_refusals():
    # the empty call returns before the launch: F32X3P on aligned rows passes every check (the launches themselves: tests/test_gpu_head_tokens_x3.py)
    assert mln(lib.F32X3P)[0] == 0 and mln(lib.F32)[0] == 0 and mln(lib.BF16)[0] == 0
    # a leading dimension that F32 / BF16 accept (any >= the row) is only refused for planes: a dtype no kernel serves gets past the planes check to "bad dtype"
    for call, over in ((frustum, dict(ld_pos=200)), (nchw, dict(ldo=40)), (mln, dict(ld_act=72, M=5))):
        for dt in (lib.F32X3, lib.F32X3W, lib.F32X6, 99):
            rc, msg = call(dt, **over)
            assert rc == ERR_ARG and "bad dtype" in msg, (dt, msg)
    # the dimension checks come first and are unchanged
    rc, msg = frustum(lib.F32X3P, ld_pos=160)
    assert rc == ERR_ARG and "bad dims" in msg
    rc, msg = nchw(lib.F32X3P, ldo=32)
    assert rc == ERR_ARG and "bad arguments" in msg
    rc, msg = mln(lib.F32X3P, ld_act=32)
    assert rc == ERR_ARG and "bad arguments" in msg
