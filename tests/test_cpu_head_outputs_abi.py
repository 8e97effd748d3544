"""CPU: every refusal of the four entry points of csrc/head_outputs.hip (toc3d_head_nan_to_num_rows, toc3d_head_ln_relu_rows, toc3d_head_outputs,
toc3d_nms_free_decode) is reached once and names its reason in toc3d_last_error().  The checks run before any launch, so the device pointers here are made-up
addresses that are never dereferenced (pc_range / post_center_range are HOST arrays and real); only refusing calls and the empty ones that return before the
launch are made."""
import ctypes

import pytest

from toc3d_amd import lib

A = 0x10000                                  # 128-byte aligned stand-in for device buffers
ERR_ARG = -1
HOST6 = (ctypes.c_float * 6)(-1, -1, -1, 1, 1, 1)


def _nan(dtype=lib.F32, **over):
    a = dict(x=A, ldx=64, out=A, ldo=64, act=A, ld_act=64, M=5, E=64)
    a.update(over)
    l = lib.load()
    rc = l.toc3d_head_nan_to_num_rows(dtype, a["x"], a["ldx"], a["out"], a["ldo"], a["act"], a["ld_act"], a["M"], a["E"], None)
    return rc, l.toc3d_last_error().decode()


@pytest.mark.parametrize("over,reason", [
    (dict(x=None), "bad arguments"), (dict(out=None, act=None), "bad arguments"), (dict(M=-1), "bad arguments"), (dict(E=0), "bad arguments"), (dict(E=62), "bad arguments"),
    (dict(ldx=60), "bad arguments"), (dict(ldx=66), "bad arguments"), (dict(x=A + 4), "bad arguments"),
    (dict(ldo=60), "out needs ldo >= E"), (dict(ldo=66), "out needs ldo >= E"), (dict(out=A + 8), "out needs ldo >= E"),
    (dict(ld_act=32), "ld_act < E"), (dict(ld_act=66), "f32 rows must be 16-byte aligned"), (dict(act=A + 8), "f32 rows must be 16-byte aligned"),
    (dict(M=((1 << 31) - 1) * 16 + 1), "too many elements"), (dict(M=1 << 40, E=1 << 24, ldx=1 << 24, ldo=1 << 24, ld_act=1 << 24), "too many elements"),
])
def test_nan_to_num_rows_refusals(over, reason):
    rc, msg = _nan(**over)
    assert rc == ERR_ARG and "toc3d_head_nan_to_num_rows" in msg and reason in msg, (rc, msg)


def test_nan_to_num_rows_dtypes_and_empty_call():
    rc, msg = _nan(dtype=lib.BF16, act=A + 4)
    assert rc == ERR_ARG and "bf16 rows must be 8-byte aligned" in msg
    rc, msg = _nan(dtype=lib.BF16, ld_act=66)
    assert rc == ERR_ARG and "bf16 rows must be 8-byte aligned" in msg
    for over in (dict(act=A + 64), dict(ld_act=80)):
        rc, msg = _nan(dtype=lib.F32X3P, **over)
        assert rc == ERR_ARG and "128-byte boundaries" in msg
    rc, msg = _nan(dtype=lib.F32X3P, E=80, ldx=96, ldo=96, ld_act=96)
    assert rc == ERR_ARG and "whole 32-element groups" in msg
    for dt in (lib.F32X3, lib.F32X3W, 99):
        rc, msg = _nan(dtype=dt)
        assert rc == ERR_ARG and "dtype must be" in msg
    assert _nan(M=0)[0] == 0 and _nan(M=0, dtype=lib.F32X3P, ld_act=96)[0] == 0
    assert _nan(M=0, act=None, ld_act=0, dtype=99)[0] == 0        # without an act output its dtype and leading dimension are not looked at


def _ln(dtype=lib.F32, **over):
    a = dict(x=A, ldx=128, gamma=A, beta=A, act=A, ld_act=128, M=5, E_ln=64, E_relu=64)
    a.update(over)
    l = lib.load()
    rc = l.toc3d_head_ln_relu_rows(dtype, a["x"], a["ldx"], a["gamma"], a["beta"], 1e-5, a["act"], a["ld_act"], a["M"], a["E_ln"], a["E_relu"], None)
    return rc, l.toc3d_last_error().decode()


@pytest.mark.parametrize("over,reason", [
    (dict(x=None), "bad arguments"), (dict(gamma=None), "bad arguments"), (dict(beta=None), "bad arguments"), (dict(act=None), "bad arguments"), (dict(M=-1), "bad arguments"),
    (dict(E_ln=0), "bad arguments"), (dict(E_ln=1028, ldx=2048, ld_act=2048), "bad arguments"), (dict(E_relu=-4), "bad arguments"),
    (dict(E_relu=1028, ldx=2048, ld_act=2048), "bad arguments"), (dict(E_ln=62), "bad arguments"), (dict(E_relu=62), "bad arguments"),
    (dict(ldx=124), "leading dimension below E_ln + E_relu"), (dict(ld_act=124), "leading dimension below E_ln + E_relu"), (dict(ldx=130), "leading dimension below"),
    (dict(x=A + 4), "must be 16-byte aligned"), (dict(gamma=A + 4), "must be 16-byte aligned"), (dict(beta=A + 8), "must be 16-byte aligned"),
    (dict(ld_act=130), "f32 rows must be 16-byte aligned"), (dict(act=A + 8), "f32 rows must be 16-byte aligned"),
    (dict(M=1 << 31), "too many rows"),
])
def test_ln_relu_rows_refusals(over, reason):
    rc, msg = _ln(**over)
    assert rc == ERR_ARG and "toc3d_head_ln_relu_rows" in msg and reason in msg, (rc, msg)


def test_ln_relu_rows_dtypes_and_empty_call():
    rc, msg = _ln(dtype=lib.BF16, act=A + 4)
    assert rc == ERR_ARG and "bf16 rows must be 8-byte aligned" in msg
    rc, msg = _ln(dtype=lib.F32X3P, ld_act=144)
    assert rc == ERR_ARG and "128-byte boundaries" in msg
    rc, msg = _ln(dtype=lib.F32X3P, E_ln=48, E_relu=80)
    assert rc == ERR_ARG and "whole 32-element groups" in msg
    for dt in (lib.F32X3, lib.F32X6, 99):
        rc, msg = _ln(dtype=dt)
        assert rc == ERR_ARG and "dtype must be" in msg
    assert _ln(M=0)[0] == 0 and _ln(M=0, E_relu=0, dtype=lib.BF16)[0] == 0


def _out(**over):
    a = dict(h=A, ldh=128, gamma=A, beta=A, w_cls=A, b_cls=A, w_reg=A, b_reg=A, ref=A, ref_rows=5, pc=HOST6, cls=A, ld_cls=10, box=A, ld_bbox=10, M=5, E=64, NC=10, CS=10)
    a.update(over)
    l = lib.load()
    rc = l.toc3d_head_outputs(a["h"], a["ldh"], a["gamma"], a["beta"], 1e-5, a["w_cls"], a["b_cls"], a["w_reg"], a["b_reg"], a["ref"], a["ref_rows"], a["pc"],
                              a["cls"], a["ld_cls"], a["box"], a["ld_bbox"], a["M"], a["E"], a["NC"], a["CS"], None)
    return rc, l.toc3d_last_error().decode()


@pytest.mark.parametrize("over,reason", [
    *[({p: None}, "null buffer") for p in ("h", "gamma", "beta", "w_cls", "b_cls", "w_reg", "b_reg", "ref", "pc", "cls", "box")],
    (dict(M=-1), "bad dims"), (dict(E=0), "bad dims"), (dict(E=1028, ldh=4096), "bad dims"), (dict(E=62), "bad dims"), (dict(NC=0), "bad dims"), (dict(NC=65, ld_cls=65), "bad dims"),
    (dict(CS=2), "bad dims"), (dict(CS=65, ld_bbox=65), "bad dims"), (dict(ref_rows=0), "bad dims"),
    (dict(E=1024, ldh=2048), "must fit 64 KB of LDS"),
    (dict(ldh=124), "leading dimension too small"), (dict(ldh=130), "leading dimension too small"), (dict(ld_cls=9), "leading dimension too small"),
    (dict(ld_bbox=9), "leading dimension too small"),
    *[({p: A + 4}, "must be 16-byte aligned") for p in ("h", "gamma", "beta", "w_cls", "w_reg")],
    (dict(M=1 << 31), "too many rows"), (dict(ref_rows=1 << 31), "too many rows"),
])
def test_head_outputs_refusals(over, reason):
    rc, msg = _out(**over)
    assert rc == ERR_ARG and "toc3d_head_outputs" in msg and reason in msg, (rc, msg)
    assert _out(M=0)[0] == 0


def _dec(**over):
    a = dict(cls=A, ld_cls=10, box=A, ld_bbox=10, B=2, Q=900, NC=10, CS=10, K=300, pcr=HOST6, boxes=A, scores=A, labels=A, qidx=A, counts=A)
    a.update(over)
    l = lib.load()
    rc = l.toc3d_nms_free_decode(a["cls"], a["ld_cls"], a["box"], a["ld_bbox"], a["B"], a["Q"], a["NC"], a["CS"], a["K"], a["pcr"], 0, 0.0, 0,
                                 a["boxes"], a["scores"], a["labels"], a["qidx"], a["counts"], None)
    return rc, l.toc3d_last_error().decode()


@pytest.mark.parametrize("over,reason", [
    *[({p: None}, "null buffer") for p in ("cls", "box", "pcr", "boxes", "scores", "labels", "qidx", "counts")],
    (dict(B=-1), "bad dims"), (dict(Q=0), "bad dims"), (dict(NC=0), "bad dims"), (dict(ld_cls=9), "bad dims"),
    (dict(CS=7), "code_size must be 8"), (dict(CS=9), "code_size must be 8"), (dict(ld_bbox=9), "code_size must be 8"),
    (dict(Q=1639), "exceeds the register-resident limit 16384"), (dict(Q=1 << 40), "exceeds the register-resident limit"), (dict(NC=1 << 40, ld_cls=1 << 40), "exceeds the register-resident limit"),
    (dict(K=0), "max_num must be in"), (dict(K=2049), "max_num must be in"), (dict(K=9001), "max_num must be in"), (dict(Q=10, K=101), "max_num must be in"),
    (dict(B=1 << 31), "batch too large"),
])
def test_nms_free_decode_refusals(over, reason):
    rc, msg = _dec(**over)
    assert rc == ERR_ARG and "toc3d_nms_free_decode" in msg and reason in msg, (rc, msg)
    assert _dec(B=0)[0] == 0
