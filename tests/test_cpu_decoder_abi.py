"""CPU: every refusal of the decoder's four entry points (toc3d_mha_attention_ex, toc3d_add_layernorm_pos, toc3d_add_pos_rows, toc3d_relu_inplace) is reached
once and names its reason in toc3d_last_error().  The checks run before any launch, so the pointers here are made-up addresses that are never dereferenced;
only refusing calls (and the empty ones that return before the launch) are made."""
import pytest

from toc3d_amd import lib

A = 0x10000                                  # 16-byte aligned stand-ins for device buffers
PTRS = dict(q=A, k=A + 0x100, v=A + 0x200, k2=A + 0x300, v2=A + 0x400, out=A + 0x500)
ERR_ARG, ERR_UNSUPPORTED = -1, -2


def _mha(dtype=lib.BF16, H=2, **over):
    W = H * 32
    a = dict(PTRS, ldq=W, ldk=W, ldv=W, ldk2=W, ldv2=W, ldo=W, B=1, Nq=5, Nk=7, Nk2=3, heads=H, head_dim=32)
    a.update(over)
    l = lib.load()
    rc = l.toc3d_mha_attention_ex(dtype, a["q"], a["ldq"], a["k"], a["ldk"], a["v"], a["ldv"], a["k2"], a["ldk2"], a["v2"], a["ldv2"], a["out"], a["ldo"],
                                  a["B"], a["Nq"], a["Nk"], a["Nk2"], a["heads"], a["head_dim"], 0.125, None)
    return rc, l.toc3d_last_error().decode()


@pytest.mark.parametrize("over,reason", [
    (dict(q=None), "null buffer or empty dimension"), (dict(out=None), "null buffer or empty dimension"),
    (dict(Nk=0, Nk2=0), "null buffer or empty dimension"), (dict(Nq=0), "null buffer or empty dimension"), (dict(Nk=-1), "null buffer or empty dimension"),
    (dict(k=None), "null key / value buffer"), (dict(v=None), "null key / value buffer"),
    (dict(k2=None), "null key / value buffer"), (dict(v2=None), "null key / value buffer"),
    (dict(B=65536), "dimension too large"), (dict(heads=65536), "dimension too large"), (dict(Nk=1 << 30), "dimension too large"),
    *[({ld: 56}, "leading dimension below heads * 32") for ld in ("ldq", "ldk", "ldv", "ldk2", "ldv2", "ldo")],
    *[({ld: 68}, "multiples of 8 (bf16) / 4 (f32)") for ld in ("ldq", "ldk", "ldv", "ldk2", "ldv2")],
    (dict(ldo=66), "multiples of 8 (bf16) / 4 (f32)"),
    *[({p: PTRS[p] + 8}, "16-byte aligned") for p in PTRS],
])
def test_mha_attention_ex_refusals_bf16(over, reason):
    rc, msg = _mha(**over)
    assert rc == ERR_ARG and "toc3d_mha_attention" in msg and reason in msg, (rc, msg)


@pytest.mark.parametrize("over,reason", [
    *[({ld: 66}, "multiples of 8 (bf16) / 4 (f32)") for ld in ("ldq", "ldk", "ldv", "ldk2", "ldv2", "ldo")],
    *[({p: PTRS[p] + 4}, "16-byte aligned") for p in PTRS],
    (dict(ldv2=60), "leading dimension below heads * 32"),
])
def test_mha_attention_ex_refusals_f32x3(over, reason):
    rc, msg = _mha(dtype=lib.F32X3, **over)
    assert rc == ERR_ARG and reason in msg, (rc, msg)


def test_mha_attention_ex_unsupported_head_dim_and_dtype():
    rc, msg = _mha(head_dim=64)
    assert rc == ERR_UNSUPPORTED and "head_dim must be 32" in msg
    for dt in (lib.F32, lib.F32X6, lib.F32X3P, 99):
        rc, msg = _mha(dtype=dt)
        assert rc == ERR_UNSUPPORTED and "dtype must be" in msg


def test_mha_attention_ex_ignores_the_leading_dimensions_of_an_absent_segment():
    """A segment of length 0 needs neither buffers nor leading dimensions (the decoder passes NULL, 0): with the other checks failing LATER the call is still
    refused, for the later reason -- nothing is launched here."""
    rc, msg = _mha(Nk2=0, k2=None, v2=None, ldk2=0, ldv2=0, out=PTRS["out"] + 8)
    assert rc == ERR_ARG and "16-byte aligned" in msg
    rc, msg = _mha(Nk=0, k=None, v=None, ldk=0, ldv=0, out=PTRS["out"] + 8)
    assert rc == ERR_ARG and "16-byte aligned" in msg


def _ln(dtype=lib.F32, **over):
    a = dict(x=A, ldx=64, gamma=A, beta=A, pos=A, ldp=64, out=A, ldo=64, act=A, ld_act=64, act_pos=A, ld_act_pos=64, gamma2=A, beta2=A, out2=A, ldo2=64, M=5, E=64)
    a.update(over)
    l = lib.load()
    rc = l.toc3d_add_layernorm_pos(dtype, a["x"], a["ldx"], a["gamma"], a["beta"], 1e-5, a["pos"], a["ldp"], a["out"], a["ldo"], a["act"], a["ld_act"],
                                   a["act_pos"], a["ld_act_pos"], a["gamma2"], a["beta2"], a["out2"], a["ldo2"], a["M"], a["E"], None)
    return rc, l.toc3d_last_error().decode()


@pytest.mark.parametrize("over,reason", [
    (dict(E=0), "bad arguments (E <= 1024)"), (dict(E=1025, ldx=2048, ldo=2048), "bad arguments (E <= 1024)"), (dict(ldx=63), "bad arguments"), (dict(ldo=63), "bad arguments"),
    (dict(x=None), "bad arguments"), (dict(gamma=None), "bad arguments"), (dict(beta=None), "bad arguments"), (dict(out=None), "bad arguments"), (dict(M=-1), "bad arguments"),
    (dict(pos=None), "an optional output lacks its inputs"), (dict(ldp=63), "an optional output lacks its inputs"), (dict(ld_act=63), "an optional output lacks its inputs"),
    (dict(ld_act_pos=63), "an optional output lacks its inputs"), (dict(gamma2=None), "an optional output lacks its inputs"),
    (dict(beta2=None), "an optional output lacks its inputs"), (dict(ldo2=63), "an optional output lacks its inputs"),
    (dict(M=1 << 31), "too many rows"),
])
def test_add_layernorm_pos_refusals(over, reason):
    for dt in (lib.F32, lib.BF16):
        rc, msg = _ln(dtype=dt, **over)
        assert rc == ERR_ARG and "toc3d_add_layernorm_pos" in msg and reason in msg, (rc, msg)


def test_add_layernorm_pos_bad_dtype_and_empty_call():
    for dt in (lib.F32X3, lib.F32X3P, 99):
        rc, msg = _ln(dtype=dt)
        assert rc == ERR_ARG and "toc3d_add_layernorm_pos: bad dtype" in msg
    assert _ln(M=0)[0] == 0                                   # nothing to do: success, no launch
    # absent optional outputs need none of their inputs: refused here only for the reason that follows them
    rc, msg = _ln(act=None, ld_act=0, act_pos=None, pos=None, ldp=0, ld_act_pos=0, out2=None, gamma2=None, beta2=None, ldo2=0, dtype=99)
    assert rc == ERR_ARG and "bad dtype" in msg


def _pos(dtype=lib.F32, **over):
    a = dict(x=A, ldx=64, pos=A, ldp=64, act=A, ld_act=64, act_pos=A, ld_act_pos=64, M=5, E=64)
    a.update(over)
    l = lib.load()
    rc = l.toc3d_add_pos_rows(dtype, a["x"], a["ldx"], a["pos"], a["ldp"], a["act"], a["ld_act"], a["act_pos"], a["ld_act_pos"], a["M"], a["E"], None)
    return rc, l.toc3d_last_error().decode()


@pytest.mark.parametrize("over,reason", [
    (dict(act=None, act_pos=None), "bad arguments"), (dict(x=None), "bad arguments"), (dict(E=0), "bad arguments"), (dict(ldx=63), "bad arguments"), (dict(M=-1), "bad arguments"),
    (dict(pos=None), "an output lacks its inputs"), (dict(ldp=63), "an output lacks its inputs"), (dict(ld_act=63), "an output lacks its inputs"),
    (dict(ld_act_pos=63), "an output lacks its inputs"),
    # one thread per element: M * E beyond 2^31 - 1 workgroups of 256 would wrap in the grid size (and M * E itself beyond int64)
    (dict(M=1 << 40, E=1 << 20, ldx=1 << 20, ldp=1 << 20, ld_act=1 << 20, ld_act_pos=1 << 20), "too many elements"),
    (dict(M=1 << 33, E=1 << 31, ldx=1 << 31, ldp=1 << 31, ld_act=1 << 31, ld_act_pos=1 << 31), "too many elements"),
    (dict(M=((1 << 31) - 1) * 4 + 1), "too many elements"),
])
def test_add_pos_rows_refusals(over, reason):
    rc, msg = _pos(**over)
    assert rc == ERR_ARG and "toc3d_add_pos_rows" in msg and reason in msg, (rc, msg)


def test_add_pos_rows_bad_dtype_and_empty_call():
    rc, msg = _pos(dtype=lib.F32X3)
    assert rc == ERR_ARG and "toc3d_add_pos_rows: bad dtype" in msg
    assert _pos(M=0)[0] == 0
    rc, msg = _pos(act_pos=None, pos=None, ldp=0, ld_act_pos=0, dtype=99)          # act alone needs no pos
    assert rc == ERR_ARG and "bad dtype" in msg


def test_relu_inplace_refusals_and_empty_call():
    l = lib.load()
    err = lambda: l.toc3d_last_error().decode()
    assert l.toc3d_relu_inplace(lib.F32, None, 5, None) == ERR_ARG and "toc3d_relu_inplace: bad arguments" in err()
    assert l.toc3d_relu_inplace(lib.F32, A, -1, None) == ERR_ARG and "toc3d_relu_inplace: bad arguments" in err()
    assert l.toc3d_relu_inplace(lib.BF16, A, ((1 << 31) - 1) * 256 + 1, None) == ERR_ARG and "too many elements" in err()
    assert l.toc3d_relu_inplace(lib.F32X3, A, 5, None) == ERR_ARG and "toc3d_relu_inplace: bad dtype" in err()
    assert l.toc3d_relu_inplace(lib.F32, A, 0, None) == 0
