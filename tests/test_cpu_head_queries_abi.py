"""CPU: every refusal of the two entry points of csrc/head_queries.hip (toc3d_head_query_inputs, toc3d_head_query_combine) is reached once and names its reason
in toc3d_last_error(); header, binding and library agree on ABI 11.  The checks run before any launch, so the device pointers here are made-up addresses that
are never dereferenced (pc_range is a HOST array and real); only refusing calls and the empty ones that return before the launch are made."""
import ctypes
import re

import pytest

from toc3d_amd import lib

A = 0x10000                                  # 128-byte aligned stand-in for device buffers
ERR_ARG = -1
PC = (ctypes.c_float * 6)(-51.2, -51.2, -5.0, 51.2, 51.2, 3.0)
FLAT = (ctypes.c_float * 6)(0, 0, 0, 1, 0, 1)      # spans nothing along x


def test_abi_version_is_11_everywhere():
    hdr = int(re.search(r"#define\s+TOC3D_ABI_VERSION\s+(\d+)", open(lib.HEADER_PATH).read()).group(1))
    assert hdr == lib.ABI_VERSION == lib.load().toc3d_abi_version() == 11
    assert {"toc3d_head_query_inputs", "toc3d_head_query_combine"} <= set(lib.header_functions()) and {"toc3d_head_query_inputs", "toc3d_head_query_combine"} <= set(lib._SIGS)


def _inp(dtype=lib.F32, **over):
    a = dict(ref=A, ref_s=81, vel=A, vel_s=54, ts=A, ts_s=27, pose=A, pose_s=432, pc=PC, d3=A, d1=A, pos=A, ld_pos=384, nerf=A, ld_nerf=192, t1d=A, ld_t1d=256,
             ref_out=A, ref_out_s=84, B=2, n=27, np=7, E=256)
    a.update(over)
    l = lib.load()
    rc = l.toc3d_head_query_inputs(dtype, a["ref"], a["ref_s"], a["vel"], a["vel_s"], a["ts"], a["ts_s"], a["pose"], a["pose_s"], a["pc"], a["d3"], a["d1"],
                                   a["pos"], a["ld_pos"], a["nerf"], a["ld_nerf"], a["t1d"], a["ld_t1d"], a["ref_out"], a["ref_out_s"], a["B"], a["n"], a["np"], a["E"], None)
    return rc, l.toc3d_last_error().decode()


@pytest.mark.parametrize("over,reason", [
    (dict(E=64), "E must be 256"), (dict(E=512), "E must be 256"),
    *[({p: None}, "null buffer") for p in ("ref", "ts", "pc", "d3", "d1", "pos", "t1d", "vel", "pose")],
    (dict(B=-1), "bad counts"), (dict(n=-1), "bad counts"), (dict(np=-1), "bad counts"), (dict(np=28), "bad counts"),
    (dict(ref_out=None), "np > 0 needs ref_out"), (dict(ref_out_s=20), "np > 0 needs ref_out"),
    (dict(ref_s=80), "sample stride smaller"), (dict(ts_s=26), "sample stride smaller"), (dict(vel_s=53), "sample stride smaller"), (dict(pose_s=431), "sample stride smaller"),
    (dict(d3=A + 4), "16-byte aligned"), (dict(d1=A + 8), "16-byte aligned"), (dict(ts=A + 4), "16-byte aligned"),
    (dict(ld_pos=380), "pos3d: leading dimension smaller than the row"), (dict(ld_t1d=252), "t1d: leading dimension smaller than the row"),
    (dict(ld_nerf=180), "nerf: leading dimension smaller than the row"),
    (dict(ld_pos=386), "pos3d: f32 rows must be 16-byte aligned"), (dict(pos=A + 8), "pos3d: f32 rows must be 16-byte aligned"), (dict(t1d=A + 4), "t1d: f32 rows"),
    (dict(nerf=A + 4), "nerf: f32 rows"),
    (dict(B=1 << 40, n=1 << 20, ref_s=1 << 40, ts_s=1 << 40, vel_s=1 << 40, pose_s=1 << 40), "too many rows"), (dict(n=1 << 31, np=0, ref_s=1 << 40, ts_s=1 << 40, vel_s=1 << 40, pose_s=1 << 40), "too many rows"),
    (dict(pc=FLAT), "pc_range spans nothing"),
])
def test_query_inputs_refusals(over, reason):
    rc, msg = _inp(**over)
    assert rc == ERR_ARG and "toc3d_head_query_inputs" in msg and reason in msg, (rc, msg)


def test_query_inputs_dtypes_and_empty_calls():
    rc, msg = _inp(dtype=lib.BF16, pos=A + 4)
    assert rc == ERR_ARG and "bf16 rows must be 8-byte aligned" in msg
    rc, msg = _inp(dtype=lib.BF16, ld_nerf=194)
    assert rc == ERR_ARG and "nerf: bf16 rows" in msg
    for over in (dict(pos=A + 64), dict(ld_pos=400), dict(t1d=A + 16), dict(ld_nerf=208)):
        rc, msg = _inp(dtype=lib.F32X3P, **over)
        assert rc == ERR_ARG and "128-byte boundaries" in msg, (over, msg)
    for dt in (lib.F32X3, lib.F32X3W, lib.F32X6, 99):
        rc, msg = _inp(dtype=dt)
        assert rc == ERR_ARG and "dtype must be" in msg
    assert _inp(B=0)[0] == 0 and _inp(n=0, np=0)[0] == 0 and _inp(B=0, dtype=lib.F32X3P)[0] == 0 and _inp(B=0, dtype=lib.BF16)[0] == 0
    # without the NeRF output, velo / egopose and their strides are not looked at; without propagated rows, ref_out is not
    assert _inp(B=0, nerf=None, vel=None, pose=None, vel_s=0, pose_s=0, ld_nerf=0)[0] == 0
    assert _inp(B=0, np=0, ref_out=None, ref_out_s=0)[0] == 0


def _cmb(**over):
    a = dict(qe=A, ld_qe=256, gb_pe=A, ld_gb_pe=512, te=A, ld_te=256, w=A, b=A, mem=A, mem_s=9216, ld_mem=256, gb_mem=A, ld_gb_mem=512, qt=A, qt_s=7168, tt=A, tt_s=7168,
             ld_tail=256, tp=A, tm=A, ld_temp=256, B=2, n=27, np=7, E=256)
    a.update(over)
    l = lib.load()
    rc = l.toc3d_head_query_combine(a["qe"], a["ld_qe"], a["gb_pe"], a["ld_gb_pe"], a["te"], a["ld_te"], a["w"], a["b"], 1e-5, a["mem"], a["mem_s"], a["ld_mem"],
                                    a["gb_mem"], a["ld_gb_mem"], a["qt"], a["qt_s"], a["tt"], a["tt_s"], a["ld_tail"], a["tp"], a["tm"], a["ld_temp"],
                                    a["B"], a["n"], a["np"], a["E"], None)
    return rc, l.toc3d_last_error().decode()


@pytest.mark.parametrize("over,reason", [
    (dict(E=64), "E must be 256"), (dict(E=1024), "E must be 256"),
    *[({p: None}, "null buffer") for p in ("qe", "te", "w", "b", "mem")],
    (dict(B=-1), "bad counts"), (dict(n=-2), "bad counts"), (dict(np=-1), "bad counts"), (dict(np=28), "bad counts"),
    (dict(qt=None), "np > 0 needs the query_pos and tgt tails"), (dict(tt=None), "np > 0 needs the query_pos and tgt tails"),
    (dict(tp=None), "np < n needs temp_pos and temp_memory"), (dict(tm=None), "np < n needs temp_pos and temp_memory"),
    (dict(ld_qe=252), "leading dimension smaller than the row"), (dict(ld_te=128), "leading dimension smaller than the row"), (dict(ld_mem=252), "leading dimension smaller"),
    (dict(ld_gb_pe=256), "leading dimension smaller than the row"), (dict(ld_gb_mem=508), "leading dimension smaller than the row"),
    (dict(mem_s=6908), "sample stride of memory_embedding"),
    (dict(ld_tail=252), "tail leading dimension"), (dict(qt_s=1788), "tail leading dimension"), (dict(tt_s=1024), "tail leading dimension"),
    (dict(ld_temp=252), "ld_temp smaller than the row"),
    (dict(ld_qe=258), "multiples of 4"), (dict(mem_s=9218), "multiples of 4"), (dict(ld_gb_pe=514), "multiples of 4"), (dict(qt_s=7170), "multiples of 4"), (dict(ld_temp=258), "multiples of 4"),
    *[({p: A + 4}, "16-byte aligned") for p in ("qe", "gb_pe", "te", "w", "b", "mem", "gb_mem", "qt", "tt", "tp", "tm")],
    (dict(B=1 << 31, n=2, np=0, mem_s=512), "too many rows"), (dict(n=1 << 31, np=0, mem_s=1 << 40), "too many rows"),
])
def test_query_combine_refusals(over, reason):
    rc, msg = _cmb(**over)
    assert rc == ERR_ARG and "toc3d_head_query_combine" in msg and reason in msg, (rc, msg)


def test_query_combine_optional_buffers_and_empty_calls():
    assert _cmb(B=0)[0] == 0 and _cmb(n=0, np=0)[0] == 0
    assert _cmb(B=0, gb_pe=None, gb_mem=None, ld_gb_pe=0, ld_gb_mem=0)[0] == 0           # with_ego_pos = False: the MLNs' buffers and leading dimensions are not looked at
    assert _cmb(B=0, np=0, qt=None, tt=None, ld_tail=0, qt_s=0, tt_s=0)[0] == 0          # num_propagated = 0: no tails
    assert _cmb(B=0, n=7, tp=None, tm=None, ld_temp=0, mem_s=1792)[0] == 0               # everything propagated: no temp_* rows
