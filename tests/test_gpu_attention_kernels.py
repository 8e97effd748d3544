"""GPU: the seven attention kernel bodies alone -- attn_small_kernel<9 | 11 | 13> and attn_kernel behind toc3d_window_attention (csrc/attention.hip),
attn_rot_kernel and attn_rot_x3_kernel<false | true> behind toc3d_window_attention_rot (csrc/attention_rot.hip) -- fed their operands directly through the C
ABI, one launch per case, every written element against ITS OWN bound around an f64 softmax of the same operands:

    |dev - ref| <= eps(kind, T_i, Tp_i) A + (n_keys + 8) 2^-24 A,     A[w, i, head, d] = sum_k P_ik |v_kd|

never against a global ratio: at n = 201 one query row that is 90 % wrong moves relative L2 to 2.8e-2, under the 3e-2 the older files allow bf16, and a key dropped
from the softmax moves every row by ~1 / n.  The derivation of eps from each kernel's own rounding points, the two input families (flat with loud edge keys; spikes
in later chunks), the cases and the wrong references the bounds are proven against on the CPU are in tests/attention_cases.py and tests/test_cpu_attention_cases.py.

The output buffer is pre-filled with a NaN bit pattern (0x7fc1 in every 16-bit half).  Rows that are virtual pads, in no list, beyond a window's count or owned by a
count-0 window, and the guard columns [C, ldo), must keep it bit for bit; a written row that kept any of it fails its bound as NaN.  Rows of the q|k|v buffer that no
list names hold +-2^100.  Cases per body: key counts at its chunk / tile / MAXSUB / LDS boundaries, ragged launches (counts n, 1, n - 1, (n + 1) / 2, 0 under one
stride), virtual kept-pad keys (count_q < count_k) against the f64 reference, analytic zero-pad keys, 16-head grids of 4 / 17 / 49 windows (the waves-per-workgroup
choice of launch_rot / launch_rot_x3 and, at n = 129, the second query tile of a wave), scattered rows with ldqkv > 3C and ldo > C, and the spike family.

The worst ratio per (body, kind, family) is printed at the end (profiles/attention_kernels_parity.txt holds a run)."""
import pytest
import torch

import attention_cases as AC
from support import DEV, S, planes_f64, planes_halves, sent, to_planes, worst_report
from toc3d_amd import lib

pytestmark = pytest.mark.gpu
DT = {("rot", "bf16"): lib.BF16, ("rot", "x3p"): lib.F32X3P, ("plain", "f32"): lib.F32, ("plain", "bf16"): lib.BF16, ("plain", "x3"): lib.F32X3,
      ("plain", "x3p"): lib.F32X3P, ("plain", "x3wo"): lib.F32X3WO}
note, _report = worst_report("attention kernels", 52)


def halves(t):
    """CPU tensor [R, ld] (bf16 or f32) -> its 16-bit halves as int16 [R, ld or 2 ld]."""
    return t.contiguous().view(torch.int16)


def upload(case, x):
    """Operands [R, ld] f64 (already rounded to the buffer type) -> the device buffer; on planes the library's converter must reproduce exactly these values."""
    if case.kind == "bf16":
        return x.to(torch.bfloat16).to(DEV)
    d = x.float().to(DEV)
    if case.path == "rot":
        d = to_planes(d, in_place=True)
        assert torch.equal(planes_f64(d.cpu()), x), "the reference's operands are the planes the device reads"
    return d


def i32(t):
    return t.to(torch.int32).contiguous().to(DEV)


def run_case(case):
    b = AC.build(case)
    ref = AC.reference(b)
    bnd = AC.bound(b, ref)
    H, C, n, nW, R, ldqkv, ldo = b["H"], b["C"], b["n"], b["nW"], b["R"], b["ldqkv"], b["ldo"]
    bf = case.kind == "bf16"
    planes_out = case.kind in ("x3p", "x3wo")
    qkv = upload(case, b["qkv"])
    pad = upload(case, b["pad"]) if b["pad"] is not None else None
    out = sent(R, ldo, bf)
    rows, slots, count = i32(b["rows"]), i32(b["slots"]), i32(b["nq"])
    count_k = i32(b["nk"]) if case.virt_q else None
    npad = i32(b["npad"]) if case.npad else None
    vb = b["v_bias"].to(DEV) if case.npad else None
    mc = int(b["nq"].max())
    if case.path == "rot":
        lib.call("toc3d_window_attention_rot", DT[case.path, case.kind], qkv, ldqkv, out, ldo, rows, slots if case.virt_q else None, count, count_k, npad, pad, n, nW, mc, H,
                 vb, 0, None, None, 0, S())
    else:
        lib.call("toc3d_window_attention", DT[case.path, case.kind], qkv, ldqkv, out, ldo, rows, slots, count, count_k, npad, pad, n, nW, mc, H,
                 b["cos"].to(DEV), b["sin"].to(DEV), b["L"], vb, AC.PLAIN_SCALE, S())
    o = out.cpu()
    # ---- what must not be written ----
    keep = torch.ones(R, dtype=torch.bool)
    keep[b["written"]] = False
    assert bool((halves(o[keep]) == 0x7FC1).all()), f"{case}: a row that is a pad, in no list or beyond its window's count was written"
    if planes_out:
        vals, (hi, lo) = planes_f64(o), planes_halves(o)
        assert bool((hi[:, C:] == 0x7FC1).all() and (lo[:, C:] == 0x7FC1).all()), f"{case}: guard columns [C, ldo) were written"
    else:
        vals = o.double()
        if ldo > C:
            assert bool((halves(o[:, C:]) == 0x7FC1).all()), f"{case}: guard columns [C, ldo) were written"
    # ---- every written element against its own bound ----
    valid = ref["valid"]
    dev = vals[b["written"], :C].reshape(-1, H, AC.HD)
    want, tol = ref["out"][valid], bnd[valid]
    assert dev.shape == want.shape
    ratio = ((dev - want).abs() / tol).nan_to_num(nan=float("inf"))
    worst = float(ratio.max())
    print(f"[attention kernels] {case.name:<34s} {AC.body_of(case):<26s} worst |dev - ref| / bound = {worst:.3f}")
    assert worst <= 1.0, f"{case}: {int((ratio > 1).sum())} elements beyond their bound, the worst at {worst:.3f} x (row {int(ratio.flatten(1).amax(1).argmax())} of the written rows)"
    key = f"{AC.body_of(case)} {case.kind} {case.family}"
    note(key, worst)


@pytest.mark.parametrize("case", AC.CASES, ids=str)
def test_attention_kernel_within_its_bound(case):
    run_case(case)
