"""What the test files share: device plumbing, raw C-ABI calls, the header parser, error measures, the (hi, lo) planes layout, guard patterns and the worst-ratio report.  A plain module -- no
conftest.py, no package, no test; importing it needs no GPU.  The restated references and case generators live beside it in the ``*_cases.py`` modules.  No
module under tests/ imports from a ``test_*`` module (tests/test_cpu_support.py checks that); a new kernel test starts from here.

Two helpers are one here only where they return the same value for every argument.  Where results can differ both forms stay, under their own names: ``relerr``
clamps its denominator and ``rel_max`` does not, ``rel_max_zero_ok`` has a branch for an all-zero reference, the canary (a finite pattern, element-wise checks) is
not the NaN sentinel (checked as a whole), and ``to_planes`` converts out of place or in place."""
import ctypes
import re
import socket

import numpy as np
import pytest
import torch

from toc3d_amd import lib

DEV = "cuda:0"


# ---- device plumbing -----------------------------------------------------------------------------------------------------------------------
def S():
    return lib.stream_ptr()


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def ru(a, b):
    return (a + b - 1) // b * b


def pack(w, dt, tdt):
    N, K = w.shape
    out = torch.empty(ru(N, 128), ru(K, 64), dtype=tdt, device=DEV)
    lib.call("toc3d_pack_weight", dt, w.to(DEV).contiguous(), N, K, out, out.shape[0], out.shape[1], S())
    return out


def as_act(x, tdt, Kp=None):
    """f32 CPU [M,K] -> act on device with K zero-padded to Kp."""
    M, K = x.shape
    Kp = Kp or ru(K, 64)
    out = torch.zeros(M, Kp, dtype=tdt, device=DEV)
    out[:, :K] = x.to(DEV).to(tdt)
    return out


def d(t):
    return None if t is None else t.to(DEV).contiguous()


def to_dev(frame):
    return {k: v.to(DEV) for k, v in frame["data"].items()}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


# ---- C-ABI calls that must be refused (the argument checks run before any launch: no GPU) ------------------------------------------------------
ERR_ARG = -1


def _call(name, *args):
    l = lib.load()
    rc = getattr(l, name)(*args)
    return rc, l.toc3d_last_error().decode()


def _refused(name, args, reason, fn=None):
    rc, msg = _call(name, *args)
    assert rc == ERR_ARG and (fn or name) in msg and reason in msg, (rc, msg)


A = 0x10000                                  # 256-byte aligned stand-in for a device buffer (never dereferenced: the checks run before any launch)


def raw_call(sigs, name, args):
    """An entry point of a side header called directly, past lib.call(): bound with ``sigs[name]`` (one of lib's tables) -> (return code, last error)."""
    l = lib.load()
    fn = getattr(l, name)
    fn.restype, fn.argtypes = ctypes.c_int, [lib._CT[c] for c in sigs[name]]
    rc = fn(*args)
    return rc, l.toc3d_last_error().decode()


class OldLibrary:
    """In place of lib._lib: a library from before a side header existed -- it has none of the header's symbols."""
    def toc3d_last_error(self):
        return b""


# ---- headers against lib's tables ----------------------------------------------------------------------------------------------------------------
def header_sigs(txt, sigs):
    """{name: signature} of the ``int toc3d_*(...)`` declarations in ``txt`` (a header without comments, lib.header_text) that ``sigs`` names, in the letters of
    lib._CT.  Declarations with other names -- the helpers lib.load() binds by hand -- are passed over; a parameter of a type not listed here fails."""
    found = {}
    for m in re.finditer(r"\bint\s+(toc3d_\w+)\s*\(([^;]*?)\)\s*;", txt, flags=re.S):
        name, args = m.group(1), m.group(2)
        if name not in sigs:
            continue
        sig = ""
        for a in (x.strip() for x in args.split(",")):
            if "*" in a or "toc3d_stream_t" in a or "toc3d_plan_t" in a:
                sig += "p"
            elif a.startswith("int64_t"):
                sig += "l"
            elif a.startswith("uint64_t"):
                sig += "L"
            elif a.startswith("int "):
                sig += "i"
            elif a.startswith("float "):
                sig += "f"
            elif a.startswith("double "):
                sig += "d"
            else:
                raise AssertionError(f"unparsed parameter {a!r} in {name}")
        found[name] = sig
    return found


class FakeNeck(torch.nn.Module):
    """The neck as the detector's sequencing tests (test_cpu_detector.py, test_cpu_streams.py) see it: only the fan-out form may run, and it logs its arguments."""
    def __init__(self, log):
        super().__init__()
        self.log = log

    def forward(self, inputs):
        raise AssertionError("the detector runs the neck with the fan-out")

    def forward_fanout(self, inputs, rows, ld_rows, dtype):
        self.log.append(("neck", tuple(inputs[0].shape), rows, ld_rows, dtype))
        out0 = torch.full((inputs[0].shape[0], 4, 2, 5), float(len(self.log)))
        return out0, out0[:, :, ::2, ::2]


# ---- launch wrappers more than one file uses -------------------------------------------------------------------------------------------------
def _topk_bufs(V, h, w, L, k):
    N = L * L
    nW = V * (-(-h // L)) * (-(-w // L))
    ms = int(lib.load().toc3d_window_topk_rows(V, h, w, L, k))
    i32 = dict(dtype=torch.int32, device=DEV)
    return dict(nW=nW, N=N, ms=ms, order=torch.empty(nW, N, **i32), tok=torch.empty(nW, N, **i32), wgt=torch.empty(nW, N, device=DEV),
                prow=torch.empty(nW, N, **i32), crow_tok=torch.full((ms,), -9, **i32), rep_index=torch.full((ms,), -9, **i32),
                rep_row=torch.empty(nW, **i32), arows=torch.full((nW, k + 1), -9, **i32), aslots=torch.full((nW, k + 1), -9, **i32),
                acount_q=torch.empty(nW, **i32), acount_k=torch.empty(nW, **i32))


def _run_topk(scores, V, h, w, L, k):
    b = _topk_bufs(V, h, w, L, k)
    b["crow_rc"] = torch.full((b["ms"],), -9, dtype=torch.int32, device=DEV)
    lib.call("toc3d_window_topk", scores.to(DEV), V, h, w, L, k, b["order"], b["tok"], b["wgt"], b["prow"], b["crow_tok"], b["rep_index"],
             b["rep_row"], b["arows"], b["aslots"], b["acount_q"], b["acount_k"], b["crow_rc"], S())
    return b


def _pack_scorer(sd, pre):
    f = lambda k: sd[pre + k].to(DEV).float().contiguous()
    l = lib.load()
    mw = torch.empty(l.toc3d_motion_weights_floats(), device=DEV)
    d3 = torch.arange(128, dtype=torch.float32)
    d3 = (10000 ** (2 * torch.div(d3, 2, rounding_mode="floor") / 128)).to(DEV)
    d1 = torch.arange(256, dtype=torch.float32)
    d1 = (10000 ** (2 * torch.div(d1, 2, rounding_mode="floor") / 256)).to(DEV)
    srcs = [f("query_embedding.0.weight"), f("query_embedding.0.bias"), f("query_embedding.2.weight"), f("query_embedding.2.bias")]
    for m in ("ego_pose_pe.", "ego_pose_queries."):
        srcs += [f(m + "reduce.0.weight"), f(m + "reduce.0.bias"), f(m + "gamma.weight"), f(m + "gamma.bias"), f(m + "beta.weight"), f(m + "beta.bias")]
    srcs += [f("time_embedding.0.weight"), f("time_embedding.0.bias"), f("time_embedding.1.weight"), f("time_embedding.1.bias"), f("pc_range"), d3, d1]
    lib.call("toc3d_pack_motion_weights", *srcs, mw, S())
    torch.cuda.synchronize()
    return mw


# ---- error measures ------------------------------------------------------------------------------------------------------------------------
def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def rel_max(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).abs().max() / b.abs().max()).item()


def rel_max_zero_ok(a, b):
    """max-abs error over max-abs reference (``rel_max``); an all-zero reference (the empty bank's rows) must be met exactly."""
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    if not b.any():
        return 0.0 if not a.any() else float("inf")
    return rel_max(a, b)


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).norm() / b.norm()).item()


def iou(a, b):
    res = []
    for ra, rb in zip(a.cpu().numpy(), np.asarray(b)):
        sa, sb = set(ra.tolist()), set(rb.tolist())
        res.append(len(sa & sb) / max(1, len(sa | sb)))
    return min(res)


def layer_norm(x, w, b, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


# ---- (hi, lo) planes: include/toc3d.h TOC3D_DTYPE_F32X3P -------------------------------------------------------------------------------------
def planes_halves(t):
    """An f32-typed planes buffer [R, ld], ld % 32 == 0 -> (hi, lo), the bf16 bit patterns as int16 [R, ld].  A row is groups of 32 elements; a group is 128
    bytes: the 32 hi halves, then the 32 lo halves.  Element c: group c // 32, hi at byte 2 (c % 32) of it, lo at byte 64 + 2 (c % 32)."""
    R, ld = t.shape
    b = t.contiguous().view(torch.int16).view(R, ld // 32, 2, 32)
    return b[:, :, 0, :].reshape(R, ld), b[:, :, 1, :].reshape(R, ld)


def planes_decode(t):
    """-> (hi, lo) as f32 tensors [R, ld]."""
    hi, lo = planes_halves(t)
    return hi.view(torch.bfloat16).float(), lo.view(torch.bfloat16).float()


def planes_values(t):
    """-> the f32 values hi + lo."""
    hi, lo = planes_decode(t)
    return hi + lo


def planes_f64(t):
    """-> the f64 values hi + lo."""
    hi, lo = planes_halves(t)
    return hi.view(torch.bfloat16).double() + lo.view(torch.bfloat16).double()


def planes_bf16(buf, M, E):
    """-> (hi, lo) of the first E columns of rows [0, M), as bf16 tensors [M, E]."""
    hi, lo = planes_halves(buf[:M])
    return hi[:, :E].view(torch.bfloat16), lo[:, :E].view(torch.bfloat16)


def to_planes(t, in_place=False):
    """f32 [rows, K] on the device -> (hi, lo) planes through the library's own converter (toc3d_x3_planes): into a new buffer, or -- in_place -- a contiguous
    copy converted in place."""
    if in_place:
        src = out = t.contiguous().clone()
    else:
        src, out = t, torch.empty_like(t)
    lib.call("toc3d_x3_planes", src, src.shape[1], out, out.shape[1], src.shape[0], src.shape[1], S())
    return out


def a_planes(dt):
    return dt in (lib.F32X3P, lib.F32X3WA)


def o_planes(dt):
    return dt in (lib.F32X3P, lib.F32X3WO)


def w_planes(dt):
    return dt in (lib.F32X3W, lib.F32X3P, lib.F32X3WO, lib.F32X3WA)


# ---- guards --------------------------------------------------------------------------------------------------------------------------------
SENT32, SENT16 = 0x7FC17FC1, 0x7FC1


def sent(rows, cols, bf16=False, device=DEV):
    """[rows, cols] filled with a NaN whose 16-bit halves are both 0x7fc1 (a bf16 NaN; 0x7fc17fc1 is an f32 NaN)."""
    if bf16:
        return torch.full((rows, cols), SENT16, dtype=torch.int16, device=device).view(torch.bfloat16)
    return torch.full((rows, cols), SENT32, dtype=torch.int32, device=device).view(torch.float32)


def is_sent(t):
    t = t.cpu().contiguous()
    return bool((t.view(torch.int16) == SENT16).all()) if t.dtype == torch.bfloat16 else bool((t.view(torch.int32) == SENT32).all())


def bits(t):
    t = t.contiguous()
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a.cpu()), bits(b.cpu()))


GUARD_BYTES, FILL = 256, 0xA5                 # the byte guard: a window of a byte buffer with GUARD_BYTES of FILL on either side of it


def guarded(nbytes, off=0, device=DEV):
    """-> (the whole buffer, its window of ``nbytes`` bytes): GUARD_BYTES + ``off`` bytes before the window (``off`` puts it at an odd address) and GUARD_BYTES
    behind it, all FILL."""
    buf = torch.full((GUARD_BYTES + off + nbytes + GUARD_BYTES,), FILL, dtype=torch.uint8, device=device)
    return buf, buf[GUARD_BYTES + off:GUARD_BYTES + off + nbytes]


def touched(buf, nbytes, off=0):
    """How many bytes of ``guarded(nbytes, off)``'s buffer outside the window are no longer FILL."""
    host = buf.cpu().numpy()
    return int((host[:GUARD_BYTES + off] != FILL).sum() + (host[GUARD_BYTES + off + nbytes:] != FILL).sum())


CAN32, CAN16 = 0x41104110, 0x4110           # the canary: bf16 9.0 in every 16-bit half, so a planes buffer decodes to hi = lo = 9.0 (as f32: 9.016...)


def canary(rows, ld, tdt):
    if tdt == torch.bfloat16:
        return torch.full((rows, ld), 9.0, dtype=tdt, device=DEV)
    t = torch.empty(rows, ld, dtype=torch.float32, device=DEV)
    t.view(torch.int32).fill_(CAN32)
    return t


def is_canary(t):
    return (t.view(torch.int16) == CAN16) if t.dtype == torch.bfloat16 else (t.view(torch.int32) == CAN32)


def check_untouched(tag, buf, M, N, planes, zero_ok=False):
    """(c) rows >= M keep the canary; so do the columns >= N of rows < M (zero_ok: each element the canary or exactly zero)."""
    assert bool(is_canary(buf[M:]).all()), f"{tag}: rows >= M = {M} were written"
    if buf.shape[1] == N:
        return
    if planes:
        hi, lo = planes_decode(buf[:M])
        hi, lo = hi[:, N:], lo[:, N:]
        ok = (hi == 9.0) & (lo == 9.0)
        if zero_ok:
            ok |= (hi == 0) & (lo == 0)
    else:
        pad = buf[:M, N:]
        ok = is_canary(pad)
        if zero_ok:
            ok |= pad == 0
    assert bool(ok.all()), f"{tag}: {int((~ok).sum())} padding elements in columns [{N}, {buf.shape[1]}) hold neither the canary{' nor zero' if zero_ok else ''} (M = {M})"


# ---- the worst-ratio report ------------------------------------------------------------------------------------------------------------------
def report_lines(title, width, worst, bound="derived bound"):
    """What a module prints when it finishes: a heading, then one line per key, sorted."""
    return [f"\n[{title}] worst measured error as a fraction of its {bound} (<= 1.0 required)"] + [f"[{title}] {key:<{width}s} {worst[key]:.3f}" for key in sorted(worst)]


def worst_report(title, width, bound="derived bound"):
    """-> (note, _report) for one test module: ``note(key, ratio)`` keeps the largest ratio per key; ``_report``, assigned at module level under that name, is the
    module-scoped autouse fixture that prints ``report_lines`` after the module's last test.  ``note.worst`` is the dict behind both."""
    worst = {}

    def note(key, ratio):
        worst[key] = max(worst.get(key, 0.0), float(ratio))

    @pytest.fixture(scope="module", autouse=True, name="_report")
    def _report():
        yield
        for line in report_lines(title, width, worst, bound):
            print(line)

    note.worst = worst
    return note, _report
