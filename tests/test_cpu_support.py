"""CPU: tests/support.py itself -- the planes layout its decoders assume, the NaN sentinel, the text of the worst-ratio report, and the rule that no module
under tests/ imports from a ``test_*`` module."""
import ast
import glob
import os

import torch

import support


def test_planes_layout_on_a_hand_built_row():
    """One row of 64 elements at ld 96 (include/toc3d.h TOC3D_DTYPE_F32X3P): element c lives in group c // 32, hi at byte 2 (c % 32) of the group's 128 bytes,
    lo at byte 64 + 2 (c % 32).  hi = c + 1 and lo = 2^-9 (c + 1) are exact in bf16 and their sum in f32; the third group holds the sentinel."""
    ld, n = 96, 64
    want_hi = torch.arange(1, n + 1, dtype=torch.float64)[None]
    want_lo = want_hi * 2.0 ** -9
    hi_bits, lo_bits = want_hi.bfloat16().view(torch.int16), want_lo.bfloat16().view(torch.int16)
    raw = torch.full((1, 2 * ld), support.SENT16, dtype=torch.int16)
    for c in range(n):
        raw[0, (128 * (c // 32) + 2 * (c % 32)) // 2] = hi_bits[0, c]
        raw[0, (128 * (c // 32) + 64 + 2 * (c % 32)) // 2] = lo_bits[0, c]
    t = raw.view(torch.float32)
    assert t.shape == (1, ld)
    hi16, lo16 = support.planes_halves(t)
    assert hi16.dtype == lo16.dtype == torch.int16 and hi16.shape == lo16.shape == (1, ld)
    assert torch.equal(hi16[:, :n], hi_bits) and torch.equal(lo16[:, :n], lo_bits)
    assert bool((hi16[:, n:] == support.SENT16).all() and (lo16[:, n:] == support.SENT16).all())
    hi, lo = support.planes_decode(t)
    assert hi.dtype == lo.dtype == torch.float32 and torch.equal(hi[:, :n].double(), want_hi) and torch.equal(lo[:, :n].double(), want_lo)
    vals, vals64 = support.planes_values(t), support.planes_f64(t)
    assert vals.dtype == torch.float32 and vals64.dtype == torch.float64
    assert torch.equal(vals[:, :n], (hi + lo)[:, :n]) and torch.equal(vals64[:, :n], want_hi + want_lo) and torch.equal(vals[:, :n].double(), vals64[:, :n])
    assert bool(vals[:, n:].isnan().all() and vals64[:, n:].isnan().all())
    bh, bl = support.planes_bf16(t, 1, 32)
    assert bh.dtype == torch.bfloat16 and torch.equal(bh.double(), want_hi[:, :32]) and torch.equal(bl.double(), want_lo[:, :32])


def test_sentinel_buffers_and_is_sent():
    for bf16, dtype, halves in ((False, torch.float32, 2), (True, torch.bfloat16, 1)):
        t = support.sent(3, 5, bf16, device="cpu")
        assert t.dtype == dtype and t.shape == (3, 5) and bool(t.isnan().all())
        assert bool((t.view(torch.int16) == support.SENT16).all()) and t.view(torch.int16).shape == (3, 5 * halves)
        assert support.is_sent(t) is True and support.is_sent(t[:, 1:4]) is True and support.is_sent(t[:0]) is True
        t[1, 2] = 0.0                                                        # one overwritten element
        assert support.is_sent(t) is False and support.is_sent(t[:1]) is True and support.is_sent(t[:, 2:3]) is False
    assert int(support.sent(1, 1, device="cpu").view(torch.int32)) == support.SENT32 == 0x7FC17FC1
    a, b = support.sent(2, 3, True, device="cpu"), support.sent(2, 3, True, device="cpu")
    assert support.same_bits(a, b) and not torch.equal(a, b)                 # NaN != NaN: the bits are what is compared
    b[0, 0] = 1.0
    assert not support.same_bits(a, b) and support.bits(a).dtype == torch.int16 and support.bits(a.float()).dtype == torch.int32


def test_byte_guard_counts_writes_around_the_window_and_not_inside():
    for off in (0, 2, 5):
        buf, win = support.guarded(24, off, device="cpu")
        assert buf.dtype == torch.uint8 and buf.numel() == 2 * support.GUARD_BYTES + off + 24 and win.numel() == 24 and bool((buf == support.FILL).all())
        assert win.data_ptr() - buf.data_ptr() == support.GUARD_BYTES + off and support.touched(buf, 24, off) == 0
        win[:] = 0                                                           # every byte of the window, its first and last included: not counted
        assert support.touched(buf, 24, off) == 0
        buf[support.GUARD_BYTES + off - 1] = 0                               # the byte before the window
        assert support.touched(buf, 24, off) == 1
        buf[support.GUARD_BYTES + off + 24] = 0                              # the byte behind it
        assert support.touched(buf, 24, off) == 2
        buf[0], buf[-1] = 1, 2                                               # the far ends of both guards
        assert support.touched(buf, 24, off) == 4
        if off:
            buf[support.GUARD_BYTES] = 0                                     # the first byte of the gap ``off`` opens between the leading guard and the window
            assert support.touched(buf, 24, off) == 5
    assert (support.GUARD_BYTES, support.FILL) == (256, 0xA5)


def test_worst_report_prints_the_present_line_format(capsys):
    note, fixture = support.worst_report("token kernels", 58)
    for ratio in (0.1, torch.tensor(0.1234), 0.05):
        note("gather merge (representative rows)", ratio)
    note("a key", 1)
    assert note.worst == {"gather merge (representative rows)": float(torch.tensor(0.1234)), "a key": 1.0}
    lines = support.report_lines("token kernels", 58, note.worst)
    assert lines == ["\n[token kernels] worst measured error as a fraction of its derived bound (<= 1.0 required)",
                     "[token kernels] a key" + " " * 53 + " 1.000", "[token kernels] gather merge (representative rows)" + " " * 24 + " 0.123"]
    assert support.report_lines("attention kernels", 52, {"attn_kernel bf16 flat": 0.5})[1] == f"[attention kernels] {'attn_kernel bf16 flat':<52s} 0.500"
    assert support.report_lines("scorer kernels", 58, {}, bound="bound") == ["\n[scorer kernels] worst measured error as a fraction of its bound (<= 1.0 required)"]
    gen = fixture._get_wrapped_function()() if hasattr(fixture, "_get_wrapped_function") else fixture.__wrapped__()
    next(gen)                                                                # the fixture prints nothing before the module's tests ...
    assert capsys.readouterr().out == ""
    assert next(gen, None) is None                                           # ... and those lines after the last one
    assert capsys.readouterr().out == "\n".join(lines) + "\n"


def test_no_module_imports_from_a_test_module():
    here = os.path.dirname(os.path.abspath(__file__))
    files = sorted(glob.glob(os.path.join(here, "*.py")))
    assert os.path.join(here, "support.py") in files and len(files) > 40
    found = []
    for path in files:
        for node in ast.walk(ast.parse(open(path).read(), path)):
            names = [a.name for a in node.names] if isinstance(node, ast.Import) else [node.module or ""] if isinstance(node, ast.ImportFrom) else []
            found += [f"{os.path.basename(path)}:{node.lineno} {n}" for n in names if n.split(".")[-1].startswith("test_")]
    assert not found, found
