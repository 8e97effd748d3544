"""Record what the fused GEMM's dispatch does with every (dtype code, epilogue, variant): tests/golden/gemm_dispatch_matrix.json, replayed by
tests/test_gpu_gemm_dispatch.py.  Only the public ABI is used (toc3d_linear_fused, toc3d_linear_fused_ws, toc3d_linear_qkv_rope), so the recording can be made
on any build of the library (TOC3D_LIB) and held against another.

Cells: every dtype code 0-7 x every epilogue 0-10 x variant 0 ... 399 and, for the residual epilogues, 1000 s + v with s in {2, 4} and v in 0 ... 99.
One character per cell:
    S   served, every output buffer bit-equal to the cell's reference (variant 0 for the unsplit cells, the first served tile of the same split for the split ones)
    d   served, bits differ from the reference
    u   refused: the tile cannot serve this launch (TOC3D_ERR_UNSUPPORTED)
    b   refused by the dispatcher: "bad epilogue or variant" / "bad variant" / "no split-K form" (TOC3D_ERR_ARG)
    e   refused by the entry point's argument checks before any dispatch (this dtype code has no such epilogue, K too short for the split, ...)
Refusals are host-side error returns; no cell launches anything out of bounds (operands are sized for the largest tile, rows and columns past M / N are the
kernels' own tail paths, tested in test_gpu_epilogue_tails.py).

Shapes: M = 161 (one row past the tallest partial tile), the column sizes of tests/epilogue_cases.py COLS["aligned"], and two K per cell: 512 (whole K-tiles of
256 elements) and 192 (not: the RB 256 / 512 tiles take their 128-byte fallback).  The 3x3 conv fixes K = 9 C: C = 256 (whole K-tiles) and C = 64.

    python tools/gen_gemm_dispatch_matrix.py [--out tests/golden/gemm_dispatch_matrix.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import epilogue_cases as ec  # noqa: E402
from toc3d_amd import lib  # noqa: E402

M = 161
PAD = 95                                # spare rows behind every output buffer
COLS = ec.COLS["aligned"]
KS = (512, 192)
CONV_C = (256, 64)                      # K = 9 C
CONV_VHW = (1, 7, 23)                   # V * h * w = M
SPLITS = (2, 4)
N_DTYPES, N_EPIS = 8, 11
RESIDUAL = (lib.EPI_RESIDUAL, lib.EPI_RESIDUAL_LN, lib.EPI_RESIDUAL_STATS)
SWIGLU = (lib.EPI_SWIGLU, lib.EPI_SWIGLU_STATS, lib.EPI_SWIGLU_STATS_LN)
LN_IN = (lib.EPI_RESIDUAL_LN, lib.EPI_SWIGLU_STATS_LN)
STATS_OUT = (lib.EPI_SWIGLU_STATS, lib.EPI_SWIGLU_STATS_LN, lib.EPI_RESIDUAL_STATS)
STATS_CAP = 16
ROPE_SIDE = 8


def _operand(x, dtype, planes):
    """f32 [rows, K] -> the buffer a launch of ``dtype`` reads: bf16, plain f32 or the (hi, lo) planes image."""
    if dtype == lib.BF16:
        return x.to(torch.bfloat16).contiguous()
    return ec.planes_encode(x).contiguous() if planes else x.contiguous()


class Cell:
    """Operands, outputs and the two launch closures of one (dtype, epilogue, K)."""

    def __init__(self, dtype, epi, K, dev):
        g = torch.Generator().manual_seed(1000 * dtype + 10 * epi + K)
        rnd = lambda *s: torch.randn(*s, generator=g)
        self.dtype, self.epi = dtype, epi
        n = 2 * COLS["Hp"] if epi in SWIGLU else COLS["C"]
        self.N = n
        planes_w = dtype >= lib.F32X3W
        planes_a = dtype in (lib.F32X3P, lib.F32X3WA)
        self.K, self.lda = K, K
        if epi == lib.EPI_CONV3X3:
            self.K, self.lda = 9 * K, K                                            # (K names the channel count here)
        a32 = rnd(M, self.lda) * 0.5
        self.A = _operand(a32, dtype, planes_a).to(dev)
        self.W = _operand(rnd(ec.ru(max(n, 512), 128), self.K) * 0.05, dtype, planes_w).to(dev)      # rows for the widest N-tile
        self.bias, self.c1 = (rnd(1024) * 0.1).to(dev), (rnd(1024) * 0.1).to(dev)
        self.res = rnd(M + PAD, n).to(dev)
        st = torch.zeros(4 + M * 2, dtype=torch.float32)                            # stats_in: header + [M, 1, 2] (sum, sum of squares) of the A rows
        st[4:] = torch.stack([a32.sum(1), (a32 * a32).sum(1)], 1).flatten()
        self.stats_in = st.to(dev)
        self.zeros = torch.zeros(256, dtype=torch.uint8, device=dev)
        self.rope_rc = (torch.arange(M, dtype=torch.int32) % ROPE_SIDE * 65537).to(dev)
        self.rope_tab = torch.cat([torch.cos(rnd(2, ROPE_SIDE, 16)), torch.sin(rnd(2, ROPE_SIDE, 16))]).contiguous().to(dev)
        # outputs: raw f32-sized buffers (large enough for either element size), compared as bits
        self.ldo = COLS["Hp"] if epi in SWIGLU else n
        self.out = torch.zeros((M + PAD) * n, dtype=torch.float32, device=dev)
        self.out_act = torch.zeros((M + PAD) * n, dtype=torch.float32, device=dev)
        self.stats = torch.zeros(4 + (M + PAD) * STATS_CAP * 2, dtype=torch.float32, device=dev)
        self.ws = torch.zeros(1 << 20, dtype=torch.int32, device=dev)              # split-K workspace (4 MiB, zeroed once: every launch re-arms its tickets)
        assert self.ws.data_ptr() % 256 == 0 and self.out.data_ptr() % 128 == 0
        self.stream = torch.cuda.current_stream().cuda_stream

    def _fused_args(self, variant):
        e = self.epi
        stats_out = (self.stats, STATS_CAP) if e in STATS_OUT else (None, 0)
        stats_in = (self.stats_in, 1 | 1 << 32) if e in LN_IN else (None, 0)
        c1, ln_n, eps = (self.c1, self.K, 1e-6) if e in LN_IN else (None, 0, 0.0)
        out_act, ld_act = (self.out_act, self.N) if e == lib.EPI_RESIDUAL_STATS else (None, 0)
        if e == lib.EPI_CONV3X3:
            out_act, ld_act = self.zeros, (CONV_VHW[1] << 32) | CONV_VHW[2]
        res, ldr = (self.res, self.N) if e in RESIDUAL else (None, 0)
        n_valid = COLS["Hd"] if e in SWIGLU else 0
        return (self.dtype, e, variant, self.A, self.lda, self.W, self.K, self.bias, self.out, self.ldo, res, ldr, 0, None, None, M, self.N, self.K, n_valid,
                stats_out[0], stats_out[1], stats_in[0], stats_in[1], c1, ln_n, eps, out_act, ld_act, None)

    def launch(self, variant):
        """-> (return code, error text) of the entry point that serves this cell."""
        L = lib.load()
        conv = lambda a: [lib._conv(x) for x in a]
        if self.epi == lib.EPI_QKV_ROPE:
            rc = L.toc3d_linear_qkv_rope(*conv((self.dtype, variant, self.A, self.lda, self.W, self.K, self.bias, self.out, self.ldo, M, self.N, self.K,
                                                 self.rope_rc, self.rope_tab, ROPE_SIDE, lib.ATTN_ROT_Q_SCALE, self.stream)))
        elif variant >= 1000:
            rc = L.toc3d_linear_fused_ws(*conv(self._fused_args(variant) + (self.ws, self.ws.numel() * 4, self.stream)))
        else:
            rc = L.toc3d_linear_fused(*conv(self._fused_args(variant) + (self.stream,)))
        return rc, (L.toc3d_last_error().decode() if rc != 0 else "")

    def outputs(self):
        """The buffers this epilogue writes (zeroed before every launch, so what a launch leaves alone compares equal)."""
        return [self.out] + ([self.out_act] if self.epi == lib.EPI_RESIDUAL_STATS else []) + ([self.stats] if self.epi in STATS_OUT else [])


def classify(rc, text):
    if rc == -2:
        return "u"
    if "bad epilogue" in text or "bad variant" in text or "no split-K form" in text:
        return "b"
    return "e"


def run_cell(dtype, epi, K, dev):
    """The cell's string: 400 unsplit variants, then (residual epilogues) 100 tile ids per split."""
    c = Cell(dtype, epi, K, dev)
    groups = [range(400)]
    if epi in RESIDUAL:
        groups += [range(1000 * s, 1000 * s + 100) for s in SPLITS]
    out = []
    for variants in groups:
        ref = None
        for v in variants:
            for t in c.outputs():
                t.zero_()
            rc, text = c.launch(v)
            if rc != 0:
                out.append(classify(rc, text))
                continue
            got = [t.view(torch.int32) for t in c.outputs()]
            if ref is None:
                ref = [t.clone() for t in got]
            out.append("S" if all(torch.equal(a, b) for a, b in zip(got, ref)) else "d")
        out.append("|")
    torch.cuda.synchronize()
    return "".join(out[:-1])


def cell_keys():
    for dtype in range(N_DTYPES):
        for epi in range(N_EPIS):
            for K in (CONV_C if epi == lib.EPI_CONV3X3 else KS):
                yield dtype, epi, K


def record(dev="cuda:0"):
    """{"<dtype>/<epilogue>/<K>": string} for every cell."""
    return {f"{d}/{e}/{K}": run_cell(d, e, K, dev) for d, e, K in cell_keys()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "gemm_dispatch_matrix.json"))
    args = ap.parse_args()
    rec = record()
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    counts = {k: sum(s.count(k) for s in rec.values()) for k in "Sdube"}
    print(f"{len(rec)} cells written to {args.out}: {counts}")


if __name__ == "__main__":
    main()
