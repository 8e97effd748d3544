"""The fused GEMM's dispatch, cell by cell.  tools/gen_gemm_dispatch_matrix.py records, through the public ABI only, what every (dtype code, epilogue,
variant) does -- served (and whether the bits equal the cell's reference), "cannot serve", "bad epilogue or variant", or refused by the entry point -- for
variants 0 ... 399 and the split-K ids 1000 s + v of the residual epilogues, at M = 161 and two K per cell.  tests/golden/gemm_dispatch_matrix.json is that
recording, made on the library BEFORE the three dispatchers were generated from one tile table (csrc/gemm_kernels.h, TOC3D_GEMM_TILES); this test replays it and
asks for equality, so a row of the table that drifts from what the hand-written switches did (a shape, a family, an id that appears or disappears) shows here.
Refusals are host-side error returns: nothing in this test launches out of bounds."""
import importlib.util
import json
import os

import pytest

def _tool():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "gen_gemm_dispatch_matrix.py")
    spec = importlib.util.spec_from_file_location("gen_gemm_dispatch_matrix", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def recorded(golden_dir):
    return json.load(open(os.path.join(golden_dir, "gemm_dispatch_matrix.json")))


def test_recording_covers_every_cell(recorded):
    tool = _tool()
    keys = [f"{d}/{e}/{K}" for d, e, K in tool.cell_keys()]
    assert sorted(recorded) == sorted(keys) and len(keys) == 8 * 11 * 2
    for k, s in recorded.items():
        split = int(k.split("/")[1]) in tool.RESIDUAL
        assert [len(g) for g in s.split("|")] == ([400, 100, 100] if split else [400]) and set(s) <= set("Sdube|"), k
    served = sum(s.count("S") + s.count("d") for s in recorded.values())
    assert served > 10000, "the recording holds real launches, not only refusals"


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", range(8))
def test_dispatch_matrix_replays_equal(recorded, dtype):
    tool = _tool()
    for d, e, K in tool.cell_keys():
        if d != dtype:
            continue
        got, want = tool.run_cell(d, e, K, "cuda:0"), recorded[f"{d}/{e}/{K}"]
        if got != want:
            ids = list(range(400)) + [1000 * s + v for s in tool.SPLITS for v in range(100)]
            diff = [(i, w, g) for i, w, g in zip(ids, want.replace("|", ""), got.replace("|", "")) if w != g]
            raise AssertionError(f"dtype {d} epilogue {e} K {K}: (variant, recorded, now) = {diff[:20]}")
