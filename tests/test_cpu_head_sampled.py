"""CPU: the sampled token side without a GPU -- the side header include/toc3d_sampled.h against the ctypes table that binds it and against the library's
exports, every refusal of its two entry points on made-up host pointers (the checks run before any launch), tests/golden/head_tokens_sampled.npz (the REAL
reference with topk_indexes, tools/gen_golden_head_tokens_sampled.py) against the oracle restatement gathered, and StreamPETRHead's token_sampling keyword off
and on.  Every test prints the figures it asserts on (run with -s)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import sampled_cases as SC
import toc3d_amd
from support import A, ERR_ARG, OldLibrary, header_sigs, raw_call
from toc3d_amd import lib, synth

FRUSTUM, GATHER = "toc3d_head_frustum_inputs_sampled", "toc3d_gather_token_rows"


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------------------------------------
def test_sampled_header_ctypes_table_and_exports_agree():
    raw = open(lib.SAMPLED_HEADER_PATH).read()
    found = header_sigs(lib.header_text(lib.SAMPLED_HEADER_PATH), lib._SAMPLED_SIGS)
    print(f"toc3d_sampled.h declares {found}")
    assert found == lib._SAMPLED_SIGS and list(found) == [FRUSTUM, GATHER]
    declared = set(re.findall(r"\b(toc3d_\w+)\s*\(", lib.header_text(lib.SAMPLED_HEADER_PATH)))
    assert declared == set(lib._SAMPLED_SIGS) | {"toc3d_sampled_abi"}, "nothing declared that the table does not bind"
    assert int(re.search(r"#define\s+TOC3D_SAMPLED_ABI\s+(\d+)", raw).group(1)) == lib.SAMPLED_ABI == 1
    assert "streampetr_head.py:379-422" in raw and "misc.py:13-23" in raw, "the header cites the reference lines it serves"
    assert re.search(r"clamp every index into \[0, LEN - 1\]", raw), "the header states the index clamp"
    dll = ctypes.CDLL(lib.LIB_PATH)
    assert all(hasattr(dll, n) for n in declared)
    dll.toc3d_sampled_abi.restype = ctypes.c_int
    assert dll.toc3d_sampled_abi() == 1
    # the pinned headers know nothing of it, and no name is bound twice
    for other in (lib.HEADER_PATH, lib.STREAMS_HEADER_PATH, lib.FOCAL_HEADER_PATH):
        assert "toc3d_sampled" not in open(other).read() and GATHER not in open(other).read()
    assert not set(lib._SAMPLED_SIGS) & (set(lib._SIGS) | set(lib._STREAMS_SIGS) | set(lib._FOCAL_SIGS))
    assert lib.ABI_VERSION == 11 and lib.ABI_MINOR == 1


def test_call_binds_the_entry_points_and_an_old_library_is_told_to_rebuild(monkeypatch):
    with pytest.raises(RuntimeError, match=r"toc3d_gather_token_rows failed \(-1\): toc3d_gather_token_rows: null buffer"):
        lib.call(GATHER, lib.F32, None, 64, None, 1, 5, 3, 32, None, 64, None)
    for n, sig in lib._SAMPLED_SIGS.items():
        assert getattr(lib.load(), n).argtypes == [lib._CT[c] for c in sig], "bound with the table's argument types (int64 counts, not C ints)"

    monkeypatch.setattr(lib, "_lib", OldLibrary())
    with pytest.raises(RuntimeError, match=r"toc3d_sampled\.h.*rebuild the library"):
        lib.call(GATHER, *gather_args())


FRUSTUM_PTRS, GATHER_PTRS = ("img2lidar", "intrinsics", "coords_d", "position_range", "index", "pos_in", "cone_act", "cone"), ("src", "index", "dst")


def frustum_args(dtype=lib.F32, **o):
    a = dict({p: A for p in FRUSTUM_PTRS}, B=1, N=6, h=20, w=50, K=3000, D=64, stride=16, pad_h=320, pad_w=800, ld_pos=192, ld_cone=64)
    a.update(o)
    return (dtype, a["img2lidar"], a["intrinsics"], a["coords_d"], a["position_range"], a["index"], a["B"], a["N"], a["h"], a["w"], a["K"], a["D"], a["stride"],
            a["pad_h"], a["pad_w"], a["pos_in"], a["ld_pos"], a["cone_act"], a["ld_cone"], a["cone"], None)


def gather_args(dtype=lib.F32, **o):
    a = dict({p: A for p in GATHER_PTRS}, ld_src=256, B=1, LEN=6000, K=3000, C=256, ld_dst=256)
    a.update(o)
    return (dtype, a["src"], a["ld_src"], a["index"], a["B"], a["LEN"], a["K"], a["C"], a["dst"], a["ld_dst"], None)


P = lib.F32X3P
PLANES_RULE = "128-byte boundaries"


@pytest.mark.parametrize("dtype,over,reason", [
    *[(lib.F32, {p: None}, "null buffer") for p in FRUSTUM_PTRS],
    (lib.F32X3, {}, "bad dtype"), (99, {}, "bad dtype"), (-1, {}, "bad dtype"),
    (lib.F32, dict(K=0), "bad K"), (lib.F32, dict(K=-3), "bad K"), (lib.F32, dict(K=6001), "bad K"),
    *[(lib.F32, {d: 0}, "must be positive") for d in ("B", "N", "h", "w", "stride", "pad_h", "pad_w")], (lib.BF16, dict(B=-1), "must be positive"),
    (lib.F32, dict(D=29), "depth_num"), (lib.F32, dict(D=0), "depth_num"),
    (lib.F32, dict(h=1 << 20, w=1 << 20), "31 bits"),
    (lib.F32, dict(ld_pos=191), "leading dimensions"), (lib.BF16, dict(ld_cone=7), "leading dimensions"),
    (P, dict(ld_pos=200), PLANES_RULE), (P, dict(ld_cone=8), PLANES_RULE), (P, dict(pos_in=A + 64), PLANES_RULE), (P, dict(cone_act=A + 16), PLANES_RULE),
    (lib.F32, dict(B=1 << 28, K=6000), "too many rows"),
])
def test_frustum_sampled_refusals(dtype, over, reason):
    rc, msg = raw_call(lib._SAMPLED_SIGS, FRUSTUM, frustum_args(dtype, **over))
    print(f"{over or dtype}: rc {rc}, {msg!r}")
    assert rc == ERR_ARG and msg.startswith(FRUSTUM + ":") and reason in msg, (rc, msg)


@pytest.mark.parametrize("dtype,over,reason", [
    *[(lib.F32, {p: None}, "null buffer") for p in GATHER_PTRS],
    (lib.F32X3, {}, "bad dtype"), (99, {}, "bad dtype"), (-1, {}, "bad dtype"),
    (lib.F32, dict(K=0), "bad K"), (lib.F32, dict(K=-1), "bad K"), (lib.BF16, dict(K=6001), "bad K"),
    *[(lib.F32, {d: 0}, "must be positive") for d in ("B", "LEN", "C")], (lib.F32, dict(LEN=-7), "must be positive"), (lib.F32, dict(LEN=1 << 31), "must be positive"),
    (lib.F32, dict(ld_src=255), "leading dimensions"), (lib.BF16, dict(ld_dst=255), "leading dimensions"),
    (P, dict(ld_src=272), PLANES_RULE), (P, dict(ld_dst=264), PLANES_RULE), (P, dict(src=A + 64), PLANES_RULE), (P, dict(dst=A + 32), PLANES_RULE),
    (lib.F32, dict(B=1 << 30, LEN=1 << 20, K=1 << 20), "too many rows"),
])
def test_gather_token_rows_refusals(dtype, over, reason):
    rc, msg = raw_call(lib._SAMPLED_SIGS, GATHER, gather_args(dtype, **over))
    print(f"{over or dtype}: rc {rc}, {msg!r}")
    assert rc == ERR_ARG and msg.startswith(GATHER + ":") and reason in msg, (rc, msg)


# ---- the fixture -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_fixture_equals_the_oracle_restatement_gathered():
    """The bar tests/test_cpu_oracle_golden.py holds the oracle to on head_tokens.npz: the same bits."""
    from oracle import head_tokens_oracle as HO
    CFG, B, N, H, W, K = SC.CFG, SC.B, SC.N, SC.H, SC.W, SC.K
    g = np.load(os.path.join(SC.GOLDEN, "head_tokens_sampled.npz"))
    idx = torch.from_numpy(g["topk_indexes"])
    assert tuple(idx.shape) == (B, K, 1) and idx.dtype == torch.int64
    idx = idx.view(B, K)
    rows = idx.tolist()
    print(f"lists {rows}")
    assert all(len(set(r)) == K and r != sorted(r) and 0 <= min(r) and max(r) < N * H * W for r in rows) and rows[0] != rows[1], "unsorted, different per sample"
    assert any(i % N != i // (H * W) for r in rows for i in r), "a token whose camera (i % N) is not its view (i // hw)"
    sd = synth.head_tokens_state_dict(CFG)
    inp = synth.head_tokens_inputs(CFG, B, N, H, W)
    pad_h, pad_w = H * CFG["stride"], W * CFG["stride"]
    with torch.no_grad():
        pos, cone = HO.position_embedding(sd, CFG, inp["intrinsics"], inp["lidar2img"], H, W, pad_h, pad_w)
        memory, pos_embed = HO.token_embeddings(sd, CFG, inp["feats"], inp["intrinsics"], inp["lidar2img"], pad_h, pad_w)
    for name, got in (("pos_raw", pos), ("cone", cone), ("memory", memory), ("pos_embed", pos_embed)):
        full, ref = torch.from_numpy(g["full_" + name]), torch.from_numpy(g[name])
        assert tuple(ref.shape) == (B, K, got.shape[-1]) and tuple(full.shape) == tuple(got.shape)
        assert torch.equal(got, full), (name, "full", float((got - full).abs().max()))
        assert torch.equal(SC.gather_rows(got, idx), ref), (name, float((SC.gather_rows(got, idx) - ref).abs().max()))


# ---- the keyword -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_token_sampling_keyword_off_and_on():
    sizes = synth.HEAD_TINY
    inp = synth.head_inputs(sizes, synth.HEAD_TINY_SHAPE)
    data, metas = inp["frames"][0], inp["img_metas"]
    topk = torch.zeros(2, 5, 1, dtype=torch.int64)
    heads = {}
    for on in (False, True):
        kw = dict(token_sampling=True) if on else {}
        h = toc3d_amd.build_head(synth.head_cfg(sizes), **kw).eval()
        assert h.token_sampling is on
        heads[on] = h
    with pytest.raises(NotImplementedError, match="topk_indexes") as e:
        heads[False](None, metas, topk, **data)
    print(str(e.value))
    assert "token_sampling" in str(e.value)
    with pytest.raises(RuntimeError, match="CUDA/HIP"):                    # on: the list reaches the token side, whose first refusal is the device's
        heads[True](None, metas, topk, **data)
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        heads[True](None, metas, None, **data)
    assert heads[True]._bank is None
    keys = [list(h.state_dict()) for h in heads.values()]
    assert keys[0] == keys[1]
    full = [list(toc3d_amd.build_head(synth.head_cfg(), **kw).state_dict()) for kw in ({}, dict(token_sampling=True))]      # the shipped sizes: 251 keys
    assert full[0] == full[1] and len(full[0]) == 251
    heads[True].load_state_dict(synth.head_state_dict(sizes), strict=True)


def test_token_module_refuses_a_list_on_the_cpu_and_an_empty_one():
    m = toc3d_amd.HeadTokenEmbedding(**SC.CFG)
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        m._index(torch.zeros(2, 5, 1, dtype=torch.int64), 2, 24)
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        m.forward_rows((2, 2, 3, 4), torch.zeros(2, 2, 4, 4), torch.zeros(2, 2, 4, 4), (48, 64, 3), "cpu", topk_indexes=[[1, 2]])
