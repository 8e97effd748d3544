"""GPU: the two kernels of include/toc3d_sampled.h alone, bit for bit.

toc3d_head_frustum_inputs_sampled at 1, 5 and 24 tokens (the shapes of tests/test_gpu_head_tokens_x3.py), depth_num 64 and 33, in all three act dtypes: every
row of pos_in, cone_act and cone equals the row of the FULL kernel, launched on the same inputs, at the listed token -- and nothing behind row B*K or beyond the
valid columns is written (canaries).  toc3d_gather_token_rows at C = 32, 40 (16-byte units) and 37 (2-byte units; in planes, a group's tail) at ld 64, and once
with ld_src != ld_dst: destination rows are the source rows' bits over the valid columns, everything else keeps its canary.
Index lists (sampled_cases.index_families): K = 1, K = LEN as a permutation, and a strict subset with one planted duplicate.  No list holds an index outside
[0, LEN): the kernels clamp (the header says so), and no test here feeds them one."""
import pytest
import torch

import sampled_cases as SC
import toc3d_amd
from toc3d_amd import lib, synth

from support import DEV, S, bits, canary, check_untouched, is_canary, planes_halves

pytestmark = pytest.mark.gpu
DTYPES = {"f32": (lib.F32, torch.float32), "bf16": (lib.BF16, torch.bfloat16), "planes": (lib.F32X3P, torch.float32)}


def valid_bits(buf, width, planes):
    """The bits of columns [0, width): int32 / int16 [rows, width], or for a planes buffer its (hi, lo) halves side by side."""
    if planes:
        hi, lo = planes_halves(buf)
        return torch.cat([hi[:, :width], lo[:, :width]], 1)
    return bits(buf)[:, :width]


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("D", [64, 33])
@pytest.mark.parametrize("tokens", list(SC.TOKENS))
def test_frustum_sampled_rows_are_the_full_kernels_rows(tokens, D, dtype):
    B, N, h, w = SC.TOKENS[tokens]
    LEN = N * h * w
    dt, tdt = DTYPES[dtype]
    planes = dtype == "planes"
    cfg = dict(synth.HEAD_TOKENS_TINY, depth_num=D)
    inp = synth.head_tokens_inputs(cfg, B, N, h, w, seed=tokens)
    m = toc3d_amd.HeadTokenEmbedding(**cfg)                                 # (for coords_d and the host position_range)
    i2l = torch.linalg.inv(inp["lidar2img"].reshape(B * N, 4, 4)).contiguous().to(DEV)
    intr = inp["intrinsics"].reshape(B * N, 4, 4).contiguous().to(DEV)
    assert N == 1 or not torch.equal(intr[0], intr[1]), "the cameras differ, or the camera rule shows nothing"
    cd = m.coords_d.to(DEV)
    ld = (3 * D + 63) // 64 * 64
    M = B * LEN
    full = canary(M + 3, ld, tdt), canary(M + 3, 64, tdt), canary(M + 3, 8, torch.float32)
    lib.call("toc3d_head_frustum_inputs", dt, i2l, intr, cd, m._pr, B, N, h, w, D, 16, h * 16, w * 16, full[0], ld, full[1], 64, full[2], S())
    fams = SC.index_families(B, LEN, seed=tokens)
    assert set(fams) == ({"one", "permutation"} if tokens == 1 else {"one", "permutation", "subset"})
    if tokens == 24:
        assert any(i % N != i // (h * w) for i in fams["subset"].flatten().tolist()), "an index whose camera (i % N) is not its view (i // hw)"
        assert tuple(fams["subset"].shape) == (2, 7) and len(set(fams["subset"][1].tolist())) == 6, "7 rows from each sample, one planted duplicate"
    for name, index in fams.items():
        K = index.shape[1]
        R = B * K
        idx = index.to(DEV)
        out = canary(R + 3, ld, tdt), canary(R + 3, 64, tdt), canary(R + 3, 8, torch.float32)
        lib.call("toc3d_head_frustum_inputs_sampled", dt, i2l, intr, cd, m._pr, idx, B, N, h, w, K, D, 16, h * 16, w * 16, out[0], ld, out[1], 64, out[2], S())
        src = (idx + torch.arange(B, device=DEV)[:, None] * LEN).flatten()      # row of the full buffers that output row b*K + j must equal
        tag = f"frustum sampled {tokens} tokens D={D} {dtype} {name} K={K}"
        for what, o, f, width in (("pos_in", out[0], full[0], 3 * D), ("cone_act", out[1], full[1], 8)):
            assert torch.equal(valid_bits(o[:R], width, planes), valid_bits(f[:M], width, planes)[src]), f"{tag}: {what} rows differ from the full kernel's"
            check_untouched(f"{tag} {what}", o, R, width, planes)
        assert torch.equal(bits(out[2][:R]), bits(full[2][:M])[src]), f"{tag}: cone rows differ from the full kernel's"
        assert bool(is_canary(out[2][R:]).all()), f"{tag}: cone rows >= {R} were written"


def source_rows(rows, ld, tdt, seed):
    """[rows, ld] of `tdt` holding random 16-bit patterns in every half: whatever the bytes mean, the gather moves them."""
    g = torch.Generator().manual_seed(seed)
    raw = torch.randint(-(1 << 15), 1 << 15, (rows, ld * (1 if tdt == torch.bfloat16 else 2)), generator=g, dtype=torch.int16)
    return raw.to(DEV).view(tdt)


def gather_case(tag, dt, tdt, planes, B, LEN, C, index, ld_src, ld_dst, seed):
    K = index.shape[1]
    R = B * K
    src, dst = source_rows(B * LEN, ld_src, tdt, seed), canary(R + 3, ld_dst, tdt)
    idx = index.to(DEV)
    lib.call("toc3d_gather_token_rows", dt, src, ld_src, idx, B, LEN, K, C, dst, ld_dst, S())
    rows = (idx + torch.arange(B, device=DEV)[:, None] * LEN).flatten()
    assert torch.equal(valid_bits(dst[:R], C, planes), valid_bits(src, C, planes)[rows]), f"{tag}: gathered rows are not the source rows' bits"
    check_untouched(tag, dst, R, C, planes)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("C", [32, 40, 37])
@pytest.mark.parametrize("tokens", list(SC.TOKENS))
def test_gather_token_rows_moves_the_valid_bytes(tokens, C, dtype):
    B, N, h, w = SC.TOKENS[tokens]
    LEN = N * h * w
    dt, tdt = DTYPES[dtype]
    for name, index in SC.index_families(B, LEN, seed=tokens + C).items():
        gather_case(f"gather {tokens} tokens C={C} {dtype} {name}", dt, tdt, dtype == "planes", B, LEN, C, index, 64, 64, seed=tokens + C)


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_gather_token_rows_between_leading_dimensions_and_blocks(dtype):
    """ld_src 128 -> ld_dst 64 and back, and more rows than one workgroup's four: B = 2, LEN = 37, K = 19."""
    dt, tdt = DTYPES[dtype]
    index = SC.index_families(2, 37, seed=9)["subset"]
    assert tuple(index.shape) == (2, 19)
    for C in (40, 37):
        gather_case(f"gather ld 128 -> 64 C={C} {dtype}", dt, tdt, dtype == "planes", 2, 37, C, index, 128, 64, seed=C)
        gather_case(f"gather ld 64 -> 128 C={C} {dtype}", dt, tdt, dtype == "planes", 2, 37, C, index, 64, 128, seed=C)
