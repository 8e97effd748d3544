"""GPU: toc3d_amd.HeadOutputs / toc3d_amd.NMSFreeCoder and the kernels of csrc/head_outputs.hip against the REAL reference's fixtures
(tests/golden/head_outputs_*.npz, written by tools/gen_golden_head_outputs.py), against f64 torch, and against the plain-torch restatement of
tests/head_outputs_cases.py.  Error measure as in tests/test_gpu_decoder.py: max-abs error over max-abs reference, per output group (class logits, centres,
sizes, rotation, velocity -- columns of different scale); the bf16 bounds are relative to a torch-bf16 control on the same card.

Every test prints the figures it asserts on (run with -s); profiles/head_outputs_parity.txt holds that output as measured on an MI355X."""
import os

import numpy as np
import pytest
import torch

import toc3d_amd
from decoder_cases import build as build_decoder
from head_outputs_cases import GROUPS, group_errors, inverse_sigmoid, restated_branches, restated_decode, rows_without_inf
from support import DEV, planes_bf16, rel_l2, rel_max
from toc3d_amd import lib, synth

pytestmark = pytest.mark.gpu
FLT_MAX = float(np.finfo(np.float32).max)


def build(sizes, precision="fp32x3", launch_mode="plan", levels="all", seed=0, coder=None):
    m = toc3d_amd.HeadOutputs(precision=precision, launch_mode=launch_mode, levels=levels, pc_range=synth.PC_RANGE, bbox_coder=coder, **sizes)
    m.load_state_dict(synth.head_outputs_state_dict(sizes, seed=seed), strict=True)
    return m.to(DEV).eval()


def run(m, inp):
    return m(inp["outs_dec"].to(DEV), inp["reference_points"].to(DEV))


def ulps(a, b):
    """Distance in f32 units in the last place between two tensors of non-negative floats."""
    a, b = (torch.as_tensor(t).float().cpu().contiguous().view(torch.int32).long() for t in (a, b))
    return (a - b).abs()


def _full(golden_dir):
    g = np.load(os.path.join(golden_dir, "head_outputs_full.npz"))
    seed = int(g["seed"])
    return g, seed, synth.head_outputs_inputs(synth.HEAD_OUTPUTS_FULL, synth.HEAD_OUTPUTS_FULL_SHAPE, seed=seed)


# ---- the module against the reference's fixtures ----------------------------------------------------------------------------------------------
def test_tiny_fp32x3_matches_reference_golden(golden_dir):
    """fp32x3 (the default) < 1e-3 per output group, the project's parity bar, on both levels -- replayed plan; the cleaned outs_dec exactly (NaN -> 0,
    +-inf -> +-FLT_MAX).  The two rows that held +-inf are compared on the cleaned tensor only (head_outputs_cases.rows_without_inf says why)."""
    g = np.load(os.path.join(golden_dir, "head_outputs_tiny.npz"))
    sizes, shape = synth.HEAD_OUTPUTS_TINY, synth.HEAD_OUTPUTS_TINY_SHAPE
    inp = synth.head_outputs_inputs(sizes, shape)
    m = build(sizes)
    assert m.precision == "fp32x3"
    for _ in range(3):                                  # eager, recorded, replayed
        clean, cls, box = run(m, inp)
    assert clean.shape == (2, 2, 32, 64) and cls.shape == box.shape == (2, 2, 32, 10) and cls.dtype == box.dtype == clean.dtype == torch.float32
    assert np.array_equal(clean.cpu().numpy(), g["outs_dec"]), "nan_to_num is exact"
    rows = rows_without_inf(inp)
    errs = group_errors(cls.cpu(), box.cpu(), g["all_cls_scores"], g["all_bbox_preds"], rows)
    print(f"[head outputs tiny fp32x3] rel max err per group { {k: f'{e:.2e}' for k, e in errs.items()} }")
    assert torch.isfinite(cls[-1]).all() and torch.isfinite(box[-1]).all()
    assert max(errs.values()) < 1e-3, errs


def test_full_size_fp32x3_matches_reference_golden(golden_dir):
    """Shipped sizes (E 256, 6 levels, 900 queries, 10 classes, code_size 10): every level, every group < 1e-3."""
    g, seed, inp = _full(golden_dir)
    m = build(synth.HEAD_OUTPUTS_FULL, seed=seed)
    for _ in range(3):
        clean, cls, box = run(m, inp)
    assert cls.shape == box.shape == (6, 1, 900, 10) and torch.equal(clean.cpu(), inp["outs_dec"])
    worst = {}
    for l in range(6):
        for k, e in group_errors(cls[l].cpu(), box[l].cpu(), g["all_cls_scores"][l], g["all_bbox_preds"][l]).items():
            worst[k] = max(worst.get(k, 0.0), e)
    print(f"[head outputs full fp32x3] worst level, rel max err per group { {k: f'{e:.2e}' for k, e in worst.items()} }")
    assert max(worst.values()) < 1e-3, worst


@pytest.mark.parametrize("size", ["tiny", "full"])
def test_bf16_within_control(golden_dir, size):
    """bf16: relative L2 against the reference's f32 output, per group, at most 1.2 x that of the torch-bf16 control (the restatement with the linear layers'
    operands rounded to bf16, f32 accumulation, on the same card) -- the convention of tests/test_gpu_decoder.py."""
    if size == "tiny":
        g, seed = np.load(os.path.join(golden_dir, "head_outputs_tiny.npz")), 0
        sizes, inp = synth.HEAD_OUTPUTS_TINY, synth.head_outputs_inputs(synth.HEAD_OUTPUTS_TINY, synth.HEAD_OUTPUTS_TINY_SHAPE)
    else:
        (g, seed, inp), sizes = _full(golden_dir), synth.HEAD_OUTPUTS_FULL
    m = build(sizes, precision="bf16", seed=seed)
    for _ in range(3):
        _, cls, box = run(m, inp)
    with torch.no_grad():
        _, ccls, cbox = restated_branches(synth.head_outputs_state_dict(sizes, seed=seed), {k: v.to(DEV) for k, v in inp.items()}, contract=torch.bfloat16)
    rows = rows_without_inf(inp)
    rcls, rbox = torch.from_numpy(g["all_cls_scores"]), torch.from_numpy(g["all_bbox_preds"])
    pick = lambda t: t.cpu()[rows]
    pairs = {"cls": (pick(cls), pick(ccls), pick(rcls))}
    pairs.update({k: (pick(box)[..., s], pick(cbox)[..., s], pick(rbox)[..., s]) for k, s in GROUPS.items()})
    res = {k: (rel_l2(a, r), rel_l2(c, r)) for k, (a, c, r) in pairs.items()}
    print(f"[head outputs {size} bf16] rel l2 vs the reference, hip / torch-bf16 control: { {k: f'{a:.3e} / {c:.3e}' for k, (a, c) in res.items()} }")
    assert torch.isfinite(pick(cls)).all() and torch.isfinite(pick(box)).all()
    for k, (a, c) in res.items():
        assert a <= 1.2 * c, (k, a, c)


@pytest.mark.parametrize("precision", ["fp32x3", "bf16"])
def test_last_level_plan_replay_and_reruns_are_bit_identical(golden_dir, precision):
    sizes, shape = synth.HEAD_OUTPUTS_FULL, synth.HEAD_OUTPUTS_FULL_SHAPE
    a, b = synth.head_outputs_inputs(sizes, shape, seed=0), synth.head_outputs_inputs(sizes, shape, seed=1)
    eager, plan, last = build(sizes, precision, "eager"), build(sizes, precision, "plan"), build(sizes, precision, "plan", levels="last")
    ea, eb = run(eager, a), run(eager, b)
    assert not torch.equal(ea[1], eb[1])
    for _ in range(3):
        pa = run(plan, a)
        la = run(last, a)
    state = plan._states[(6, 1, 900)]
    assert state.get("cplan") is not None and state["cplan"].num_launches == 6           # three row kernels around three GEMMs
    assert all(torch.equal(x, y) for x, y in zip(pa, ea)), "eager launches and the replayed plan differ"
    assert all(t.shape[0] == 1 for t in la) and all(torch.equal(x[0], y[-1]) for x, y in zip(la, pa)), "levels='last' differs from the last level of 'all'"
    pb = run(plan, b)                                   # other inputs through the SAME recorded plan
    assert plan._states[(6, 1, 900)]["cplan"] is state["cplan"]
    assert all(torch.equal(x, y) for x, y in zip(pb, eb)) and all(torch.equal(x, y) for x, y in zip(pa, ea)), "an output aliases a workspace"
    pa2 = run(plan, a)
    assert all(torch.equal(x, y) for x, y in zip(pa2, pa)), "two runs differ"


# ---- the row kernels alone, against f64 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [64, 192, 256])
def test_nan_to_num_rows_is_exact_in_every_output_form(E):
    M, ldx, ldo, lda = 13, E + 8, E + 4, E + 32
    g = torch.Generator().manual_seed(E)
    x = torch.randn(M + 2, ldx, generator=g)
    x[0, 0], x[3, E - 1], x[5, 7], x[12, E // 2], x[12, 1] = float("nan"), float("inf"), float("-inf"), -float("nan"), float("inf")
    want = torch.nan_to_num(x[:M, :E])
    assert want.abs().max() == FLT_MAX and torch.isfinite(want).all()
    x = x.to(DEV)
    for dt, tdt in ((lib.F32, torch.float32), (lib.BF16, torch.bfloat16), (lib.F32X3P, torch.float32)):
        out = torch.full((M + 2, ldo), 777.0, device=DEV)
        act = torch.full((M + 2, lda), 777.0, dtype=tdt, device=DEV)
        lib.call("toc3d_head_nan_to_num_rows", dt, x, ldx, out, ldo, act, lda, M, E, lib.stream_ptr())
        torch.cuda.synchronize()
        assert torch.equal(out[:M, :E].cpu(), want) and bool((out[M:] == 777.0).all()) and bool((out[:, E:] == 777.0).all())
        assert bool((act[M:] == 777.0).all())
        if dt == lib.F32X3P:
            hi, lo = planes_bf16(act, M, E)
            assert torch.equal(hi.cpu(), want.bfloat16()) and torch.equal(lo.cpu(), (want - want.bfloat16().float()).bfloat16())
            assert bool((act[:M, E:] == 777.0).all())
        else:
            assert torch.equal(act[:M, :E].cpu(), want.to(tdt)) and bool((act[:, E:] == 777.0).all())
    only = torch.full((M, E), 777.0, device=DEV)                                       # either output alone
    lib.call("toc3d_head_nan_to_num_rows", lib.BF16, x, ldx, only, E, None, 0, M, E, lib.stream_ptr())
    assert torch.equal(only.cpu(), want)


@pytest.mark.parametrize("E", [64, 192, 256])
def test_ln_relu_rows_against_f64(E):
    """relu(LayerNorm) on the class tower's columns, relu on the box tower's: 1e-4, a tenth of the end-to-end budget (tests/test_gpu_decoder.py:70)."""
    M, ldx, lda = 13, 2 * E + 8, 2 * E + 32
    g = torch.Generator().manual_seed(E + 1)
    x = (torch.randn(M + 1, ldx, generator=g) * 3.0 + 0.5).to(DEV)
    gamma, beta = (1.0 + 0.1 * torch.randn(E, generator=g)).to(DEV), (0.1 * torch.randn(E, generator=g)).to(DEV)
    xd = x[:M, :E].double()
    mu = xd.mean(-1, keepdim=True)
    want = torch.cat([torch.relu((xd - mu) / torch.sqrt(((xd - mu) ** 2).mean(-1, keepdim=True) + 1e-5) * gamma.double() + beta.double()),
                      torch.relu(x[:M, E:2 * E].double())], -1)
    got = {}
    for dt, tdt in ((lib.F32, torch.float32), (lib.BF16, torch.bfloat16), (lib.F32X3P, torch.float32)):
        act = torch.full((M + 1, lda), 777.0, dtype=tdt, device=DEV)
        lib.call("toc3d_head_ln_relu_rows", dt, x, ldx, gamma, beta, 1e-5, act, lda, M, E, E, lib.stream_ptr())
        torch.cuda.synchronize()
        assert bool((act[M:] == 777.0).all()) and bool((act[:M, 2 * E:] == 777.0).all())
        got[dt] = act
    f32 = got[lib.F32][:M, :2 * E]
    err = max(rel_max(f32[:, :E], want[:, :E]), rel_max(f32[:, E:], want[:, E:]))
    print(f"[ln_relu_rows E={E}] rel max err vs f64 {err:.2e}")
    assert err < 1e-4 and bool((f32 >= 0).all())
    assert torch.equal(got[lib.BF16][:M, :2 * E], f32.bfloat16()), "the bf16 form is the f32 form rounded once"
    hi, lo = planes_bf16(got[lib.F32X3P], M, 2 * E)
    assert torch.equal(hi, f32.bfloat16()) and torch.equal(lo, (f32 - f32.bfloat16().float()).bfloat16())
    solo = torch.full((M, E), 777.0, device=DEV)                                       # the LayerNorm half alone (E_relu = 0)
    lib.call("toc3d_head_ln_relu_rows", lib.F32, x, ldx, gamma, beta, 1e-5, solo, E, M, E, 0, lib.stream_ptr())
    assert torch.equal(solo, f32[:, :E])


@pytest.mark.parametrize("E,M,NC,CS", [(64, 13, 10, 10), (192, 13, 10, 10), (256, 13, 10, 10), (256, 4101, 10, 10), (64, 7, 3, 8)])
def test_head_outputs_kernel_against_f64(E, M, NC, CS):
    """Last LayerNorm + ReLU / ReLU on load, the two narrow layers, reference points at 0, 1, below the 1e-5 clamp and outside [0, 1], sigmoid, pc_range: each
    output group to 1e-4 of f64; padded leading dimensions, sentinels around the outputs, more rows than one pass of the grid (M = 4101)."""
    g = torch.Generator().manual_seed(E + M)
    r = lambda *s: torch.randn(*s, generator=g)
    ldh, ldc, ldb, R = 2 * E + 8, NC + 2, CS + 6, 5
    h = (r(M + 1, ldh) * 2.0).to(DEV)
    gamma, beta = (1.0 + 0.1 * r(E)).to(DEV), (0.1 * r(E)).to(DEV)
    wc, bc, wr, br = (r(NC, E) * E ** -0.5).to(DEV), (r(NC) - 2.0).to(DEV), (r(CS, E) * E ** -0.5).to(DEV), (r(CS) * 0.1).to(DEV)
    ref = torch.tensor([[0.0, 1.0, 0.5], [3e-6, 1.0 - 3e-6, 0.25], [-0.5, 1.5, 0.9], [0.3, 0.6, 1e-5], [0.7, 0.2, 0.999]]).to(DEV)
    pc = torch.tensor(synth.PC_RANGE)
    cls = torch.full((M + 1, ldc), 777.0, device=DEV)
    box = torch.full((M + 1, ldb), 777.0, device=DEV)
    lib.call("toc3d_head_outputs", h, ldh, gamma, beta, 1e-5, wc, bc, wr, br, ref, R, pc, cls, ldc, box, ldb, M, E, NC, CS, lib.stream_ptr())
    torch.cuda.synchronize()
    assert bool((cls[M:] == 777.0).all()) and bool((cls[:, NC:] == 777.0).all()) and bool((box[M:] == 777.0).all()) and bool((box[:, CS:] == 777.0).all())
    d = lambda t: t.double()
    c, b = d(h[:M, :E]), torch.relu(d(h[:M, E:2 * E]))
    mu = c.mean(-1, keepdim=True)
    c = torch.relu((c - mu) / torch.sqrt(((c - mu) ** 2).mean(-1, keepdim=True) + 1e-5) * d(gamma) + d(beta))
    want_cls, want_box = c @ d(wc).T + d(bc), b @ d(wr).T + d(br)
    refs = d(ref)[torch.arange(M, device=DEV) % R]
    pcd = pc.double().to(DEV)
    want_box[:, :3] = torch.sigmoid(want_box[:, :3] + inverse_sigmoid(refs)) * (pcd[3:6] - pcd[0:3]) + pcd[0:3]
    errs = {"cls": rel_max(cls[:M, :NC], want_cls)}
    errs.update({k: rel_max(box[:M, s], want_box[:, s]) for k, s in GROUPS.items() if s.stop <= CS})
    print(f"[head_outputs kernel E={E} M={M} NC={NC} CS={CS}] rel max err vs f64 { {k: f'{e:.2e}' for k, e in errs.items()} }")
    assert max(errs.values()) < 1e-4, errs


# ---- decoding --------------------------------------------------------------------------------------------------------------------------------
def gpu_decode(cls, box, max_num, pcr, thr=None, sub=False):
    """(B, Q, NC), (B, Q, CS) -> per sample (bboxes, scores, labels, flat indices) of the survivors, and the fixed-capacity tensors."""
    c = toc3d_amd.NMSFreeCoder(pc_range=synth.PC_RANGE, post_center_range=pcr, max_num=max_num, score_threshold=thr, num_classes=cls.shape[-1])
    cls0, box0 = cls.clone(), box.clone()
    boxes, scores, labels, qidx, counts = c.decode_fixed(cls, box, sub_half_height=sub)
    torch.cuda.synchronize()
    assert torch.equal(cls, cls0) and torch.equal(box, box0), "the inputs are not modified"
    n = counts.tolist()
    for b, k in enumerate(n):                           # rows past the count: zeros, indices -1
        assert bool((boxes[b, k:] == 0).all()) and bool((scores[b, k:] == 0).all()) and bool((labels[b, k:] == -1).all()) and bool((qidx[b, k:] == -1).all())
    return [(boxes[b, :k].cpu(), scores[b, :k].cpu(), labels[b, :k].cpu(), (qidx[b, :k] * cls.shape[-1] + labels[b, :k]).cpu()) for b, k in enumerate(n)]


def test_decode_of_the_reference_logits_and_boxes(golden_dir):
    """On the fixture's REFERENCE logits and boxes: the (query, label) list is the reference's, scores non-increasing and within 2 ulp of the reference's, every box
    column within 4 x decode_f32_err of the f64 decode (the reference's own f32 error is the yardstick; the device expf / atan2f may be a few ulp off libm's)."""
    g = np.load(os.path.join(golden_dir, "head_outputs_full.npz"))
    cls, box = torch.from_numpy(g["all_cls_scores"][-1]).to(DEV), torch.from_numpy(g["all_bbox_preds"][-1]).to(DEV)
    (bb, sc, lb, idx), = gpu_decode(cls, box, int(g["max_num"]), g["post_center_range"].tolist())
    assert len(idx) == 300 and np.array_equal(idx.numpy(), g["dec_index"]) and np.array_equal(lb.numpy(), g["dec_labels"])
    assert bool((sc[1:] <= sc[:-1]).all())
    u = int(ulps(sc, g["dec_scores"]).max())
    col_err = (bb.double() - torch.from_numpy(g["dec_bboxes_f64"])).abs().max(0).values.numpy()
    yard = g["decode_f32_err"][:9]
    ratios = [f"{e / y:.2f}" if y > 0 else ("exact" if e == 0 else "inf") for e, y in zip(col_err, yard)]
    print(f"[decode of the reference's last level] score ulps vs the reference {u}; box columns, error vs f64 decode / decode_f32_err: {ratios}")
    assert u <= 2
    assert (col_err <= 4 * yard).all(), (col_err, yard)


def _expect(cls, box, max_num, pcr, thr=None, sub=False):
    return [restated_decode(cls[b].cpu(), box[b].cpu(), max_num, pcr, thr, sub) for b in range(cls.shape[0])]


def _same(got, want, tag):
    for b, ((bb, sc, lb, idx), (wbb, wsc, wlb, widx, _)) in enumerate(zip(got, want)):
        assert len(idx) == len(widx), (tag, b, len(idx), len(widx))
        assert torch.equal(idx, widx) and torch.equal(lb, wlb), (tag, b)
        assert int(ulps(sc, wsc).max() if len(sc) else 0) <= 2 and bool((sc[1:] <= sc[:-1]).all()), (tag, b)
        if len(sc):
            assert torch.allclose(bb, wbb, rtol=2e-6, atol=1e-6), (tag, b)
            assert torch.equal(bb[:, [0, 1, 7, 8] if bb.shape[1] == 9 else [0, 1]], wbb[:, [0, 1, 7, 8] if bb.shape[1] == 9 else [0, 1]]), (tag, b)


def _boxes(B, Q, CS, g, inside=None):
    """Box rows whose centres lie well inside (True) / well outside (False) a [-10, 10]^3 range, or on a coarse grid for `inside=None`."""
    box = torch.randn(B, Q, CS, generator=g) * 0.5
    centre = torch.randint(-9, 10, (B, Q, 3), generator=g).float()
    if inside is not None:
        centre = torch.where(inside[..., None], centre, centre + 30.0)
    box[..., :3] = centre
    return box


PCR10 = [-10.0, -10.0, -10.0, 10.0, 10.0, 10.0]


def test_decode_well_separated_logits_ties_and_saturated_scores():
    """Families whose expected answer is exact on both sides: distinct logits far apart; blocks of equal logits (the tie goes to the lowest flat index); logits
    >= 30, whose sigmoid is exactly 1.0f."""
    g = torch.Generator().manual_seed(11)
    B, Q, NC = 2, 900, 10
    box = _boxes(B, Q, 10, g).to(DEV)
    spread = torch.stack([torch.linspace(-8, 8, Q * NC)[torch.randperm(Q * NC, generator=g)] for _ in range(B)]).view(B, Q, NC)
    ties = torch.randint(-6, 7, (B, Q, NC), generator=g).float()
    ones = torch.tensor([30.0, 35.0, 40.0, 100.0, 31.5])[torch.randint(0, 5, (B, Q, NC), generator=g)]
    mixed = torch.where(torch.rand(B, Q, NC, generator=g) < 0.02, ones, ties)
    for tag, cls in (("spread", spread), ("ties", ties), ("ones", ones), ("mixed", mixed)):
        for K in (1, 64, 300, 1500, 2048):
            _same(gpu_decode(cls.to(DEV), box, K, PCR10), _expect(cls, box, K, PCR10), (tag, K))
    sat = gpu_decode(ones.to(DEV), box, 300, PCR10)
    assert all(bool((sc == 1.0).all()) and torch.equal(idx, torch.arange(300)) for _, sc, _, idx in sat)


def test_decode_mask_threshold_counts_and_code_size_8():
    """max_num equal to, below and above what the mask keeps; a narrowed post_center_range with centres exactly on its bounds (inclusive at both ends);
    score_threshold; B > 1 with different survivor counts; code_size 8 (7 output columns); the z shift of get_bboxes."""
    g = torch.Generator().manual_seed(12)
    B, Q, NC = 3, 200, 10
    cls = torch.stack([torch.linspace(-6, 6, Q * NC)[torch.randperm(Q * NC, generator=g)] for _ in range(B)]).view(B, Q, NC)
    inside = torch.rand(B, Q, generator=g) < torch.tensor([0.8, 0.3, 0.0])[:, None]          # sample 2 keeps nothing
    inside[0, :50] = True
    box = _boxes(B, Q, 10, g, inside)
    box[0, :10, 0], box[0, 10:20, 1], box[0, 20:30, 2] = 10.0, -10.0, 10.0                   # on the bounds: kept
    box[0, 30:40, 0] = torch.nextafter(torch.tensor(10.0), torch.tensor(11.0))               # one ulp outside: dropped
    box[0, 40:50, 2] = torch.nextafter(torch.tensor(-10.0), torch.tensor(-11.0))
    cls[0, :50] = torch.linspace(6.2, 9.0, 50 * NC)[torch.randperm(50 * NC, generator=g)].view(50, NC)   # ... and among the best (distinct, unsaturated): every K sees them
    dev = lambda t: t.to(DEV)
    for K in (17, 300, 1000, 2000):
        for thr in (None, 0.0, 0.6):
            for sub in (False, True):
                got, want = gpu_decode(dev(cls), dev(box), K, PCR10, thr, sub), _expect(cls, box, K, PCR10, thr, sub)
                _same(got, want, (K, thr, sub))
                assert len(got[2][3]) == 0
    counts = [len(s[3]) for s in gpu_decode(dev(cls), dev(box), 300, PCR10)]
    kept = [int(inside[b].sum()) for b in range(B)]
    assert counts[0] != counts[1] and 0 < counts[1] < 300 and counts[2] == 0, counts
    # max_num equal to / above what the mask keeps: every (query, class) pair of the surviving queries, nothing else
    all_k = Q * NC
    full = gpu_decode(dev(cls), dev(box), all_k, PCR10)
    assert len(full[1][3]) == kept[1] * NC and len(full[0][3]) == (kept[0] - 20) * NC
    eq = gpu_decode(dev(cls[1:2, inside[1]]), dev(box[1:2, inside[1]]), kept[1] * NC, PCR10)
    assert len(eq[0][3]) == kept[1] * NC
    # code_size 8: no velocity, 7 output columns
    got8 = gpu_decode(dev(cls), dev(box[..., :8].contiguous()), 300, PCR10, None, True)
    assert got8[0][0].shape[1] == 7
    _same(got8, _expect(cls, box[..., :8], 300, PCR10, None, True), "code_size 8")


def test_decode_of_the_modules_own_output_and_get_bboxes(golden_dir):
    """The GPU's own all_cls_scores / all_bbox_preds through the GPU coder against the restatement's decode of the SAME tensors: candidates whose score lies
    within 4 ulp of the boundary score may differ, at most 2 of them.  get_bboxes returns the same survivors with z -= h / 2 and edits none of its inputs."""
    g, seed, inp = _full(golden_dir)
    seen = []

    class Boxes:                                        # stands in for img_metas[i]['box_type_3d']
        def __init__(self, t, dim):
            seen.append(dim)
            self.tensor = t
    m = build(synth.HEAD_OUTPUTS_FULL, seed=seed, coder=synth.bbox_coder_cfg())
    for _ in range(3):
        _, cls, box = run(m, inp)
    preds = dict(all_cls_scores=cls, all_bbox_preds=box)
    cls0, box0 = cls.clone(), box.clone()
    (gbb, gsc, glb), = m.get_bboxes(preds, [dict(box_type_3d=Boxes)])
    (pbb, psc, plb), = m.get_bboxes(preds)
    assert torch.equal(cls, cls0) and torch.equal(box, box0) and seen == [9] and torch.equal(gbb.tensor, pbb) and pbb.shape == (300, 9)
    dec, = m.bbox_coder.decode(preds)
    one = m.bbox_coder.decode_single(cls[-1, 0], box[-1, 0])
    assert torch.equal(dec["scores"], psc) and torch.equal(dec["labels"], plb) and torch.equal(one["bboxes"], dec["bboxes"]) and dec["labels"].dtype == torch.int64
    assert torch.equal(dec["bboxes"][:, 2] - dec["bboxes"][:, 5] * 0.5, pbb[:, 2]) and torch.equal(dec["bboxes"][:, [0, 1, 3, 4, 5, 6, 7, 8]], pbb[:, [0, 1, 3, 4, 5, 6, 7, 8]])
    wbb, wsc, wlb, widx, _ = restated_decode(cls[-1, 0].cpu(), box[-1, 0].cpu(), 300, synth.bbox_coder_cfg()["post_center_range"], None, True)
    gidx = gpu_decode(cls[-1], box[-1], 300, synth.bbox_coder_cfg()["post_center_range"], None, True)[0][3]
    diff = set(gidx.tolist()) ^ set(widx.tolist())
    flat = cls[-1, 0].cpu().sigmoid().view(-1)
    boundary = wsc[-1]
    print(f"[decode of the module's own output] candidates that differ from the restatement's: {len(diff)}")
    assert len(diff) <= 2 and all(int(ulps(flat[i], boundary)) <= 4 for i in diff), diff
    assert bool((psc[1:] <= psc[:-1]).all())
    if not diff:
        assert int(ulps(psc, wsc).max()) <= 2 and torch.allclose(pbb.cpu(), wbb, rtol=2e-6, atol=1e-6)


# ---- streaming: decoder -> HeadOutputs -> TemporalMemory --------------------------------------------------------------------------------------
def test_streaming_two_frames_decoder_head_outputs_memory():
    """Two frames of PETRTemporalTransformer -> HeadOutputs -> TemporalMemory.post_update_memory at tiny sizes, tensors handed over as they come.  After each
    frame the bank's first topk_proposals rows are exactly the outs_dec[-1] rows ranked by the module's own class scores (max sigmoid over the classes as
    toc3d_memory_scores computes it, descending, ties to the lowest query).  The expected order below comes from toc3d_memory_scores itself: that kernel is pinned
    on its own, per element against f64, by tests/test_gpu_head_row_kernels.py::test_memory_scores."""
    dsz, dshape, hsz = synth.DECODER_TINY, synth.DECODER_TINY_SHAPE, synth.HEAD_OUTPUTS_TINY
    B, Q, E, TOPK = dshape["B"], dshape["num_query"] + dshape["num_propagated"], dsz["embed_dims"], 8
    mcfg = dict(memory_len=dshape["Nm"], topk_proposals=TOPK, num_propagated=dshape["num_propagated"], embed_dims=E)
    minp = synth.memory_inputs(mcfg, B, dshape["num_query"], 10, 2, seed=5)
    dec, head = build_decoder(dsz), build(hsz, levels="last")
    mem = toc3d_amd.TemporalMemory(pseudo_reference_points=minp["pseudo"], pc_range=synth.PC_RANGE, **mcfg)
    d = lambda t: None if t is None else t.to(DEV)
    banks = []
    for f in range(2):
        qin = synth.decoder_inputs(dsz, dshape, seed=20 + f)
        ref = torch.rand(B, Q, 3, generator=torch.Generator().manual_seed(30 + f))
        data = {k: d(v) for k, v in minp["frames"][f]["data"].items()}
        mem.pre_update_memory(data)
        temp_memory = mem.memory_embedding
        outs_dec, _, _ = dec(d(qin["memory"]), d(qin["tgt"]), d(qin["query_pos"]), d(qin["pos_embed"]), None, temp_memory, d(qin["temp_pos"])[:, :temp_memory.shape[1]])
        outs, cls, box = head(outs_dec, d(ref))
        assert outs.shape == (1, B, Q, E) and cls.shape == box.shape == (1, B, Q, 10) and torch.equal(outs[0], outs_dec[-1])
        mem.post_update_memory(data, d(minp["frames"][f]["rec_ego_pose"]), cls, box, outs)
        score = torch.empty(B, Q, device=DEV)
        lib.call("toc3d_memory_scores", cls[-1].contiguous(), B * Q, 10, score, lib.stream_ptr())
        order = torch.sort(score, dim=1, descending=True, stable=True).indices[:, :TOPK]
        want = torch.gather(outs[-1], 1, order[..., None].expand(B, TOPK, E))
        assert mem.memory_embedding.shape == (B, dshape["Nm"] + TOPK, E) and torch.equal(mem.memory_embedding[:, :TOPK], want), f"frame {f}"
        assert torch.equal(score, cls[-1].sigmoid().amax(-1)) or float((score - cls[-1].sigmoid().amax(-1)).abs().max()) < 1e-6
        banks.append(mem.memory_embedding.clone())
    assert not torch.equal(banks[0][:, :TOPK], banks[1][:, :TOPK])
