"""GPU: toc3d_amd.HeadQueries and the kernels of csrc/head_queries.hip against the REAL reference's fixtures (tests/golden/head_queries_*.npz, written by
tools/gen_golden_head_queries.py), against torch on the CPU / f64 torch, and against the plain-torch restatement of tests/head_queries_cases.py.  Error measure as
in tests/test_gpu_head_outputs.py: max-abs error over max-abs reference per output; the bf16 bounds are relative to a torch-bf16 control on the same card.

Every test prints the figures it asserts on (run with -s); profiles/head_queries_parity.txt holds that output as measured on an MI355X."""
import pytest
import torch

import toc3d_amd
from decoder_cases import build as build_decoder
from head_queries_cases import BANK, OUTPUTS, full_cases, nerf, pos3d, posemb, restated_queries, tiny_cases
from support import DEV, planes_bf16, rel_l2, rel_max_zero_ok
from toc3d_amd import lib, synth
from toc3d_amd.head_queries import dim_t

pytestmark = pytest.mark.gpu
SENT = 768.0                                     # exact in bf16
GEMM_OUTPUTS, EXACT_OUTPUTS = ("tgt", "query_pos", "temp_memory", "temp_pos"), ("reference_points", "rec_ego_pose")


def build(sizes, with_ego_pos=True, precision="fp32x3", launch_mode="plan", seed=0):
    m = toc3d_amd.HeadQueries(precision=precision, launch_mode=launch_mode, with_ego_pos=with_ego_pos, pc_range=synth.PC_RANGE, **sizes)
    m.load_state_dict(synth.head_queries_state_dict(sizes, with_ego_pos=with_ego_pos, seed=seed), strict=True)
    return m.to(DEV).eval()


def run(m, bank):
    return dict(zip(OUTPUTS, m(*(bank[k].to(DEV) for k in BANK))))


def capacity_views(bank, extra):
    """The bank as a TemporalMemory holds it: views [:, :n] of (B, n + extra, ...) buffers -- sample stride (n + extra) * row for B > 1."""
    out = {}
    for k in BANK:
        t = bank[k]
        buf = torch.full((t.shape[0], t.shape[1] + extra, *t.shape[2:]), 3.0, dtype=t.dtype, device=DEV)
        buf[:, :t.shape[1]] = t.to(DEV)
        out[k] = buf[:, :t.shape[1]]
    return out


# ---- 1. the input kernel alone, against torch on the CPU -------------------------------------------------------------------------------------------
def test_query_inputs_kernel_against_torch_cpu(golden_dir):
    """Same ops in torch on the CPU, f32 act dtype, the tiny fixture's bank of frame 1 (B 2, 27 entries) plus two rows per sample: an epoch-scale timestamp
    (1.5e9 + 0.5: arguments up to 2 pi * 1.5e9 in f64 and 32 * 1.5e9 in f32) and a 40 m translation (32 * 40 rad).  Bounds from the number formats: both libraries
    lie within 2 ulp of the true value and |value| <= 1, so 4 * 2^-24 absolute for pos3d and nerf; t1d is an f64 result rounded once: 2^-24."""
    _, sizes, _, bank, _ = tiny_cases(golden_dir)[1]
    B, n0, np_ = 2, 27, 7
    ext = {k: torch.cat([bank[k], bank[k][:, :2].clone()], 1) for k in BANK}
    n = n0 + 2
    ext["memory_timestamp"][:, n0] = 1.5e9 + 0.5
    ext["memory_egopose"][:, n0 + 1, :3, 3] = torch.tensor([40.0, -40.0, 39.5])
    dv = capacity_views(ext, 9)
    pc = torch.tensor(synth.PC_RANGE)
    tref = (ext["memory_reference_point"] - pc[:3]) / (pc[3:] - pc[:3])
    want = dict(pos3d=pos3d(tref).view(B * n, 384),
                nerf=nerf(torch.cat([ext["memory_velo"], ext["memory_timestamp"], ext["memory_egopose"][..., :3, :].flatten(-2)], -1).float()).view(B * n, 180),
                t1d=posemb(ext["memory_timestamp"][..., 0], 256).float().view(B * n, 256))
    assert want["t1d"].dtype == torch.float32 and ext["memory_timestamp"].dtype == torch.float64
    d3, d1 = dim_t(128).to(DEV), dim_t(256).to(DEV)
    M, lds, widths = B * n, dict(pos3d=384 + 32, nerf=192 + 64, t1d=256 + 96), dict(pos3d=384, nerf=192, t1d=256)
    Q = 21 + np_
    outs = {}
    for dt, tdt in ((lib.F32, torch.float32), (lib.BF16, torch.bfloat16), (lib.F32X3P, torch.float32)):
        o = {k: torch.full((M + 3, lds[k]), SENT, dtype=tdt, device=DEV) for k in lds}
        ref_out = torch.full((B, Q + 2, 3), SENT, device=DEV)
        ts = dv["memory_timestamp"]
        lib.call("toc3d_head_query_inputs", dt, dv["memory_reference_point"], dv["memory_reference_point"].stride(0), dv["memory_velo"], dv["memory_velo"].stride(0),
                 ts, ts.stride(0), dv["memory_egopose"], dv["memory_egopose"].stride(0), pc, d3, d1, o["pos3d"], lds["pos3d"], o["nerf"], lds["nerf"],
                 o["t1d"], lds["t1d"], ref_out[:, 21:], ref_out.stride(0), B, n, np_, 256, lib.stream_ptr())
        torch.cuda.synchronize()
        outs[dt] = {k: v.cpu() for k, v in o.items()}
        if dt != lib.F32X3P:                                # (a row of planes owns its whole 128-byte groups: the padding is checked on the plain forms)
            for k, v in outs[dt].items():
                assert bool((v[M:].float() == SENT).all()) and bool((v[:M, widths[k]:].float() == SENT).all()), f"{k}: sentinels past the rows / columns were overwritten"
        ref_out = ref_out.cpu()
        assert bool((ref_out[:, :21] == SENT).all()) and bool((ref_out[:, Q:] == SENT).all()), "reference-point tail: sentinels overwritten"
        assert torch.equal(ref_out[:, 21:Q], tref[:, :np_]), "the normalised reference points of the first np rows (same f32 ops: exact)"
    f32 = outs[lib.F32]
    errs = {k: float((f32[k][:M, :want[k].shape[1]] - want[k]).abs().max()) for k in want}
    big = {"t1d epoch row": float((f32["t1d"][:M].view(B, n, -1)[:, n0, :256] - want["t1d"].view(B, n, -1)[:, n0]).abs().max()),
           "nerf epoch row": float((f32["nerf"][:M].view(B, n, -1)[:, n0, :180] - want["nerf"].view(B, n, -1)[:, n0]).abs().max()),
           "nerf 40 m row": float((f32["nerf"][:M].view(B, n, -1)[:, n0 + 1, :180] - want["nerf"].view(B, n, -1)[:, n0 + 1]).abs().max())}
    print(f"[query inputs kernel] max abs err vs torch CPU, in units of 2^-24: { {k: round(e * 2 ** 24, 3) for k, e in {**errs, **big}.items()} }")
    assert bool((f32["nerf"][:M, 180:192] == 0).all()), "the 12 padding columns of nerf"
    assert errs["pos3d"] <= 4 * 2.0 ** -24 and errs["nerf"] <= 4 * 2.0 ** -24, errs
    assert errs["t1d"] <= 2.0 ** -24, errs
    for k, w in widths.items():
        assert torch.equal(outs[lib.BF16][k][:M, :w].view(torch.int16), f32[k][:M, :w].to(torch.bfloat16).view(torch.int16)), f"{k}: bf16 output is RNE of the f32 output"
        hi, lo = planes_bf16(outs[lib.F32X3P][k], M, w)
        x = f32[k][:M, :w]
        assert torch.equal(hi.view(torch.int16), x.to(torch.bfloat16).view(torch.int16)), f"{k}: hi plane"
        assert torch.equal(lo.view(torch.int16), (x - x.to(torch.bfloat16).float()).to(torch.bfloat16).view(torch.int16)), f"{k}: lo plane"


# ---- 2. the combine kernel alone, against f64 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,n,np_", [(1, 1, 0), (1, 1, 1), (1, 5, 0), (1, 5, 5), (2, 27, 0), (2, 27, 7)])
@pytest.mark.parametrize("ego", [True, False])
def test_query_combine_kernel_against_f64(B, n, np_, ego):
    """Rows 1, 5 and 2 * 27, nothing / some / everything propagated (np is capped by the n of the small cases), every buffer with its own padded leading dimension
    and sample stride; a zero memory row (LN0(0) = 0 exactly: the output row is the beta row bit for bit); 1e-4 of f64, the row kernels' bar in
    tests/test_gpu_head_outputs.py; sentinels everywhere the concatenation does not write."""
    E, M, nt = 256, B * n, n - np_
    g = torch.Generator().manual_seed(100 * n + 10 * np_ + B)
    r = lambda *s: torch.randn(*s, generator=g)
    ld = dict(qe=260, gb_pe=516, te=264, mem=268, gb_mem=520, tail=272, temp=276)
    mem_s, tail_s = n * ld["mem"] + 8, max(np_, 1) * ld["tail"] + 16
    qe, gb_pe, te, gb_mem = r(M, ld["qe"]) * 2 + 0.5, r(M, ld["gb_pe"]), r(M, ld["te"]) * 3 - 1, r(M, ld["gb_mem"])
    mem = r(B, mem_s)
    memv = torch.as_strided(mem, (B, n, E), (mem_s, ld["mem"], 1))
    memv[B - 1, n - 1] = 0.0
    w, b = 1 + 0.1 * r(E), 0.1 * r(E)
    d = lambda t: t.to(DEV)
    dq, dgp, dte, dgm, dmem, dw, db = map(d, (qe, gb_pe, te, gb_mem, mem, w, b))
    qt, tt = (torch.full((B, tail_s), SENT, device=DEV) for _ in range(2))
    tp, tm = (torch.full((B * nt + 2, ld["temp"]), SENT, device=DEV) for _ in range(2))
    lib.call("toc3d_head_query_combine", dq, ld["qe"], dgp if ego else None, ld["gb_pe"], dte, ld["te"], dw, db, 1e-5, dmem, mem_s, ld["mem"], dgm if ego else None, ld["gb_mem"],
             qt if np_ else None, tail_s, tt if np_ else None, tail_s, ld["tail"], tp if nt else None, tm if nt else None, ld["temp"], B, n, np_, E, lib.stream_ptr())
    torch.cuda.synchronize()
    D = torch.float64
    ln0 = lambda x: torch.nn.functional.layer_norm(x.to(D), (E,))
    x, t, mm = qe[:, :E].to(D), te[:, :E], memv.reshape(M, E).to(D)
    pos = (gb_pe[:, :E].to(D) * ln0(x) + gb_pe[:, E:2 * E].to(D)) if ego else x
    pos = pos + torch.nn.functional.layer_norm(t.to(D), (E,), w.to(D), b.to(D))
    mo = (gb_mem[:, :E].to(D) * ln0(mm) + gb_mem[:, E:2 * E].to(D)) if ego else mm
    pos, mo = pos.view(B, n, E), mo.view(B, n, E)
    qt_v, tt_v = (torch.as_strided(t_.cpu(), (B, np_, E), (tail_s, ld["tail"], 1)) for t_ in (qt, tt))
    tp_v, tm_v = (t_.cpu()[:B * nt, :E].view(B, nt, E) for t_ in (tp, tm))
    errs = {}
    if np_:
        errs.update(query_pos_tail=rel_max_zero_ok(qt_v, pos[:, :np_]), tgt_tail=rel_max_zero_ok(tt_v, mo[:, :np_]))
    if nt:
        errs.update(temp_pos=rel_max_zero_ok(tp_v, pos[:, np_:]), temp_memory=rel_max_zero_ok(tm_v, mo[:, np_:]))
    print(f"[query combine kernel B={B} n={n} np={np_} ego={ego}] rel max err vs f64 { {k: f'{e:.2e}' for k, e in errs.items()} }")
    assert max(errs.values()) < 1e-4, errs
    # the zero row: the last memory row of the last sample
    got_zero = tt_v[B - 1, np_ - 1] if np_ == n else tm_v[B - 1, nt - 1]
    assert torch.equal(got_zero, gb_mem[M - 1, E:2 * E] if ego else torch.zeros(E)), "LN0 of a zero row must be exactly zero"
    # sentinels: what lies between and behind the rows written
    for t_, v in ((qt.cpu(), qt_v), (tt.cpu(), tt_v)):
        mask = torch.ones_like(t_, dtype=torch.bool)
        torch.as_strided(mask, (B, np_, E), (tail_s, ld["tail"], 1)).fill_(False)
        assert bool((t_[mask] == SENT).all()) and (np_ == 0 or bool((v != SENT).any()))
    for t_ in (tp.cpu(), tm.cpu()):
        assert bool((t_[B * nt:] == SENT).all()) and bool((t_[:, E:] == SENT).all())


# ---- 3. / 4. the module against the reference's fixtures ---------------------------------------------------------------------------------------------
def _check(tag, got, want, step=1):
    errs = {k: rel_max_zero_ok(got[k].cpu()[:, ::step], want[k]) for k in OUTPUTS}
    print(f"[head queries {tag}] rel max err { {k: f'{e:.2e}' for k, e in errs.items()} }")
    assert all(got[k].dtype == torch.float32 and got[k].is_contiguous() for k in OUTPUTS)
    assert max(errs[k] for k in GEMM_OUTPUTS) < 1e-3, errs
    assert max(errs[k] for k in EXACT_OUTPUTS) < 1e-4, errs


def test_tiny_fp32x3_matches_reference_golden(golden_dir):
    """Every case and frame, each run three times (eager, recorded, replayed): < 1e-3 per output (reference_points and rec_ego_pose, which involve no GEMM, to the
    row kernels' 1e-4); the replay is bit-equal to the eager run; strided views of a capacity buffer give the bits of their contiguous copies."""
    mods = {}
    for tag, sizes, ego, bank, want in tiny_cases(golden_dir):
        key = (ego, sizes["num_propagated"])
        m = mods[key] = mods.get(key) or build(sizes, with_ego_pos=ego)
        dbank = {k: v.to(DEV) for k, v in bank.items()}
        runs = [run(m, dbank) for _ in range(3)]
        assert all(got[k].shape == want[k].shape for got in runs for k in OUTPUTS), tag
        _check(f"tiny fp32x3 {tag}", runs[2], want)
        assert all(torch.equal(runs[0][k], runs[j][k]) for j in (1, 2) for k in OUTPUTS), f"{tag}: eager, recorded and replayed runs differ"
        plans = [s["cplan"] for s in m._states.values() if s.get("cplan") is not None]
        assert plans and plans[-1].num_launches == (10 if ego else 6), [p.num_launches for p in plans]
        views = capacity_views(bank, 9)
        assert views["memory_embedding"].stride(0) == 36 * 256 and not views["memory_embedding"].is_contiguous()
        strided = [run(m, views) for _ in range(3)][2]
        assert all(torch.equal(strided[k], runs[0][k]) for k in OUTPUTS), f"{tag}: strided views differ from their contiguous copies"
        assert all(torch.equal(views[k], dbank[k]) for k in BANK), "the inputs are not modified"
    assert all(m.fresh_builds == 1 for m in mods.values())


def test_full_size_fp32x3_matches_reference_golden(golden_dir):
    """Shipped sizes (B 1, 644 + 256 queries, 1024 entries): < 1e-3 per output on the kept rows of both frames."""
    step, cases = full_cases(golden_dir)
    m = build(synth.HEAD_QUERIES_FULL)
    for f, bank, want in cases:
        for _ in range(3):
            got = run(m, bank)
        assert got["tgt"].shape == got["query_pos"].shape == (1, 900, 256) and got["temp_pos"].shape == (1, 768, 256) and got["rec_ego_pose"].shape == (1, 900, 4, 4)
        _check(f"full fp32x3 frame {f}", got, want, step)


@pytest.mark.parametrize("precision", ["fp32"])
def test_tiny_exact_f32_matches_reference_golden(golden_dir, precision):
    tag, sizes, ego, bank, want = tiny_cases(golden_dir)[3]
    m = build(sizes, precision=precision)
    for _ in range(3):
        got = run(m, bank)
    _check(f"tiny {precision} {tag}", got, want)


# ---- 5. bf16 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ["tiny", "full"])
def test_bf16_within_control(golden_dir, size):
    """bf16: relative L2 per output against the reference's f32 at most 1.2 x that of the torch-bf16 control (the restatement with the linear operands rounded to
    bf16 and f32 accumulation, on the same card) -- the convention of tests/test_gpu_decoder.py."""
    if size == "tiny":
        tag, sizes, ego, bank, want = tiny_cases(golden_dir)[3]
        step = 1
    else:
        step, cases = full_cases(golden_dir)
        (_, bank, want), sizes = cases[1], synth.HEAD_QUERIES_FULL
    m = build(sizes, precision="bf16")
    for _ in range(3):
        got = run(m, bank)
    with torch.no_grad():
        ctl = restated_queries(synth.head_queries_state_dict(sizes), {k: v.to(DEV) for k, v in bank.items()}, sizes, contract=torch.bfloat16)
    res = {k: (rel_l2(got[k].cpu()[:, ::step], want[k]), rel_l2(ctl[k].cpu()[:, ::step], want[k])) for k in GEMM_OUTPUTS}
    print(f"[head queries {size} bf16] rel l2 vs the reference, hip / torch-bf16 control: { {k: f'{a:.3e} / {c:.3e}' for k, (a, c) in res.items()} }")
    assert all(torch.isfinite(got[k]).all() for k in OUTPUTS)
    for k, (a, c) in res.items():
        assert a <= 1.2 * c, (k, a, c)
    for k in EXACT_OUTPUTS:
        assert rel_max_zero_ok(got[k].cpu()[:, ::step], want[k]) < 1e-4, k


# ---- 6. derived state --------------------------------------------------------------------------------------------------------------------------------
def test_fresh_query_rows_are_derived_state(golden_dir):
    """The learned queries' rows of query_pos / tgt / reference_points are computed once per set of weights: a second forward does not recompute them, new weights
    do, and the result equals a newly built module's bit for bit."""
    tag, sizes, ego, bank, want = tiny_cases(golden_dir)[1]
    nq = sizes["num_query"]
    m = build(sizes, seed=0)
    a = run(m, bank)
    assert m.fresh_builds == 1
    a2 = run(m, bank)
    a3 = run(m, tiny_cases(golden_dir)[3][3])                   # another frame, same weights
    assert m.fresh_builds == 1, "a forward with the same weights recomputed the learned queries' half"
    assert all(torch.equal(a[k], a2[k]) for k in OUTPUTS) and all(torch.equal(a[k][:, :nq], a3[k][:, :nq]) for k in ("tgt", "query_pos", "reference_points"))
    m.load_state_dict(synth.head_queries_state_dict(sizes, seed=1), strict=True)
    assert m._fresh is None and m._packed is None and m._ws == {} and m._states == {}
    b = run(m, bank)
    assert m.fresh_builds == 2
    fresh = build(sizes, seed=1)
    c = run(fresh, bank)
    moved = {k: float((a[k][:, :nq] - b[k][:, :nq]).abs().max()) for k in ("tgt", "query_pos", "reference_points")}
    print(f"[head queries derived state] fresh-query rows moved by { {k: f'{v:.2e}' for k, v in moved.items()} } after load_state_dict; fresh_builds {m.fresh_builds}")
    assert min(moved.values()) > 1e-3
    assert all(torch.equal(b[k], c[k]) for k in OUTPUTS), "after load_state_dict the module differs from a newly built one"
    m.to(DEV)                                                   # a move drops them too
    assert m._fresh is None
    run(m, bank)
    assert m.fresh_builds == 3


# ---- 7. hand-over ------------------------------------------------------------------------------------------------------------------------------------
def test_outputs_feed_decoder_and_head_outputs_without_conversion(golden_dir):
    """The six outputs go to a one-layer PETRTemporalTransformer (E 256) and on to HeadOutputs as they are: finite results of the right shapes, bit-equal to feeding
    clones (nothing downstream depends on the outputs sharing one buffer).  No parity claim: that belongs to the assembled head."""
    tag, sizes, ego, bank, want = tiny_cases(golden_dir)[3]
    B, Q, Nk = 2, sizes["num_query"] + sizes["num_propagated"], 40
    dec_sizes = dict(embed_dims=256, num_heads=8, feedforward_channels=512, num_layers=1)
    out_sizes = dict(num_classes=10, embed_dims=256, num_reg_fcs=2, code_size=10, num_pred=1)
    dec = build_decoder(dec_sizes)
    head = toc3d_amd.HeadOutputs(pc_range=synth.PC_RANGE, **out_sizes)
    head.load_state_dict(synth.head_outputs_state_dict(out_sizes), strict=True)
    head = head.to(DEV).eval()
    g = torch.Generator().manual_seed(5)
    memory, pos_embed = (torch.randn(B, Nk, 256, generator=g).to(DEV) for _ in range(2))
    o = run(build(sizes), bank)

    def downstream(o):
        outs_dec, _, _ = dec(memory, o["tgt"], o["query_pos"], pos_embed, None, o["temp_memory"], o["temp_pos"])
        return (outs_dec, *head(outs_dec, o["reference_points"])[1:])
    first = downstream(o)
    second = downstream({k: v.clone() for k, v in o.items()})
    assert first[0].shape == (1, B, Q, 256) and first[1].shape == first[2].shape == (1, B, Q, 10) and o["rec_ego_pose"].shape == (B, Q, 4, 4)
    assert all(torch.isfinite(t).all() for t in first)
    assert all(torch.equal(x, y) for x, y in zip(first, second))
    print(f"[head queries hand-over] outs_dec {tuple(first[0].shape)}, cls {tuple(first[1].shape)}, bbox {tuple(first[2].shape)}: finite, bit-equal to feeding clones")


def test_forward_from_a_temporal_memory_over_two_frames():
    """memory -> queries -> memory on the package's own bank: ``forward_from`` reads a TemporalMemory's strided views in place (bit-equal to ``forward`` on contiguous
    copies, < 1e-3 of the restatement on the same bank) and its ``rec_ego_pose`` is what ``post_update_memory`` takes."""
    sizes, shape = synth.HEAD_QUERIES_TINY, synth.HEAD_QUERIES_TINY_SHAPE
    B, nq, np_ = shape["B"], sizes["num_query"], sizes["num_propagated"]
    inp = synth.memory_inputs(dict(num_propagated=np_, embed_dims=256), B, nq, shape["num_classes"], 2)
    bank = toc3d_amd.TemporalMemory(memory_len=sizes["memory_len"], topk_proposals=shape["topk_proposals"], num_propagated=np_, embed_dims=256,
                                    pc_range=synth.PC_RANGE, pseudo_reference_points=inp["pseudo"], device=DEV)
    m, sd = build(sizes), synth.head_queries_state_dict(sizes)
    for f, fr in enumerate(inp["frames"]):
        data = {k: v.to(DEV) for k, v in fr["data"].items()}
        bank.pre_update_memory(data)
        assert bank.memory_embedding.stride(0) == (sizes["memory_len"] + shape["topk_proposals"]) * 256
        got = dict(zip(OUTPUTS, m.forward_from(bank)))
        held = {k: getattr(bank, k) for k in BANK}
        assert bool(held["memory_embedding"].any()) == (f == 1), "frame 0 runs on the empty bank, frame 1 on a populated one"
        same = run(m, {k: v.contiguous() for k, v in held.items()})
        assert all(torch.equal(got[k], same[k]) for k in OUTPUTS), f"frame {f}: the bank's views differ from their contiguous copies"
        want = restated_queries(sd, {k: v.cpu() for k, v in held.items()}, sizes)
        errs = {k: rel_max_zero_ok(got[k].cpu(), want[k]) for k in OUTPUTS}
        print(f"[head queries on a TemporalMemory, frame {f}] rel max err vs the restatement { {k: f'{e:.2e}' for k, e in errs.items()} }")
        assert max(errs.values()) < 1e-3, errs
        bank.post_update_memory(data, got["rec_ego_pose"], fr["cls"][None].to(DEV), fr["bbox"][None].to(DEV), fr["dec"][None].to(DEV))
