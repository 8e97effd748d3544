"""GPU: the LayerNorm-consuming GEMM epilogues (toc3d_linear_fused EPI_SWIGLU_STATS_LN = w1|w2 behind the folded norm2, EPI_RESIDUAL_LN = w3 behind the folded ffn_ln,
and EPI_RESIDUAL_LN under split-K through toc3d_linear_fused_ws), every written element against its own f64 bound, over the CONDITIONING of the rows and the number of
statistics slots the consumer combines.  Cases, reference, bound and its derivation: tests/lnfold_cases.py (proved sound on the CPU by test_cpu_lnfold_cases.py).

One test per (form, stage, slot count, tile variant).  The rows of one launch interleave 23 families (centred; |mean| / sigma up to 1000 in both signs; outlier channels in
slot 0 and in the last, partly valid slot; sigma down to 1e-4 around a mean of 1; exactly constant rows; a row that is non-zero in the padding columns [ln_n, K) only).
The producers run in front with the default tile, as in test_gpu_epilogue_tails.py, and are what puts the designed rows in place: EPI_RESIDUAL_STATS with a zero A (output =
residual = the designed row, asserted bit for bit) in front of w1|w2, EPI_SWIGLU_STATS with w1 = 0 (lnfold_cases.producer_operands) in front of w3; the reference takes
the values they WROTE, read back, and the statistics are the ones they left.

Named cases of ln_rows_prepare_fn's paths:  the prefetch beyond the first `part + 4 j` slots -- w12 slots 5, 6, 16 (16 = the last prefetched slot, PRE = 4) and w3 slots
5, 43, 48 (48 = the last, PRE = 12);  the remainder loop `sl >= 4 * PRE` -- w12 slots 17, 20 and w3 slots 49, 52;  parts without a slot -- slots 1 and 3.  Each on the
plain path (variant 19 in bf16, 16 in the bf16 x 3 forms), the early one (variant 16 in bf16: PREP_EARLY; the bf16 x 3 forms have none) and the phased kernel (variant 63;
a bf16 x 3 form whose A is plain f32 is refused there, asserted).  The slot count reaches the consumer through stats_in_cap's upper half in front of w1|w2 and through the
header word in front of w3.

Every test asserts: each written element within its bound (hidden units; f32 output; representative rows); nothing else written (canaries with spare rows and columns,
padding hidden units exactly 0); header word 0 of the statistics the consumer writes = its slot count, and those statistics within TOL_STATS (slot by slot, of sum |h| and sum h^2)
of f64 sums of the written hidden units, on the ill-conditioned rows too; the bits of every output equal to the default tile's (rows do not depend on the tile); constant
rows finite.  The module ends with the worst ratio per (form, stage, output, family) and the ENVELOPE table: the largest |mean| / sigma family at which every element still
meets the bar the suite holds that output class to (TOL_F32 / TOL_BF16 of the row's own largest |ref|), per form and output -- profiles/lnfold_conditioning.txt keeps a run."""
import functools

import pytest
import torch

import epilogue_cases as E
import lnfold_cases as L
from support import CAN32, DEV, S, a_planes, bits, canary, check_untouched, is_canary, o_planes, planes_f64, to_planes, w_planes, worst_report
from toc3d_amd import lib

pytestmark = pytest.mark.gpu
M, EPS = L.M, L.EPS
note, _report = worst_report("lnfold", 44)
ENV = {}                                                   # (form, stage output, family) -> worst |err| / (bar * the row's largest |ref|)


@pytest.fixture(scope="module", autouse=True)
def _envelope_table():
    yield
    print("\n[lnfold envelope] worst |err| / (bar * row max |ref|) per nominal |mean| / sigma (both signs); bar = TOL_F32 2e-5, hidden units of the bf16 form TOL_BF16 6e-3")
    print("[lnfold envelope] " + f"{'form / output':<22s}" + "".join(f"{r:>10d}" for r in (0,) + L.RATIOS) + "   envelope")
    for fo in sorted({k[:2] for k in ENV}):
        by_ratio = {}
        for (form, key, fam), v in ENV.items():
            r = L.FAMILIES[fam][4]
            if (form, key) == fo and r is not None:
                by_ratio[r] = max(by_ratio.get(r, 0.0), v)
        env = L.envelope({r: v <= 1.0 for r, v in by_ratio.items()})
        print("[lnfold envelope] " + f"{fo[0] + ' ' + fo[1]:<22s}" + "".join(f"{by_ratio.get(r, float('nan')):>10.3g}" for r in (0,) + L.RATIOS) + f"   {env}")
    others = sorted({k[2] for k in ENV if L.FAMILIES[k[2]][4] is None})
    for fam in others:
        print(f"[lnfold envelope] {fam:<16s} " + "  ".join(f"{f} {k} {v:.3g}" for (f, k, ff), v in sorted(ENV.items()) if ff == fam))


def dtv(name):
    return getattr(lib, name)


def values(t, planes):
    return (planes_f64(t) if planes else t.double()).cpu()


def poke(buf, rows, c0, c1, planes, val=L.PAD_VALUE):
    """Columns [c0, c1) of the given rows := val, in the buffer's own layout (planes: hi = bf16(val) at group c / 32, element c % 32; lo = 0 at + 32)."""
    if c1 <= c0:
        return
    rows = torch.tensor(rows, device=DEV)[:, None]
    cols = torch.arange(c0, c1, device=DEV)
    if planes:
        v = buf.view(torch.int16)
        at = (cols // 32) * 64 + cols % 32
        v[rows, at] = int(torch.tensor(val, dtype=torch.bfloat16).view(torch.int16))
        v[rows, at + 32] = 0
    else:
        buf[rows, cols] = val


def stats_buf(cap):
    return canary(1, 4 + (M + 8) * cap * 2, torch.float32).view(-1)


def check_stats_region(tag, st, slots, cap):
    hdr = st[:4].view(torch.int32)
    assert int(hdr[0]) == slots, f"{tag}: header says {int(hdr[0])} slots, {slots} documented"
    assert bool((hdr[1:] == CAN32).all()), f"{tag}: header words 1-3 written"
    body = st[4:].view(M + 8, cap, 2)
    assert bool(is_canary(body[M:]).all()) and bool(is_canary(body[:M, slots:]).all()), f"{tag}: statistics written outside [0, M) x [0, slots)"


REP = len(range(3, M, 7))


@functools.lru_cache(maxsize=None)
def rep_index():
    idx = torch.full((M,), -1, dtype=torch.int32)
    idx[3::7] = torch.arange(REP, dtype=torch.int32)
    return idx.to(DEV)


class Case:
    """Operands of one (form, stage, slot count) on the device, the producer's outputs read back, the f64 reference and bounds, and the default tile's outputs."""
    def __init__(self, form, stage, slots):
        self.form, self.stage, self.slots = form, stage, slots
        self.sh = sh = L.shape_of(stage, slots)
        bf = form == "bf16"
        self.pdt, self.tdt = (lib.BF16, torch.bfloat16) if bf else (lib.F32, torch.float32)
        self.dt = dtv(L.dt_name(form, stage))
        sw = {k: v.to(DEV).contiguous() for k, v in L.stage_weights(stage, slots).items()}
        n, K = sh["ln_n"], sh["K"]
        dv = lambda t: t.to(DEV).contiguous()
        if stage == "w12":
            dtp = dtv(L.FORMS[form][0])
            x = L.designed_rows(n, seed=slots)
            self.x = dv(x)
            a0, w0 = torch.zeros(M, 64, dtype=self.tdt, device=DEV), torch.zeros(E.ru(n, 128), 64, dtype=self.tdt, device=DEV)
            out = canary(M + 8, E.ru(n, 32) + 32, torch.float32)
            self.act, self.cap_in = canary(M + 8, K + 32, self.tdt), slots + 1
            self.stats_in = stats_buf(self.cap_in)
            lib.call("toc3d_linear_fused", dtp, lib.EPI_RESIDUAL_STATS, 16, a0, 64, w0, 64, None, out, out.shape[1], self.x, n, 0, None, None, M, n, 64, 0,
                     self.stats_in, self.cap_in, None, 0, None, 0, EPS, self.act, self.act.shape[1], None, S())
            assert torch.equal(bits(out[:M, :n]), bits(self.x)), "the producer must pass the designed rows through (residual + 0)"
            self.planes_in = o_planes(dtp)
            Hd, Hp, Hpk = sh["Hd"], sh["Hp"], E.ru(sh["Hp"], 64)
            self.W = torch.zeros(E.ru(2 * Hpk, 128), K, dtype=self.tdt, device=DEV)
            self.c1, self.c2 = torch.zeros(2 * Hpk, device=DEV), torch.zeros(2 * Hpk, device=DEV)
            lib.call("toc3d_pack_swiglu_lnfold", self.pdt, sw["w1"], sw["w2"], sw["b1"], sw["b2"], sw["gamma"], sw["beta"], Hd, n, self.W, self.c1, self.c2, Hpk, K, S())
            self.res, nrows = None, 2 * Hp
            self.cap_word = self.cap_in | slots << 32         # the host tells the consumer the slot count
        else:
            dtp = dtv(L.FORMS[form][1])
            Hd, Hp, Hpk = sh["Hd"], sh["Hp"], E.ru(sh["Hp"], 64)
            A, w1, w2, b1, b2 = L.producer_operands(Hd, seed=slots)
            Wp, bp = torch.zeros(E.ru(2 * Hpk, 128), 64, dtype=self.tdt, device=DEV), torch.zeros(2 * Hpk, device=DEV)
            lib.call("toc3d_pack_swiglu", self.pdt, dv(w1), dv(w2), dv(b1), dv(b2), Hd, 64, Wp, bp, Hpk, 64, S())
            a_in = dv(A).to(self.tdt)
            a_in, w_in = (to_planes(a_in) if a_planes(dtp) else a_in), (to_planes(Wp) if w_planes(dtp) else Wp)
            self.act, self.cap_in = canary(M + 8, K + 32, self.tdt), slots + 1
            self.stats_in = stats_buf(self.cap_in)
            lib.call("toc3d_linear_fused", dtp, lib.EPI_SWIGLU_STATS, 16, a_in, 64, w_in, 64, bp, self.act, self.act.shape[1], None, 0, 0, None, None, M, 2 * Hp, 64, Hd,
                     self.stats_in, self.cap_in, None, 0, None, 0, EPS, None, 0, None, S())
            self.planes_in = o_planes(dtp)
            N = sh["N"]
            self.W = torch.zeros(E.ru(N, 128), K, dtype=self.tdt, device=DEV)
            self.c1, self.c2 = torch.zeros(E.ru(N, 128), device=DEV), torch.zeros(E.ru(N, 128), device=DEV)
            lib.call("toc3d_pack_weight_lnfold", self.pdt, sw["w"], sw["gamma"], sw["beta"], sw["b"], N, Hd, self.W, self.W.shape[0], K, self.c1, self.c2, S())
            self.res, nrows = sw["res"], N
            self.cap_word = self.cap_in                       # the consumer reads the header word
        check_stats_region(f"{form} {stage} {slots} producer", self.stats_in, slots, self.cap_in)
        assert a_planes(self.dt) == self.planes_in
        poke(self.act, L.pad_rows(), n, K, self.planes_in)
        self.W_in = to_planes(self.W) if w_planes(self.dt) else self.W
        a = values(self.act[:M], self.planes_in)[:, :K].contiguous()
        # the rows are the designed families: constant rows constant, the padding-only row zero on [0, ln_n) and PAD_VALUE behind it
        for f in ("const0", "const3", "padonly"):
            blk = a[L.family_rows(f), :n]
            assert bool((blk == blk[:, :1]).all()) and (f == "const3" or not blk.any()), f
        assert bool((a[L.pad_rows(), n:] == L.PAD_VALUE).all())
        self.c = dict(form=form, stage=stage, slots=slots, a=a, a_planes=self.planes_in, w=self.W[:nrows].double().cpu(), c1=self.c1[:nrows].cpu(), c2=self.c2[:nrows].cpu(),
                      res=None if self.res is None else self.res.cpu(), split=1, **sh)
        self._an, self._base = {}, None

    def an(self, split=1):
        if split not in self._an:
            self._an[split] = L.analyse(dict(self.c, split=split))
        return self._an[split]

    def run(self, v):
        sh, K = self.sh, self.sh["K"]
        if self.stage == "w12":
            Hd, Hp = sh["Hd"], sh["Hp"]
            o = dict(hid=canary(M + 8, E.ru(Hp, 64) + 32, self.tdt), cap=3)
            o["stats"] = stats_buf(3)
            lib.call("toc3d_linear_fused", self.dt, lib.EPI_SWIGLU_STATS_LN, v, self.act, self.act.shape[1], self.W_in, K, self.c2, o["hid"], o["hid"].shape[1], None, 0, 0, None, None,
                     M, 2 * Hp, K, Hd, o["stats"], 3, self.stats_in, self.cap_word, self.c1, sh["ln_n"], EPS, None, 0, None, S())
            return o
        N = sh["N"]
        o = dict(out=canary(M + 8, E.ru(N, 32) + 32, torch.float32), rep=canary(REP + 2, N, torch.float32))
        args = (self.dt, lib.EPI_RESIDUAL_LN, v, self.act, self.act.shape[1], self.W_in, K, self.c2, o["out"], o["out"].shape[1], self.res, N, 0, o["rep"], rep_index(), M, N, K, 0,
                None, 0, self.stats_in, self.cap_word, self.c1, sh["ln_n"], EPS, None, 0, None)
        if v >= 1000:
            need = lib.load().toc3d_linear_splitk_workspace_bytes(v, M, N)
            ws = torch.zeros((max(need, 4) + 3) // 4, dtype=torch.int32, device=DEV)
            lib.call("toc3d_linear_fused_ws", *args, ws, ws.numel() * 4, S())
            assert not ws[:16384].any(), "the arrival tickets (the first TOC3D_SPLITK_TICKET_BYTES) re-arm themselves"
        else:
            lib.call("toc3d_linear_fused", *args, S())
        return o

    def base(self):
        if self._base is None:
            self._base = self.run(16)
        return self._base


@functools.lru_cache(maxsize=2)
def case_of(form, stage, slots):
    return Case(form, stage, slots)


def check_case(cs, o, tag, split=1):
    form, stage, sh = cs.form, cs.stage, cs.sh
    an = cs.an(split)
    if stage == "w12":
        Hd, Hp = sh["Hd"], sh["Hp"]
        pl = o_planes(cs.dt)
        got = {"hid": values(o["hid"][:M], pl)[:, :Hp]}
        check_untouched(tag + " hidden units", o["hid"], M, Hp, pl, zero_ok=True)
        check_stats_region(tag + " statistics", o["stats"], Hp // 64, o["cap"])
        # the statistics the consumer writes, against f64 sums of the hidden units it wrote.  Per SLOT, and of the scale a summation error has: sum |h| for the sum,
        # sum h^2 for the squares (the tree errs by <= 7 u / 8 u of them; where the units leave as planes the kernel sums the f32 values it then splits, 2^-18 more:
        # 4.2e-6 in all, inside TOL_STATS = 1e-5).  Of the slot's own |sum| the bar would ask for digits that a cancelling sum of 64 values never had.
        want = E.slot_sums(got["hid"], Hp, 64)
        scale = E.slot_sums(got["hid"].abs(), Hp, 64)
        scale[..., 1] = want[..., 1]
        have = o["stats"][4:].view(M + 8, o["cap"], 2)[:M, :Hp // 64].double().cpu()
        err = (have - want).abs()
        assert bool((err <= E.TOL_STATS * scale).all()), f"{tag}: statistics of the hidden units off by up to {float((err / scale.clamp_min(1e-300)).max()):.3e} of the slot's sum |h| / sum h^2"
    else:
        N = sh["N"]
        got = {"out": o["out"][:M, :N].double().cpu(), "raw": o["rep"][:REP].double().cpu()}
        check_untouched(tag + " out", o["out"], M, N, False)
        assert bool(is_canary(o["rep"][REP:]).all()), f"{tag}: representative rows nobody references were written"
    for key, g in got.items():
        sub = dict(an)
        rows = list(range(M))
        if key == "raw":
            rows = list(range(3, M, 7))
            sub = {"raw": an["raw"][3::7], "b_raw": an["b_raw"][3::7]}
        assert bool(torch.isfinite(g).all()), f"{tag}: non-finite {key} on finite rows"
        r = L.ratios(g, sub, key)
        ref = sub[key]
        bar = (g - ref).abs().amax(1) / (L.bar_of(form, key) * ref.abs().amax(1).clamp_min(1e-300))
        for j, i in enumerate(rows):
            fam = L.family_of(i)
            note(f"{form} {stage} {key} {fam}", float(r[j].max()))
            if split == 1:
                k = (form, f"{stage} {key}", fam)
                ENV[k] = max(ENV.get(k, 0.0), float(bar[j]))
        worst = float(r.max())
        if worst > 1.0:
            j, n_ = divmod(int(r.argmax()), r.shape[1])
            assert False, (f"{tag}: {key}[{rows[j]}, {n_}] ({L.family_of(rows[j])}, cond {float(an['cond'][rows[j]]):.3g}) is {worst:.3f} of its bound: got {float(g[j, n_])!r}, "
                           f"ref {float(ref[j, n_])!r}, bound {float(sub['b_' + key][j, n_]):.3e}; {int((r > 1).sum())} elements outside")
    return got


PARAMS = [(form, stage, slots, v) for form in L.FORMS for stage in L.STAGES for slots in L.widths(stage) for v in L.VSET + ((L.SPLIT_VARIANT,) if stage == "w3" else ())]


@pytest.mark.parametrize("form,stage,slots,variant", PARAMS, ids=[f"{f}-{s}-slots{n}-{L.slot_class(s, n)}-v{v}" for f, s, n, v in PARAMS])
def test_folded_layernorm_over_conditioning_and_slot_counts(form, stage, slots, variant):
    cs = case_of(form, stage, slots)
    tag = f"{form} {stage} slots {slots} v{variant}"
    if variant == L.SPLIT_VARIANT:
        if cs.sh["K"] < 256:
            with pytest.raises(RuntimeError, match="too short for a split of 2"):
                cs.run(variant)
            return
        check_case(cs, cs.run(variant), tag, split=2)          # another order of the K sum: its own bits, the same bound (+ 2 u per slice)
        return
    if L.path_of(form, stage, variant) == "refused":
        with pytest.raises(RuntimeError, match="cannot serve"):
            cs.run(variant)
        return
    o = cs.run(variant)
    check_case(cs, o, tag)
    base = cs.base()
    for k in ("hid", "stats") if stage == "w12" else ("out", "rep"):
        assert torch.equal(bits(o[k]), bits(base[k])), f"{tag}: {k} differs from the default tile's bits"
