"""GPU: the fused GEMM epilogues (toc3d_linear_fused: EPI_RESIDUAL_STATS, EPI_SWIGLU_STATS, EPI_SWIGLU_STATS_LN, EPI_RESIDUAL_LN; toc3d_linear_qkv_rope; the plain
epilogues on planes) at every row / column TAIL class of the launch table, against f64.

The variant axis of these kernels is covered in test_gpu_ops.py / test_gpu_attn_rot.py (thirty to forty tile variants, bit-identical to each other) -- at ONE shape,
M, C, Hd, Hp = 777, 384, 300, 320.  Here the shape axis: the classes are derived from the launch table in tests/epilogue_cases.py (its docstring states the
derivation; tests/test_cpu_epilogue_reference.py proves that every class has a case for every variant of the set and that the references are sound).

The launches form the block half of the backbone (eva_vit.py:44-51, 262-263): proj (+ residual, act copy, statistics) -> w1|w2 (norm2 folded; hidden units,
statistics) -> w3 (ffn_ln folded, + residual), plus the SwiGLU epilogue without a LayerNorm in front and the plain epilogues.  Every stage reads the outputs the
stage before it wrote with the default tile (variant 16) at M_ALIGNED rows, so a tile that is refused for one stage does not take the later stages with it.

Each (form, column configuration, stage, variant) asserts
  a. accuracy: the launch at M_ALIGNED rows against a plain-torch f64 reference on the operands the kernel reads (rounded A, packed weights read back, c2 as packed;
     for the _LN epilogues an explicit two-pass f64 LayerNorm THEN the matmul -- not the folded formula).  Bounds: the ones the suite already holds these output
     classes to -- f32 outputs 2e-5 of the output's max, bf16-rounded outputs 6e-3, bf16 x 3 forms 2e-5, row statistics 1e-5 against f64 sums of the written values;
  b. prefix bit-identity: a row depends on its A row and W only, so the launch at M' < M_ALIGNED returns the bits of rows [0, M') -- outputs, act copy, planes
     images, representative rows, statistics -- and the launch on the first N' packed weight rows the bits of columns [0, N') (statistics: every whole slot);
  c. nothing else is written: every output starts as a finite canary with spare rows and columns; rows >= M, padding columns and unreferenced representative rows
     keep it (padding of the act copy / hidden units: canary or exactly zero; hidden units [Hd, Hp) exactly zero), header word 0 = the slot count.
Combinations the argument checks refuse are asserted as refusals (RuntimeError and its message), never skipped."""
import functools

import pytest
import torch

import epilogue_cases as E
from attention_cases import compact_tables, rc_of, rope_ref
from epilogue_cases import TOL_BF16, TOL_F32, TOL_STATS
from support import CAN32, DEV, S, a_planes, bits, canary, check_untouched, is_canary, o_planes, pack, planes_f64, relerr, rnd, to_planes, w_planes
from toc3d_amd import lib, synth

pytestmark = pytest.mark.gpu
BF16, X3, X3W, X3P, X3WO, X3WA = lib.BF16, lib.F32X3, lib.F32X3W, lib.F32X3P, lib.F32X3WO, lib.F32X3WA
# dtype of (proj, w1|w2, w3): the mixed forms as a block launches them -- a producer whose own A is not split yet (WO), a consumer whose outputs stay f32 (WA)
FORMS = {"bf16": (BF16, BF16, BF16), "f32x3": (X3, X3, X3), "f32x3w": (X3W, X3W, X3W), "f32x3p": (X3P, X3P, X3P), "f32x3wo": (X3WO, X3P, X3WA),
         "f32x3wa": (X3WA, X3WO, X3WA)}
SWIGLU_EPIS = (lib.EPI_SWIGLU, lib.EPI_SWIGLU_STATS, lib.EPI_SWIGLU_STATS_LN)
EPS = 1e-6
MA = E.M_ALIGNED


def tdt_of(dt):
    return torch.bfloat16 if dt == BF16 else torch.float32


def refusal(dt, epi, v):
    """The message of the refusal toc3d_linear_fused owes this combination, or None (csrc/gemm_kernels.h launch_cfg / launch_phased)."""
    if epi in SWIGLU_EPIS and v % 100 == 52:
        return "cannot serve"                               # 48-column wave slabs are not whole (w1, w2) groups
    if dt != BF16 and E.VARIANTS[v][4] and not a_planes(dt):
        return "cannot serve"                               # the bf16 x 3 forms of the 96- / 160-row and phased tiles take both operands as planes only
    return None


def values(t, planes):
    """The numbers a buffer holds, as f64: plain act / f32 values, or hi + lo of a planes image."""
    return planes_f64(t) if planes else t.double()


def check_stats(tag, st, M, slots, cap):
    """(c) for a statistics buffer: header word 0 = the slot count, the rest of the header, slots >= the count and rows >= M untouched."""
    hdr = st[:4].view(torch.int32)
    assert int(hdr[0]) == slots, f"{tag}: header says {int(hdr[0])} slots, {slots} documented"
    assert bool((hdr[1:] == CAN32).all()), f"{tag}: header words 1-3 written"
    body = st[4:].view(MA + 8, cap, 2)
    assert bool(is_canary(body[M:]).all()) and bool(is_canary(body[:M, slots:]).all()), f"{tag}: statistics written outside [0, M) x [0, slots) (M = {M})"


def stats_body(st, cap):
    return st[4:].view(MA + 8, cap, 2)


def rep_rows(M):
    return len(range(3, M, 7))


@functools.lru_cache(maxsize=None)
def rep_index():
    """Representative rows: every 7th row from row 3 on captures the raw branch output (int32 [MA], -1 elsewhere)."""
    idx = torch.full((MA,), -1, dtype=torch.int32)
    idx[3::7] = torch.arange(rep_rows(MA), dtype=torch.int32)
    return idx.to(DEV)


# ---- the launches: fresh canary outputs with spare rows (MA + 8) and columns every time -------------------------------------------------------------------------
def run_residual(epi, dt, v, M, A, lda, W, ldw, bias, N, K, res, stats_in=None, cap_in=0, c1=None, ln_n=0):
    """EPI_RESIDUAL_STATS (stats_in None) / EPI_RESIDUAL_LN / EPI_RESIDUAL: out f32 [M, ldo], representative rows, and for _STATS the act copy + statistics."""
    tdt = tdt_of(dt)
    o = dict(out=canary(MA + 8, E.ru(N, 32) + 32, torch.float32), rep=canary(rep_rows(MA) + 2, N, torch.float32), N=N, M=M)
    st_out, cap, act, ld_act = None, 0, None, 0
    if epi == lib.EPI_RESIDUAL_STATS:
        o["slots"], o["cap"] = (N + 63) // 64, (N + 63) // 64 + 1
        o["stats"] = canary(1, 4 + (MA + 8) * o["cap"] * 2, torch.float32).view(-1)
        o["act"] = canary(MA + 8, E.ru(N, 64) + 32, tdt)
        st_out, cap, act, ld_act = o["stats"], o["cap"], o["act"], o["act"].shape[1]
    lib.call("toc3d_linear_fused", dt, epi, v, A, lda, W, ldw, bias, o["out"], o["out"].shape[1], res, res.shape[1], 0, o["rep"], rep_index(), M, N, K, 0,
             st_out, cap, stats_in, cap_in, c1, ln_n, EPS, act, ld_act, None, S())
    return o


def run_swiglu(epi, dt, v, M, A, lda, W, ldw, bias, Hd, Hp, K, stats_in=None, cap_in=0, c1=None, ln_n=0):
    """EPI_SWIGLU_STATS / EPI_SWIGLU_STATS_LN: hidden units act [M, ldo] (planes where the form says so) + statistics, one slot per 64 hidden units."""
    slots = (2 * Hp + 127) // 128
    o = dict(hid=canary(MA + 8, E.ru(Hp, 64) + 32, tdt_of(dt)), slots=slots, cap=slots + 1, Hd=Hd, Hp=Hp, M=M)
    o["stats"] = canary(1, 4 + (MA + 8) * o["cap"] * 2, torch.float32).view(-1)
    lib.call("toc3d_linear_fused", dt, epi, v, A, lda, W, ldw, bias, o["hid"], o["hid"].shape[1], None, 0, 0, None, None, M, 2 * Hp, K, Hd,
             o["stats"], o["cap"], stats_in, cap_in, c1, ln_n, EPS, None, 0, None, S())
    return o


def check_c_residual(tag, o, dt):
    M, N = o["M"], o["N"]
    check_untouched(tag + " out", o["out"], M, N, False)
    n = rep_rows(M)
    assert bool(is_canary(o["rep"][n:]).all()), f"{tag}: representative rows nobody references were written (M = {M})"
    if "act" in o:
        check_untouched(tag + " act copy", o["act"], M, N, o_planes(dt), zero_ok=True)
        check_stats(tag + " statistics", o["stats"], M, o["slots"], o["cap"])


def check_c_swiglu(tag, o, dt):
    M, Hd, Hp = o["M"], o["Hd"], o["Hp"]
    check_untouched(tag + " hidden units", o["hid"], M, Hp, o_planes(dt), zero_ok=True)
    if Hd < Hp:
        assert torch.count_nonzero(values(o["hid"][:M], o_planes(dt))[:, Hd:Hp]) == 0, f"{tag}: hidden units [Hd, Hp) must be written as zeros (M = {M})"
    check_stats(tag + " statistics", o["stats"], M, o["slots"], o["cap"])


def check_b_rows(tag, o, full, keys):
    """(b) the launch at M rows returned the bits of rows [0, M) of the launch at M_ALIGNED (whole rows: padding columns included)."""
    M = o["M"]
    for k in keys:
        if k == "stats":
            a, b = stats_body(o["stats"], o["cap"])[:M], stats_body(full["stats"], full["cap"])[:M]
        elif k == "rep":
            a, b = o["rep"][:rep_rows(M)], full["rep"][:rep_rows(M)]
        else:
            a, b = o[k][:M], full[k][:M]
        assert torch.equal(bits(a), bits(b)), f"{tag}: {k} at M = {M} is not the bits of rows [0, M) of the launch at M = {MA}"


def stats_errors(st, cap, vals, width, slot, M):
    """Relative error of the written slots against f64 sums of the written values (sum and sum of squares)."""
    want = E.slot_sums(vals[:M], width, slot)
    got = stats_body(st, cap)[:M, :want.shape[1]]
    return max(relerr(got[..., 0], want[..., 0]), relerr(got[..., 1], want[..., 1]))


# ---- operands and f64 references of one (form, column configuration) ----------------------------------------------------------------------------------------
class Chain:
    def __init__(self, form, col):
        self.form, self.col, self.dts = form, col, FORMS[form]
        cfg = E.COLS[col]
        self.C, self.K1, self.Hd, self.Hp = C, K1, Hd, Hp = cfg["C"], cfg["K1"], cfg["Hd"], cfg["Hp"]
        self.Hpk = Hpk = E.ru(Hp, 64)                      # toc3d_pack_swiglu* packs whole 64-unit groups: the launches at Hp take the first 2 * Hp packed rows
        self.K12, self.K3 = K12, K3 = E.ru(C, 64), E.ru(Hp, 64)
        CF = E.C_FULL
        bf = form == "bf16"
        self.pdt, self.tdt = (BF16, torch.bfloat16) if bf else (lib.F32, torch.float32)
        pdt, tdt = self.pdt, self.tdt
        dv = lambda t: t.to(DEV).contiguous()
        # proj: A = attention output [MA, K1], W [C_FULL, K1] (the launches take the first C rows), residual stream x0 with a mean
        att = rnd(MA, K1, seed=1)
        self.att = dv(att).to(tdt)
        self.Wp = pack(rnd(CF, K1, seed=2, scale=K1 ** -0.5), pdt, tdt)
        self.bp = dv(rnd(CF, seed=3))
        self.x0 = dv(3.0 * rnd(MA, CF, seed=4) + 0.7)
        # w1|w2 with norm2 folded in; and the same layers without a LayerNorm in front (toc3d_pack_swiglu) on the attention output
        g2, b2 = dv(1.0 + 0.3 * rnd(C, seed=5)), dv(0.2 * rnd(C, seed=6))
        w1, w2, bb1, bb2 = dv(rnd(Hd, C, seed=7, scale=C ** -0.5)), dv(rnd(Hd, C, seed=8, scale=C ** -0.5)), dv(rnd(Hd, seed=9)), dv(rnd(Hd, seed=10))
        rows12 = E.ru(2 * Hpk, 128)
        self.W12 = torch.zeros(rows12, K12, dtype=tdt, device=DEV)
        self.c1_12, self.c2_12 = torch.zeros(2 * Hpk, device=DEV), torch.zeros(2 * Hpk, device=DEV)
        lib.call("toc3d_pack_swiglu_lnfold", pdt, w1, w2, bb1, bb2, g2, b2, Hd, C, self.W12, self.c1_12, self.c2_12, Hpk, K12, S())
        v1, v2 = dv(rnd(Hd, K1, seed=15, scale=K1 ** -0.5)), dv(rnd(Hd, K1, seed=16, scale=K1 ** -0.5))
        self.W12p = torch.zeros(rows12, K1, dtype=tdt, device=DEV)
        self.b12p = torch.zeros(2 * Hpk, device=DEV)
        lib.call("toc3d_pack_swiglu", pdt, v1, v2, bb1, bb2, Hd, K1, self.W12p, self.b12p, Hpk, K1, S())
        # w3 with ffn_ln folded in: [C_FULL, K3]
        gf, bfb = dv(1.0 + 0.3 * rnd(Hd, seed=11)), dv(0.2 * rnd(Hd, seed=12))
        W3, b3 = dv(rnd(CF, Hd, seed=13, scale=Hd ** -0.5)), dv(rnd(CF, seed=14))
        self.W3 = torch.zeros(CF, K3, dtype=tdt, device=DEV)
        self.c1_3, self.c2_3 = torch.zeros(CF, device=DEV), torch.zeros(CF, device=DEV)
        lib.call("toc3d_pack_weight_lnfold", pdt, W3, gf, bfb, b3, CF, Hd, self.W3, CF, K3, self.c1_3, self.c2_3, S())
        # the pack entry points: c1 = row sums of the ROUNDED weights, the weights zero outside [0, valid K)
        assert relerr(self.c1_3, self.W3.double().sum(1)) < 1e-5 and relerr(self.c1_12, self.W12[:2 * Hpk].double().sum(1)) < 1e-5
        assert torch.count_nonzero(self.W3[:, Hd:]) == 0 and torch.count_nonzero(self.W12[:, C:]) == 0
        self._base = {}

    # operands in the layout a dtype form reads them
    def w(self, t, dt):
        return to_planes(t) if w_planes(dt) else t

    def a_first(self, dt):
        return to_planes(self.att) if a_planes(dt) else self.att

    # -- stage launches (v = tile variant, M rows, N / Hp columns) --
    def proj(self, v, M, N=None):
        dt = self.dts[0]
        return run_residual(lib.EPI_RESIDUAL_STATS, dt, v, M, self.a_first(dt), self.K1, self.w(self.Wp, dt), self.K1, self.bp, N or self.C, self.K1, self.x0)

    def swiglu_plain(self, v, M, Hp=None, Hd=None):
        dt = self.dts[0]                                    # reads the attention output like proj
        return run_swiglu(lib.EPI_SWIGLU_STATS, dt, v, M, self.a_first(dt), self.K1, self.w(self.W12p, dt), self.K1, self.b12p, Hd or self.Hd, Hp or self.Hp, self.K1)

    def w12(self, v, M, Hp=None, Hd=None):
        dt, p = self.dts[1], self.base("proj")
        assert a_planes(dt) == o_planes(self.dts[0])
        return run_swiglu(lib.EPI_SWIGLU_STATS_LN, dt, v, M, p["act"], p["act"].shape[1], self.w(self.W12, dt), self.K12, self.c2_12, Hd or self.Hd, Hp or self.Hp,
                          self.K12, p["stats"], p["cap"] | p["slots"] << 32, self.c1_12, self.C)

    def w3(self, v, M, N=None):
        dt, h = self.dts[2], self.base("w12")
        assert a_planes(dt) == o_planes(self.dts[1])
        return run_residual(lib.EPI_RESIDUAL_LN, dt, v, M, h["hid"], h["hid"].shape[1], self.w(self.W3, dt), self.K3, self.c2_3, N or self.C, self.K3, self.x0,
                            h["stats"], h["cap"], self.c1_3, self.Hd)

    def base(self, stage):
        """The stage's outputs with the default tile at M_ALIGNED rows: what the next stage reads."""
        if stage not in self._base:
            self._base[stage] = getattr(self, stage)(16, MA)
        return self._base[stage]

    # -- f64 references on the operands the kernels read --
    def ref_proj(self):
        a, w = self.att.double(), self.Wp.double()         # (planes of A / W: the (hi, lo) split of these very values)
        raw = a @ w[:self.C].T + self.bp[:self.C].double()
        return raw, self.x0[:, :self.C].double() + raw

    def ref_swiglu_plain(self):
        z = self.att.double() @ self.W12p[:2 * self.Hp].double().T + self.b12p[:2 * self.Hp].double()
        return E.swiglu_units(z, self.Hd, self.Hp)

    def ln_operands(self, stage):
        if stage == "w12":
            p = self.base("proj")
            return values(p["act"][:MA], o_planes(self.dts[0])), self.W12[:2 * self.Hp], self.c1_12[:2 * self.Hp], self.c2_12[:2 * self.Hp], self.C
        h = self.base("w12")
        return values(h["hid"][:MA], o_planes(self.dts[1])), self.W3[:self.C], self.c1_3[:self.C], self.c2_3[:self.C], self.Hd

    def ref_w12(self, control=False):
        a, w, c1, c2, n = self.ln_operands("w12")
        z = E.folded_ln_matmul(a, w, c1, c2, n, EPS, torch.float32) if control else E.explicit_ln_matmul(a, w, c2, n, EPS)
        return E.swiglu_units(z, self.Hd, self.Hp)

    def ref_w3(self, control=False):
        a, w, c1, c2, n = self.ln_operands("w3")
        raw = E.folded_ln_matmul(a, w, c1, c2, n, EPS, torch.float32) if control else E.explicit_ln_matmul(a, w, c2, n, EPS)
        return raw, self.x0[:, :self.C].double() + raw


def expect_refused(fn, msg, tag):
    with pytest.raises(RuntimeError, match=msg):
        fn()
    return None


def check_a_residual(tag, ch, o, dt, raw_ref, x_ref, ctl=None):
    """(a) for a residual stage at M_ALIGNED rows: f32 output, representative rows, and for _STATS the act copy and its statistics."""
    C = o["N"]
    e_x, e_rep = relerr(o["out"][:MA, :C], x_ref), relerr(o["rep"][:rep_rows(MA)], raw_ref[3::7])
    msg = f"[{tag}] rel err vs f64: output {e_x:.3e}, representative rows {e_rep:.3e}"
    if ctl is not None:
        msg += f" (f32 control of the folded form {relerr(ctl, x_ref):.3e})"
    if "act" in o:
        av = values(o["act"][:MA], o_planes(dt))
        e_act = relerr(av[:, :C], x_ref)
        e_st = stats_errors(o["stats"], o["cap"], av, C, 64, MA)
        msg += f", act copy {e_act:.3e}, statistics {e_st:.3e}"
        assert e_act < (TOL_BF16 if dt == BF16 else TOL_F32), msg
        assert e_st < TOL_STATS, msg
        if dt != BF16:                                     # the f32 copy IS the f32 output (or its planes image)
            want = o["out"][:MA, :C]
            assert torch.equal(av[:, :C], values(to_planes(torch.nn.functional.pad(want, (0, o["act"].shape[1] - C))), True)[:, :C] if o_planes(dt) else want.double()), msg
    print(msg)
    assert e_x < TOL_F32 and e_rep < TOL_F32, msg


def check_a_swiglu(tag, o, dt, h_ref, ctl=None):
    Hd, Hp = o["Hd"], o["Hp"]
    hv = values(o["hid"][:MA], o_planes(dt))
    e_h = relerr(hv[:, :Hd], h_ref[:, :Hd])
    e_st = stats_errors(o["stats"], o["cap"], hv, Hp, 64, MA)
    msg = f"[{tag}] rel err vs f64: hidden units {e_h:.3e}, statistics {e_st:.3e}"
    if ctl is not None:
        msg += f" (f32 control of the folded form {relerr(ctl[:, :Hd], h_ref[:, :Hd]):.3e})"
    print(msg)
    assert e_h < (TOL_BF16 if dt == BF16 else TOL_F32), msg
    assert e_st < TOL_STATS, msg


@functools.lru_cache(maxsize=2)
def chain(form, col):
    return Chain(form, col)


@pytest.mark.parametrize("col", list(E.COLS))
@pytest.mark.parametrize("form", list(FORMS))
def test_residual_epilogues_at_the_tails(form, col):
    """EPI_RESIDUAL_STATS (the attention projection) and EPI_RESIDUAL_LN (w3 behind the folded ffn_ln): f32 output, representative rows, act copy (planes where the
    form writes them), statistics -- (a) / (b) / (c) of the module docstring for every variant of the set, every M of the row list, and in N."""
    ch = chain(form, col)
    C = ch.C
    refs = {"proj": ch.ref_proj(), "w3": ch.ref_w3()}
    ctl3 = ch.ref_w3(control=True)[1]
    for stage, epi, dt, keys in (("proj", lib.EPI_RESIDUAL_STATS, ch.dts[0], ("out", "rep", "act", "stats")), ("w3", lib.EPI_RESIDUAL_LN, ch.dts[2], ("out", "rep"))):
        launch = getattr(ch, stage)
        for v in E.VARIANTS:
            tag = f"{form} {col} {stage} v{v}"
            msg = refusal(dt, epi, v)
            if msg:
                expect_refused(lambda: launch(v, MA), msg, tag)
                continue
            full = launch(v, MA)
            check_a_residual(tag, ch, full, dt, *refs[stage], ctl=ctl3 if stage == "w3" else None)
            check_c_residual(tag, full, dt)
            for M in E.ROWS:
                o = launch(v, M)
                check_b_rows(tag, o, full, keys)
                check_c_residual(tag, o, dt)
            if C < E.C_FULL:
                # (b) in N: the launch on the first C of C_FULL packed weight rows returns the bits of columns [0, C) of the launch on all of them
                wide = launch(v, MA, E.C_FULL)
                check_c_residual(tag + " N = C_FULL", wide, dt)
                assert torch.equal(full["out"][:MA, :C], wide["out"][:MA, :C]) and torch.equal(full["rep"][:, :C], wide["rep"][:, :C]), f"{tag}: columns [0, N) depend on N"
                if "act" in full:
                    pl = o_planes(dt)
                    assert torch.equal(values(full["act"][:MA], pl)[:, :C], values(wide["act"][:MA], pl)[:, :C]), f"{tag}: act copy columns [0, N) depend on N"
                    whole = C // 64                        # whole statistics slots: bit-equal; the last, partial one was held to the f64 sums in (a)
                    assert torch.equal(stats_body(full["stats"], full["cap"])[:MA, :whole], stats_body(wide["stats"], wide["cap"])[:MA, :whole]), f"{tag}: whole slots depend on N"


@pytest.mark.parametrize("col", list(E.COLS))
@pytest.mark.parametrize("form", list(FORMS))
def test_swiglu_epilogues_at_the_tails(form, col):
    """EPI_SWIGLU_STATS_LN (w1|w2 behind the folded norm2) and EPI_SWIGLU_STATS: hidden units (planes where the form writes them) and their statistics --
    (a) / (b) / (c) for every variant of the set, every M of the row list, and in N (a launch on fewer packed rows)."""
    ch = chain(form, col)
    Hd, Hp = ch.Hd, ch.Hp
    for stage, epi, dt in (("w12", lib.EPI_SWIGLU_STATS_LN, ch.dts[1]), ("swiglu_plain", lib.EPI_SWIGLU_STATS, ch.dts[0])):
        launch = getattr(ch, stage)
        h_ref = ch.ref_w12() if stage == "w12" else ch.ref_swiglu_plain()
        ctl = ch.ref_w12(control=True) if stage == "w12" else None
        for v in E.VARIANTS:
            tag = f"{form} {col} {stage} v{v}"
            msg = refusal(dt, epi, v)
            if msg:
                expect_refused(lambda: launch(v, MA), msg, tag)
                continue
            full = launch(v, MA)
            check_a_swiglu(tag, full, dt, h_ref, ctl)
            check_c_swiglu(tag, full, dt)
            for M in E.ROWS:
                o = launch(v, M)
                check_b_rows(tag, o, full, ("hid", "stats"))
                check_c_swiglu(tag, o, dt)
            # (b) in N: fewer packed weight rows (Hp2 hidden units, min(Hd, Hp2) of them valid) -- the valid units and every whole slot of valid units keep their bits
            Hp2 = ch.Hpk if Hp < ch.Hpk else Hp - 16
            lo, hi = (full, launch(v, MA, Hp2, min(Hd, Hp2))) if Hp2 > Hp else (launch(v, MA, Hp2, min(Hd, Hp2)), full)
            other = hi if Hp2 > Hp else lo
            check_c_swiglu(tag + f" Hp = {Hp2}", other, dt)
            nv, pl = min(Hd, Hp, Hp2), o_planes(dt)
            assert torch.equal(values(lo["hid"][:MA], pl)[:, :nv], values(hi["hid"][:MA], pl)[:, :nv]), f"{tag}: hidden units [0, {nv}) depend on N"
            whole = nv // 64
            assert torch.equal(stats_body(lo["stats"], lo["cap"])[:MA, :whole], stats_body(hi["stats"], hi["cap"])[:MA, :whole]), f"{tag}: whole slots depend on N"
            e_st = stats_errors(other["stats"], other["cap"], values(other["hid"][:MA], pl), other["Hp"], 64, MA)
            assert e_st < TOL_STATS, f"{tag}: statistics of the launch at Hp = {Hp2}: {e_st:.3e}"


@pytest.mark.parametrize("form", ["f32x3w", "f32x3p", "f32x3wo", "f32x3wa"])
def test_plain_epilogues_on_planes_at_the_tails(form):
    """EPI_BIAS / EPI_GELU / EPI_RESIDUAL with W (and A) as planes: every output stays plain f32.  Row tails and a ragged N (130: scalar stores) against f64, prefix
    bit-identity in M, canaries."""
    dt = FORMS[form][0]
    K, NF = 128, 256
    A = rnd(MA, K, seed=21).to(DEV)
    W = pack(rnd(NF, K, seed=22, scale=K ** -0.5), lib.F32, torch.float32)
    b, res = rnd(NF, seed=23).to(DEV), (2.0 * rnd(MA, NF, seed=24) + 0.3).to(DEV)
    a_in, w_in = (to_planes(A) if a_planes(dt) else A), to_planes(W)
    lin = A.double() @ W.double().T + b.double()

    def launch(epi, v, M, N):
        out = canary(MA + 8, E.ru(N, 32) + 32, torch.float32)
        r = res if epi == lib.EPI_RESIDUAL else None
        lib.call("toc3d_linear_ex", dt, epi, v, a_in, K, w_in, K, b, out, out.shape[1], r, NF if r is not None else 0, 0, None, None, M, N, K, 0, S())
        return out

    for N in (256, 130, 132):
        for epi, ref in ((lib.EPI_BIAS, lin), (lib.EPI_GELU, torch.nn.functional.gelu(lin)), (lib.EPI_RESIDUAL, res.double() + lin)):
            for v in E.VARIANTS:
                tag = f"{form} plain epilogue {epi} N={N} v{v}"
                msg = refusal(dt, epi, v)
                if msg:
                    expect_refused(lambda: launch(epi, v, MA, N), msg, tag)
                    continue
                full = launch(epi, v, MA, N)
                e = relerr(full[:MA, :N], ref[:, :N])
                assert e < TOL_F32, f"{tag}: {e:.3e}"
                check_untouched(tag, full, MA, N, False)
                for M in E.ROWS_SHORT:
                    o = launch(epi, v, M, N)
                    assert torch.equal(bits(o[:M]), bits(full[:M])), f"{tag}: M = {M} is not the bits of rows [0, M)"
                    check_untouched(tag, o, M, N, False)
    with pytest.raises(RuntimeError, match="whole 32-element groups"):      # rows of planes are whole 32-element groups: a planes A with lda % 32 != 0 is refused
        if a_planes(dt):
            bad = torch.zeros(MA, K + 8, device=DEV)
            lib.call("toc3d_linear_ex", dt, lib.EPI_BIAS, 16, bad, K + 8, w_in, K, b, canary(MA, NF, torch.float32), NF, None, 0, 0, None, None, MA, NF, K, 0, S())
        else:                                                                # ... and so is an act copy in planes with ld_act % 32 != 0 (F32X3WO)
            o = canary(MA, NF, torch.float32)
            st = canary(1, 4 + MA * 5 * 2, torch.float32).view(-1)
            lib.call("toc3d_linear_fused", X3WO, lib.EPI_RESIDUAL_STATS, 16, A, K, w_in, K, b, o, NF, res, NF, 0, None, None, MA, NF, K, 0,
                     st, 5, None, 0, None, 0, 0.0, canary(MA, NF + 8, torch.float32), NF + 8, None, S())


def test_refused_combinations_stay_refused():
    """Argument checks of csrc/gemm.hip the tail matrix runs into: each is asserted with its message."""
    ch = chain("f32x3p", "n_mod8_is4")
    p = ch.base("proj")
    hid = canary(MA, 96, torch.float32)                     # SwiGLU hidden units as planes: ldo must be a whole number of 32-element groups
    st = canary(1, 4 + MA * 3 * 2, torch.float32).view(-1)
    with pytest.raises(RuntimeError, match="whole 32-element groups"):
        lib.call("toc3d_linear_fused", X3P, lib.EPI_SWIGLU_STATS_LN, 16, p["act"], p["act"].shape[1], to_planes(ch.W12), ch.K12, ch.c2_12, hid[:, :72], 72, None, 0, 0, None, None,
                 MA, 128, ch.K12, 50, st, 3, p["stats"], p["cap"], ch.c1_12, ch.C, EPS, None, 0, None, S())
    with pytest.raises(RuntimeError, match="N%32==0"):      # packed SwiGLU columns come in whole (w1, w2) groups of 32
        lib.call("toc3d_linear_fused", X3P, lib.EPI_SWIGLU_STATS_LN, 16, p["act"], p["act"].shape[1], to_planes(ch.W12), ch.K12, ch.c2_12, hid, 96, None, 0, 0, None, None,
                 MA, 2 * 56, ch.K12, 50, st, 3, p["stats"], p["cap"], ch.c1_12, ch.C, EPS, None, 0, None, S())
    with pytest.raises(RuntimeError, match="stats_out_cap"):  # one slot per 64 output columns, the partial one included
        o = canary(MA, 160, torch.float32)
        lib.call("toc3d_linear_fused", X3P, lib.EPI_RESIDUAL_STATS, 16, to_planes(ch.att), ch.K1, to_planes(ch.Wp), ch.K1, ch.bp, o, 160, ch.x0, E.C_FULL, 0, None, None,
                 MA, 132, ch.K1, 0, st, 2, None, 0, None, 0, 0.0, canary(MA, 160, torch.float32), 160, None, S())
    with pytest.raises(RuntimeError, match="ld_act >= N"):   # the act copy needs rows of >= N elements, a multiple of 4
        o = canary(MA, 160, torch.float32)
        lib.call("toc3d_linear_fused", X3, lib.EPI_RESIDUAL_STATS, 16, ch.att, ch.K1, ch.Wp, ch.K1, ch.bp, o, 160, ch.x0, E.C_FULL, 0, None, None,
                 MA, 130, ch.K1, 0, st, 3, None, 0, None, 0, 0.0, canary(MA, 134, torch.float32), 134, None, S())


ROPE_FORMS = {"bf16": BF16, "f32x3p": X3P, "f32x3wo": X3WO}


@pytest.mark.parametrize("form", list(ROPE_FORMS))
def test_qkv_rope_epilogue_at_the_row_tails(form):
    """toc3d_linear_qkv_rope (N = 3C with C % 64 == 0: no column tails): every row-tail class, against the oracle's RoPE (eva_utils.py:378-379) in f64 on the rounded
    operands; prefix bit-identity in M; canaries.  N % 192 != 0 is refused."""
    dt = ROPE_FORMS[form]
    bf = dt == BF16
    tdt = torch.bfloat16 if bf else torch.float32
    C, L = 128, 16
    heads = C // 64
    cos, sin = synth.rope_tables(L)
    A, W, b = rnd(MA, C, seed=1), rnd(3 * C, C, seed=2, scale=C ** -0.5), rnd(3 * C, seed=3)
    slots = torch.randint(0, L * L, (MA,), generator=torch.Generator().manual_seed(4))
    Ar, Wr = A.to(tdt).double(), W.to(tdt).double()
    y = (Ar @ Wr.T + b.double()).view(MA, 3, heads, 64)
    cs, sn = cos[slots].double()[:, None, :], sin[slots].double()[:, None, :]
    ref = torch.stack([rope_ref(y[:, 0], cs, sn) * lib.ATTN_ROT_Q_SCALE, rope_ref(y[:, 1], cs, sn), y[:, 2]], 1).reshape(MA, 3 * C)
    tab, _ = compact_tables(cos, sin)
    rc, b_d = rc_of(slots, L), b.to(DEV)
    a_d = A.to(DEV).to(tdt)
    w_d = pack(W, BF16 if bf else lib.F32, tdt)
    if not bf:
        w_d = to_planes(w_d)
        if a_planes(dt):
            a_d = to_planes(a_d)
    ldo = 3 * C + 32

    def launch(v, M, N=3 * C):
        out = canary(MA + 8, ldo, tdt)
        lib.call("toc3d_linear_qkv_rope", dt, v, a_d, C, w_d, C, b_d, out, ldo, M, N, C, rc, tab, L, lib.ATTN_ROT_Q_SCALE, S())
        return out

    for v in E.VARIANTS:
        tag = f"rope {form} v{v}"
        if not bf and E.VARIANTS[v][4] and not a_planes(dt):
            expect_refused(lambda: launch(v, MA), "cannot serve", tag)
            continue
        full = launch(v, MA)
        e = relerr(values(full[:MA], not bf)[:, :3 * C], ref)
        print(f"[{tag}] rel err vs f64 {e:.3e}")
        assert e < (TOL_BF16 if bf else TOL_F32), f"{tag}: {e:.3e}"
        check_untouched(tag, full, MA, 3 * C, not bf)
        for M in E.ROWS:
            o = launch(v, M)
            assert torch.equal(bits(o[:M]), bits(full[:M])), f"{tag}: M = {M} is not the bits of rows [0, M) of the launch at M = {MA}"
            check_untouched(tag, o, M, 3 * C, not bf)
    with pytest.raises(RuntimeError, match="N = 3C"):
        launch(16, MA, 3 * C - 64)
