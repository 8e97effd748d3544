"""Shape classes and f64 references of the fused GEMM epilogues (shared by test_gpu_epilogue_tails.py and test_cpu_epilogue_reference.py; no GPU needed here).

Where the classes come from -- the launch table of csrc/gemm_kernels.h (launch_epi / launch_epi_x / launch_phased) and the epilogue (gemm_epilogue, tile_finish):

  * a workgroup owns a BM x BN tile, split over WM x WN wavefronts; a wavefront owns a "slab" of TM = BM / WM rows = MT row tiles of 16 rows and TN = BN / WN
    columns = NT column tiles of 16 columns; a lane holds 4 consecutive columns (lane group g = lane / 16 -> columns g * 4 ..) of one row per tile;
  * planes and wide bf16 stores leave in PAIRS of row tiles (2i, 2i + 1) with a lane-group exchange (store_pair_wide / store_planes_pair), so what matters in M
    is M mod 32 (which tile of the last pair is partial) and where M ends inside a slab (tiles 0, 1 valid and the rest of the slab past M; M below one slab; one
    row past a whole workgroup tile);
  * in N the epilogue distinguishes: a lane's 4 columns partly valid (N % 4 != 0: scalar stores), a lane group valid whose exchange partner is not (N % 8 == 4),
    a 16-column tile partly valid (N % 16 != 0), a statistics slot partly valid (N % 64 != 0 for the residual epilogues; 64 hidden units = 128 packed columns for
    SwiGLU), the last N-tile partly valid (N % 128 != 0), fewer columns than one slot (N < 64); for SwiGLU the valid hidden units Hd against the packed Hp.

VARIANTS is the small set the tail tests run: one tile per slab height and per store path of the launch table (the exhaustive variant lists stay in test_gpu_ops.py)."""
import torch

# variant -> (BM, TM, BN, TN, x3 form needs both operands as planes).  csrc/gemm_kernels.h launch_epi_x / launch_phased:
#   16: 128x128 on 2x4 waves (64-row slab)        19: 256x128 on 4x2 (64-row slab, 256-row block)      49: 192x128 on 2x4 (96-row slab)
#   52: 192x192 on 2x4 (96 x 48: no SwiGLU)       54: 96x128 on 2x4 (48-row slab, MT odd)              57: 160x128 on 2x4 (80-row slab, MT odd)
#   60 / 61 / 63: phased 256x256 on 2x4 (128-row slab) / 256x128 on 4x2 / 128x128 on 2x4               116: variant 16 in the per-XCD band order
VARIANTS = {
    16: (128, 64, 128, 32, False), 19: (256, 64, 128, 64, False), 49: (192, 96, 128, 32, False), 52: (192, 96, 192, 48, False),
    54: (96, 48, 128, 32, True), 57: (160, 80, 128, 32, True), 60: (256, 128, 256, 64, True), 61: (256, 64, 128, 64, True), 63: (128, 64, 128, 32, True),
    116: (128, 64, 128, 32, False),
}
TOL_F32, TOL_BF16, TOL_STATS = 2e-5, 6e-3, 1e-5      # the bars of these output classes: f32 and bf16 x 3 outputs (of the output's max), bf16-rounded outputs, row statistics
M_ALIGNED = 576                      # whole pairs of row tiles (576 % 32 == 0): the launch that is checked against f64 and that every prefix launch is compared with
ROWS = (1, 16, 24, 41, 48, 59, 120, 152, 161, 184, 193, 216, 257, 555)
ROWS_SHORT = (1, 24, 41, 59, 216, 257)   # the plain epilogues on planes (every output plain f32: no paired planes stores)
ROW_CLASSES = ("m1", "m16", "even_partial", "even_alone", "odd_partial", "pair_then_past", "pair_then_past_later_slab", "below_slab", "block_plus_one")


def row_classes(M, bm, tm):
    """The row-tail classes (see the module docstring) M falls into for a tile of bm rows with tm-row wavefront slabs."""
    out = set()
    if M == 1:
        out.add("m1")
    if M == 16:
        out.add("m16")
    r32 = M % 32
    if 1 <= r32 <= 15:
        out.add("even_partial")          # the even tile of the last pair is partial, its partner lies past M
    if r32 == 16:
        out.add("even_alone")            # the even tile is whole, its partner lies past M
    if 17 <= r32 <= 31:
        out.add("odd_partial")           # the odd tile is partial
    rs = (M % bm) % tm                   # valid rows of the last, partly filled slab (0: none)
    if tm > 32 and 17 <= rs <= 32:
        out.add("pair_then_past")        # tiles 0, 1 of a slab valid, every later tile of the slab past M
        if M > tm:
            out.add("pair_then_past_later_slab")
    if M < tm:
        out.add("below_slab")
    if M > bm and M % bm == 1:
        out.add("block_plus_one")
    return out


def row_cases(cls, variant, rows=ROWS):
    bm, tm = VARIANTS[variant][:2]
    return [M for M in rows if cls in row_classes(M, bm, tm)]


# column configurations: C = output columns of the projection (= the normalised width ln_n and the valid K of the w1|w2 GEMM that follows), K1 = its own K,
# (Hd, Hp) = valid / packed hidden units of the SwiGLU GEMM (N = 2 * Hp packed columns; the w3 GEMM then has K = ceil(Hp / 64) * 64 and ln_n = Hd)
COLS = {
    "aligned": dict(C=384, K1=192, Hd=300, Hp=320),        # today's widths; 3 / 6 / 5 K-tiles; ln_n == K in front of w1|w2
    "n_mod4": dict(C=130, K1=64, Hd=20, Hp=64),            # N % 4 != 0 (scalar stores); 1 / 3 / 1 K-tiles, ln_n < K
    "n_mod8_is4": dict(C=132, K1=128, Hd=100, Hp=112),     # a lane group whose exchange partner holds no column; Hp % 64 != 0 (partial SwiGLU slot and N-tile)
    "n_mod16": dict(C=200, K1=64, Hd=40, Hp=128),          # N % 16 == 8; a whole padding slot of hidden units (Hp - Hd >= 64); 4 K-tiles
    "n_lt_64": dict(C=40, K1=64, Hd=192, Hp=192),          # fewer columns than one statistics slot; Hd == Hp; 3 K-tiles, ln_n == K in front of w3
}
C_FULL = 384                                                  # the N-prefix launches take the first C of C_FULL packed weight rows
COL_CLASSES = ("n_mod4", "n_mod8_is4", "n_mod16_mult4", "slot_partial", "ntile_partial", "n_lt_64", "hd_mod16", "hd_mod64", "pad_slot", "hd_eq_hp",
               "k_tiles_1", "k_tiles_2", "k_tiles_3", "k_tiles_odd_ln", "ln_lt_k", "ln_eq_k")


def ru(a, b):
    return (a + b - 1) // b * b


def col_classes(cfg):
    C, K1, Hd, Hp = cfg["C"], cfg["K1"], cfg["Hd"], cfg["Hp"]
    out = set()
    if C % 4:
        out.add("n_mod4")
    if C % 8 == 4:
        out.add("n_mod8_is4")
    if C % 16 and C % 4 == 0:
        out.add("n_mod16_mult4")
    if C % 64:
        out.add("slot_partial")
    if C % 128 or (2 * Hp) % 128:
        out.add("ntile_partial")
    if C < 64:
        out.add("n_lt_64")
    if Hd % 16:
        out.add("hd_mod16")
    if Hd % 64:
        out.add("hd_mod64")
    if Hp - Hd >= 64:
        out.add("pad_slot")
    if Hd == Hp:
        out.add("hd_eq_hp")
    k12, k3 = ru(C, 64), ru(Hp, 64)                         # K of the two LayerNorm-consuming GEMMs
    for k in (K1, k12, k3):
        if k // 64 <= 3:
            out.add(f"k_tiles_{k // 64}")
    if (k12 // 64) % 2 or (k3 // 64) % 2:
        out.add("k_tiles_odd_ln")
    if C < k12 or Hd < k3:
        out.add("ln_lt_k")
    if C == k12 or Hd == k3:
        out.add("ln_eq_k")
    return out


def ln_shapes():
    """(ln_n, K) of every LayerNorm-consuming launch of the matrix."""
    out = set()
    for cfg in COLS.values():
        out.add((cfg["C"], ru(cfg["C"], 64)))
        out.add((cfg["Hd"], ru(cfg["Hp"], 64)))
    return sorted(out)


# ---- (hi, lo) bf16 planes on the host (include/toc3d.h, TOC3D_DTYPE_F32X3W / F32X3P): element c of a row lives in the 128-byte group c / 32, hi = bf16(x) at
# byte 2 (c % 32), lo = bf16(x - hi) at byte 64 + 2 (c % 32)
def planes_split(x):
    """f32 [rows, K] -> (hi, lo) as f32 tensors holding bf16 values."""
    hi = x.to(torch.bfloat16).float()
    return hi, (x - hi).to(torch.bfloat16).float()


def planes_encode(x):
    """f32 [rows, K] (K % 32 == 0) -> the planes image as an f32-typed tensor of the same shape."""
    rows, K = x.shape
    hi, lo = planes_split(x)
    img = torch.stack([hi.view(rows, K // 32, 32), lo.view(rows, K // 32, 32)], 2).to(torch.bfloat16)       # [rows, groups, 2, 32]
    return img.contiguous().view(rows, K * 2).view(torch.float32)


def planes_planes(p):
    """planes image [rows, K] -> (hi, lo) as f32 tensors [rows, K]."""
    rows, K = p.shape
    b = p.contiguous().view(torch.bfloat16).view(rows, K // 32, 2, 32)
    return b[:, :, 0, :].reshape(rows, K).float(), b[:, :, 1, :].reshape(rows, K).float()


# ---- f64 references -----------------------------------------------------------------------------------------------------------------------------
def layernorm_rows_f64(a, ln_n, eps):
    """Two-pass LayerNorm statistics over the first ln_n columns (F.layer_norm: biased variance), no affine: the normalised [rows, ln_n] block in f64."""
    x = a[:, :ln_n].double()
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps)


def explicit_ln_matmul(a, w, c2, ln_n, eps):
    """LayerNorm of the rows, THEN the matmul with the gamma-scaled packed weights w [N, >= ln_n] (+ c2 = beta . w + b): the reference of the _LN epilogues."""
    return layernorm_rows_f64(a, ln_n, eps) @ w[:, :ln_n].double().T + c2.double()


def folded_ln_matmul(a, w, c1, c2, ln_n, eps, dtype=torch.float64):
    """What the kernels evaluate (include/toc3d.h): rstd * (a . w - mean * c1) + c2 with (mean, rstd) from the one-pass sums; in `dtype` arithmetic
    (f64: the identity test; f32: the same-precision control of the tail tests)."""
    x, wv = a[:, :ln_n].to(dtype), w[:, :ln_n].to(dtype)
    s1, s2 = x.double().sum(1, keepdim=True), (x.double() ** 2).sum(1, keepdim=True)
    mean = s1 / ln_n
    var = (s2 / ln_n - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + eps)
    return (rstd.to(dtype) * (x @ wv.T - mean.to(dtype) * c1.to(dtype)) + c2.to(dtype)).double()


def swiglu_units(z, Hd, Hp):
    """Packed columns z [rows, 2 * Hp] (per 32: 16 w1 units, then w2 of the same units; toc3d_pack_swiglu) -> hidden units [rows, Hp], zero from Hd on."""
    zz = z.view(z.shape[0], Hp // 16, 2, 16)
    h = (torch.nn.functional.silu(zz[:, :, 0]) * zz[:, :, 1]).reshape(z.shape[0], Hp)
    h[:, Hd:] = 0
    return h


def slot_sums(vals, width, slot):
    """Per-row (sum, sum of squares) of vals[:, :width] per `slot` columns -> [rows, ceil(width / slot), 2] in f64."""
    rows = vals.shape[0]
    n = (width + slot - 1) // slot
    v = torch.zeros(rows, n * slot, dtype=torch.float64, device=vals.device)
    v[:, :width] = vals[:, :width].double()
    v = v.view(rows, n, slot)
    return torch.stack([v.sum(2), (v * v).sum(2)], 2)
