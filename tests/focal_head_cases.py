"""The plain-torch restatement of FocalHead's eval forward (shared by test_cpu_focal_head.py, test_gpu_focal_head.py, test_gpu_focal_head_kernels.py,
tools/gen_golden_focal_head.py and tools/focal_head_time.py; importing this needs no GPU), the case lists of the kernel tests and their derived per-element
bounds.  The restatement pins tests/golden/focal_head_*.npz -- output of the REAL reference (tools/gen_golden_focal_head.py) -- to something checkable where the
reference does not exist, and is the GPU tests' control (``contract=torch.bfloat16``)."""
import torch
import torch.nn.functional as F

from support import rel_max
from toc3d_amd import synth

U = 2.0 ** -24                                         # f32 unit roundoff
GN_EPS = 1e-5
ARITH = ("enc_cls_scores", "enc_bbox_preds", "pred_centers2d", "centerness", "sample_weight")
SIZES = dict(tiny=(synth.FOCAL_HEAD_TINY, synth.FOCAL_HEAD_TINY_SHAPE), full=(synth.FOCAL_HEAD_FULL, synth.FOCAL_HEAD_FULL_SHAPE))


def inverse_sigmoid(x, eps=1e-5):                      # mmdet's definition (models/utils/transformer.py)
    x = x.clamp(min=0, max=1)
    return torch.log(x.clamp(min=eps) / (1 - x).clamp(min=eps))


def geometry(location, ltrb_logits, offset):
    """ltrb.sigmoid() + apply_ltrb (misc.py:26-43) + mmdet's bbox_xyxy_to_cxcywh, and apply_center_offset (:45-56), on (..., 2) / (..., 4) / (..., 2)."""
    s = ltrb_logits.sigmoid()
    lx, ly = location[..., 0], location[..., 1]
    xyxy = torch.stack([lx - s[..., 0], ly - s[..., 1], lx + s[..., 2], ly + s[..., 3]], -1).clamp(0, 1)
    x1, y1, x2, y2 = xyxy.unbind(-1)
    boxes = torch.stack([(x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1], -1)
    return boxes, (inverse_sigmoid(location) + offset).sigmoid()


def restated_forward(sd, inp, infer_ratio, dtype=torch.float32, contract=None):
    """FocalHead.forward at eval (focal_head.py:140-193) from the formulas -> the reference's dict plus ``sample_weight`` (B, N*h*w, 1).  ``contract`` = dtype the
    operands of the two 3x3 convs are rounded to (None: none) -- the products the module forms on the matrix cores; accumulation and everything behind the
    convs in ``dtype``: contract=torch.bfloat16 is the torch-bf16 control.  The ranking is stable-descending (ties to the lower index)."""
    c = lambda t: t if contract is None else t.to(contract).to(dtype)
    src = inp["img_feats"]
    dev = src.device
    p = {k: v.to(dev, dtype) for k, v in sd.items()}
    B, N, C, h, w = src.shape
    K = int(N * h * w * infer_ratio)
    x = src.flatten(0, 1).to(dtype)
    NC = p["cls.weight"].shape[0]

    def tower(name):
        t = F.conv2d(c(x), c(p[name + ".0.weight"]), None, padding=1) + p[name + ".0.bias"][None, :, None, None]
        return F.relu(F.group_norm(t, 32, p[name + ".1.weight"], p[name + ".1.bias"], GN_EPS))
    rows = lambda t: t.permute(0, 2, 3, 1)
    cls_feat, reg_feat = tower("shared_cls"), tower("shared_reg")
    one = lambda feat, name: rows(F.conv2d(feat, p[name + ".weight"], p[name + ".bias"]))
    cls_logits = one(cls_feat, "cls").reshape(B * N, -1, NC)
    centerness = one(cls_feat, "centerness").reshape(B * N, -1, 1)
    boxes, centers = geometry(inp["location"].to(dev, dtype), one(reg_feat, "ltrb"), one(reg_feat, "center2d"))
    weight = cls_logits.max(-1).values.view(B, -1, 1).sigmoid() * centerness.view(B, -1, 1).sigmoid()
    order = torch.sort(weight, dim=1, descending=True, stable=True).indices
    return dict(enc_cls_scores=cls_logits, enc_bbox_preds=boxes.reshape(B * N, -1, 4), pred_centers2d=centers.reshape(B * N, -1, 2), centerness=centerness,
                topk_indexes=order[:, :K], sample_weight=weight)


def group_errors(out, ref):
    """max-abs error over max-abs reference, per arithmetic output (outputs of different scale: one max over all hides errors)."""
    return {k: rel_max(torch.as_tensor(out[k]), torch.as_tensor(ref[k])) for k in ARITH}


def index_band(weight_ref, K, half_width):
    """Per sample of ``weight_ref`` (B, n): (mask of the tokens OUTSIDE the band of ``half_width[b]`` around the K-th largest reference value, the band's share
    of the tokens).  0 < K < n.  The K-th token is the band's centre, in it at any width: the share counts the OTHER tokens the band holds (with the centre
    counted, no band on the 30 tokens of the tiny fixture could stay under 0.5 %)."""
    w = torch.as_tensor(weight_ref).double().reshape(weight_ref.shape[0], -1)
    kth = torch.sort(w, dim=1, descending=True).values[:, K - 1:K]
    inside = (w - kth).abs() <= torch.as_tensor(half_width, dtype=torch.float64).reshape(-1, 1)
    return ~inside, (inside.double().sum(1) - 1.0) / w.shape[1]


def membership(indexes, n):
    """(B, K[, 1]) index lists -> (B, n) bool."""
    idx = torch.as_tensor(indexes).reshape(indexes.shape[0], -1).long()
    m = torch.zeros(idx.shape[0], n, dtype=torch.bool)
    m.scatter_(1, idx.cpu(), True)
    return m


# ---- the kernel tests' cases and bounds ----------------------------------------------------------------------------------------------------------------------------
# statistics: (T = h*w, E, V, offset in units of the spread).  T = 1: one pixel; 15: fewer rows than a workgroup keeps in flight; 1000: the shipped view.
# E = 64 / 256: 2 / 8 channels per group.  The last case shifts every channel by 100 x its spread: a one-pass E[x^2] - E[x]^2 loses all digits there.
STATS_CASES = [(T, E, V, 0.0) for T in (1, 15, 1000) for E in (64, 256) for V in (1, 2)] + [(1000, 256, 1, 100.0)]
# heads: (num_classes, V, T, E).  M = V*T in {1, 15, 2000, 33}: 33 = one past the 32 rows of a workgroup (a second workgroup with one row)
HEADS_CASES = [(NC, V, T, E) for NC in (1, 3, 10) for V, T, E in ((1, 1, 64), (1, 15, 64), (2, 1000, 256), (1, 33, 256))] + [(10, 3, 5, 64)]
RANK_CASES = [(B, n) for n in (15, 2000) for B in (1, 2)]


def stats_bounds(x64, cpg, T, eps=GN_EPS):
    """x64 f64 [V, T, G, cpg] -> (mean, var, bound on |mean' - mean|, relative bound on rstd'^-2 against var + eps).  n = cpg*T terms per group.  Any order of
    f32 additions of n terms errs by at most (n - 1) u sum|x| (first order); the division adds one rounding: |mean' - mean| <= n u mean|x|.  The second pass sums
    (x - m)^2 about the COMPUTED mean m: exactly, sum (x - m)^2 / n = var + (m - mean)^2, which the bound on the mean covers; in f32 each term carries three
    roundings (the difference, twice; the square), the sum n - 1, the division and the add of eps one each, and 1 / sqrt two more, which count twice in
    rstd^-2: n + 8, and two of slack -- (n + 10) u."""
    n = cpg * T
    g = x64.permute(0, 2, 1, 3).reshape(x64.shape[0], x64.shape[2], -1)
    mean, var = g.mean(-1), g.var(-1, unbiased=False)
    b_mean = n * U * g.abs().mean(-1)
    b_var = (n + 10) * U + b_mean ** 2 / (var + eps)
    return mean, var, b_mean, b_var


def dot_bound(h_abs, w_abs, bias_abs, K, extra=4):
    """(K + extra) u (sum |h||w| + |b|): K products and additions in any order, the bias add, and ``extra`` roundings of slack for the inputs' own affine."""
    return (K + extra) * U * (h_abs @ w_abs.T + bias_abs)
