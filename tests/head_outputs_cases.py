"""The plain-torch restatement of the head's prediction branches and box decoding (shared by test_cpu_head_outputs.py and test_gpu_head_outputs.py; importing
this needs no GPU).  It pins tests/golden/head_outputs_*.npz -- output of the REAL reference (tools/gen_golden_head_outputs.py) -- to something checkable where
the reference does not exist, and is the GPU tests' control."""
import torch

from support import layer_norm, rel_max
from toc3d_amd import synth

GROUPS = dict(centres=slice(0, 3), sizes=slice(3, 6), rotation=slice(6, 8), velocity=slice(8, 10))      # columns of different scale: one max over all hides errors


def inverse_sigmoid(x, eps=1e-5):                      # mmdet's definition (oracle/head_tokens_oracle.py)
    x = x.clamp(min=0, max=1)
    return torch.log(x.clamp(min=eps) / (1 - x).clamp(min=eps))


def restated_branches(sd, inp, pc_range=synth.PC_RANGE, dtype=torch.float32, contract=None):
    """get_transformer_outputs behind the transformer call (streampetr_head.py:582-602) from the formulas -> (cleaned outs_dec, all_cls_scores, all_bbox_preds).
    ``contract`` = dtype the operands of every linear layer are rounded to (None: none), accumulation and everything else in ``dtype``:
    contract=torch.bfloat16 is the torch-bf16 control."""
    c = lambda t: t if contract is None else t.to(contract).to(dtype)
    dev = inp["outs_dec"].device
    p = {k: v.to(dev, dtype) for k, v in sd.items()}
    lin = lambda x, pre: c(x) @ c(p[pre + ".weight"].T) + p[pre + ".bias"]
    x = torch.nan_to_num(inp["outs_dec"].float()).to(dtype)
    t = x
    for i in (0, 3):
        t = torch.relu(layer_norm(lin(t, f"cls_branches.0.{i}"), p[f"cls_branches.0.{i + 1}.weight"], p[f"cls_branches.0.{i + 1}.bias"]))
    cls = lin(t, "cls_branches.0.6")
    r = torch.relu(lin(torch.relu(lin(x, "reg_branches.0.0")), "reg_branches.0.2"))
    box = lin(r, "reg_branches.0.4")
    pc = torch.tensor(pc_range, dtype=dtype, device=dev)
    centre = torch.sigmoid(box[..., 0:3] + inverse_sigmoid(inp["reference_points"].to(dtype)))
    box = torch.cat([centre * (pc[3:6] - pc[0:3]) + pc[0:3], box[..., 3:]], -1)
    return x, cls, box


def restated_decode(cls, box, max_num, post_center_range, score_threshold=None, sub_half_height=False):
    """NMSFreeCoder.decode_single (nms_free_coder.py:39-90) on (Q, NC) logits and (Q, CS) boxes, ties to the lowest flat index -> (bboxes, scores, labels,
    flat indices of the survivors, flat indices of the whole top-k list)."""
    NC = cls.shape[-1]
    s, idx = torch.sort(cls.sigmoid().reshape(-1), descending=True, stable=True)
    s, idx = s[:max_num], idx[:max_num]
    b = box[torch.div(idx, NC, rounding_mode="floor")]
    cols = [b[:, 0:3], b[:, 3:6].exp(), torch.atan2(b[:, 6:7], b[:, 7:8])] + ([b[:, 8:10]] if box.shape[-1] > 8 else [])
    out = torch.cat(cols, -1)
    pcr = torch.tensor(post_center_range, dtype=out.dtype, device=out.device)
    mask = (out[:, :3] >= pcr[:3]).all(1) & (out[:, :3] <= pcr[3:]).all(1)
    if score_threshold:
        mask &= s >= score_threshold
    out = out[mask]
    if sub_half_height:
        out = torch.cat([out[:, :2], out[:, 2:3] - out[:, 5:6] * 0.5, out[:, 3:]], -1)
    return out, s[mask], (idx % NC)[mask], idx[mask], idx


def rows_without_inf(inp):
    """(L, B, Q) mask.  nan_to_num turns +-inf into +-FLT_MAX; the linear layers behind it overflow, and what a row of inf / NaN sums becomes depends on the
    order of the additions -- for such rows only the cleaned outs_dec is comparable (exactly), not the branches' outputs."""
    return ~torch.isinf(inp["outs_dec"]).any(-1)


def group_errors(cls, box, ref_cls, ref_box, rows=None):
    cls, box, ref_cls, ref_box = (torch.as_tensor(t) for t in (cls, box, ref_cls, ref_box))
    if rows is not None:
        cls, box, ref_cls, ref_box = cls[rows], box[rows], ref_cls[rows], ref_box[rows]
    errs = {"cls": rel_max(cls, ref_cls)}
    errs.update({k: rel_max(box[..., s], ref_box[..., s]) for k, s in GROUPS.items()})
    return errs
