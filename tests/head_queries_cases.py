"""The plain-torch restatement of the head's query side -- StreamPETRHead.forward :641-652 with temporal_alignment :424-453 -- and the cases of the REAL reference's
fixtures (tests/golden/head_queries_*.npz, written by tools/gen_golden_head_queries.py); shared by test_cpu_head_queries.py and test_gpu_head_queries.py, importing
this needs no GPU.  The restatement is the GPU tests' control where the reference is absent."""
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from support import rel_max_zero_ok
from toc3d_amd import synth
from toc3d_amd.head_queries import dim_t

OUTPUTS = ("tgt", "query_pos", "reference_points", "temp_memory", "temp_pos", "rec_ego_pose")
BANK = ("memory_embedding", "memory_reference_point", "memory_timestamp", "memory_egopose", "memory_velo")
TINY_FRAMES = (0, 1, 3, 4)


def posemb(pos, nf):
    """pos2posemb1d / one coordinate of pos2posemb3d: sin on the even, cos on the odd columns of pos * 2 pi / dim_t, in the dtype of ``pos``."""
    a = (pos * (2 * math.pi))[..., None] / dim_t(nf).to(pos.device)
    return torch.where(torch.arange(nf, device=pos.device) % 2 == 0, a.sin(), a.cos())


def pos3d(x):
    """pos2posemb3d: concatenated (y, x, z)."""
    return torch.cat([posemb(x[..., 1], 128), posemb(x[..., 0], 128), posemb(x[..., 2], 128)], -1)


def nerf(x):
    """nerf_positional_encoding: frequency-major, sin of all scalars then cos of all scalars."""
    return torch.cat([f(x * 2.0 ** k) for k in range(6) for f in (torch.sin, torch.cos)], -1)


def restated_queries(sd, bank, sizes, with_ego_pos=True, pc_range=synth.PC_RANGE, dtype=torch.float32, contract=None):
    """The six outputs from the formulas.  ``contract`` = dtype the operands of every linear layer are rounded to (None: none), accumulation and everything else
    in ``dtype``: contract=torch.bfloat16 is the torch-bf16 control.  dtype=torch.float64 keeps the motion vector and the time embedding in f64 as well."""
    dev, E, nq, np_ = bank["memory_embedding"].device, sizes["embed_dims"], sizes["num_query"], sizes["num_propagated"]
    B = bank["memory_embedding"].shape[0]
    c = lambda t: t if contract is None else t.to(contract).to(dtype)
    p = {k: v.to(dev, dtype) for k, v in sd.items()}
    lin = lambda x, pre: c(x) @ c(p[pre + ".weight"].T) + p[pre + ".bias"]
    qemb = lambda x: lin(F.relu(lin(pos3d(x), "query_embedding.0")), "query_embedding.2")
    temb = lambda ts: F.layer_norm(lin(posemb(ts[..., 0], 256).to(dtype), "time_embedding.0"), (E,), p["time_embedding.1.weight"], p["time_embedding.1.bias"])

    def mln(x, cond, pre):
        h = F.relu(lin(cond, pre + ".reduce.0"))
        return lin(h, pre + ".gamma") * F.layer_norm(x, (E,)) + lin(h, pre + ".beta")
    pc = torch.tensor(pc_range, dtype=torch.float32, device=dev).to(dtype)             # (an f32 parameter of the head, :215)
    ref = p["reference_points.weight"][None].repeat(B, 1, 1)
    query_pos, tgt = qemb(ref), torch.zeros(B, nq, E, dtype=dtype, device=dev)
    tref = (bank["memory_reference_point"].to(dtype) - pc[:3]) / (pc[3:] - pc[:3])
    temp_pos, temp_memory = qemb(tref), bank["memory_embedding"].to(dtype)
    ts = bank["memory_timestamp"]
    if with_ego_pos:
        eye = torch.eye(4, dtype=dtype, device=dev)[:3].flatten()
        n0 = nerf(torch.cat([torch.zeros(B, nq, 3, dtype=dtype, device=dev), eye.expand(B, nq, 12)], -1))
        tgt, query_pos = mln(tgt, n0, "ego_pose_memory"), mln(query_pos, n0, "ego_pose_pe")
        nm = nerf(torch.cat([bank["memory_velo"], ts, bank["memory_egopose"][..., :3, :].flatten(-2)], -1).to(dtype))
        temp_pos, temp_memory = mln(temp_pos, nm, "ego_pose_pe"), mln(temp_memory, nm, "ego_pose_memory")
    query_pos = query_pos + temb(torch.zeros(B, nq, 1, dtype=dtype, device=dev))
    temp_pos = temp_pos + temb(ts)
    if np_ > 0:
        tgt, query_pos, ref = (torch.cat([a, b[:, :np_]], 1) for a, b in ((tgt, temp_memory), (query_pos, temp_pos), (ref, tref)))
        temp_memory, temp_pos = temp_memory[:, np_:], temp_pos[:, np_:]
    rec = torch.eye(4, device=dev).repeat(B, ref.shape[1], 1, 1)
    return dict(zip(OUTPUTS, (tgt, query_pos, ref, temp_memory, temp_pos, rec)))


def _trim_rec_ego_pose(outs, Q):
    """The reference sizes rec_ego_pose from query_pos AFTER the concatenation (:447, :449): num_query + 2 num_propagated identities, of which only the first
    num_query + num_propagated are ever indexed (post_update_memory gathers by query index, :367).  The module returns those; the fixtures keep what the reference
    returned, and the surplus rows are checked here to be identities like the rest."""
    rec = outs["rec_ego_pose"]
    assert rec.shape[1] >= Q == outs["tgt"].shape[1]
    assert bool((rec == torch.eye(4)).all())
    outs["rec_ego_pose"] = rec[:, :Q]
    return outs


def tiny_cases(golden_dir):
    """(tag, sizes, with_ego_pos, bank, reference outputs) of every case and frame of head_queries_tiny.npz."""
    g = np.load(os.path.join(golden_dir, "head_queries_tiny.npz"))
    assert g["ego_f1_rec_ego_pose"].shape == (2, 21 + 2 * 7, 4, 4) and g["np0_f1_rec_ego_pose"].shape == (2, 21, 4, 4)
    t = lambda k: torch.from_numpy(g[k])
    sizes = synth.HEAD_QUERIES_TINY
    cases = []
    for tag, ego in (("ego", True), ("noego", False)):
        for f in TINY_FRAMES:
            cases.append((f"{tag}_f{f}", sizes, ego, {k: t(f"f{f}_{k}") for k in BANK}, _trim_rec_ego_pose({k: t(f"{tag}_f{f}_{k}") for k in OUTPUTS}, 28)))
    cases.append(("np0_f1", dict(sizes, num_propagated=0), True, {k: t(f"np0_f1_{k}") for k in BANK}, _trim_rec_ego_pose({k: t(f"np0_f1_{k}") for k in OUTPUTS}, 21)))
    return cases


def full_cases(golden_dir):
    """(frame, bank, every 8th row of the reference's f32 outputs) of head_queries_full.npz; the banks are regenerated from synth."""
    g = np.load(os.path.join(golden_dir, "head_queries_full.npz"))
    step = int(g["row_step"])
    cases = []
    for f in (0, 1):
        want = {k: torch.from_numpy(g[f"f{f}_{k}"]) for k in OUTPUTS}
        assert bool((want["rec_ego_pose"] == torch.eye(4)).all())
        want["rec_ego_pose"] = want["rec_ego_pose"][:, :-(-900 // step)]          # (the reference returns 644 + 2 * 256 rows: see _trim_rec_ego_pose)
        cases.append((f, synth.head_queries_bank(synth.HEAD_QUERIES_FULL, 1, f), want))
    return step, cases


def group_errors(got, want, step=1):
    return {k: rel_max_zero_ok(got[k][:, ::step], want[k]) for k in OUTPUTS}
