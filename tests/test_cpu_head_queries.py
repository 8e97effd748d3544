"""CPU: the query side of the head (toc3d_amd.HeadQueries) -- a plain-torch restatement of StreamPETRHead.forward :641-652 with temporal_alignment :424-453
reproduces the REAL reference's fixtures (tests/golden/head_queries_*.npz, written by tools/gen_golden_head_queries.py); the module's state dict equals the
reference's; the fixtures satisfy what the concatenation promises.  The restatement is the GPU tests' control where the reference is absent.

Every test prints the figures it asserts on (run with -s)."""
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import toc3d_amd
from test_cpu_decoder import rel_max as _rel_max
from toc3d_amd import synth
from toc3d_amd.head_queries import dim_t

OUTPUTS = ("tgt", "query_pos", "reference_points", "temp_memory", "temp_pos", "rec_ego_pose")
BANK = ("memory_embedding", "memory_reference_point", "memory_timestamp", "memory_egopose", "memory_velo")
TINY_FRAMES = (0, 1, 3, 4)


def rel_max(a, b):
    """max-abs error over max-abs reference (tests/test_cpu_decoder.py); an all-zero reference (the empty bank's rows) must be met exactly."""
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    if not b.any():
        return 0.0 if not a.any() else float("inf")
    return _rel_max(a, b)


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
    return {k: rel_max(got[k][:, ::step], want[k]) for k in OUTPUTS}


def test_restatement_reproduces_the_tiny_fixture(golden_dir):
    worst = {}
    for tag, sizes, ego, bank, want in tiny_cases(golden_dir):
        got = restated_queries(synth.head_queries_state_dict(sizes, with_ego_pos=ego), bank, sizes, with_ego_pos=ego)
        assert all(got[k].shape == want[k].shape and got[k].dtype == torch.float32 for k in OUTPUTS), tag
        errs = group_errors(got, want)
        print(f"[head queries restated, tiny {tag}] rel max err { {k: f'{e:.1e}' for k, e in errs.items()} }")
        worst[tag] = max(errs.values())
    assert max(worst.values()) <= 1e-5, worst


def test_restatement_reproduces_the_full_fixture(golden_dir):
    sizes, sd = synth.HEAD_QUERIES_FULL, synth.head_queries_state_dict(synth.HEAD_QUERIES_FULL)
    step, cases = full_cases(golden_dir)
    for f, bank, want in cases:
        got = restated_queries(sd, bank, sizes)
        assert got["tgt"].shape == (1, 900, 256) and got["temp_pos"].shape == (1, 768, 256) and got["rec_ego_pose"].shape == (1, 900, 4, 4)
        errs = group_errors(got, want, step)
        print(f"[head queries restated, full frame {f}] rel max err { {k: f'{e:.1e}' for k, e in errs.items()} }")
        assert max(errs.values()) <= 1e-5, errs
    g64 = np.load(os.path.join(golden_dir, "head_queries_full_f64.npz"))
    got = restated_queries(sd, cases[1][1], sizes, dtype=torch.float64)
    errs = {k: rel_max(got[k][:, ::step], g64[f"f1_{k}"][:, :got[k][:, ::step].shape[1]]) for k in OUTPUTS}
    print(f"[head queries restated in f64, full frame 1] rel max err vs the reference's f64 run { {k: f'{e:.1e}' for k, e in errs.items()} }")
    assert g64["f1_tgt"].dtype == np.float64 and max(errs.values()) <= 1e-9, errs


def test_state_dict_matches_the_reference(golden_dir):
    spec = json.load(open(os.path.join(golden_dir, "head_queries_state_dict_spec.json")))
    tiny = synth.HEAD_QUERIES_TINY
    for name, kw in (("tiny", tiny), ("tiny_no_ego_pos", dict(tiny, with_ego_pos=False)), ("tiny_np0", dict(tiny, num_propagated=0)), ("full", synth.HEAD_QUERIES_FULL)):
        m = toc3d_amd.HeadQueries(**kw)
        assert {k: list(v.shape) for k, v in m.state_dict().items()} == spec[name], name
        sd = synth.head_queries_state_dict(kw, with_ego_pos=kw.get("with_ego_pos", True))
        m.load_state_dict(sd, strict=True)
    assert len(spec["full"]) == 21 and len(spec["tiny_no_ego_pos"]) == 9 and "pseudo_reference_points.weight" not in spec["full"]
    # under the head's prefix, as a checkpoint carries them
    parent = torch.nn.Module()
    parent.pts_bbox_head = m
    parent.load_state_dict({"pts_bbox_head." + k: v for k, v in sd.items()}, strict=True)


def test_constructor_refusals_and_no_cpu_path():
    for E in (64, 128, 512):
        with pytest.raises(NotImplementedError, match="embed_dims"):
            toc3d_amd.HeadQueries(embed_dims=E)
    with pytest.raises(NotImplementedError, match="precision"):
        toc3d_amd.HeadQueries(precision="fp32x6")
    with pytest.raises(ValueError, match="num_propagated"):
        toc3d_amd.HeadQueries(memory_len=8, num_propagated=9)
    for p in ("bf16", "fp32x3", "fp32"):
        assert toc3d_amd.HeadQueries(precision=p, **synth.HEAD_QUERIES_TINY).precision == p
    m = toc3d_amd.HeadQueries(**synth.HEAD_QUERIES_TINY)
    assert m.precision == "fp32x3" and isinstance(m, toc3d_amd.plan.DerivedState) and m.fresh_builds == 0
    bank = synth.head_queries_bank(synth.HEAD_QUERIES_TINY, 2, 1)
    with pytest.raises(RuntimeError, match="no CPU"):
        m(*(bank[k] for k in BANK))


def test_derived_state_is_dropped_by_new_weights_and_copies():
    import copy
    m = toc3d_amd.HeadQueries(**synth.HEAD_QUERIES_TINY)
    m._packed, m._fresh, m._ws, m._states = {"w": 1}, {"query_pos": torch.zeros(2)}, {(2, 27): {}}, {(2, 27): {}}
    c = copy.deepcopy(m)
    assert c._packed is None and c._fresh is None and c._ws == {} and c._states == {} and c.num_query == 21
    m.load_state_dict(m.state_dict())
    assert m._packed is None and m._fresh is None and m._ws == {} and m._states == {}


def test_fixture_self_checks(golden_dir):
    """What the concatenation promises, on the reference's own outputs: the tails of tgt / query_pos / reference_points continue into temp_* as one sequence of
    memory rows (checked through the restatement's un-concatenated rows), rec_ego_pose is identities, the learned queries' rows do not depend on the frame."""
    cases = tiny_cases(golden_dir)
    eye = torch.eye(4)
    first = {}
    for tag, sizes, ego, bank, want in cases:
        nq, np_, n = sizes["num_query"], sizes["num_propagated"], sizes["memory_len"]
        assert want["tgt"].shape == want["query_pos"].shape == (2, nq + np_, 256) and want["reference_points"].shape == (2, nq + np_, 3)
        assert want["temp_memory"].shape == want["temp_pos"].shape == (2, n - np_, 256) and want["rec_ego_pose"].shape == (2, nq + np_, 4, 4)
        assert bool((want["rec_ego_pose"] == eye).all()), tag
        # the whole sequence of memory rows with nothing split off: its first np rows are the tails, the rest is temp_*
        whole = restated_queries(synth.head_queries_state_dict(sizes, with_ego_pos=ego), bank, dict(sizes, num_propagated=0), with_ego_pos=ego)
        for tail, rest in (("tgt", "temp_memory"), ("query_pos", "temp_pos")):
            joined = torch.cat([want[tail][:, nq:], want[rest]], 1)
            e = rel_max(joined, whole[rest])
            print(f"[head queries fixture {tag}] {tail} tail + {rest} vs the unsplit rows: {e:.1e}")
            assert joined.shape == whole[rest].shape and e <= 1e-5
        pc = torch.tensor(synth.PC_RANGE)
        tref = (bank["memory_reference_point"] - pc[:3]) / (pc[3:] - pc[:3])
        assert torch.equal(want["reference_points"][:, nq:], tref[:, :np_]), tag
        if not ego:
            assert torch.equal(want["tgt"][:, nq:], bank["memory_embedding"][:, :np_]) and torch.equal(want["temp_memory"], bank["memory_embedding"][:, np_:])
            assert not want["tgt"][:, :nq].any()
        key = tag.split("_")[0]
        fresh = {k: want[k][:, :nq] for k in ("tgt", "query_pos", "reference_points")}
        assert all(torch.equal(v[0], v[1]) for v in fresh.values()), "the learned queries' rows are the same for every sample"
        if key in first:
            assert all(torch.equal(fresh[k], first[key][k]) for k in fresh), f"{tag}: the learned queries' rows changed between frames"
        first.setdefault(key, fresh)
    # frame 3 resets sample 1 of the batch; frame 0 is the empty bank
    bank0, bank3 = cases[0][3], cases[2][3]
    assert not bank0["memory_embedding"].any() and not bank3["memory_embedding"][1].any() and bank3["memory_embedding"][0].any()
    assert bank3["memory_timestamp"].dtype == torch.float64 and float(bank3["memory_timestamp"][0].abs().max()) > 0.4
