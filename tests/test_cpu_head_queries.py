"""CPU: the query side of the head (toc3d_amd.HeadQueries) -- a plain-torch restatement of StreamPETRHead.forward :641-652 with temporal_alignment :424-453
(tests/head_queries_cases.py) reproduces the REAL reference's fixtures (tests/golden/head_queries_*.npz, written by tools/gen_golden_head_queries.py); the module's state dict equals the
reference's; the fixtures satisfy what the concatenation promises.  The restatement is the GPU tests' control where the reference is absent.

Every test prints the figures it asserts on (run with -s)."""
import json
import os

import numpy as np
import pytest
import torch

import toc3d_amd
from head_queries_cases import BANK, OUTPUTS, full_cases, group_errors, restated_queries, tiny_cases
from support import rel_max_zero_ok
from toc3d_amd import synth


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
    errs = {k: rel_max_zero_ok(got[k][:, ::step], g64[f"f1_{k}"][:, :got[k][:, ::step].shape[1]]) for k in OUTPUTS}
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
            e = rel_max_zero_ok(joined, whole[rest])
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
