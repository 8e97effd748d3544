"""CPU: the assignment side header (include/toc3d_assign.h) against lib's row, the entry point's refusals (all before any launch), the numpy restatement of
tests/tracking_hungarian_cases.py against the fixture made from the reference's PubTracker(hungarian=True) -- every integer, the solver's scan rounds and every bit
of the tracks held --, the restated solver against scipy's where scipy imports, what the fixture's frames are witnesses of, the host classes and the detector's
keyword."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import detector_cases as DC
import tracking_cases as TC
import tracking_hungarian_cases as HC
import toc3d_amd
from support import A, ERR_ARG, header_sigs, raw_call
from toc3d_amd import lib, tracking

ENTRY = "toc3d_tracks_step_hungarian"


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------------------------------------
def test_assign_header_constants_exports_and_makefile():
    raw = open(lib.ASSIGN_HEADER_PATH).read()
    txt = lib.header_text(lib.ASSIGN_HEADER_PATH)
    assert header_sigs(txt, lib._ASSIGN_SIGS) == lib._ASSIGN_SIGS and list(lib._ASSIGN_SIGS) == [ENTRY]
    assert lib._ASSIGN_SIGS[ENTRY] == lib._TRACKS_SIGS["toc3d_tracks_step"][:-1] + "pp", "the greedy step's arguments, rounds, the stream"
    define = lambda n: int(re.search(rf"#define\s+{n}\s+(\d+)", raw).group(1))
    assert define("TOC3D_ASSIGN_ABI") == lib.ASSIGN_ABI == 1
    assert (define("TOC3D_ASSIGN_MAX_BOXES"), define("TOC3D_ASSIGN_MAX_TRACKS")) == (lib.ASSIGN_MAX_BOXES, lib.ASSIGN_MAX_TRACKS) == (HC.MAX_BOXES, HC.MAX_TRACKS) == (512, 2048)
    assert lib.ASSIGN_MAX_TRACKS >= 300 * 4, "the shipped max_num at max_age 3"
    for cited in ("pub_tracker.py:27", "pub_test.py:28,81", ":127-129", ":143-150", ":126-128", ":145-149", ":162-168", ":172-183", "QUIRK A", "QUIRK B", "607 of 3000",
                  "LAST position", "FIRST position", "no inline assembly"):
        assert cited in raw, f"the header cites {cited}"
    dll = ctypes.CDLL(lib.LIB_PATH)
    dll.toc3d_assign_abi.restype = ctypes.c_int
    assert dll.toc3d_assign_abi() == 1 and hasattr(dll, ENTRY)
    assert lib.TRACKS_ABI == 1 and list(lib._TRACKS_SIGS) == ["toc3d_tracks_state_bytes", "toc3d_tracks_step"], "the greedy header stays where it is"
    assert lib.SIDES["assign"] == (lib.ASSIGN_HEADER_PATH, "toc3d_assign_abi", 1, lib._ASSIGN_SIGS)
    csrc = os.path.join(os.path.dirname(lib.LIB_PATH), "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert " tracking_hungarian.hip " in mk and "$(BUILD)/tracking_hungarian.hip.o: ../../include/toc3d_assign.h" in mk
    assert "$(BUILD)/tracking.hip.o $(BUILD)/tracking_hungarian.hip.o: tracks_steps.h" in mk
    src = open(os.path.join(csrc, "tracking_hungarian.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "atomic" not in src.lower() and "asm" not in src and "while (" not in src, "once-rounded arithmetic, bounded loops"
    assert src.index("#pragma clang fp contract(off)") < src.index('#include "tracks_steps.h"'), "the shared steps are compiled under the pragma"
    assert '#include "tracks_steps.h"' in open(os.path.join(csrc, "tracking.hip")).read()


def entry_args(**o):
    a = dict(rec=A, score=A, name=A, kept=A, B=2, K=300, label=A, ncls=10, gate=A, nl=7, thr=0.25, max_age=3, ts=A, first=A, sin=A, sout=A + 0x100000, cap=1200, track_id=A,
             active=A, order=A, num_out=A, rounds=A)
    a.update(o)
    return tuple(a[k] for k in ("rec", "score", "name", "kept", "B", "K", "label", "ncls", "gate", "nl", "thr", "max_age", "ts", "first", "sin", "sout", "cap", "track_id",
                                "active", "order", "num_out", "rounds")) + (None,)


POINTERS = ("rec", "score", "name", "kept", "label", "gate", "ts", "first", "sin", "sout", "track_id", "active", "order", "num_out", "rounds")


@pytest.mark.parametrize("over,reason", [
    *[({p: None}, "null buffer") for p in POINTERS],
    (dict(K=513, cap=2048, max_age=0), "K at most 512, TOC3D_ASSIGN_MAX_BOXES"), (dict(K=2048, cap=8192, max_age=0), "K at most 512"), (dict(cap=2049), "bad capacity (at most 2048"),
    (dict(cap=8192), "bad capacity (at most 2048"), (dict(cap=-1), "bad capacity"), (dict(K=512, cap=2047), "capacity >= K * (max_age + 1)"),
    (dict(K=512, cap=2048, max_age=4), "capacity >= K * (max_age + 1)"), (dict(cap=1199), "capacity >= K * (max_age + 1)"),
    (dict(max_age=2 ** 63 - 1, cap=2048), "capacity >= K * (max_age + 1)"),
    (dict(B=-1), "must not be negative"), (dict(K=-1), "must not be negative"), (dict(B=65536), "at most 65535"), (dict(max_age=-1), "bad max_age"),
    (dict(ncls=0), "bad num_classes"), (dict(ncls=65), "bad num_classes"), (dict(nl=0), "bad num_track_labels"), (dict(nl=65), "bad num_track_labels"),
    (dict(thr=float("nan")), "bad score_thr"), (dict(thr=float("inf")), "bad score_thr"),
    (dict(rec=A + 4), "8-byte boundary"), (dict(ts=A + 4), "8-byte boundary"), (dict(sin=A + 4), "8-byte boundary"), (dict(sout=A + 0x100004), "8-byte boundary"),
    (dict(sout=A), "overlap"), (dict(sout=A + 8), "overlap"), (dict(sin=A + 0x100000, sout=A + 0x100000 + 2 * (32 + 48 * 1200) - 8), "overlap"),
    ({}, "host pointer"), (dict(K=512, cap=2048), "host pointer"), (dict(K=0, cap=0, rec=None, score=None, name=None, track_id=None, active=None, order=None), "host pointer"),
])
def test_entry_point_refusals(over, reason):
    rc, msg = raw_call(lib._ASSIGN_SIGS, ENTRY, entry_args(**over))
    print(f"{over}: rc {rc}, {msg!r}")
    assert rc == ERR_ARG and msg.startswith(ENTRY + ":") and reason in msg, (rc, msg)


def test_no_stream_is_legal_and_host_buffers_are_left_alone():
    for over in (dict(B=0), dict(B=0, **{p: None for p in POINTERS}), dict(B=0, K=0, cap=0)):
        rc, msg = raw_call(lib._ASSIGN_SIGS, ENTRY, entry_args(**over))
        assert rc == 0, (over, rc, msg)
    p = ctypes.addressof
    rec, score, name, kept = (ctypes.c_double * 24)(*([1.0] * 24)), (ctypes.c_float * 2)(0.9, 0.8), (ctypes.c_int32 * 2)(0, 0), (ctypes.c_int64 * 1)(2)
    label, gate = (ctypes.c_int32 * 10)(*TC.track_label_table().tolist()), (ctypes.c_float * 7)(*([2.5] * 7))
    ts, first = (ctypes.c_double * 1)(1.0), (ctypes.c_int32 * 1)(1)
    n = tracking.state_bytes(8)
    sin, sout = (ctypes.c_uint8 * n)(*([7] * n)), (ctypes.c_uint8 * n)(*([7] * n))
    track_id, active, order = ((ctypes.c_int32 * 2)(7, 7) for _ in range(3))
    num_out, rounds = (ctypes.c_int64 * 1)(7), (ctypes.c_int32 * 1)(7)
    rc, msg = raw_call(lib._ASSIGN_SIGS, ENTRY, entry_args(rec=p(rec), score=p(score), name=p(name), kept=p(kept), B=1, K=2, label=p(label), gate=p(gate), ts=p(ts), first=p(first),
                                                            sin=p(sin), sout=p(sout), cap=8, track_id=p(track_id), active=p(active), order=p(order), num_out=p(num_out), rounds=p(rounds)))
    assert rc == ERR_ARG and "host pointer" in msg
    assert bytes(sout) == bytes([7] * n) == bytes(sin) and list(track_id) == list(active) == list(order) == [7, 7] and list(num_out) == [7] == list(rounds)


# ---- the restatement and the fixture ---------------------------------------------------------------------------------------------------------------------------------
def test_fixture_says_what_made_it_and_is_small():
    z = np.load(HC.FIXTURE)
    by = str(z["generated_by"])
    assert "pub_tracker.PubTracker(hungarian=True)" in by and str(z["scipy_version"]) in by and re.fullmatch(r"\d+\.\d+\.\d+.*", str(z["scipy_version"]))
    assert os.path.getsize(HC.FIXTURE) < 1 << 20
    assert set(n.split("/")[0] for n in z.files) == set(HC.CASES) | {"generated_by", "scipy_version"}


@pytest.mark.parametrize("name", HC.CASES)
def test_restatement_equals_the_reference(name):
    c, e = HC.build_case(name), HC.expected(name)
    outs, states = HC.run_case(c)
    assert e["order"].shape == (len(c["frames"]), c["B"], c["K"]) and e["rounds"].shape == e["num_out"].shape and e["flags"].shape == e["num_out"].shape + (len(HC.FLAGS),)
    for f in range(len(outs)):
        for b in range(c["B"]):
            for k in ("track_id", "active", "order"):
                assert np.array_equal(outs[f][b][k], e[k][f, b]), f"{name}, frame {f}, stream {b}: {k}"
            assert outs[f][b]["num_out"] == e["num_out"][f, b] and outs[f][b]["rounds"] == e["rounds"][f, b], f"{name}, frame {f}, stream {b}: num_out, rounds"
            HC.compare_state(f"{name}, frame {f}, stream {b}", states[f][b], e, f, b)
    print(f"{name}: shown {e['num_out'].tolist()}, held {e['count'].tolist()}, rounds {e['rounds'].tolist()}: every integer and every bit of the tracks equal the reference's")


def test_restated_solver_equals_scipy_on_seeded_matrices():
    """3000 tracker-shaped matrices, rectangular both ways, with duplicate positions and positions on a grid (exact ties): the same row and column indices."""
    lsa = pytest.importorskip("scipy.optimize").linear_sum_assignment
    rng = np.random.default_rng(2025)
    absorbed = 0
    for k in range(3000):
        N, M = rng.integers(2, 30, 2)
        nl = int(rng.integers(1, 4))
        p, q = rng.uniform(0, 9, (N, 2)).astype(np.float32), rng.uniform(0, 9, (M, 2)).astype(np.float32)
        if k % 3 == 0:
            q[:M // 2] = q[M // 2:2 * (M // 2)]
        if k % 5 == 0:
            p, q = np.round(p), np.round(q)
        dl, tl = rng.integers(0, nl, N).astype(np.int32), rng.integers(0, nl, M).astype(np.int32)
        cost, valid = HC.cost_matrix(p, q, dl, tl, TC.max_diff_table())
        a, t = lsa(cost)
        d, j, rounds = HC.solve(cost)
        assert np.array_equal(a, d) and np.array_equal(t, j) and min(N, M) <= rounds <= min(N, M) * (min(N, M) + 1) // 2, f"matrix {k} ({N} x {M})"
        a, t = lsa(np.where(valid, cost, HC.CLEAN_INVALID))
        absorbed += {(x, y) for x, y in zip(d, j) if valid[x, y]} != {(x, y) for x, y in zip(a, t) if valid[x, y]}
    print(f"3000 of 3000 matrices: the restated solver's indices are scipy's; on {absorbed} the valid matches differ from an uncontaminated solve's")
    assert absorbed > 100, "the absorption at 1e18 decides matches often"


def test_cases_cover_what_they_are_named_for():
    e = {n: HC.expected(n) for n in HC.CASES}
    flags = {flag: sum(int(e[n]["flags"][:, :, k].sum()) for n in HC.CASES) for k, flag in enumerate(HC.FLAGS)}
    print(f"frames that are witnesses: {flags}")
    assert flags["differs_from_greedy"] >= 8 and flags["differs_from_clean"] >= 8 and flags["quirk_b"] >= 4 and flags["quirk_a"] >= 4 and flags["ties"] >= 4
    b = e["quirk_b"]
    assert b["track_id"][1, 0, :3].tolist() == [4, 2, 3] and b["order"][1, 0, :3].tolist() == [1, 2, 0], \
        "one track (id 1), detections at 10, 20 and 30 m: the first is parked on the track and numbered last -- ids 4, 2, 3 in row order, where greedy gives 2, 3, 4"
    assert TC.expected("tie_dets")["num_out"].shape == e["tie_dets"]["num_out"].shape
    a = e["quirk_a"]
    assert a["count"][1, 0] == 2 and a["states"][1][0]["tracking_id"].tolist() == [1, 3], "the second track, parked with the far detection, is gone at age 1 of max_age 3"
    greedy = TC.Tracker(3)
    c = HC.build_case("quirk_a")
    for fr in c["frames"][:2]:
        greedy.step(fr["rec"][0], fr["score"][0], fr["name"][0], fr["kept"][0], fr["timestamp"][0], fr["first"][0], c["thr"])
    assert greedy.state["tracking_id"].tolist() == [1, 3, 2] and greedy.state["age"].tolist() == [1, 1, 2], "greedy keeps track 2 with age 2"
    assert e["first_frame_n1"]["rounds"].sum() == 0 and e["kept_zero"]["num_out"][0, 0] == 0 and e["empty_twice_age3"]["num_out"][1:3, 0].tolist() == [0, 0]
    assert e["all_invalid"]["rounds"][1:, 0].tolist() == [3, 3, 2] and (e["all_invalid"]["active"][1:] <= 1).all(), "every pair invalid: every row parked, nothing continued"
    assert e["counts_1_2"]["rounds"][:, 0].tolist() == [0, 1, 1, 2, 1, 1]
    shapes = set()
    for n in HC.CASES:
        c = HC.build_case(n)
        if c.get("init") is not None:
            shapes.add((int(e[n]["num_out"][0, 0]), len(c["init"][0]["label"])))
    P = HC.PASS
    want = {(40, 63), (40, 64), (40, 65), (63, 40), (64, 40), (65, 40), (100, P - 1), (100, P), (100, P + 1), (P - 1, 100), (P, 100), (P + 1, 100), (128, 128), (512, 2048)}
    assert want <= shapes, f"N x M of the given states: {sorted(want - shapes)} missing"
    caps = HC.build_case(HC.CAPS_CASE)
    assert set(caps["init"][0]["label"].tolist()) == {0} and e[HC.CAPS_CASE]["rounds"][0, 0] == 647 and e[HC.CAPS_CASE]["count"][0, 0] <= HC.MAX_TRACKS
    assert len(set(HC.build_case("n100_m256")["init"][0]["label"].tolist())) == 7
    s3 = HC.build_case(HC.STREAMS_CASE)
    assert len({tuple(fr["first"][b] for fr in s3["frames"]) for b in range(3)}) == 3, "the streams reset on different frames"


# ---- the classes -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_build_tracker_and_the_caps():
    with pytest.raises(NotImplementedError, match="greedy assignment .* is the path built"):
        toc3d_amd.PubTracker(hungarian=True)
    g = toc3d_amd.build_tracker()
    assert type(g) is toc3d_amd.PubTracker and (g.hungarian, g.max_age, g.num_streams) == (False, 0, 1)
    g = toc3d_amd.build_tracker(False, 3, num_streams=2)
    assert type(g) is toc3d_amd.PubTracker and (g.max_age, g.num_streams) == (3, 2)
    h = toc3d_amd.build_tracker(hungarian=True, max_age=3, num_streams=2, class_names=("pedestrian", "car"), tracking_names=("car", "pedestrian"))
    assert type(h) is toc3d_amd.HungarianPubTracker and isinstance(h, toc3d_amd.PubTracker) and h.hungarian is True and (h.max_age, h.num_streams, h.track_label) == (3, 2, (1, 0))
    assert toc3d_amd.HungarianPubTracker is tracking.HungarianPubTracker and {"HungarianPubTracker", "build_tracker"} <= set(toc3d_amd.__all__)
    assert h._ENTRY == ENTRY and toc3d_amd.PubTracker._ENTRY == "toc3d_tracks_step"
    for name in ("step", "records_to_annos", "track_file", "reset", "_ensure_state", "tracks", "pack_annos"):
        assert getattr(toc3d_amd.HungarianPubTracker, name) is getattr(toc3d_amd.PubTracker, name), f"{name} is inherited"
    with pytest.raises(ValueError, match="max_age"):
        toc3d_amd.build_tracker(hungarian=True, max_age=-1)
    with pytest.raises(ValueError, match="512 rows a stream with max_age 4 need 2560 tracks, more than 2048 \\(TOC3D_ASSIGN_MAX_TRACKS\\)"):
        toc3d_amd.build_tracker(hungarian=True, max_age=4)._ensure_state(512, torch.device("cpu"))
    h = toc3d_amd.build_tracker(hungarian=True, max_age=3)
    h._ensure_state(512, torch.device("cpu"))
    assert h.capacity == 2048
    with pytest.raises(RuntimeError, match="the HIP extension is the only compute path"):
        h.step_fixed(torch.zeros(1, 4, 12, dtype=torch.float64), torch.zeros(1, 4), torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1, dtype=torch.int64), [0.0])


def restated(tracker):
    return TC.restated(tracker, HC.Tracker)


def test_step_on_the_restatement():
    name = "quirk_b"
    c, e = HC.build_case(name), HC.expected(name)
    trk = restated(toc3d_amd.build_tracker(hungarian=True, max_age=c["max_age"]))
    for f, fr in enumerate(c["frames"]):
        annos = [dict(translation=fr["rec"][0, i, 0:3].tolist(), size=fr["rec"][0, i, 3:6].tolist(), rotation=fr["rec"][0, i, 6:10].tolist(), velocity=fr["rec"][0, i, 10:12].tolist(),
                      detection_name=TC.CLASS_NAMES[int(fr["name"][0, i])], detection_score=float(fr["score"][0, i])) for i in range(int(fr["kept"][0]))]
        items = trk.step([annos], [float(fr["timestamp"][0])], [bool(fr["first"][0])], c["thr"])[0]
        rows = e["order"][f, 0, :int(e["num_out"][f, 0])].tolist()
        assert [x["tracking_id"] for x in items] == e["track_id"][f, 0, rows].tolist() and [x["active"] for x in items] == e["active"][f, 0, rows].tolist()


# ---- the detector's keyword ------------------------------------------------------------------------------------------------------------------------------------------
class FakeResults:
    """Three trucks a frame: the first moves a metre, the other two are far from every track in the second frame."""
    class_names = TC.CLASS_NAMES
    xs = [[0.0, 200.0, 300.0], [1.0, 20.0, 30.0]]

    def __init__(self):
        self.results, self.calls = {}, 0

    def format_device(self, bbox_list, poses, tokens):
        B = len(bbox_list)
        rec = torch.zeros(B, 3, 12, dtype=torch.float64)
        rec[:, :, 0] = torch.tensor(self.xs[min(self.calls, 1)], dtype=torch.float64)
        self.calls += 1
        fixed = dict(rec=rec, score=torch.full((B, 3), 0.5), name=torch.full((B, 3), TC.TRUCK, dtype=torch.int32), kept=torch.full((B,), 3, dtype=torch.int64))
        return fixed, [[dict(sample_token=t)] for t in tokens]

    def format(self, bbox_list, poses, tokens):
        return self.format_device(bbox_list, poses, tokens)[1]

    def add(self, token, annos):
        self.results[token] = annos


class FakeHungarian:
    """In place of HungarianPubTracker in the detector: records what it is built with and handed, and answers with the restatement."""
    def __init__(self, num_streams=1, **kw):
        self.num_streams, self.kw, self.calls = num_streams, kw, []
        self.inner = restated(toc3d_amd.build_tracker(hungarian=True, num_streams=num_streams, **kw))

    def step_fixed(self, rec, score, name, kept, timestamps, first, thr):
        self.calls.append((timestamps.tolist(), list(first), thr))
        out = self.inner._step_host(rec.numpy(), score.numpy(), name.numpy(), kept.numpy(), timestamps.tolist(), first, thr)
        return {k: torch.from_numpy(np.asarray(v)) for k, v in out.items()}

    def records_to_annos(self, *a):
        return self.inner.records_to_annos(*a)


def test_enable_tracking_hungarian_builds_through_build_tracker(monkeypatch):
    from toc3d_amd import detector as D
    det = DC.fake_detector()
    det.enable_nusc_results()
    assert type(det.enable_tracking().tracker) is toc3d_amd.PubTracker and det.tracker.max_age == 3
    assert type(det.enable_tracking(hungarian=True, max_age=2).tracker) is toc3d_amd.HungarianPubTracker and det.tracker.max_age == 2
    monkeypatch.setattr(D, "HungarianPubTracker", FakeHungarian)
    assert det.enable_tracking(max_age=0, score_threshold=0.3, hungarian=True) is det
    assert isinstance(det.tracker, FakeHungarian) and det.tracker.kw == dict(max_age=0, class_names=TC.CLASS_NAMES), "hungarian chooses the class and is not handed on"
    det.nusc_results = FakeResults()
    DC.frame(det, [DC.posed_meta("t0")], 100.0)
    DC.frame(det, [DC.posed_meta("t1")], 100.5)
    assert det.tracker.calls == [([100.0], [True], 0.3), ([100.5], [False], 0.3)]
    assert [a["tracking_id"] for a in det.tracking_results["t1"]] == ["1", "4", "5"], "the first truck continued; those at 20 and 30 m are parked on the other two tracks and numbered anew"
    # another number of streams: the second place the detector builds a tracker, through build_tracker again
    DC.frame(det, [DC.posed_meta("u0"), DC.posed_meta("v0")], 200.0)
    assert isinstance(det.tracker, FakeHungarian) and det.tracker.num_streams == 2 and det.tracker.kw == dict(max_age=0, class_names=TC.CLASS_NAMES)
