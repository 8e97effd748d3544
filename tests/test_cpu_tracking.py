"""CPU: the tracking side header against lib's row, the entry point's refusals (all before any launch), the numpy restatement of tests/tracking_cases.py against
the fixture made from the reference's PubTracker -- every integer and every bit of the tracks held -- the near-tie rows the fixture stores, the host class
(constructor, capacity arithmetic, records, track_file with the device step replaced by the restatement) and the detector's hook."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import detector_cases as DC
import tracking_cases as TC
import toc3d_amd
from support import A, ERR_ARG, header_sigs, raw_call
from toc3d_amd import lib, tracking
from tracking_cases import case_annos, restated

ENTRY = "toc3d_tracks_step"


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------------------------------------
def test_tracks_header_constants_exports_and_makefile():
    raw = open(lib.TRACKS_HEADER_PATH).read()
    txt = lib.header_text(lib.TRACKS_HEADER_PATH)
    assert header_sigs(txt, lib._TRACKS_SIGS) == lib._TRACKS_SIGS and list(lib._TRACKS_SIGS) == ["toc3d_tracks_state_bytes", ENTRY]
    define = lambda n: int(re.search(rf"#define\s+{n}\s+(\d+)", raw).group(1))
    assert define("TOC3D_TRACKS_ABI") == lib.TRACKS_ABI == 1
    assert (define("TOC3D_TRACKS_MAX_TRACKS"), define("TOC3D_TRACKS_MAX_BOXES"), define("TOC3D_TRACKS_MAX_CLASSES"), define("TOC3D_TRACKS_REC")) == (8192, 2048, 64, 12)
    assert (lib.TRACKS_MAX_TRACKS, lib.TRACKS_MAX_BOXES, lib.TRACKS_MAX_CLASSES, lib.TRACKS_REC) == (8192, 2048, 64, 12)
    assert (define("TOC3D_TRACKS_HEADER_BYTES"), define("TOC3D_TRACKS_ROW_BYTES")) == (lib.TRACKS_HEADER_BYTES, lib.TRACKS_ROW_BYTES) == (32, 48)
    assert (TC.HEADER_BYTES, TC.state_bytes(1) - TC.HEADER_BYTES) == (lib.TRACKS_HEADER_BYTES, lib.TRACKS_ROW_BYTES), "the state's bytes as tests/tracking_cases.py lays them out"
    assert (lib.TRACKS_MAX_BOXES, lib.TRACKS_MAX_CLASSES, lib.TRACKS_REC) == (lib.RESULTS_MAX_BOXES, lib.RESULTS_MAX_CLASSES, lib.RESULTS_REC), "the records' own limits"
    for cited in ("pub_tracker.py:26-186", "track_utils.py:3-12", "pub_test.py:77-153", "pub_test.py:101-105", "pub_test.py:107-108", ":62-72", ":103-116", ":119-124",
                  "track_utils.py:7-11", ":155-160", ":162-168", ":172-183", ":42-59", ":81-98", "EMPTY-FRAME QUIRK", "No atomics", "no inline assembly"):
        assert cited in raw, f"the header cites {cited}"
    dll = ctypes.CDLL(lib.LIB_PATH)
    dll.toc3d_tracks_abi.restype = ctypes.c_int
    assert dll.toc3d_tracks_abi() == 1 and hasattr(dll, ENTRY)
    assert lib.ABI_VERSION == 11 and lib.ABI_MINOR == 1, "the 11.1 surface stays where it is"
    assert "toc3d_tracks" not in open(lib.HEADER_PATH).read()
    mk = open(os.path.join(os.path.dirname(lib.LIB_PATH), "csrc", "Makefile")).read()
    assert " tracking.hip " in mk and "$(BUILD)/tracking.hip.o: ../../include/toc3d_tracks.h" in mk
    src = open(os.path.join(os.path.dirname(lib.LIB_PATH), "csrc", "tracking.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "atomic" not in src.lower() and "asm" not in src


def test_exports():
    assert toc3d_amd.PubTracker is tracking.PubTracker and "PubTracker" in toc3d_amd.__all__
    assert all(hasattr(toc3d_amd.Petr3D, m) for m in ("enable_tracking", "disable_tracking", "dump_tracking"))
    assert tracking.NUSCENES_TRACKING_NAMES == TC.TRACKING_NAMES and set(tracking.NUSCENE_CLS_VELOCITY_ERROR.values()) == {TC.MAX_DIFF}
    assert hasattr(toc3d_amd.NuScenesResults, "format_device")


def entry_args(**o):
    a = dict(rec=A, score=A, name=A, kept=A, B=2, K=300, label=A, ncls=10, gate=A, nl=7, thr=0.25, max_age=3, ts=A, first=A, sin=A, sout=A + 0x100000, cap=1200, track_id=A,
             active=A, order=A, num_out=A)
    a.update(o)
    return tuple(a[k] for k in ("rec", "score", "name", "kept", "B", "K", "label", "ncls", "gate", "nl", "thr", "max_age", "ts", "first", "sin", "sout", "cap", "track_id",
                                "active", "order", "num_out")) + (None,)


POINTERS = ("rec", "score", "name", "kept", "label", "gate", "ts", "first", "sin", "sout", "track_id", "active", "order", "num_out")


@pytest.mark.parametrize("over,reason", [
    *[({p: None}, "null buffer") for p in POINTERS],
    (dict(B=-1), "must not be negative"), (dict(K=-1), "must not be negative"), (dict(K=2049, cap=8192, max_age=0), "at most 2048"), (dict(B=65536), "at most 65535"),
    (dict(max_age=-1), "bad max_age"), (dict(cap=8193), "bad capacity"), (dict(cap=-1), "bad capacity"), (dict(cap=1199), "capacity >= K * (max_age + 1)"),
    (dict(K=2048, cap=8191), "capacity >= K * (max_age + 1)"), (dict(K=2048, cap=8192, max_age=4), "capacity >= K * (max_age + 1)"),
    (dict(max_age=2 ** 62, cap=8192), "capacity >= K * (max_age + 1)"), (dict(max_age=2 ** 63 - 1, cap=8192), "capacity >= K * (max_age + 1)"),
    (dict(ncls=0), "bad num_classes"), (dict(ncls=65), "bad num_classes"), (dict(nl=0), "bad num_track_labels"), (dict(nl=65), "bad num_track_labels"),
    (dict(thr=float("nan")), "bad score_thr"), (dict(thr=float("-inf")), "bad score_thr"),
    (dict(rec=A + 4), "8-byte boundary"), (dict(ts=A + 4), "8-byte boundary"), (dict(sin=A + 4), "8-byte boundary"), (dict(sout=A + 0x100004), "8-byte boundary"),
    (dict(sout=A), "overlap"), (dict(sout=A + 8), "overlap"), (dict(sin=A + 0x100000, sout=A + 0x100000 + 2 * (32 + 48 * 1200) - 8), "overlap"),
    ({}, "host pointer"), (dict(K=2048, cap=8192), "host pointer"), (dict(K=0, cap=0, rec=None, score=None, name=None, track_id=None, active=None, order=None), "host pointer"),
    (dict(B=65535, ncls=64, nl=64, max_age=0, cap=300, sout=A + 0x40000000), "host pointer"),
])
def test_entry_point_refusals(over, reason):
    rc, msg = raw_call(lib._TRACKS_SIGS, ENTRY, entry_args(**over))
    print(f"{over}: rc {rc}, {msg!r}")
    assert rc == ERR_ARG and msg.startswith(ENTRY + ":") and reason in msg, (rc, msg)


def test_no_stream_is_legal_and_state_bytes():
    """B == 0: nothing is launched, no pointer is looked at, and the call succeeds."""
    for over in (dict(B=0), dict(B=0, **{p: None for p in POINTERS}), dict(B=0, K=0, cap=0)):
        rc, msg = raw_call(lib._TRACKS_SIGS, ENTRY, entry_args(**over))
        assert rc == 0, (over, rc, msg)
    for cap in (0, 1, 300, 1200, 8192):
        assert tracking.library_state_bytes(cap) == tracking.state_bytes(cap) == 32 + 48 * cap
    for cap in (-1, 8193):
        with pytest.raises(RuntimeError, match="bad capacity"):
            tracking.library_state_bytes(cap)
    rc, msg = raw_call(lib._TRACKS_SIGS, "toc3d_tracks_state_bytes", (4, None))
    assert rc == ERR_ARG and "null buffer" in msg


def test_real_host_buffers_are_refused_and_left_alone():
    p = ctypes.addressof
    B, K, cap = 1, 2, 8
    rec, score, name, kept = (ctypes.c_double * 24)(*([1.0] * 24)), (ctypes.c_float * 2)(0.9, 0.8), (ctypes.c_int32 * 2)(0, 0), (ctypes.c_int64 * 1)(2)
    label, gate = (ctypes.c_int32 * 10)(*TC.track_label_table().tolist()), (ctypes.c_float * 7)(*([2.5] * 7))
    ts, first = (ctypes.c_double * 1)(1.0), (ctypes.c_int32 * 1)(1)
    n = tracking.state_bytes(cap)
    sin, sout = (ctypes.c_uint8 * n)(*([7] * n)), (ctypes.c_uint8 * n)(*([7] * n))
    track_id, active, order = ((ctypes.c_int32 * 2)(7, 7) for _ in range(3))
    num_out = (ctypes.c_int64 * 1)(7)
    rc, msg = raw_call(lib._TRACKS_SIGS, ENTRY, entry_args(rec=p(rec), score=p(score), name=p(name), kept=p(kept), B=B, K=K, label=p(label), gate=p(gate), ts=p(ts), first=p(first),
                                                            sin=p(sin), sout=p(sout), cap=cap, track_id=p(track_id), active=p(active), order=p(order), num_out=p(num_out)))
    print(f"rc {rc}, {msg!r}")
    assert rc == ERR_ARG and "host pointer" in msg
    assert bytes(sout) == bytes([7] * n) == bytes(sin) and list(track_id) == list(active) == list(order) == [7, 7] and list(num_out) == [7]


# ---- the restatement and the fixture ---------------------------------------------------------------------------------------------------------------------------------
def test_fixture_says_what_made_it_and_is_small():
    z = np.load(TC.FIXTURE)
    assert "pub_tracker.PubTracker" in str(z["generated_by"]) and os.path.getsize(TC.FIXTURE) < 1 << 20
    assert set(n.split("/")[0] for n in z.files) == set(TC.CASES) | {"generated_by", "near_choice", "near_gate"}
    TC.check_near_ties(z["near_choice"], z["near_gate"])
    print(f"{len(z['near_choice'])} stored detections whose match a fused multiply-add would change, {len(z['near_gate'])} whose 2.5 m gate it would change")


@pytest.mark.parametrize("name", TC.CASES)
def test_restatement_equals_the_reference(name):
    c, e = TC.build_case(name), TC.expected(name)
    outs, states = TC.run_case(c)
    assert e["order"].shape == (len(c["frames"]), c["B"], c["K"])
    for f in range(len(outs)):
        for b in range(c["B"]):
            for k in ("track_id", "active", "order"):
                assert np.array_equal(outs[f][b][k], e[k][f, b]), f"{name}, frame {f}, stream {b}: {k}"
            assert outs[f][b]["num_out"] == e["num_out"][f, b]
            TC.compare_state(f"{name}, frame {f}, stream {b}", states[f][b], e, f, b)
    print(f"{name}: shown {e['num_out'].tolist()}, held {e['count'].tolist()}: every integer and every bit of the tracks equal the reference's")


def test_cases_cover_what_they_are_named_for():
    e = {n: TC.expected(n) for n in TC.CASES}
    assert e["first_frame_n1"]["num_out"][0, 0] == 1 and e["kept_zero"]["count"][0, 0] == 0
    for n, age in (("empty_twice_age0", 0), ("empty_twice_age3", 3)):
        assert e[n]["num_out"][1:3, 0].tolist() == [0, 0] and (e[n]["count"][0:3, 0] == e[n]["count"][0, 0]).all(), "two empty frames drop nothing"
        ids = e[n]["track_id"][3, 0]
        assert ((ids > 0) & (ids <= e[n]["id_count"][0, 0])).any(), f"{n}: a track kept over the empty frames matches on the next"
    st = e["empty_twice_age0"]["states"]
    assert (st[2][0]["age"] >= 0).all() and np.array_equal(st[2][0]["ct"], st[0][0]["ct"]), "max_age 0: the old tracks are left untouched by the empty frames"
    old = TC.expected("empty_thrice_age1")
    assert old["num_out"][1:4, 0].tolist() == [0, 0, 0] and old["active"][4, 0].max() >= 2, "tracks at age >= max_age match after the empty frames"
    for n, k in (("n63_age0", 63), ("n64_age0", 64), ("n65_age0", 65), ("n256_age0", 256), ("n257_one_label_age0", 257)):
        assert (e[n]["num_out"] == k).all() and (e[n]["count"] == k).all(), f"{n}: N = M = K"
    assert (e["large_one_label"]["num_out"] == 2048).all() and len(TC.build_case("large_one_label")["init"][0]["label"]) == 8192
    assert set(TC.build_case("large_one_label")["init"][0]["label"].tolist()) == {0} and len(set(TC.build_case("large_spread")["init"][0]["label"].tolist())) == 7
    g = e["gate_and_labels"]
    assert g["track_id"][1, 0, :6].tolist() == [1, 5, 6, 7, 0, 4], "d == 2.5 matches; the float above does not; another label at the same place does not; a cone is not tracked"
    t = e["tie_tracks"]
    assert t["track_id"][1, 0, 0] == 1 and t["track_id"][2, 0, :3].tolist() == [1, 2, 3], "two tracks at one place: the lower index first"
    d = e["tie_dets"]
    assert d["track_id"][1, 0, :2].tolist() == [1, 2] and d["order"][1, 0, :2].tolist() == [0, 1], "two detections equidistant: the earlier one takes the track"
    for n in ("score_at_f32_thr", "score_at_f64_thr"):
        assert e[n]["num_out"][0, 0] == 1 and e[n]["active"][0, 0, :2].tolist() == [1, 0], f"{n}: at the threshold kept, one float below dropped"
    s3 = TC.build_case(TC.STREAMS_CASE)
    assert len({tuple(fr["first"][b] for fr in s3["frames"]) for b in range(3)}) == 3, "the streams reset on different frames"


def test_near_tie_rows_decide_differently_under_contraction():
    """What the near-tie case is for: with sqrt(fma(dx, dx, dy * dy)) in place of the once-rounded distance, its detections take other tracks."""
    z = np.load(TC.FIXTURE)
    e = TC.expected(TC.NEAR_TIES)
    nc, ng = len(z["near_choice"]), len(z["near_gate"])
    ids = e["track_id"][1, 0]
    for k, r in enumerate(z["near_choice"]):
        once = [TC.d_once(r[2 + 2 * j], r[3 + 2 * j], r[0], r[1]) for j in (0, 1)]
        fused = [TC.d_fused(r[2 + 2 * j], r[3 + 2 * j], r[0], r[1]) for j in (0, 1)]
        want = 2 * k + (1 if once[0] <= once[1] else 2)
        other = 2 * k + (1 if fused[0] <= fused[1] else 2)
        assert ids[k] == want != other, f"choice row {k}: the reference took track {ids[k]}, the once-rounded distance says {want}, the fused one {other}"
    for k, r in enumerate(z["near_gate"]):
        inside = TC.d_once(r[2], r[3], r[0], r[1]) <= np.float32(2.5)
        assert (ids[nc + k] == 2 * nc + k + 1) == bool(inside), f"gate row {k}"
    assert (e["num_out"][1:, 0] == nc + ng).all()


# ---- the class -------------------------------------------------------------------------------------------------------------------------------------------------------
def test_constructor_refusals_and_tables(capsys):
    with pytest.raises(NotImplementedError, match="greedy assignment .* is the path built"):
        toc3d_amd.PubTracker(hungarian=True)
    with pytest.raises(ValueError, match="unknown class name 'tram'"):
        toc3d_amd.PubTracker(class_names=("car", "tram"))
    with pytest.raises(ValueError, match="unknown tracking name 'barrier'"):
        toc3d_amd.PubTracker(tracking_names=("car", "barrier"))
    with pytest.raises(ValueError, match="max_age"):
        toc3d_amd.PubTracker(max_age=-1)
    with pytest.raises(ValueError, match="num_streams"):
        toc3d_amd.PubTracker(num_streams=0)
    with pytest.raises(ValueError, match="no entry for \\['truck'\\]"):
        toc3d_amd.PubTracker(cls_velocity_error=dict(car=2.5), tracking_names=("car", "truck"))
    t = toc3d_amd.PubTracker()
    assert capsys.readouterr().out == "", "nothing prints"
    assert (t.hungarian, t.max_age, t.num_streams) == (False, 0, 1) and t.class_names == TC.CLASS_NAMES and t.tracking_names == TC.TRACKING_NAMES
    assert list(t.track_label) == TC.track_label_table().tolist() == [0, 1, -1, 2, 3, -1, 4, 5, 6, -1]
    assert t.NUSCENE_CLS_VELOCITY_ERROR == {n: 2.5 for n in TC.TRACKING_NAMES}
    t = toc3d_amd.PubTracker(max_age=3, class_names=("pedestrian", "car"), tracking_names=("car", "pedestrian"), cls_velocity_error=dict(car=4, pedestrian=1))
    assert t.track_label == (1, 0) and t.NUSCENE_CLS_VELOCITY_ERROR == dict(car=4.0, pedestrian=1.0)


def test_capacity_arithmetic_and_device_refusals():
    assert tracking.capacity_for(300, 3) == 1200 and tracking.capacity_for(2048, 3) == 8192 == lib.TRACKS_MAX_TRACKS and tracking.capacity_for(0, 3) == 0
    assert tracking.capacity_for(2048, 0) == 2048 and tracking.state_bytes(8192) == 393248
    t = toc3d_amd.PubTracker(max_age=4)
    with pytest.raises(ValueError, match="need 10240 tracks, more than 8192"):
        t._ensure_state(2048, torch.device("cpu"))
    with pytest.raises(RuntimeError, match="rec must be a CUDA/HIP tensor -- the HIP extension is the only compute path"):
        t.step_fixed(torch.zeros(1, 4, 12, dtype=torch.float64), torch.zeros(1, 4), torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1, dtype=torch.int64), [0.0])
    # the state grows field by field (plain tensor copies: they run anywhere)
    t = toc3d_amd.PubTracker(max_age=1, num_streams=2)
    t._ensure_state(2, torch.device("cpu"))
    assert t.capacity == 4 and t._state[0].shape == (2, 32 + 48 * 4)
    f = tracking._fields(t._state[0], 4)
    f["header"][:, 0], f["header"][:, 1] = 3, 9
    f["last_timestamp"][:, 0] = 12.5
    f["ct"][:] = torch.arange(16.0).reshape(2, 8)
    f["age"][:] = torch.arange(8).reshape(2, 4).int()
    t._pending = [False, False]
    t._ensure_state(5, torch.device("cpu"))
    g = tracking._fields(t._state[0], 10)
    assert t.capacity == 10 and g["header"][:, :2].tolist() == [[3, 9], [3, 9]] and g["last_timestamp"][:, 0].tolist() == [12.5, 12.5]
    assert torch.equal(g["ct"][:, :8], torch.arange(16.0, dtype=torch.float64).reshape(2, 8)) and (g["ct"][:, 8:] == 0).all()
    assert torch.equal(g["age"][:, :4], torch.arange(8).reshape(2, 4).int()) and (g["age"][:, 4:] == 0).all()
    held = t.tracks(1)
    assert held["age"].tolist() == [4, 5, 6] and held["id_count"] == 9 and held["ct"].tolist() == [[8.0, 9.0], [10.0, 11.0], [12.0, 13.0]]


def test_step_records_and_track_file_on_the_restatement(tmp_path):
    name = "reset_midway"
    c, e = TC.build_case(name), TC.expected(name)
    trk = restated(toc3d_amd.PubTracker(max_age=c["max_age"]))
    results, frames, want = {}, [], {}
    for f, fr in enumerate(c["frames"]):
        annos = case_annos(c, f, 0)
        rec, score, nm, kept = trk.pack_annos([annos])
        n = int(fr["kept"][0])
        assert rec.shape == (1, n, 12) and np.array_equal(rec[0], fr["rec"][0, :n]) and np.array_equal(score[0], fr["score"][0, :n]) and np.array_equal(nm[0], fr["name"][0, :n])
        items = trk.step([annos], [float(fr["timestamp"][0])], [bool(fr["first"][0])], c["thr"])[0]
        rows = e["order"][f, 0, :int(e["num_out"][f, 0])].tolist()
        assert [x["tracking_id"] for x in items] == e["track_id"][f, 0, rows].tolist() and [x["active"] for x in items] == e["active"][f, 0, rows].tolist()
        assert all(list(x)[-2:] == ["tracking_id", "active"] and {k: v for k, v in x.items() if k not in ("tracking_id", "active")} == annos[r] for x, r in zip(items, rows))
        results[f"s{f}"] = annos
        frames.append(dict(token=f"s{f}", timestamp=float(fr["timestamp"][0]), first=bool(fr["first"][0])))
        want[f"s{f}"] = TC.want_annos(annos, e, f, rows)
        # the numpy route of the detector's hook: the same dicts
        got = trk.records_to_annos(fr["rec"], fr["score"], fr["name"], e["track_id"][f], e["order"][f], e["num_out"][f], [f"s{f}"])
        assert got == [want[f"s{f}"]] and all(list(a) == list(tracking.TRACK_ANNO_KEYS) and isinstance(a["tracking_id"], str) for a in got[0])
    with open(tmp_path / "results_nusc.json", "w") as fh:
        json.dump(dict(meta=None, results=results), fh)
    with open(tmp_path / "frames_meta.json", "w") as fh:
        json.dump(dict(frames=frames), fh)
    for given in (frames, str(tmp_path / "frames_meta.json"), dict(frames=frames)):
        path = restated(toc3d_amd.PubTracker(max_age=c["max_age"])).track_file(str(tmp_path / "results_nusc.json"), given, str(tmp_path / "out"))
        text = open(path).read()
        got = json.loads(text)
        assert path == str(tmp_path / "out" / "tracking_result.json") and list(got) == ["results", "meta"]
        assert got["meta"] == dict(use_camera=False, use_lidar=True, use_radar=False, use_map=False, use_external=False) and got["results"] == want
    assert text == json.dumps(dict(results=want, meta=tracking.TRACKING_META)), "the file is what pub_test.py would dump"
    with pytest.raises(ValueError, match="num_streams must be 1"):
        toc3d_amd.PubTracker(num_streams=2).track_file(dict(results={}), [], str(tmp_path / "out"))
    # a class the tracker does not know is passed over, as the reference does
    odd = trk.pack_annos([[dict(annos[0], detection_name="animal")]])
    assert odd[2].tolist() == [[-1]]
    print(f"step, records_to_annos and track_file on {name}: {sum(map(len, want.values()))} records over {len(frames)} frames equal the reference's")


# ---- the detector's hook -------------------------------------------------------------------------------------------------------------------------------------------------
class FakeResults:
    class_names = TC.CLASS_NAMES

    def __init__(self):
        self.results = {}

    def format_device(self, bbox_list, poses, tokens):
        B = len(bbox_list)
        rec = torch.zeros(B, 3, 12, dtype=torch.float64)
        rec[:, :, 0] = torch.arange(3.0, dtype=torch.float64) * 10
        fixed = dict(rec=rec, score=torch.full((B, 3), 0.5), name=torch.zeros(B, 3, dtype=torch.int32), kept=torch.full((B,), 3, dtype=torch.int64))
        return fixed, [[dict(sample_token=t)] for t in tokens]

    def format(self, bbox_list, poses, tokens):
        return self.format_device(bbox_list, poses, tokens)[1]

    def add(self, token, annos):
        self.results[token] = annos


class FakeTracker:
    """Records what the detector hands to PubTracker.step_fixed, and answers with the restatement."""
    def __init__(self, num_streams=1, **kw):
        self.num_streams, self.kw, self.calls = num_streams, kw, []
        self.inner = restated(toc3d_amd.PubTracker(num_streams=num_streams, **kw))

    def step_fixed(self, rec, score, name, kept, timestamps, first, thr):
        self.calls.append((timestamps.tolist(), list(first), thr))
        out = self.inner._step_host(rec.numpy(), score.numpy(), name.numpy(), kept.numpy(), timestamps.tolist(), first, thr)
        return {k: torch.from_numpy(np.asarray(v)) for k, v in out.items()}

    def records_to_annos(self, *a):
        return self.inner.records_to_annos(*a)


def frame(det, tokens, scenes, t):
    return DC.frame(det, [DC.posed_meta(tok, s) for tok, s in zip(tokens, scenes)], t)


def test_detector_hook_hands_over_timestamps_and_scene_starts(monkeypatch, tmp_path):
    det = DC.fake_detector()
    assert det.track_results is False and det.tracker is None and det.tracking_results == {}
    with pytest.raises(ValueError, match="enable_tracking needs the submission records it tracks: call enable_nusc_results\\(\\) first"):
        det.enable_tracking()
    from toc3d_amd import detector as D
    monkeypatch.setattr(D, "PubTracker", FakeTracker)
    assert det.enable_nusc_results().enable_tracking(score_threshold=0.3, cls_velocity_error=None) is det and det.track_results
    assert det.tracker.kw == dict(max_age=3, class_names=TC.CLASS_NAMES, cls_velocity_error=None), "pub_test.py's default max_age; the records' class names"
    det.nusc_results = FakeResults()
    for f, scene in enumerate("aab"):
        frame(det, [f"t{f}"], [scene], 100.0 + 0.5 * f)
    assert det.tracker.calls == [([100.0], [True], 0.3), ([100.5], [False], 0.3), ([101.0], [True], 0.3)]
    ids = [[a["tracking_id"] for a in det.tracking_results[f"t{f}"]] for f in range(3)]
    assert ids == [["1", "2", "3"]] * 3, "the same three cars: matched in the second frame, numbered afresh in the new scene"
    assert all(list(a) == list(tracking.TRACK_ANNO_KEYS) for a in det.tracking_results["t1"])
    # two streams in one step: a tracker for two streams is made, and each stream has its own scene start
    frame(det, ["u0", "v0"], ["a", "b"], 200.0)
    frame(det, ["u1", "v1"], ["a", "c"], 200.5)
    assert det.tracker.num_streams == 2 and det.tracker.calls == [([200.0, 207.0], [True, True], 0.3), ([200.5, 207.5], [False, True], 0.3)]
    path = det.dump_tracking(str(tmp_path / "trk"))
    got = json.load(open(path))
    assert list(got) == ["results", "meta"] and list(got["results"]) == ["t0", "t1", "t2", "u0", "v0", "u1", "v1"] and got["meta"] == tracking.TRACKING_META
    assert det.disable_tracking() is det
    n = len(det.tracker.calls)
    frame(det, ["u2", "v2"], ["a", "c"], 201.0)
    assert len(det.tracker.calls) == n and "u2" not in det.tracking_results and "u2" in det.nusc_results.results
    det.enable_tracking()
    det.disable_nusc_results()
    with pytest.raises(ValueError, match="tracking is enabled but the submission records are not"):
        frame(det, ["u3", "v3"], ["a", "c"], 201.5)
