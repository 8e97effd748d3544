"""CPU: the nuScenes submission records without a GPU -- the side header include/toc3d_results.h against the ctypes table that binds it and the library's exports;
the refusals of its entry point on made-up and on real host pointers (the checks run before any launch); the class-range and attribute tables built from the class
names against the reference's branch; the max_depth clamp; the pose checks; the fixture of tests/nusc_results_cases.py (its seeded inputs, its margins, the
restatement's two rotation routes held together, the exact cases); records_to_annos and dump; and the detector hook on recording fakes.  Every test prints the
figures it asserts on (run with -s)."""
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import nusc_results_cases as NC
import toc3d_amd
from detector_cases import fake_detector, frame
from support import A, ERR_ARG, OldLibrary, header_sigs, raw_call
from toc3d_amd import lib
from toc3d_amd import nusc_results as NR

ENTRY = "toc3d_boxes_to_global"


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------------------------------------
def test_results_header_ctypes_table_and_exports_agree():
    raw = open(lib.RESULTS_HEADER_PATH).read()
    txt = lib.header_text(lib.RESULTS_HEADER_PATH)
    found = header_sigs(txt, lib._RESULTS_SIGS)
    print(f"toc3d_results.h declares {found}")
    assert found == lib._RESULTS_SIGS and list(found) == [ENTRY]
    declared = set(re.findall(r"\b(toc3d_\w+)\s*\(", txt))
    assert declared == set(lib._RESULTS_SIGS) | {"toc3d_results_abi"}, "nothing declared that the table does not bind"
    define = lambda n: int(re.search(rf"#define\s+{n}\s+(\d+)", raw).group(1))
    assert define("TOC3D_RESULTS_ABI") == lib.RESULTS_ABI == 1
    assert (define("TOC3D_RESULTS_MAX_BOXES"), define("TOC3D_RESULTS_MAX_CLASSES"), define("TOC3D_RESULTS_REC")) == (2048, 64, 12)
    assert (lib.RESULTS_MAX_BOXES, lib.RESULTS_MAX_CLASSES, lib.RESULTS_REC) == (2048, 64, 12)
    from toc3d_amd.head_outputs import DECODE_MAX_NUM
    assert lib.RESULTS_MAX_BOXES == DECODE_MAX_NUM, "the decoder's own cap"
    for cited in ("nuscenes_dataset.py:301-368", ":576-619", ":622-657", "nuscenes_dataset.py:56-58", "lidar_box3d.py:41-47", "NumPy 1.x", "DROPPED"):
        assert cited in raw, f"the header cites {cited}"
    dll = ctypes.CDLL(lib.LIB_PATH)
    assert all(hasattr(dll, n) for n in declared)
    dll.toc3d_results_abi.restype = ctypes.c_int
    assert dll.toc3d_results_abi() == 1
    # the other headers know nothing of it, no name is bound twice, and the 11.1 surface stays where it is
    others = (lib.HEADER_PATH, lib.STREAMS_HEADER_PATH, lib.FOCAL_HEADER_PATH, lib.SAMPLED_HEADER_PATH, lib.SELECT_HEADER_PATH, lib.INGEST_HEADER_PATH, lib.VIS_HEADER_PATH,
              lib.BOXES_HEADER_PATH)
    for other in others:
        text = open(other).read()
        assert "toc3d_results" not in text and ENTRY not in text
    tables = (lib._SIGS, lib._STREAMS_SIGS, lib._FOCAL_SIGS, lib._SAMPLED_SIGS, lib._SELECT_SIGS, lib._INGEST_SIGS, lib._VIS_SIGS, lib._BOXES_SIGS, lib._RESULTS_SIGS)
    names = [n for t in tables for n in t]
    assert len(names) == len(set(names)), "no name is bound twice across the tables"
    assert lib.ABI_VERSION == 11 and lib.ABI_MINOR == 1
    main = open(lib.HEADER_PATH).read()
    assert int(re.search(r"#define\s+TOC3D_ABI_VERSION\s+(\d+)", main).group(1)) == 11 and int(re.search(r"#define\s+TOC3D_ABI_MINOR\s+(\d+)", main).group(1)) == 1
    l = lib.load()
    l.toc3d_abi_minor.restype = ctypes.c_int
    assert l.toc3d_abi_version() == 11 and l.toc3d_abi_minor() == 1
    mk = open(os.path.join(os.path.dirname(lib.LIB_PATH), "csrc", "Makefile")).read()
    assert " nusc_results.hip " in mk and "$(BUILD)/nusc_results.hip.o: ../../include/toc3d_results.h" in mk


def test_exports():
    assert toc3d_amd.NuScenesResults is NR.NuScenesResults and "NuScenesResults" in toc3d_amd.__all__
    assert {"BoxVis", "TokenVis", "Petr3D", "NMSFreeCoder"} <= set(toc3d_amd.__all__)
    assert all(hasattr(toc3d_amd.Petr3D, m) for m in ("enable_nusc_results", "disable_nusc_results"))


def entry_args(**o):
    a = dict(boxes=A, box_stride=9, sample_stride=2700, scores=A, labels=A, counts=A, B=2, K=300, vel=1, poses=A, rng=A, mov=A, still=A, ncls=10, thr=0.2, rec=A, score=A,
             name=A, attr=A, src=A, kept=A)
    a.update(o)
    return tuple(a[k] for k in ("boxes", "box_stride", "sample_stride", "scores", "labels", "counts", "B", "K", "vel", "poses", "rng", "mov", "still", "ncls", "thr", "rec",
                                "score", "name", "attr", "src", "kept")) + (None,)


POINTERS = ("boxes", "scores", "labels", "counts", "poses", "rng", "mov", "still", "rec", "score", "name", "attr", "src", "kept")


def test_call_binds_the_entry_point_and_an_old_library_is_told_to_rebuild(monkeypatch):
    with pytest.raises(RuntimeError, match=r"toc3d_boxes_to_global failed \(-1\): toc3d_boxes_to_global: null buffer"):
        lib.call(ENTRY, *entry_args(boxes=None))
    assert getattr(lib.load(), ENTRY).argtypes == [lib._CT[c] for c in lib._RESULTS_SIGS[ENTRY]], "bound with the table's argument types"

    monkeypatch.setattr(lib, "_lib", OldLibrary())
    with pytest.raises(RuntimeError, match=r"toc3d_results\.h.*rebuild the library"):
        lib.call(ENTRY, *entry_args())


@pytest.mark.parametrize("over,reason", [
    *[({p: None}, "null buffer") for p in POINTERS],
    (dict(B=-1), "must not be negative"), (dict(K=-1), "must not be negative"), (dict(K=2049), "at most 2048"), (dict(B=65536), "at most 65535"),
    (dict(box_stride=8), "a stride smaller than a row"), (dict(vel=0, box_stride=6), "a stride smaller than a row"), (dict(box_stride=-9), "a stride smaller than a row"),
    (dict(sample_stride=2699), "samples that overlap"), (dict(sample_stride=0), "samples that overlap"), (dict(box_stride=11), "samples that overlap"),
    (dict(ncls=0), "bad num_classes"), (dict(ncls=65), "bad num_classes"),
    (dict(thr=float("nan")), "bad speed_thr"), (dict(thr=float("inf")), "bad speed_thr"),
    (dict(boxes=A + 2), "4-byte boundary"), (dict(rec=A + 4), "8-byte boundary"), (dict(poses=A + 4), "8-byte boundary"),
    ({}, "host pointer"), (dict(vel=0, box_stride=7, sample_stride=2100), "host pointer"), (dict(K=2048, sample_stride=2048 * 9), "host pointer"),
    (dict(B=65535, ncls=64, box_stride=11, sample_stride=4000), "host pointer"),
])
def test_entry_point_refusals(over, reason):
    rc, msg = raw_call(lib._RESULTS_SIGS, ENTRY, entry_args(**over))
    print(f"{over}: rc {rc}, {msg!r}")
    assert rc == ERR_ARG and msg.startswith(ENTRY + ":") and reason in msg, (rc, msg)


def test_no_boxes_is_legal():
    """B == 0 or K == 0: nothing is launched, no pointer is looked at (none is device memory here), and the call succeeds."""
    nulls = {p: None for p in POINTERS}
    for over in (dict(B=0), dict(K=0, sample_stride=0), dict(B=0, **nulls), dict(K=0, sample_stride=0, **nulls)):
        rc, msg = raw_call(lib._RESULTS_SIGS, ENTRY, entry_args(**over))
        assert rc == 0, (over, rc, msg)


def test_real_host_buffers_are_refused_and_left_alone():
    """Host memory that could be read and written: the entry point refuses it (not device memory) and touches none of it."""
    p = ctypes.addressof
    boxes = (ctypes.c_float * 18)(*([1.0] * 18))
    scores, labels, counts = (ctypes.c_float * 2)(0.9, 0.8), (ctypes.c_int64 * 2)(0, 1), (ctypes.c_int64 * 1)(2)
    poses = (ctypes.c_double * 14)(*(NC.IDENTITY_POSE * 2))
    rng, mov, still = (ctypes.c_double * 10)(*([50.0] * 10)), (ctypes.c_int32 * 10)(*([5] * 10)), (ctypes.c_int32 * 10)(*([6] * 10))
    rec, score = (ctypes.c_double * 24)(*([7.0] * 24)), (ctypes.c_float * 2)(7.0, 7.0)
    name, attr, src = ((ctypes.c_int32 * 2)(7, 7) for _ in range(3))
    kept = (ctypes.c_int64 * 1)(7)
    args = entry_args(boxes=p(boxes), sample_stride=18, scores=p(scores), labels=p(labels), counts=p(counts), B=1, K=2, poses=p(poses), rng=p(rng), mov=p(mov),
                      still=p(still), rec=p(rec), score=p(score), name=p(name), attr=p(attr), src=p(src), kept=p(kept))
    rc, msg = raw_call(lib._RESULTS_SIGS, ENTRY, args)
    print(f"rc {rc}, {msg!r}")
    assert rc == ERR_ARG and "host pointer" in msg
    assert list(rec) == [7.0] * 24 and list(score) == [7.0, 7.0] and list(name) == list(attr) == list(src) == [7, 7] and list(kept) == [7] and list(boxes) == [1.0] * 18


# ---- the tables ---------------------------------------------------------------------------------------------------------------------------------------------------------
def test_tables_built_from_the_class_names():
    res = toc3d_amd.NuScenesResults()
    assert res.class_names == NR.CLASS_NAMES == NC.CLASS_NAMES and len(res.class_names) == 10
    assert res.class_names == ("car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle", "pedestrian", "traffic_cone")
    assert list(NR.ATTRIBUTES) == NC.ATTR_REV and NR.SPEED_THR == 0.2 and res.speed_thr == 0.2
    rng, mov, still = NC.tables()
    assert [res.class_range[n] for n in res.class_names] == rng.tolist() == [50, 50, 50, 50, 50, 30, 40, 40, 40, 30]
    for i, n in enumerate(res.class_names):
        assert res.attr_moving[i] == NC.reference_attribute(n, True) and res.attr_still[i] == NC.reference_attribute(n, False), n
        assert NR.attribute_index(res.attr_moving[i]) == mov[i] and NR.attribute_index(res.attr_still[i]) == still[i]
    by = dict(zip(res.class_names, zip(res.attr_moving, res.attr_still)))
    print(f"(moving, still) by class: {by}")
    assert by["bus"] == ("vehicle.moving", "vehicle.stopped") and by["pedestrian"] == ("pedestrian.moving", "pedestrian.standing")
    assert by["car"] == ("vehicle.moving", "vehicle.parked") and by["bicycle"] == ("cycle.with_rider", "cycle.without_rider")
    assert by["barrier"] == by["traffic_cone"] == ("", "") and NR.attribute_index("") == -1
    # another order and a subset: the tables follow the names, not the positions
    sub = toc3d_amd.NuScenesResults(class_names=["pedestrian", "bus"])
    assert sub.attr_still == ("pedestrian.standing", "vehicle.stopped") and [sub.class_range[n] for n in sub.class_names] == [40, 50]
    with pytest.raises(ValueError, match="unknown class name 'tram'"):
        toc3d_amd.NuScenesResults(class_names=["car", "tram"])
    with pytest.raises(ValueError, match="class names"):
        toc3d_amd.NuScenesResults(class_names=[])


def test_max_depth_clamp_and_class_range_override():
    assert toc3d_amd.NuScenesResults().max_depth == 60
    r35 = toc3d_amd.NuScenesResults(max_depth=35)
    assert [r35.class_range[n] for n in r35.class_names] == [35, 35, 35, 35, 35, 30, 35, 35, 35, 30], "min(range, max_depth), class by class"
    assert NC.tables(max_depth=35)[0].tolist() == [r35.class_range[n] for n in r35.class_names]
    with pytest.raises(ValueError, match="unknown eval_version 'detection_2030'"):
        toc3d_amd.NuScenesResults(eval_version="detection_2030")
    own = toc3d_amd.NuScenesResults(eval_version="detection_2030", class_range={n: 70 for n in NR.CLASS_NAMES})
    assert set(own.class_range.values()) == {60}, "an override is clamped like the table"
    with pytest.raises(ValueError, match="no entry for"):
        toc3d_amd.NuScenesResults(class_range=dict(car=50))
    assert toc3d_amd.NuScenesResults(with_velocity=False).with_velocity is False and toc3d_amd.NuScenesResults(modality=dict(use_camera=True)).modality == dict(use_camera=True)


def pose(**over):
    p = dict(lidar2ego_rotation=[1.0, 0.0, 0.0, 0.0], lidar2ego_translation=[0.9, 0.0, 1.8], ego2global_rotation=[0.6, 0.0, 0.0, 0.8], ego2global_translation=[400.0, 1100.0, 0.0])
    p.update(over)
    return p


def test_pose_records_are_normalised_and_checked():
    q = np.array([0.6, 0.0, 0.0, 0.8]) * (1 + 5e-7)                          # off 1 by less than 1e-6: normalised in float64
    arr = NR.pose_array([pose(), pose(ego2global_rotation=q.tolist(), lidar2ego_rotation=np.float32([0.5, 0.5, -0.5, 0.5]))])
    assert arr.shape == (2, 2, 7) and arr.dtype == np.float64
    assert arr[0, 0].tolist() == [1, 0, 0, 0, 0.9, 0, 1.8] and arr[0, 1, 4:].tolist() == [400, 1100, 0]
    norms = np.sqrt((arr[:, :, :4] ** 2).sum(-1))
    print(f"norms after normalisation: {norms.tolist()}")
    assert np.abs(norms - 1).max() <= 2 ** -52 and np.array_equal(arr[1, 1, :4], q / math.sqrt(float((q * q).sum())))
    for key in NR.POSE_KEYS:
        bad = pose()
        del bad[key]
        with pytest.raises(ValueError, match=f"no '{key}'"):
            NR.pose_array([pose(), bad])
    for bad, what in (([0.0] * 4, "no unit quaternion"), ([1.0, 0.0, 0.0, 2e-3], "no unit quaternion"), ([400.0, 1100.0, 0.0, 1.0], "no unit quaternion"),
                      ([float("nan"), 0, 0, 0], "four finite numbers"), ([1.0, 0.0, 0.0], "four finite numbers"), ([float("inf"), 0, 0, 0], "four finite numbers")):
        for key in ("lidar2ego_rotation", "ego2global_rotation"):
            with pytest.raises(ValueError, match=what):
                NR.pose_array([pose(**{key: bad})])
    with pytest.raises(ValueError, match="three finite numbers"):
        NR.pose_array([pose(ego2global_translation=[1.0, float("nan"), 0.0])])
    with pytest.raises(ValueError, match="three finite numbers"):
        NR.pose_array([pose(lidar2ego_translation=[1.0, 0.0])])


# ---- the fixture ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_fixture_holds_the_seeded_inputs_and_the_restatement():
    z = np.load(NC.FIXTURE)
    made = NC.fixture_arrays()
    assert set(z.files) == set(made) | {"generated_by"}
    for k, v in made.items():
        assert np.array_equal(z[k], v, equal_nan=True) and z[k].dtype == v.dtype, k
    print(f"{len(made)} arrays of {len(NC.CASES)} cases equal a fresh run; generated by: {str(z['generated_by'])}")
    assert "restatement" in str(z["generated_by"]) or "devkit" in str(z["generated_by"])
    assert os.path.getsize(NC.FIXTURE) < 1 << 20


def test_fixture_margins_patterns_and_ranges():
    """Every box of the random cases decides its range test and its attribute by more than 1e-6; about half lie beyond their range; the inputs span what the
    issue asks for."""
    total = beyond = 0
    worst_r = worst_s = np.inf
    seen = set()
    for name in NC.RANDOM_CASES:
        c = NC.load_case(name)
        counts, K, pattern, invalid, vel, _ = NC.RANDOM_CASES[name]
        B = len(counts)
        assert c["boxes"].shape == (B, K, 9) and c["counts"].tolist() == list(counts) and c["with_velocity"] == vel
        for b in range(B):
            n = counts[b]
            valid = np.isfinite(c["radius"][b])
            assert not valid[n:].any() and n - invalid <= valid.sum() <= n, "rows beyond the count are not looked at; invalid rows have no radius"
            mr, ms = np.abs(c["radius"][b, valid] - c["limit"][b, valid]), np.abs(c["speed"][b, valid] - NC.SPEED_THR)
            assert (mr > NC.MARGIN).all() and (ms > NC.MARGIN).all(), (name, b)
            if valid.any():
                worst_r, worst_s = min(worst_r, mr.min()), min(worst_s, ms.min())
            inside = c["radius"][b, valid] <= c["limit"][b, valid]
            assert c["kept"][b] == inside.sum()
            total, beyond = total + int(valid.sum()), beyond + int((~inside).sum())
            pat = pattern if isinstance(pattern, str) else pattern[b]
            seen.add(pat)
            if pat == "all":
                assert inside.all() and n - invalid <= c["kept"][b] == valid.sum()
            elif pat == "none":
                assert not inside.any() and c["kept"][b] == 0
            elif pat == "alternating" and invalid == 0:
                assert np.array_equal(inside, np.arange(n) % 2 == 0) and np.array_equal(c["src"][b, :c["kept"][b]], np.arange(0, n, 2))
            k = c["kept"][b]
            assert (np.diff(c["src"][b, :k]) > 0).all() and (c["src"][b, k:] == -1).all() and (c["rec"][b, k:] == 0).all(), "stable compaction, a zeroed tail"
    full = NC.load_case("full")
    yaw, t2 = full["boxes"][0, np.isfinite(full["boxes"][0, :, 6]), 6], np.abs(np.concatenate([NC.load_case(n)["poses"][:, 1, 4:6].reshape(-1) for n in NC.RANDOM_CASES]))
    print(f"{total} valid boxes, {beyond} beyond their range ({beyond / total:.2f}); smallest |radius - range| {worst_r:.2e}, |speed - 0.2| {worst_s:.2e}; "
          f"yaw in [{yaw.min():.2f}, {yaw.max():.2f}], global translations up to {t2.max():.0f} m")
    assert seen == set(NC.PATTERNS) and 0.35 < beyond / total < 0.65
    assert yaw.min() < -6.2 and yaw.max() > 6.2 and 1500 < t2.max() <= 2000
    assert sorted({n for c in NC.RANDOM_CASES.values() for n in c[0]}) == [0, 1, 63, 64, 65, 256, 257, 2048], "the shapes the issue names"


def test_matrix_route_equals_the_sandwich_route():
    """The restatement turns vectors with the rotation matrix; q v q* is another formula for the same rotation.  Both are a few roundings of terms of magnitude
    S = |c_0| + |c_1| + |c_2| (+ |t|) away from the exact result: the sandwich has two Hamilton products of four terms each (at most 2 * 4 roundings a component, on
    terms bounded by S), the matrix route the bound of the module docstring.  Held together within the sum: bound + 16 u (S' + |t|) a pose, taken as 2 * bound +
    64 u max|rec| -- and every decision (kept, src, attr) must be the same."""
    worst = 0.0
    for name in ("wave_random", "wave_novel", "chunk_random", NC.EXACT_CASE):
        c = NC.load_case(name)
        other = NC.restate(c["boxes"], c["scores"], c["labels"], c["counts"], c["poses"], c["with_velocity"], route="sandwich")
        assert all(np.array_equal(other[k], c[k]) for k in ("kept", "src", "name", "attr", "score"))
        assert np.array_equal(other["rec"][..., 3:10], c["rec"][..., 3:10]), "size and orientation do not pass through either route"
        tol = 2 * c["bound"] + 64 * NC.U * np.abs(c["rec"]).max(axis=-1, keepdims=True)
        cols = [0, 1, 2, 10, 11]
        live = np.arange(c["rec"].shape[1])[None] < c["kept"][:, None]
        frac = (np.abs(other["rec"] - c["rec"])[..., cols] / np.where(live[..., None], tol[..., cols], 1.0)).max()
        worst = max(worst, float(frac))
        assert (np.abs(other["rec"] - c["rec"])[..., cols][live].max() > 0) or name == NC.EXACT_CASE, "the two routes round differently: they are independent"
    print(f"matrix and sandwich routes: worst difference {worst:.3f} of the tolerance")
    assert worst <= 1.0


def test_exact_cases():
    c = NC.load_case(NC.EXACT_CASE)
    res = toc3d_amd.NuScenesResults()
    annos = res.records_to_annos(c["rec"], c["score"], c["name"], c["attr"], c["kept"])[0]
    want = [(i, r) for i, r in enumerate(NC.EXACT_ROWS) if r[4] is not None]
    assert c["kept"][0] == len(want) == len(NC.EXACT_ROWS) - 1 and c["src"][0, :len(want)].tolist() == [i for i, _ in want]
    for anno, (i, (name, x, y, vx, attr)) in zip(annos, want):
        print(f"row {i}: {name} at ({x}, {y}), vx {vx!r} -> {anno['attribute_name']!r}")
        assert anno["detection_name"] == name and anno["attribute_name"] == attr
        assert anno["translation"] == [x, y, -0.25] and anno["size"] == [2.0, 4.0, 1.5] and anno["rotation"] == [1.0, 0.0, 0.0, 0.0] and anno["velocity"] == [vx, 0.0]
    assert c["radius"][0, 0] == 50.0 == c["limit"][0, 0] and c["radius"][0, 1] > 50.0 and c["radius"][0, 1] - 50.0 < 1e-5, "exactly at the range: kept; the next float32: dropped"
    assert c["speed"][0, 2] > 0.2 > c["speed"][0, 3] and c["speed"][0, 2] - c["speed"][0, 3] < 2e-8
    assert c["radius"][0, 8] == 30.0 and c["radius"][0, 9] == 40.0


# ---- the host half ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_records_to_annos_and_dump_round_trip(tmp_path):
    c = NC.load_case("wave_random")
    res = toc3d_amd.NuScenesResults(modality=dict(use_camera=True, use_lidar=False))
    tokens = ["tok_a", "tok_b", "tok_c"]
    per = res.records_to_annos(c["rec"], c["score"], c["name"], c["attr"], c["kept"], tokens)
    assert [len(a) for a in per] == c["kept"].tolist()
    for b, annos in enumerate(per):
        for i, anno in enumerate(annos):
            assert tuple(anno) == NR.ANNO_KEYS == ("sample_token", "translation", "size", "rotation", "velocity", "detection_name", "detection_score", "attribute_name")
            assert anno["sample_token"] == tokens[b] and [len(anno[k]) for k in ("translation", "size", "rotation", "velocity")] == [3, 3, 4, 2]
            nums = anno["translation"] + anno["size"] + anno["rotation"] + anno["velocity"] + [anno["detection_score"]]
            assert all(type(v) is float for v in nums), "Python floats"
            assert nums[:12] == c["rec"][b, i].tolist() and anno["detection_score"] == float(c["score"][b, i])
            assert anno["detection_name"] == NC.CLASS_NAMES[c["name"][b, i]] and anno["attribute_name"] == ("" if c["attr"][b, i] < 0 else NC.ATTR_REV[c["attr"][b, i]])
    bare = res.records_to_annos(c["rec"], c["score"], c["name"], c["attr"], c["kept"])
    assert tuple(bare[0][0]) == NR.ANNO_KEYS[1:], "no token, no key"
    for token, annos in zip(tokens, per):
        assert res.add(token, annos) is res
    res.add("tok_a", per[0])                                                # again: replaced, not appended
    path = res.dump(str(tmp_path / "out" / "pts_bbox"))
    assert path == str(tmp_path / "out" / "pts_bbox" / "results_nusc.json")
    back = json.load(open(path))
    assert list(back) == ["meta", "results"] and back["meta"] == dict(use_camera=True, use_lidar=False) and list(back["results"]) == tokens
    assert back["results"] == dict(zip(tokens, per)), "every number survives the round trip (repr of a float64)"
    print(f"{sum(map(len, per))} records of 3 samples written to and read back from {os.path.basename(path)} ({os.path.getsize(path)} bytes)")
    with pytest.raises(ValueError, match="sample tokens"):
        res.records_to_annos(c["rec"], c["score"], c["name"], c["attr"], c["kept"], ["one"])
    with pytest.raises(ValueError, match="expected"):
        res.records_to_annos(c["rec"][..., :11], c["score"], c["name"], c["attr"], c["kept"])
    with pytest.raises(RuntimeError, match="only compute path"):
        res.format_fixed(torch.zeros(1, 2, 9), torch.zeros(1, 2), torch.zeros(1, 2, dtype=torch.int64), torch.zeros(1, dtype=torch.int64), [pose()])


# ---- the detector hook --------------------------------------------------------------------------------------------------------------------------------------------------
class FakeResults:
    """Records what the detector hands to NuScenesResults."""
    def __init__(self):
        self.calls, self.results = [], {}

    def format(self, bbox_list, poses, tokens):
        self.calls.append((len(bbox_list), [float(b[0][0, 0]) for b in bbox_list], [p["ego2global_translation"] for p in poses], list(tokens)))
        return [[dict(sample_token=t, n=int(b[0].shape[0]))] for b, t in zip(bbox_list, tokens)]

    def add(self, token, annos):
        self.results[token] = annos


def meta(token, scene="a", **over):
    return dict(pose(**over), scene_token=scene, pad_shape=[(32, 80, 3)], sample_idx=token)


def test_detector_hook_reads_the_poses_and_names_a_missing_key():
    det = fake_detector()
    assert det.format_nusc_results is False and det.nusc_results is None
    frame(det, [dict(scene_token="a", pad_shape=[(32, 80, 3)])])             # not enabled: a frame without poses is nobody's business
    assert det.enable_nusc_results(max_depth=35, with_velocity=False) is det and det.format_nusc_results
    assert isinstance(det.nusc_results, toc3d_amd.NuScenesResults) and det.nusc_results.max_depth == 35 and not det.nusc_results.with_velocity, "the keywords reach the class"
    for key in NR.POSE_KEYS + ("sample_idx",):
        bad = meta("t0")
        del bad[key]
        with pytest.raises(ValueError, match=f"img_metas\\[0\\] has no '{key}'"):
            frame(det, [bad])
    assert det.nusc_results.results == {}
    fake = det.nusc_results = FakeResults()
    out = frame(det, [meta("t0")])
    assert fake.calls == [(1, [0.0], [[400.0, 1100.0, 0.0]], ["t0"])] and fake.results == {"t0": [dict(sample_token="t0", n=3)]}
    assert list(out[0]) == ["pts_bbox"] and torch.equal(torch.as_tensor(out[0]["pts_bbox"]["scores_3d"]), torch.arange(3.0)), "the returned lists are what they were"
    # two streams in one step: one call for both, each with its own pose and token
    frame(det, [meta("s0"), meta("s1", scene="b", ego2global_translation=[1.0, 2.0, 3.0])])
    assert fake.calls[-1] == (2, [0.0, 1.0], [[400.0, 1100.0, 0.0], [1.0, 2.0, 3.0]], ["s0", "s1"]) and list(fake.results) == ["t0", "s0", "s1"]
    bad = meta("s1", scene="b")
    del bad["ego2global_rotation"]
    with pytest.raises(ValueError, match=r"img_metas\[1\] has no 'ego2global_rotation'"):
        frame(det, [meta("s0"), bad])
    assert det.disable_nusc_results() is det and not det.format_nusc_results
    n = len(fake.calls)
    frame(det, [dict(scene_token="a", pad_shape=[(32, 80, 3)])])
    assert len(fake.calls) == n and list(fake.results) == ["t0", "s0", "s1"], "off: nothing formatted, what was gathered stays"
    print(f"{n} formatting calls for 2 steps; results gathered under {list(fake.results)}")
