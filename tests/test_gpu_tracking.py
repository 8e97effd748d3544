"""GPU: toc3d_tracks_step and toc3d_amd.PubTracker against the fixture of tests/tracking_cases.py (tests/golden/tracking_cases.npz: what the reference's PubTracker
returned and held on the seeded cases).  Everything is exact: track_id, active, order and num_out per frame, and the tracks held after every frame bit for bit,
floats included; every output and both states lie between guard bytes; the same sequence twice; three streams in one launch against three launches; the class on
top of it; and the detector with tracking switched on against one without, bit for bit.  Every test prints the figures it asserts on (run with -s)."""
import functools
import json

import numpy as np
import pytest
import torch

import detector_cases as DC
import tracking_cases as TC
import tracking_steps as TS
import toc3d_amd
from support import DEV, S, to_dev
from toc3d_amd import lib, synth, tracking

pytestmark = pytest.mark.gpu
ENTRY = "toc3d_tracks_step"
dv = TS.dv
run_against_fixture = functools.partial(TS.run_against_fixture, entry=ENTRY, out_keys=TC.OUT_KEYS, cases=TC)


# ---- the entry point against the fixture --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TC.CASES)
def test_steps_equal_the_reference(name):
    """No tolerance: the matching is exact arithmetic in the order include/toc3d_tracks.h states, and the fixture holds the reference's own results."""
    line, _ = run_against_fixture(name)
    print(line)


@pytest.mark.parametrize("name,extra", [("reset_midway", 5), ("n65_mixed", 1000), ("empty_twice_age0", 3)])
def test_a_capacity_above_the_least(name, extra):
    line, _ = run_against_fixture(name, extra_capacity=extra)
    print(line)


def test_the_same_sequence_twice_gives_identical_bytes():
    _, a = run_against_fixture("n257_mixed")
    _, b = run_against_fixture("n257_mixed")
    assert a == b
    print(f"n257_mixed from reset, twice: {len(a)} buffers (outputs and whole states, frame by frame), identical bytes")


def test_three_streams_equal_three_single_runs():
    _, all3 = run_against_fixture(TC.STREAMS_CASE)
    singles = [run_against_fixture(TC.STREAMS_CASE, streams=[b])[1] for b in range(3)]
    c = TC.build_case(TC.STREAMS_CASE)
    for i, blob in enumerate(all3):
        width = len(blob) // 3
        for b in range(3):
            assert blob[b * width:(b + 1) * width] == singles[b][i], f"buffer {i}, stream {b}"
    print(f"{TC.STREAMS_CASE}: B = 3 in one launch a frame, streams starting scenes at {[np.nonzero([fr['first'][b] for fr in c['frames']])[0].tolist() for b in range(3)]}: "
          "each stream's outputs and state bytes equal its B = 1 run")


def test_refusals_reach_python():
    c = TC.build_case("n64")
    st = TS.Stepper(c, ENTRY, TC.OUT_KEYS)
    fr = c["frames"][0]
    args = lambda cap, max_age=3: (dv(fr["rec"]), dv(fr["score"]), dv(fr["name"]), dv(fr["kept"]), 1, 64, st.label, 10, st.gate, 7, 0.25, max_age, dv(fr["timestamp"]),
                                   dv(fr["first"]), st.state[0][1], st.state[1][1], cap, *[torch.zeros(64, dtype=torch.int32, device=DEV)] * 3,
                                   torch.zeros(1, dtype=torch.int64, device=DEV), S())
    with pytest.raises(RuntimeError, match=r"capacity >= K \* \(max_age \+ 1\)"):
        lib.call(ENTRY, *args(255))
    with pytest.raises(RuntimeError, match="bad capacity"):
        lib.call(ENTRY, *args(8193))
    with pytest.raises(RuntimeError, match="bad max_age"):
        lib.call(ENTRY, *args(256, -1))
    assert tracking.library_state_bytes(8192) == tracking.state_bytes(8192) == 32 + 48 * 8192


# ---- the class -------------------------------------------------------------------------------------------------------------------------------------------------------
def class_outputs_equal(name, out, f, e):
    for k in ("track_id", "active", "order", "num_out"):
        assert np.array_equal(out[k].cpu().numpy(), e[k][f]), f"{name}, frame {f}: {k}"


def test_step_fixed_with_host_and_device_arguments():
    for name, device_args in (("reset_midway", False), (TC.STREAMS_CASE, True), ("kept_zero", False)):
        c, e = TC.build_case(name), TC.expected(name)
        trk = toc3d_amd.PubTracker(max_age=c["max_age"], num_streams=c["B"])
        for f, fr in enumerate(c["frames"]):
            ts, first = (dv(fr["timestamp"]), dv(fr["first"])) if device_args else (fr["timestamp"].tolist(), [bool(x) for x in fr["first"]])
            if f == 0 and not device_args:
                first = None                                                # the first call starts every stream
            out = trk.step_fixed(dv(fr["rec"]), dv(fr["score"]), dv(fr["name"]), dv(fr["kept"]), ts, first, c["thr"])
            assert all(out[k].is_cuda for k in TC.OUT_KEYS) and out["num_out"].dtype == torch.int64 and out["order"].dtype == torch.int32
            class_outputs_equal(name, out, f, e)
            for b in range(c["B"]):
                held = trk.tracks(b)
                TC.compare_state(f"{name}, frame {f}, stream {b}", held, e, f, b)
        print(f"PubTracker.step_fixed on {name} ({'device' if device_args else 'host'} timestamps and first flags): outputs and tracks held equal the reference's")
    with pytest.raises(ValueError, match="finite timestamps"):
        trk.step_fixed(dv(fr["rec"]), dv(fr["score"]), dv(fr["name"]), dv(fr["kept"]), [float("nan")], None, 0.25)
    with pytest.raises(RuntimeError, match="the HIP extension is the only compute path"):
        trk.step_fixed(torch.from_numpy(fr["rec"]), dv(fr["score"]), dv(fr["name"]), dv(fr["kept"]), [0.0], None, 0.25)


def test_state_grows_with_k_and_reset_restarts_a_stream():
    """K differs from frame to frame in the detector (the longest list of the step): the state is laid out again with the tracks kept."""
    c, e = TC.build_case("n65_mixed"), TC.expected("n65_mixed")
    trk = toc3d_amd.PubTracker(max_age=3)
    for f, fr in enumerate(c["frames"]):
        K = (65, 72, 90, 70)[f]                                             # the case's 65 rows and unread rows behind them
        pad = TC.blank_frame(1, K - 65, fr["timestamp"], fr["first"])
        wide = {k: np.concatenate([fr[k], pad[k]], axis=1) for k in ("rec", "score", "name")}
        out = trk.step_fixed(dv(wide["rec"]), dv(wide["score"]), dv(wide["name"]), dv(fr["kept"]), fr["timestamp"].tolist(), None, c["thr"])
        assert tuple(out["order"].shape) == (1, K) and trk.capacity == (260, 288, 360, 360)[f]
        for k, rest in (("track_id", 0), ("active", 0), ("order", -1)):
            got = out[k].cpu().numpy()
            assert np.array_equal(got[:, :65], e[k][f]) and (got[:, 65:] == rest).all(), f"frame {f}: {k}"
        TC.compare_state(f"frame {f}", trk.tracks(0), e, f, 0)
    trk.reset()
    fr = c["frames"][0]
    out = trk.step_fixed(dv(fr["rec"]), dv(fr["score"]), dv(fr["name"]), dv(fr["kept"]), fr["timestamp"].tolist(), [False], c["thr"])
    class_outputs_equal("after reset()", out, 0, e)
    print("K 65, 72, 90, 70 over four frames (capacity 260, 288, 360, 360): the tracks survive the growth of the state; reset() restarts the stream whatever first says")


def test_step_and_track_file(tmp_path):
    name = "reset_midway"
    path, got, want, frames = TS.step_and_track_file(lambda: toc3d_amd.PubTracker(max_age=TC.build_case(name)["max_age"]), TC, name, tmp_path)
    assert path == str(tmp_path / "out" / "tracking_result.json") and list(got) == ["results", "meta"] and got["meta"] == tracking.TRACKING_META
    assert got["results"] == want and all(list(a) == list(tracking.TRACK_ANNO_KEYS) for annos in got["results"].values() for a in annos)
    print(f"step and track_file on {name}: {sum(map(len, want.values()))} tracking records over {len(frames)} frames equal the reference's, ids as str, keys in its order")


# ---- the detector ------------------------------------------------------------------------------------------------------------------------------------------------
TINY = synth.DETECTOR_TINY
WIDE = dict(max_depth=1e4, class_range={n: 1e4 for n in TC.CLASS_NAMES})     # no box of the synthetic detector is beyond its class range: more records to track
build_detector = functools.partial(DC.build_detector, TINY)
run, assert_same_bits, with_pose = DC.run, DC.assert_same_bits, DC.with_pose


def stand_alone(records, tokens, timestamps, firsts, max_age, thr):
    """The tracking records of one stream from a PubTracker of its own, fed the gathered submission records frame by frame."""
    trk, out = toc3d_amd.PubTracker(max_age=max_age), {}
    for token, ts, first in zip(tokens, timestamps, firsts):
        out[token] = trk.items_to_annos(trk.step([records[token]], [ts], [first], thr)[0], token)
    return out


@pytest.mark.parametrize("precision", ["fp32x3", "bf16"])
def test_detector_keeps_its_bits_and_tracks_the_records(precision, tmp_path):
    frames = []
    for f, fr in enumerate(synth.detector_inputs(dict(TINY, new_scene_at=2))[:3]):
        frames.append(dict(img_metas=[with_pose(fr["img_metas"][0], f"sample{f}", 40)], gumbel=fr["gumbel"], dev=to_dev(fr)))      # one pose: the scene stands still
    with pytest.raises(ValueError, match="enable_nusc_results"):
        build_detector(precision).enable_tracking()
    plain = run(build_detector(precision).enable_nusc_results(**WIDE), frames)
    det = build_detector(precision).enable_nusc_results(**WIDE).enable_tracking(max_age=3, score_threshold=0.0)
    got = run(det, frames)
    assert_same_bits(got, plain)
    tokens = [f"sample{f}" for f in range(3)]
    assert list(det.tracking_results) == tokens == list(det.nusc_results.results)
    ts = [float(fr["dev"]["timestamp"][0]) for fr in frames]
    want = stand_alone(det.nusc_results.results, tokens, ts, [True, False, True], 3, 0.0)
    assert det.tracking_results == want
    ids = [[a["tracking_id"] for a in det.tracking_results[t]] for t in tokens]
    print(f"{precision}: three frames (a new scene at the third) equal a detector without tracking bit for bit; tracking ids per frame {ids}: equal to a stand-alone "
          "PubTracker fed the gathered records")
    assert sum(map(len, ids)) > 0 and ids[0] == [str(k + 1) for k in range(len(ids[0]))] and ids[2] == [str(k + 1) for k in range(len(ids[2]))]
    path = det.dump_tracking(str(tmp_path / "trk"))
    assert json.load(open(path))["results"] == want
    det.disable_tracking()
    run(det, frames[:1])
    assert list(det.tracking_results) == tokens


def test_detector_streams_track_per_stream():
    steps, _ = synth.detector_stream_steps(TINY, seeds=(0, 1), new_scene_at=(3, 2))
    frames = []
    for f, st in enumerate(steps[:3]):
        metas = [with_pose(m, f"f{f}s{b}", 50 + b) for b, m in enumerate(st["img_metas"])]
        frames.append(dict(img_metas=metas, gumbel=st["gumbel"], dev=to_dev(st)))
    plain = run(build_detector("fp32x3").enable_nusc_results(**WIDE), frames, streams=True)
    det = build_detector("fp32x3").enable_nusc_results(**WIDE).enable_tracking(max_age=3, score_threshold=0.0)
    got = run(det, frames, streams=True)
    assert_same_bits(got, plain)
    firsts = [[True, False, False], [True, False, True]]                    # stream 1 starts a scene at the third step
    for b in range(2):
        tokens = [f"f{f}s{b}" for f in range(3)]
        ts = [float(fr["dev"]["timestamp"][b]) for fr in frames]
        want = stand_alone(det.nusc_results.results, tokens, ts, firsts[b], 3, 0.0)
        assert {t: det.tracking_results[t] for t in tokens} == want
        print(f"stream {b}: tracking ids per step {[[a['tracking_id'] for a in want[t]] for t in tokens]}: equal to a stand-alone B = 1 PubTracker")
    assert sum(len(v) for v in det.tracking_results.values()) > 0
