"""GPU: toc3d_tracks_step_hungarian and toc3d_amd.HungarianPubTracker against the fixture of tests/tracking_hungarian_cases.py
(tests/golden/tracking_hungarian_cases.npz: what the reference's PubTracker(hungarian=True) returned and held, with scipy's solver).  No tolerance anywhere:
track_id, active, order, num_out and the solver's scan rounds per frame, and the tracks held after every frame bit for bit; every output and both states lie
between guard bytes; a capacity above the least; the same sequence twice; three streams in one launch against three launches; the class on top of it; the detector
with enable_tracking(hungarian=True) against one without; and the greedy entry on the same inputs against its own restatement, which the header the two kernels
share must not have changed.  Every test prints the figures it asserts on (run with -s)."""
import functools

import numpy as np
import pytest
import torch

import detector_cases as DC
import tracking_cases as TC
import tracking_hungarian_cases as HC
import tracking_steps as TS
import toc3d_amd
from support import DEV, S, to_dev
from toc3d_amd import lib, synth, tracking

pytestmark = pytest.mark.gpu
HUNGARIAN, GREEDY = "toc3d_tracks_step_hungarian", "toc3d_tracks_step"
dv = TS.dv
run_against_fixture = functools.partial(TS.run_against_fixture, entry=HUNGARIAN, out_keys=HC.OUT_KEYS, cases=HC)


# ---- the entry point against the fixture --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", HC.CASES)
def test_steps_equal_the_reference(name):
    """No tolerance: the solver is exact arithmetic in the order include/toc3d_assign.h states, and the fixture holds the reference's own results."""
    line, _ = run_against_fixture(name)
    print(line)


@pytest.mark.parametrize("name,extra", [("quirk_b", 5), ("n65_mixed", 1000), ("n100_m256", 1), ("n256_m100", 300)])
def test_a_capacity_above_the_least(name, extra):
    line, _ = run_against_fixture(name, extra_capacity=extra)
    print(line)


def test_the_same_sequence_twice_gives_identical_bytes():
    _, a = run_against_fixture("scene300")
    _, b = run_against_fixture("scene300")
    assert a == b
    print(f"scene300 twice: {len(a)} buffers (outputs, rounds and whole states, frame by frame), identical bytes")


def test_three_streams_equal_three_single_runs():
    _, all3 = run_against_fixture(HC.STREAMS_CASE)
    singles = [run_against_fixture(HC.STREAMS_CASE, streams=[b])[1] for b in range(3)]
    c = HC.build_case(HC.STREAMS_CASE)
    for i, blob in enumerate(all3):
        width = len(blob) // 3
        for b in range(3):
            assert blob[b * width:(b + 1) * width] == singles[b][i], f"buffer {i}, stream {b}"
    print(f"{HC.STREAMS_CASE}: B = 3 in one launch a frame, streams starting scenes at {[np.nonzero([fr['first'][b] for fr in c['frames']])[0].tolist() for b in range(3)]}: "
          "each stream's outputs and state bytes equal its B = 1 run")


@pytest.mark.parametrize("name", [n for n in HC.CASES if n not in TC.CASES])
def test_greedy_entry_on_the_same_inputs_equals_its_restatement(name):
    """toc3d_tracks_step shares its filter and its state write with the new kernel (csrc/tracks_steps.h): on the Hungarian cases' inputs it still equals the greedy
    restatement of tests/tracking_cases.py, every integer and every bit of the tracks held."""
    c = HC.build_case(name)
    outs, states = TC.run_case(c)
    st = TS.Stepper(c, GREEDY, TC.OUT_KEYS)
    for f in range(len(c["frames"])):
        out = st.step(f)
        raw = st.raw_state()
        for b in range(c["B"]):
            for k in TC.OUT_KEYS:
                assert np.array_equal(out[k][b], outs[f][b][k]), f"{name}, frame {f}, stream {b}: {k}"
            state, _, dirty = TC.bytes_to_state(raw[b], st.cap)
            assert dirty == 0 and np.array_equal(TC.state_digest(state), TC.state_digest(states[f][b])), f"{name}, frame {f}, stream {b}: the tracks held"
    assert st.guard_bytes == 0
    print(f"{name}: the greedy entry on these inputs: shown {[[int(o['num_out']) for o in fr] for fr in outs]}: equal to the greedy restatement, bit for bit")


def test_refusals_reach_python():
    c = HC.build_case("n64_age0")
    st = TS.Stepper(c, HUNGARIAN, HC.OUT_KEYS)
    fr = c["frames"][0]
    args = lambda cap, K=64, max_age=0: (dv(fr["rec"]), dv(fr["score"]), dv(fr["name"]), dv(fr["kept"]), 1, K, st.label, 10, st.gate, 7, 0.25, max_age, dv(fr["timestamp"]),
                                         dv(fr["first"]), st.state[0][1], st.state[1][1], cap, *[torch.zeros(64, dtype=torch.int32, device=DEV)] * 3,
                                         torch.zeros(1, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV), S())
    with pytest.raises(RuntimeError, match=r"capacity >= K \* \(max_age \+ 1\)"):
        lib.call(HUNGARIAN, *args(63))
    with pytest.raises(RuntimeError, match="bad capacity \\(at most 2048"):
        lib.call(HUNGARIAN, *args(2049))
    with pytest.raises(RuntimeError, match="K at most 512"):
        lib.call(HUNGARIAN, *args(2048, K=513))


# ---- the class -------------------------------------------------------------------------------------------------------------------------------------------------------
def test_step_fixed_with_host_and_device_arguments():
    for name, device_args in (("reset_midway", False), (HC.STREAMS_CASE, True), ("kept_zero", False), ("quirk_b", False)):
        c, e = HC.build_case(name), HC.expected(name)
        trk = toc3d_amd.build_tracker(hungarian=True, max_age=c["max_age"], num_streams=c["B"])
        assert isinstance(trk, toc3d_amd.HungarianPubTracker) and trk.hungarian is True
        for f, fr in enumerate(c["frames"]):
            ts, first = (dv(fr["timestamp"]), dv(fr["first"])) if device_args else (fr["timestamp"].tolist(), [bool(x) for x in fr["first"]])
            out = trk.step_fixed(dv(fr["rec"]), dv(fr["score"]), dv(fr["name"]), dv(fr["kept"]), ts, first, c["thr"])
            assert all(out[k].is_cuda for k in HC.OUT_KEYS) and out["rounds"].dtype == torch.int32 and tuple(out["rounds"].shape) == (c["B"],)
            for k in HC.OUT_KEYS:
                assert np.array_equal(out[k].cpu().numpy(), e[k][f]), f"{name}, frame {f}: {k}"
            for b in range(c["B"]):
                HC.compare_state(f"{name}, frame {f}, stream {b}", trk.tracks(b), e, f, b)
        print(f"HungarianPubTracker.step_fixed on {name} ({'device' if device_args else 'host'} timestamps and first flags): outputs, rounds and tracks held equal the reference's")
    with pytest.raises(ValueError, match="513 rows a stream exceed 512 \\(TOC3D_ASSIGN_MAX_BOXES\\)"):
        toc3d_amd.build_tracker(hungarian=True).step_fixed(torch.zeros(1, 513, 12, dtype=torch.float64, device=DEV), torch.zeros(1, 513, device=DEV),
                                                           torch.zeros(1, 513, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV), [0.0])


def test_step_and_track_file(tmp_path):
    name = "reset_midway"
    make = lambda: toc3d_amd.build_tracker(hungarian=True, max_age=HC.build_case(name)["max_age"])
    path, got, want, frames = TS.step_and_track_file(make, HC, name, tmp_path)
    assert list(got) == ["results", "meta"] and got["meta"] == tracking.TRACKING_META and got["results"] == want
    greedy, e = TC.expected(name), HC.expected(name)
    assert any(not np.array_equal(greedy["track_id"][f], e["track_id"][f]) for f in range(len(frames))), "the case tells the two assignments apart"
    print(f"step and track_file on {name} with hungarian=True: {sum(map(len, want.values()))} tracking records over {len(frames)} frames equal the reference's")


# ---- the detector ------------------------------------------------------------------------------------------------------------------------------------------------
TINY = synth.DETECTOR_TINY
WIDE = dict(max_depth=1e4, class_range={n: 1e4 for n in TC.CLASS_NAMES})     # no box of the synthetic detector is beyond its class range: more records to track
build_detector = functools.partial(DC.build_detector, TINY)


def test_detector_keeps_its_bits_and_tracks_the_records_with_hungarian():
    frames = []
    for f, fr in enumerate(synth.detector_inputs(dict(TINY, new_scene_at=2))[:3]):
        frames.append(dict(img_metas=[DC.with_pose(fr["img_metas"][0], f"sample{f}", 40)], gumbel=fr["gumbel"], dev=to_dev(fr)))      # one pose: the scene stands still
    plain = DC.run(build_detector("fp32x3").enable_nusc_results(**WIDE), frames)
    det = build_detector("fp32x3").enable_nusc_results(**WIDE).enable_tracking(max_age=3, score_threshold=0.0, hungarian=True)
    assert isinstance(det.tracker, toc3d_amd.HungarianPubTracker)
    got = DC.run(det, frames)
    DC.assert_same_bits(got, plain)
    tokens = [f"sample{f}" for f in range(3)]
    assert list(det.tracking_results) == tokens == list(det.nusc_results.results)
    ts = [float(fr["dev"]["timestamp"][0]) for fr in frames]
    trk, want = toc3d_amd.build_tracker(hungarian=True, max_age=3), {}
    for token, t, first in zip(tokens, ts, [True, False, True]):
        want[token] = trk.items_to_annos(trk.step([det.nusc_results.results[token]], [t], [first], 0.0)[0], token)
    assert det.tracking_results == want and sum(map(len, want.values())) > 0
    print(f"fp32x3: three frames (a new scene at the third) with enable_tracking(hungarian=True) equal a detector without tracking bit for bit; tracking ids per frame "
          f"{[[a['tracking_id'] for a in want[t]] for t in tokens]}: equal to a stand-alone HungarianPubTracker fed the gathered records")
