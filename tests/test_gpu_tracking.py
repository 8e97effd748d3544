"""GPU: toc3d_tracks_step and toc3d_amd.PubTracker against the fixture of tests/tracking_cases.py (tests/golden/tracking_cases.npz: what the reference's PubTracker
returned and held on the seeded cases).  Everything is exact: track_id, active, order and num_out per frame, and the tracks held after every frame bit for bit,
floats included; every output and both states lie between guard bytes; the same sequence twice; three streams in one launch against three launches; the class on
top of it; and the detector with tracking switched on against one without, bit for bit.  Every test prints the figures it asserts on (run with -s)."""
import json
import os

import numpy as np
import pytest
import torch

import tracking_cases as TC
import toc3d_amd
from support import DEV, S, to_dev
from toc3d_amd import lib, synth, tracking

pytestmark = pytest.mark.gpu
GUARD_BYTES, FILL = 256, 0xA5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "toc3d_tracks_step"
dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def guarded(nbytes, fill=FILL):
    buf = torch.full((GUARD_BYTES + nbytes + GUARD_BYTES,), fill, dtype=torch.uint8, device=DEV)
    return buf, buf[GUARD_BYTES:GUARD_BYTES + nbytes]


def touched(buf, nbytes):
    host = buf.cpu().numpy()
    return int((host[:GUARD_BYTES] != FILL).sum() + (host[GUARD_BYTES + nbytes:] != FILL).sum())


def state_to_bytes(state, last, cap):
    """A state dict -> the bytes of include/toc3d_tracks.h."""
    n = len(state["label"])
    raw = np.zeros(tracking.state_bytes(cap), dtype=np.uint8)
    raw[0:8].view(np.int32)[:] = [n, state["id_count"]]
    raw[8:16].view(np.float64)[0] = last
    at = lib.TRACKS_HEADER_BYTES
    for k, size in (("ct", 16), ("tracking", 16), ("label", 4), ("tracking_id", 4), ("age", 4), ("active", 4)):
        raw[at:at + size * n] = np.ascontiguousarray(state[k], dtype=TC.STATE_DTYPES[k]).reshape(-1).view(np.uint8)
        at += size * cap
    return raw


def bytes_to_state(raw, cap):
    """-> (state dict of the live rows, last_timestamp, bytes that should be zero and are not: the header's padding and every row at or beyond count)."""
    n, id_count = raw[0:8].view(np.int32).tolist()
    assert 0 <= n <= cap
    dirty = int((raw[16:32] != 0).sum())
    state, at = dict(id_count=id_count), lib.TRACKS_HEADER_BYTES
    for k, size in (("ct", 16), ("tracking", 16), ("label", 4), ("tracking_id", 4), ("age", 4), ("active", 4)):
        field = raw[at:at + size * cap]
        live = field[:size * n].view(TC.STATE_DTYPES[k])
        state[k] = live.reshape(-1, 2).copy() if size == 16 else live.copy()
        dirty += int((field[size * n:] != 0).sum())
        at += size * cap
    return state, float(raw[8:16].view(np.float64)[0]), dirty


class Stepper:
    """The entry point stepped on a case's streams ``streams``: two guarded state buffers swapped after every step, every output between guard bytes."""

    def __init__(self, c, streams=None, extra_capacity=0):
        self.c, self.streams = c, list(range(c["B"])) if streams is None else list(streams)
        self.B, self.K = len(self.streams), c["K"]
        self.cap = tracking.capacity_for(self.K, c["max_age"]) + extra_capacity
        self.sbytes = tracking.state_bytes(self.cap)
        self.state = [guarded(self.B * self.sbytes), guarded(self.B * self.sbytes)]       # (the fill is no valid state: the first step must not depend on it)
        if c.get("init") is not None:
            raw = np.concatenate([state_to_bytes(c["init"][b], c["init_last"][b], self.cap) for b in self.streams])
            self.state[0][1].copy_(dv(raw))
        self.label, self.gate = dv(TC.track_label_table()), dv(TC.max_diff_table())
        self.guard_bytes = 0

    def step(self, f):
        fr, B, K, s = self.c["frames"][f], self.B, self.K, self.streams
        shapes = dict(track_id=(B, K), active=(B, K), order=(B, K), num_out=(B,))
        dtypes = dict(track_id=np.int32, active=np.int32, order=np.int32, num_out=np.int64)
        bufs = {k: guarded(int(np.prod(shapes[k])) * np.dtype(dtypes[k]).itemsize) for k in TC.OUT_KEYS}
        read = self.state[0][1].clone()
        lib.call(ENTRY, dv(fr["rec"][s]), dv(fr["score"][s]), dv(fr["name"][s]), dv(fr["kept"][s]), B, K, self.label, len(TC.CLASS_NAMES), self.gate,
                 len(TC.TRACKING_NAMES), float(self.c["thr"]), self.c["max_age"], dv(fr["timestamp"][s]), dv(fr["first"][s]), self.state[0][1], self.state[1][1], self.cap,
                 *[bufs[k][1] for k in TC.OUT_KEYS], S())
        torch.cuda.synchronize()
        assert torch.equal(read, self.state[0][1]), "the state a step reads is left as it was"
        self.state.reverse()
        out = {k: bufs[k][1].cpu().numpy().view(dtypes[k]).reshape(shapes[k]) for k in TC.OUT_KEYS}
        self.guard_bytes += sum(touched(bufs[k][0], bufs[k][1].numel()) for k in TC.OUT_KEYS) + sum(touched(b, self.B * self.sbytes) for b, _ in self.state)
        return out

    def raw_state(self):
        return self.state[0][1].cpu().numpy().reshape(self.B, self.sbytes)


def run_against_fixture(name, streams=None, extra_capacity=0):
    """-> (what the test prints, all output and state bytes of the run)."""
    c, e = TC.build_case(name), TC.expected(name)
    st = Stepper(c, streams, extra_capacity)
    trace, dirty = [], 0
    for f in range(len(c["frames"])):
        out = st.step(f)
        raw = st.raw_state()
        for i, b in enumerate(st.streams):
            tag = f"{name}, frame {f}, stream {b}"
            for k in ("track_id", "active", "order"):
                assert np.array_equal(out[k][i], e[k][f, b]), f"{tag}: {k}"
            assert out["num_out"][i] == e["num_out"][f, b], f"{tag}: num_out"
            state, last, d = bytes_to_state(raw[i], st.cap)
            TC.compare_state(tag, state, e, f, b)
            assert last == c["frames"][f]["timestamp"][b], f"{tag}: last_timestamp"
            dirty += d
        trace += [out[k].tobytes() for k in TC.OUT_KEYS] + [raw.tobytes()]
    assert dirty == 0, f"{name}: {dirty} bytes of the states at or beyond count are not zero"
    assert st.guard_bytes == 0, f"{name}: {st.guard_bytes} guard bytes written"
    line = (f"{name}: K {c['K']}, max_age {c['max_age']}, capacity {st.cap}: shown {e['num_out'][:, st.streams].tolist()}, held {e['count'][:, st.streams].tolist()}: ids, active, "
            f"order, num_out and every bit of the tracks equal the reference's; 0 guard bytes written")
    return line, trace


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
    st = Stepper(c)
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


def case_annos(c, f, b):
    fr = c["frames"][f]
    return [dict(sample_token=f"s{f}", translation=fr["rec"][b, i, 0:3].tolist(), size=fr["rec"][b, i, 3:6].tolist(), rotation=fr["rec"][b, i, 6:10].tolist(),
                 velocity=fr["rec"][b, i, 10:12].tolist(), detection_name=TC.CLASS_NAMES[int(fr["name"][b, i])], detection_score=float(fr["score"][b, i]),
                 attribute_name="") for i in range(int(fr["kept"][b]))]


def test_step_and_track_file(tmp_path):
    name = "reset_midway"
    c, e = TC.build_case(name), TC.expected(name)
    trk = toc3d_amd.PubTracker(max_age=c["max_age"])
    results, frames, want = {}, [], {}
    for f, fr in enumerate(c["frames"]):
        annos = case_annos(c, f, 0)
        items = trk.step([annos], [float(fr["timestamp"][0])], [bool(fr["first"][0])], c["thr"])[0]
        rows = e["order"][f, 0, :int(e["num_out"][f, 0])].tolist()
        assert [x["tracking_id"] for x in items] == e["track_id"][f, 0, rows].tolist() and [x["active"] for x in items] == e["active"][f, 0, rows].tolist()
        assert all({k: v for k, v in x.items() if k not in ("tracking_id", "active")} == annos[r] for x, r in zip(items, rows))
        results[f"s{f}"], frames = annos, frames + [dict(token=f"s{f}", timestamp=float(fr["timestamp"][0]), first=bool(fr["first"][0]))]
        want[f"s{f}"] = [dict(sample_token=f"s{f}", translation=annos[r]["translation"], size=annos[r]["size"], rotation=annos[r]["rotation"], velocity=annos[r]["velocity"],
                              tracking_id=str(int(e["track_id"][f, 0, r])), tracking_name=annos[r]["detection_name"], tracking_score=annos[r]["detection_score"]) for r in rows]
    with open(tmp_path / "results_nusc.json", "w") as fh:
        json.dump(dict(meta=None, results=results), fh)
    path = toc3d_amd.PubTracker(max_age=c["max_age"]).track_file(str(tmp_path / "results_nusc.json"), frames, str(tmp_path / "out"))
    got = json.load(open(path))
    assert path == str(tmp_path / "out" / "tracking_result.json") and list(got) == ["results", "meta"] and got["meta"] == tracking.TRACKING_META
    assert got["results"] == want and all(list(a) == list(tracking.TRACK_ANNO_KEYS) for annos in got["results"].values() for a in annos)
    print(f"step and track_file on {name}: {sum(map(len, want.values()))} tracking records over {len(frames)} frames equal the reference's, ids as str, keys in its order")


# ---- the detector ------------------------------------------------------------------------------------------------------------------------------------------------
TINY = synth.DETECTOR_TINY
WIDE = dict(max_depth=1e4, class_range={n: 1e4 for n in TC.CLASS_NAMES})     # no box of the synthetic detector is beyond its class range: more records to track
BANK = ("memory_embedding", "memory_reference_point", "memory_timestamp", "memory_egopose", "memory_velo")
_SD = {}


def build_detector(precision):
    det = toc3d_amd.build_detector(synth.detector_cfg(TINY), precision=precision)
    if "sd" not in _SD:
        _SD["sd"] = synth.detector_state_dict(TINY)
    det.load_state_dict(_SD["sd"], strict=True)
    det = det.to(DEV)
    det.img_backbone.autotune = det.img_neck.autotune = False
    tuned = os.path.join(ROOT, "toc3d_amd", "tuned", f"{TINY['backbone']}_320x800_{precision}.json")
    if os.path.exists(tuned):
        det.img_backbone.load_tuning(tuned)
        det.img_neck._tuned.update(det.img_backbone._tuned)
    return det


def snapshot(det, outs, results, B):
    last, N = det.last_frame, det.last_frame["img_feats"].shape[1]
    return [dict(keep=[k[b * N:(b + 1) * N].clone() for k in last["keep_idxes"]], img_feats=last["img_feats"][b].clone(),
                 out={k: outs[k][:, b].clone() for k in ("all_cls_scores", "all_bbox_preds")}, bank={k: getattr(det.pts_bbox_head, k)[b].clone() for k in BANK},
                 dec=results[b]["pts_bbox"]) for b in range(B)]


def run(det, frames, streams=False):
    seen, res = [], []
    hook = det.pts_bbox_head.register_forward_hook(lambda m, a, out: seen.append(out))
    try:
        for fr in frames:
            step = det.simple_test_streams if streams else det.simple_test
            results = step(fr["img_metas"], gumbel_noise=fr["gumbel"], **fr["dev"])
            res.append(snapshot(det, seen[-1], results, len(fr["img_metas"])))
    finally:
        hook.remove()
    return res


def assert_same_bits(a, b):
    for f, (xs, ys) in enumerate(zip(a, b)):
        for x, y in zip(xs, ys):
            assert all(torch.equal(p, q) for p, q in zip(x["keep"], y["keep"])) and torch.equal(x["img_feats"], y["img_feats"]), f"frame {f}: kept sets, img_feats"
            assert all(torch.equal(x["out"][k], y["out"][k]) for k in x["out"]) and all(torch.equal(x["bank"][k], y["bank"][k]) for k in BANK), f"frame {f}: head outputs, bank"
            assert all(torch.equal(torch.as_tensor(x["dec"][k]), torch.as_tensor(y["dec"][k])) for k in ("boxes_3d", "scores_3d", "labels_3d")), f"frame {f}: decoded lists"


def with_pose(meta, token, seed):
    import nusc_results_cases as NC
    p = NC.random_poses(np.random.default_rng(seed), 1)
    return dict(meta, sample_idx=token, **NC.pose_records(p)[0])


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
