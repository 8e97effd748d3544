"""GPU: toc3d_tracks_step_hungarian and toc3d_amd.HungarianPubTracker against the fixture of tests/tracking_hungarian_cases.py
(tests/golden/tracking_hungarian_cases.npz: what the reference's PubTracker(hungarian=True) returned and held, with scipy's solver).  No tolerance anywhere:
track_id, active, order, num_out and the solver's scan rounds per frame, and the tracks held after every frame bit for bit; every output and both states lie
between guard bytes; a capacity above the least; the same sequence twice; three streams in one launch against three launches; the class on top of it; the detector
with enable_tracking(hungarian=True) against one without; and the greedy entry on the same inputs against its own restatement, which the header the two kernels
share must not have changed.  Every test prints the figures it asserts on (run with -s)."""
import json
import os

import numpy as np
import pytest
import torch

import tracking_cases as TC
import tracking_hungarian_cases as HC
import toc3d_amd
from support import DEV, S, to_dev
from toc3d_amd import lib, synth, tracking

pytestmark = pytest.mark.gpu
GUARD_BYTES, FILL = 256, 0xA5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HUNGARIAN, GREEDY = "toc3d_tracks_step_hungarian", "toc3d_tracks_step"
FIELDS = (("ct", 16), ("tracking", 16), ("label", 4), ("tracking_id", 4), ("age", 4), ("active", 4))
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
    for k, size in FIELDS:
        raw[at:at + size * n] = np.ascontiguousarray(state[k], dtype=TC.STATE_DTYPES[k]).reshape(-1).view(np.uint8)
        at += size * cap
    return raw


def bytes_to_state(raw, cap):
    """-> (state dict of the live rows, last_timestamp, bytes that should be zero and are not: the header's padding and every row at or beyond count)."""
    n, id_count = raw[0:8].view(np.int32).tolist()
    assert 0 <= n <= cap
    dirty = int((raw[16:32] != 0).sum())
    state, at = dict(id_count=id_count), lib.TRACKS_HEADER_BYTES
    for k, size in FIELDS:
        field = raw[at:at + size * cap]
        live = field[:size * n].view(TC.STATE_DTYPES[k])
        state[k] = live.reshape(-1, 2).copy() if size == 16 else live.copy()
        dirty += int((field[size * n:] != 0).sum())
        at += size * cap
    return state, float(raw[8:16].view(np.float64)[0]), dirty


class Stepper:
    """An entry point stepped on a case's streams ``streams``: two guarded state buffers swapped after every step, every output between guard bytes."""
    SHAPES = dict(track_id="BK", active="BK", order="BK", num_out="B", rounds="B")
    DTYPES = dict(track_id=np.int32, active=np.int32, order=np.int32, num_out=np.int64, rounds=np.int32)

    def __init__(self, c, streams=None, extra_capacity=0, entry=HUNGARIAN):
        self.c, self.streams, self.entry = c, list(range(c["B"])) if streams is None else list(streams), entry
        self.keys = HC.OUT_KEYS if entry == HUNGARIAN else TC.OUT_KEYS
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
        shapes = {k: (B, K) if self.SHAPES[k] == "BK" else (B,) for k in self.keys}
        bufs = {k: guarded(int(np.prod(shapes[k])) * np.dtype(self.DTYPES[k]).itemsize) for k in self.keys}
        read = self.state[0][1].clone()
        lib.call(self.entry, dv(fr["rec"][s]), dv(fr["score"][s]), dv(fr["name"][s]), dv(fr["kept"][s]), B, K, self.label, len(TC.CLASS_NAMES), self.gate,
                 len(TC.TRACKING_NAMES), float(self.c["thr"]), self.c["max_age"], dv(fr["timestamp"][s]), dv(fr["first"][s]), self.state[0][1], self.state[1][1], self.cap,
                 *[bufs[k][1] for k in self.keys], S())
        torch.cuda.synchronize()
        assert torch.equal(read, self.state[0][1]), "the state a step reads is left as it was"
        self.state.reverse()
        out = {k: bufs[k][1].cpu().numpy().view(self.DTYPES[k]).reshape(shapes[k]) for k in self.keys}
        self.guard_bytes += sum(touched(bufs[k][0], bufs[k][1].numel()) for k in self.keys) + sum(touched(b, self.B * self.sbytes) for b, _ in self.state)
        return out

    def raw_state(self):
        return self.state[0][1].cpu().numpy().reshape(self.B, self.sbytes)


def run_against_fixture(name, streams=None, extra_capacity=0):
    """-> (what the test prints, all output and state bytes of the run)."""
    c, e = HC.build_case(name), HC.expected(name)
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
            assert out["rounds"][i] == e["rounds"][f, b], f"{tag}: the solver made {out['rounds'][i]} scan rounds, the restated one {e['rounds'][f, b]}"
            state, last, d = bytes_to_state(raw[i], st.cap)
            HC.compare_state(tag, state, e, f, b)
            assert last == c["frames"][f]["timestamp"][b], f"{tag}: last_timestamp"
            dirty += d
        trace += [out[k].tobytes() for k in HC.OUT_KEYS] + [raw.tobytes()]
    assert dirty == 0, f"{name}: {dirty} bytes of the states at or beyond count are not zero"
    assert st.guard_bytes == 0, f"{name}: {st.guard_bytes} guard bytes written"
    line = (f"{name}: K {c['K']}, max_age {c['max_age']}, capacity {st.cap}: shown {e['num_out'][:, st.streams].tolist()}, held {e['count'][:, st.streams].tolist()}, rounds "
            f"{e['rounds'][:, st.streams].tolist()}: ids, active, order, num_out, rounds and every bit of the tracks equal the reference's; 0 guard bytes written")
    return line, trace


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
    st = Stepper(c, entry=GREEDY)
    for f in range(len(c["frames"])):
        out = st.step(f)
        raw = st.raw_state()
        for b in range(c["B"]):
            for k in TC.OUT_KEYS:
                assert np.array_equal(out[k][b], outs[f][b][k]), f"{name}, frame {f}, stream {b}: {k}"
            state, _, dirty = bytes_to_state(raw[b], st.cap)
            assert dirty == 0 and np.array_equal(TC.state_digest(state), TC.state_digest(states[f][b])), f"{name}, frame {f}, stream {b}: the tracks held"
    assert st.guard_bytes == 0
    print(f"{name}: the greedy entry on these inputs: shown {[[int(o['num_out']) for o in fr] for fr in outs]}: equal to the greedy restatement, bit for bit")


def test_refusals_reach_python():
    c = HC.build_case("n64_age0")
    st = Stepper(c)
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


def case_annos(c, f, b):
    fr = c["frames"][f]
    return [dict(sample_token=f"s{f}", translation=fr["rec"][b, i, 0:3].tolist(), size=fr["rec"][b, i, 3:6].tolist(), rotation=fr["rec"][b, i, 6:10].tolist(),
                 velocity=fr["rec"][b, i, 10:12].tolist(), detection_name=TC.CLASS_NAMES[int(fr["name"][b, i])], detection_score=float(fr["score"][b, i]),
                 attribute_name="") for i in range(int(fr["kept"][b]))]


def test_step_and_track_file(tmp_path):
    name = "reset_midway"
    c, e = HC.build_case(name), HC.expected(name)
    trk = toc3d_amd.build_tracker(hungarian=True, max_age=c["max_age"])
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
    path = toc3d_amd.build_tracker(hungarian=True, max_age=c["max_age"]).track_file(str(tmp_path / "results_nusc.json"), frames, str(tmp_path / "out"))
    got = json.load(open(path))
    assert list(got) == ["results", "meta"] and got["meta"] == tracking.TRACKING_META and got["results"] == want
    greedy = TC.expected(name)
    assert any(not np.array_equal(greedy["track_id"][f], e["track_id"][f]) for f in range(len(frames))), "the case tells the two assignments apart"
    print(f"step and track_file on {name} with hungarian=True: {sum(map(len, want.values()))} tracking records over {len(frames)} frames equal the reference's")


# ---- the detector ------------------------------------------------------------------------------------------------------------------------------------------------
TINY = synth.DETECTOR_TINY
WIDE = dict(max_depth=1e4, class_range={n: 1e4 for n in TC.CLASS_NAMES})     # no box of the synthetic detector is beyond its class range: more records to track
BANK = ("memory_embedding", "memory_reference_point", "memory_timestamp", "memory_egopose", "memory_velo")


def build_detector(precision):
    det = toc3d_amd.build_detector(synth.detector_cfg(TINY), precision=precision)
    det.load_state_dict(synth.detector_state_dict(TINY), strict=True)
    det = det.to(DEV)
    det.img_backbone.autotune = det.img_neck.autotune = False
    tuned = os.path.join(ROOT, "toc3d_amd", "tuned", f"{TINY['backbone']}_320x800_{precision}.json")
    if os.path.exists(tuned):
        det.img_backbone.load_tuning(tuned)
        det.img_neck._tuned.update(det.img_backbone._tuned)
    return det


def run(det, frames):
    seen, res = [], []
    hook = det.pts_bbox_head.register_forward_hook(lambda m, a, out: seen.append(out))
    try:
        for fr in frames:
            results = det.simple_test(fr["img_metas"], gumbel_noise=fr["gumbel"], **fr["dev"])
            last, outs = det.last_frame, seen[-1]
            res.append(dict(keep=[k.clone() for k in last["keep_idxes"]], img_feats=last["img_feats"].clone(),
                            out={k: outs[k].clone() for k in ("all_cls_scores", "all_bbox_preds")}, bank={k: getattr(det.pts_bbox_head, k).clone() for k in BANK},
                            dec=results[0]["pts_bbox"]))
    finally:
        hook.remove()
    return res


def test_detector_keeps_its_bits_and_tracks_the_records_with_hungarian():
    import nusc_results_cases as NC
    pose = NC.pose_records(NC.random_poses(np.random.default_rng(40), 1))[0]
    frames = []
    for f, fr in enumerate(synth.detector_inputs(dict(TINY, new_scene_at=2))[:3]):
        frames.append(dict(img_metas=[dict(fr["img_metas"][0], sample_idx=f"sample{f}", **pose)], gumbel=fr["gumbel"], dev=to_dev(fr)))      # one pose: the scene stands still
    plain = run(build_detector("fp32x3").enable_nusc_results(**WIDE), frames)
    det = build_detector("fp32x3").enable_nusc_results(**WIDE).enable_tracking(max_age=3, score_threshold=0.0, hungarian=True)
    assert isinstance(det.tracker, toc3d_amd.HungarianPubTracker)
    got = run(det, frames)
    for f, (x, y) in enumerate(zip(got, plain)):
        assert all(torch.equal(p, q) for p, q in zip(x["keep"], y["keep"])) and torch.equal(x["img_feats"], y["img_feats"]), f"frame {f}: kept sets, img_feats"
        assert all(torch.equal(x["out"][k], y["out"][k]) for k in x["out"]) and all(torch.equal(x["bank"][k], y["bank"][k]) for k in BANK), f"frame {f}: head outputs, bank"
        assert all(torch.equal(torch.as_tensor(x["dec"][k]), torch.as_tensor(y["dec"][k])) for k in ("boxes_3d", "scores_3d", "labels_3d")), f"frame {f}: decoded lists"
    tokens = [f"sample{f}" for f in range(3)]
    assert list(det.tracking_results) == tokens == list(det.nusc_results.results)
    ts = [float(fr["dev"]["timestamp"][0]) for fr in frames]
    trk, want = toc3d_amd.build_tracker(hungarian=True, max_age=3), {}
    for token, t, first in zip(tokens, ts, [True, False, True]):
        want[token] = trk.items_to_annos(trk.step([det.nusc_results.results[token]], [t], [first], 0.0)[0], token)
    assert det.tracking_results == want and sum(map(len, want.values())) > 0
    print(f"fp32x3: three frames (a new scene at the third) with enable_tracking(hungarian=True) equal a detector without tracking bit for bit; tracking ids per frame "
          f"{[[a['tracking_id'] for a in want[t]] for t in tokens]}: equal to a stand-alone HungarianPubTracker fed the gathered records")
