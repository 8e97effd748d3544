"""The device half of the tracking tests, shared by tests/test_gpu_tracking.py and tests/test_gpu_tracking_hungarian.py: an entry point of include/toc3d_tracks.h
or include/toc3d_assign.h stepped over a case between guard bytes (``Stepper``), a whole run held to a fixture (``run_against_fixture``), and the records and
tracking file of a tracker class on one case (``step_and_track_file``).  Parametrised by the entry point, its output keys and the cases module
(tests/tracking_cases.py or tests/tracking_hungarian_cases.py); importing it needs no GPU."""
import json

import numpy as np
import torch

import tracking_cases as TC
from support import DEV, S, guarded, touched
from toc3d_amd import lib, tracking

SHAPES = dict(track_id="BK", active="BK", order="BK", num_out="B", rounds="B")
DTYPES = dict(track_id=np.int32, active=np.int32, order=np.int32, num_out=np.int64, rounds=np.int32)
dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Stepper:
    """The entry point ``entry`` with outputs ``out_keys`` stepped on a case's streams ``streams``: two guarded state buffers swapped after every step, every output
    between guard bytes."""

    def __init__(self, c, entry, out_keys, streams=None, extra_capacity=0):
        self.c, self.entry, self.keys, self.streams = c, entry, out_keys, list(range(c["B"])) if streams is None else list(streams)
        self.B, self.K = len(self.streams), c["K"]
        self.cap = tracking.capacity_for(self.K, c["max_age"]) + extra_capacity
        self.sbytes = tracking.state_bytes(self.cap)
        assert self.sbytes == TC.state_bytes(self.cap)
        self.state = [guarded(self.B * self.sbytes), guarded(self.B * self.sbytes)]       # (the fill is no valid state: the first step must not depend on it)
        if c.get("init") is not None:
            raw = np.concatenate([TC.state_to_bytes(c["init"][b], c["init_last"][b], self.cap) for b in self.streams])
            self.state[0][1].copy_(dv(raw))
        self.label, self.gate = dv(TC.track_label_table()), dv(TC.max_diff_table())
        self.guard_bytes = 0

    def step(self, f):
        fr, B, K, s = self.c["frames"][f], self.B, self.K, self.streams
        shapes = {k: (B, K) if SHAPES[k] == "BK" else (B,) for k in self.keys}
        bufs = {k: guarded(int(np.prod(shapes[k])) * np.dtype(DTYPES[k]).itemsize) for k in self.keys}
        read = self.state[0][1].clone()
        lib.call(self.entry, dv(fr["rec"][s]), dv(fr["score"][s]), dv(fr["name"][s]), dv(fr["kept"][s]), B, K, self.label, len(TC.CLASS_NAMES), self.gate,
                 len(TC.TRACKING_NAMES), float(self.c["thr"]), self.c["max_age"], dv(fr["timestamp"][s]), dv(fr["first"][s]), self.state[0][1], self.state[1][1], self.cap,
                 *[bufs[k][1] for k in self.keys], S())
        torch.cuda.synchronize()
        assert torch.equal(read, self.state[0][1]), "the state a step reads is left as it was"
        self.state.reverse()
        out = {k: bufs[k][1].cpu().numpy().view(DTYPES[k]).reshape(shapes[k]) for k in self.keys}
        self.guard_bytes += sum(touched(bufs[k][0], bufs[k][1].numel()) for k in self.keys) + sum(touched(b, self.B * self.sbytes) for b, _ in self.state)
        return out

    def raw_state(self):
        return self.state[0][1].cpu().numpy().reshape(self.B, self.sbytes)


def run_against_fixture(name, entry, out_keys, cases, streams=None, extra_capacity=0):
    """The case ``name`` of the module ``cases`` through ``entry`` against that module's fixture -> (what the test prints, all output and state bytes of the run).
    ``rounds`` is compared where it is among ``out_keys``."""
    c, e = cases.build_case(name), cases.expected(name)
    st = Stepper(c, entry, out_keys, streams, extra_capacity)
    rounds = "rounds" in out_keys
    trace, dirty = [], 0
    for f in range(len(c["frames"])):
        out = st.step(f)
        raw = st.raw_state()
        for i, b in enumerate(st.streams):
            tag = f"{name}, frame {f}, stream {b}"
            for k in ("track_id", "active", "order"):
                assert np.array_equal(out[k][i], e[k][f, b]), f"{tag}: {k}"
            assert out["num_out"][i] == e["num_out"][f, b], f"{tag}: num_out"
            if rounds:
                assert out["rounds"][i] == e["rounds"][f, b], f"{tag}: the solver made {out['rounds'][i]} scan rounds, the restated one {e['rounds'][f, b]}"
            state, last, d = TC.bytes_to_state(raw[i], st.cap)
            cases.compare_state(tag, state, e, f, b)
            assert last == c["frames"][f]["timestamp"][b], f"{tag}: last_timestamp"
            dirty += d
        trace += [out[k].tobytes() for k in out_keys] + [raw.tobytes()]
    assert dirty == 0, f"{name}: {dirty} bytes of the states at or beyond count are not zero"
    assert st.guard_bytes == 0, f"{name}: {st.guard_bytes} guard bytes written"
    line = f"{name}: K {c['K']}, max_age {c['max_age']}, capacity {st.cap}: shown {e['num_out'][:, st.streams].tolist()}, held {e['count'][:, st.streams].tolist()}"
    if rounds:
        line += f", rounds {e['rounds'][:, st.streams].tolist()}: ids, active, order, num_out, rounds and every bit of the tracks equal the reference's; 0 guard bytes written"
    else:
        line += ": ids, active, order, num_out and every bit of the tracks equal the reference's; 0 guard bytes written"
    return line, trace


def step_and_track_file(make, cases, name, tmp_path):
    """A tracker ``make()`` stepped over the records of the case (stream 0) with ``step``, each frame's items held to the fixture; then a second one over the same
    records as a file, with ``track_file`` -> (the file's path, its content, the records the reference makes, the frames)."""
    c, e = cases.build_case(name), cases.expected(name)
    trk = make()
    results, frames, want = {}, [], {}
    for f, fr in enumerate(c["frames"]):
        annos = TC.case_annos(c, f, 0)
        items = trk.step([annos], [float(fr["timestamp"][0])], [bool(fr["first"][0])], c["thr"])[0]
        rows = e["order"][f, 0, :int(e["num_out"][f, 0])].tolist()
        assert [x["tracking_id"] for x in items] == e["track_id"][f, 0, rows].tolist() and [x["active"] for x in items] == e["active"][f, 0, rows].tolist()
        assert all({k: v for k, v in x.items() if k not in ("tracking_id", "active")} == annos[r] for x, r in zip(items, rows))
        results[f"s{f}"], frames = annos, frames + [dict(token=f"s{f}", timestamp=float(fr["timestamp"][0]), first=bool(fr["first"][0]))]
        want[f"s{f}"] = TC.want_annos(annos, e, f, rows)
    with open(tmp_path / "results_nusc.json", "w") as fh:
        json.dump(dict(meta=None, results=results), fh)
    path = make().track_file(str(tmp_path / "results_nusc.json"), frames, str(tmp_path / "out"))
    return path, json.load(open(path)), want, frames
