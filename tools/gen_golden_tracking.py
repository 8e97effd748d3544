"""Generates tests/golden/tracking_cases.npz: what the REFERENCE's PubTracker (nusc_tracking/pub_tracker.py, track_utils.py) returns and holds on the cases of
tests/tracking_cases.py, driven frame by frame as nusc_tracking/pub_test.py:97-112 drives it (reset and last_time_stamp on a first frame, time_lag as the
difference of two Python floats).

Runs only where the reference tree exists (oracle/ref_harness.py: REF): the reference's module is imported from there at generation time, with numpy and scipy;
none of its text is copied.  Per case the archive holds, per frame and stream, track_id / active per input row, the rows in output order, num_out, and the tracks
after the frame (in full for the small cases, as a SHA-256 always: tests/tracking_cases.py).  The inputs are made again from seeds by that module; the near-tie
rows, which come out of a seeded search, are stored, and their count is asserted here (tracking_cases.check_near_ties): at least 4 detections whose match a fused
multiply-add would change, at least 4 whose 2.5 m gate it would change.  The restatement of tests/tracking_cases.py is held to the reference on every case before
anything is written.

Written with fixed zip timestamps, so a second run reproduces the archive byte for byte.
"""
import contextlib
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tracking_cases as TC                      # noqa: E402
from oracle.ref_harness import REF               # noqa: E402
from tools.gen_golden_focal_head import save_npz  # noqa: E402


def reference_tracker():
    path = os.path.join(REF, "nusc_tracking")
    if not os.path.isdir(path):
        raise RuntimeError(f"reference tree not found at {REF}: this tool runs where the reference exists")
    sys.path.insert(0, path)
    import pub_tracker
    assert tuple(pub_tracker.NUSCENES_TRACKING_NAMES) == TC.TRACKING_NAMES and set(pub_tracker.NUSCENE_CLS_VELOCITY_ERROR.values()) == {TC.MAX_DIFF}
    return pub_tracker.PubTracker


def detections(fr, b):
    """The dicts results_nusc.json holds for a sample, with the input row beside them."""
    return [dict(translation=fr["rec"][b, i, 0:3].tolist(), velocity=fr["rec"][b, i, 10:12].tolist(), detection_name=TC.CLASS_NAMES[int(fr["name"][b, i])],
                 detection_score=float(fr["score"][b, i]), row=i) for i in range(int(fr["kept"][b]))]


def held(tracker):
    t = tracker.tracks
    return dict(ct=np.array([x["ct"] for x in t], dtype=np.float64).reshape(-1, 2), tracking=np.array([x["tracking"] for x in t], dtype=np.float64).reshape(-1, 2),
                label=np.array([x["label_preds"] for x in t], dtype=np.int32), tracking_id=np.array([x["tracking_id"] for x in t], dtype=np.int32),
                age=np.array([x["age"] for x in t], dtype=np.int32), active=np.array([x["active"] for x in t], dtype=np.int32), id_count=int(tracker.id_count))


def run_reference(PubTracker, c):
    B, K = c["B"], c["K"]
    outs, states = [[None] * B for _ in c["frames"]], [[None] * B for _ in c["frames"]]
    for b in range(B):
        with contextlib.redirect_stdout(io.StringIO()):
            tracker = PubTracker(hungarian=False, max_age=c["max_age"])
        last = None
        if c.get("init") is not None:
            s = c["init"][b]
            tracker.id_count = int(s["id_count"])
            tracker.tracks = [dict(ct=s["ct"][t].copy(), tracking=s["tracking"][t].copy(), label_preds=int(s["label"][t]), tracking_id=int(s["tracking_id"][t]),
                                   age=int(s["age"][t]), active=int(s["active"][t])) for t in range(len(s["label"]))]
            last = float(c["init_last"][b])
        for f, fr in enumerate(c["frames"]):
            ts = float(fr["timestamp"][b])
            if fr["first"][b]:                                              # pub_test.py:101-105
                tracker.reset()
                last = ts
            lag = ts - last                                                 # :107-108
            last = ts
            ret = tracker.step_centertrack(detections(fr, b), lag, c["thr"])
            out = dict(track_id=np.zeros(K, np.int32), active=np.zeros(K, np.int32), order=np.full(K, -1, np.int32))
            shown = [x for x in ret if x["active"] > 0]                     # the unmatched tracks the reference returns as well have active 0 (pub_test.py:116 skips them)
            assert all(x["age"] == 1 for x in shown) and all(x is y for x, y in zip(ret, shown))
            for k, x in enumerate(shown):
                out["order"][k], out["track_id"][x["row"]], out["active"][x["row"]] = x["row"], x["tracking_id"], x["active"]
            out["num_out"] = np.int64(len(shown))
            outs[f][b], states[f][b] = out, held(tracker)
    return outs, states


def main():
    PubTracker = reference_tracker()
    choice, gate = TC.search_near_ties()
    TC.check_near_ties(choice, gate)
    print(f"near ties: {len(choice)} detections whose match a fused multiply-add changes, {len(gate)} whose gate it changes")
    arrays = dict(near_choice=choice, near_gate=gate)
    TC._BUILT[TC.NEAR_TIES] = TC.near_tie_case(choice, gate)
    rows = 0
    for name in TC.CASES:
        c = TC.build_case(name)
        outs, states = run_reference(PubTracker, c)
        mine, mine_states = TC.run_case(c)
        for f in range(len(outs)):
            for b in range(c["B"]):
                for k in TC.OUT_KEYS:
                    assert np.array_equal(mine[f][b][k], outs[f][b][k]), f"{name}, frame {f}, stream {b}: the restatement's {k} is not the reference's"
                assert np.array_equal(TC.state_digest(mine_states[f][b]), TC.state_digest(states[f][b])), f"{name}, frame {f}, stream {b}: tracks held"
        TC.pack_expected(name, outs, states, arrays)
        rows += int(arrays[f"{name}/num_out"].sum())
        print(f"case {name}: K {c['K']}, B {c['B']}, max_age {c['max_age']}: shown {arrays[f'{name}/num_out'].tolist()}, held {arrays[f'{name}/count'].tolist()}, "
              f"last id {arrays[f'{name}/id_count'][-1].tolist()}; the restatement agrees bit for bit")
    arrays["generated_by"] = np.array("the reference's nusc_tracking.pub_tracker.PubTracker (greedy), driven as nusc_tracking/pub_test.py drives it")
    save_npz(TC.FIXTURE, **arrays)
    print(f"wrote {TC.FIXTURE}: {len(TC.CASES)} cases, {rows} rows shown, {os.path.getsize(TC.FIXTURE)} bytes")


if __name__ == "__main__":
    main()
