"""Generates tests/golden/tracking_hungarian_cases.npz: what the REFERENCE's PubTracker(hungarian=True) (nusc_tracking/pub_tracker.py, with scipy's
linear_sum_assignment) returns and holds on the cases of tests/tracking_hungarian_cases.py, driven frame by frame as nusc_tracking/pub_test.py:97-112 drives it.

Runs only where the reference tree and scipy exist; the reference's module is imported from there at generation time and none of its text is copied.  The layout
is the greedy fixture's (tools/gen_golden_tracking.py, whose helpers are imported), with per frame and stream the scan rounds of the restated solver and the flags
of tracking_hungarian_cases.FLAGS beside.  The restatement is held to the reference on every case before anything is written -- outputs, tracks held, and its
solver's pairs and rounds against scipy's pairs and a second, element-by-element replay's rounds -- and the counts the tests rely on are asserted here:
frames whose valid matches differ from greedy's and from an uncontaminated solve's (invalid pairs at 1e4 instead of 1e18), frames with quirks A and B, frames with
exact ties.  The scipy version is recorded.  Written with fixed zip timestamps, so a second run reproduces the archive byte for byte.
"""
import contextlib
import io
import os
import sys

import numpy as np
import scipy
from scipy.optimize import linear_sum_assignment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tracking_cases as TC                                              # noqa: E402
import tracking_hungarian_cases as HC                                    # noqa: E402
from tools.gen_golden_focal_head import save_npz                         # noqa: E402
from tools.gen_golden_tracking import detections, held, reference_tracker  # noqa: E402

MINIMUM = dict(differs_from_greedy=8, differs_from_clean=8, quirk_b=4, quirk_a=4, ties=4)


def rounds_by_elements(cost):
    """The scan rounds of scipy's loop, replayed element by element (no vector operation): what HC.solve's count is held to."""
    c = cost.T if cost.shape[0] > cost.shape[1] else cost
    nr, nc = c.shape
    u, v, col4row, row4col, path, rounds = [0.0] * nr, [0.0] * nc, [-1] * nr, [-1] * nc, [-1] * nc, 0
    c = c.tolist()
    for cur in range(nr):
        min_val, i, sink, remaining, nrem = 0.0, cur, -1, list(range(nc - 1, -1, -1)), nc
        spc, sr, sc = [float("inf")] * nc, [False] * nr, [False] * nc
        while sink == -1:
            rounds += 1
            sr[i], index, lowest = True, -1, float("inf")
            for it in range(nrem):
                j = remaining[it]
                r = min_val + c[i][j] - u[i] - v[j]
                if r < spc[j]:
                    path[j], spc[j] = i, r
                if spc[j] < lowest or (spc[j] == lowest and row4col[j] == -1):
                    lowest, index = spc[j], it
            min_val, j = lowest, remaining[index]
            if row4col[j] == -1:
                sink = j
            else:
                i = row4col[j]
            sc[j] = True
            nrem -= 1
            remaining[index] = remaining[nrem]
        u[cur] += min_val
        for i in range(nr):
            if sr[i] and i != cur:
                u[i] += min_val - spc[col4row[i]]
        for j in range(nc):
            if sc[j]:
                v[j] -= min_val - spc[j]
        j = sink
        while True:
            i = path[j]
            row4col[j] = i
            col4row[i], j = j, col4row[i]
            if i == cur:
                break
    return rounds


def run_reference(PubTracker, c):
    B, K = c["B"], c["K"]
    outs, states = [[None] * B for _ in c["frames"]], [[None] * B for _ in c["frames"]]
    for b in range(B):
        with contextlib.redirect_stdout(io.StringIO()):
            tracker = PubTracker(hungarian=True, max_age=c["max_age"])
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
            shown = [x for x in ret if x["active"] > 0]
            assert all(x["age"] == 1 for x in shown) and all(x is y for x, y in zip(ret, shown))
            for k, x in enumerate(shown):
                out["order"][k], out["track_id"][x["row"]], out["active"][x["row"]] = x["row"], x["tracking_id"], x["active"]
            out["num_out"] = np.int64(len(shown))
            outs[f][b], states[f][b] = out, held(tracker)
    return outs, states


def main():
    PubTracker = reference_tracker()
    arrays, totals, rows = {}, dict.fromkeys(HC.FLAGS, 0), 0
    for name in HC.CASES:
        c = HC.build_case(name)
        outs, states = run_reference(PubTracker, c)
        F, B = len(c["frames"]), c["B"]
        flags = [[None] * B for _ in range(F)]

        def on_step(f, b, tracker):
            seen = tracker.seen
            clean = set()
            if seen is not None:
                a, t = linear_sum_assignment(seen["cost"])                  # the restated solver against scipy's, on the reference's matrix
                d, j, r = HC.solve(seen["cost"])
                assert np.array_equal(a, d) and np.array_equal(t, j), f"{name}, frame {f}, stream {b}: the restated solver's pairs are not scipy's"
                if seen["N"] * seen["M"] <= 1 << 16:
                    assert r == rounds_by_elements(seen["cost"]), f"{name}, frame {f}, stream {b}: rounds"
                a, t = linear_sum_assignment(np.where(seen["valid"], seen["cost"], HC.CLEAN_INVALID))
                clean = {(int(x), int(y)) for x, y in zip(a, t) if seen["valid"][x, y]}
            flags[f][b] = HC.frame_flags(seen, clean)

        mine, mine_states = HC.run_case(c, on_step=on_step)
        for f in range(F):
            for b in range(B):
                for k in TC.OUT_KEYS:
                    assert np.array_equal(mine[f][b][k], outs[f][b][k]), f"{name}, frame {f}, stream {b}: the restatement's {k} is not the reference's"
                assert np.array_equal(TC.state_digest(mine_states[f][b]), TC.state_digest(states[f][b])), f"{name}, frame {f}, stream {b}: tracks held"
        rounds = [[int(mine[f][b]["rounds"]) for b in range(B)] for f in range(F)]
        HC.pack_expected(name, outs, states, rounds, flags, arrays)
        for k, flag in enumerate(HC.FLAGS):
            totals[flag] += int(np.asarray(flags)[:, :, k].sum())
        rows += int(arrays[f"{name}/num_out"].sum())
        print(f"case {name}: K {c['K']}, B {B}, max_age {c['max_age']}: shown {arrays[f'{name}/num_out'].tolist()}, held {arrays[f'{name}/count'].tolist()}, rounds {rounds}, "
              f"flags {np.asarray(flags).sum(axis=(0, 1)).tolist()}; the restatement agrees bit for bit")
    print("frames that are witnesses:", totals)
    for flag, least in MINIMUM.items():
        assert totals[flag] >= least, f"{flag}: {totals[flag]} frames, at least {least} wanted"
    arrays["scipy_version"] = np.array(scipy.__version__)
    arrays["generated_by"] = np.array("the reference's nusc_tracking.pub_tracker.PubTracker(hungarian=True), driven as nusc_tracking/pub_test.py drives it, with scipy "
                                      + scipy.__version__)
    save_npz(HC.FIXTURE, **arrays)
    print(f"wrote {HC.FIXTURE}: {len(HC.CASES)} cases, {rows} rows shown, {os.path.getsize(HC.FIXTURE)} bytes")


if __name__ == "__main__":
    main()
