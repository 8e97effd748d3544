"""The cases of the Hungarian tracking tests and a numpy restatement of the step (include/toc3d_assign.h: points 0-3 and 6 of include/toc3d_tracks.h, points 4h
and 5h), shared by tests/test_cpu_tracking_hungarian.py, tests/test_gpu_tracking_hungarian.py, tools/gen_golden_tracking_hungarian.py and
tools/tracking_hungarian_time.py.  Built on tests/tracking_cases.py: its Tracker with another ``_assign``, its ``run_case`` and its fixture reader.

The fixture (tests/golden/tracking_hungarian_cases.npz, written by tools/gen_golden_tracking_hungarian.py where the reference tree and scipy exist) holds what the
REFERENCE's PubTracker(hungarian=True) returned and held on these cases, per frame and stream, laid out as the greedy fixture is, and beside it the scan rounds of
the restated solver and the flags the generator computed per frame (what a frame is a witness of).

THE SOLVER is scipy's rectangular shortest augmenting path (scipy/optimize/rectangular_lsap), restated operation for operation: its float64 arithmetic on the
reference's matrix -- 1e18 for an invalid pair beside distances of 2.5 at most -- decides which matches come out, not optimality: once a dual variable is of the
size of 1e18, whose neighbours are 128 apart, the small costs are absorbed.  :func:`solve` needs no scipy; where scipy imports, the CPU test holds it to
``linear_sum_assignment`` on 3000 seeded matrices.
"""
import os

import numpy as np

import tracking_cases as TC
from tracking_cases import BUS, CAR, PEDESTRIAN, TRACKED, TRUCK

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tracking_hungarian_cases.npz")
INVALID, SHOWN_BELOW, CLEAN_INVALID = 1e18, 1e16, 1e4      # pub_tracker.py:126-128, :146; the invalid cost of the uncontaminated solve the flags compare against
MAX_BOXES, MAX_TRACKS, PASS = 512, 2048, 256               # TOC3D_ASSIGN_MAX_BOXES, _MAX_TRACKS; the list positions one pass of the kernel's workgroup covers
OUT_KEYS = TC.OUT_KEYS + ("rounds",)
FLAGS = ("differs_from_greedy", "differs_from_clean", "quirk_b", "quirk_a", "ties")


def solve(cost):
    """``cost`` (N, M) float64, every entry finite, N, M >= 1 -> (detections, tracks, rounds): the min(N, M) pairs scipy's ``linear_sum_assignment`` returns,
    sorted by detection, and the scan rounds made.  The scan of a round is one vector operation over the list; every float64 operation is rounded once, in scipy's
    order."""
    cost = np.asarray(cost, dtype=np.float64)
    transposed = cost.shape[0] > cost.shape[1]                               # N > M: rows are tracks, columns detections
    c = np.ascontiguousarray(cost.T) if transposed else cost
    nr, nc = c.shape
    u, v = np.zeros(nr), np.zeros(nc)
    col4row, row4col, path = np.full(nr, -1, np.int64), np.full(nc, -1, np.int64), np.full(nc, -1, np.int64)
    rounds = 0
    for cur in range(nr):
        min_val, i, sink = np.float64(0.0), cur, -1
        remaining, nrem = np.arange(nc - 1, -1, -1), nc
        spc = np.full(nc, np.inf)
        sr, sc = np.zeros(nr, dtype=bool), np.zeros(nc, dtype=bool)
        for _ in range(cur + 1):                                             # every cost is finite: a row's search takes at most cur + 1 rounds
            rounds += 1
            sr[i] = True
            js = remaining[:nrem]
            r = ((min_val + c[i, js]) - u[i]) - v[js]
            upd = r < spc[js]
            path[js[upd]], spc[js[upd]] = i, r[upd]
            s = spc[js]
            low = s.min()
            eq = s == low
            free = np.nonzero(eq & (row4col[js] == -1))[0]
            pick = free[-1] if len(free) else np.nonzero(eq)[0][0]          # the last unassigned column of the smallest, else the first of the smallest
            min_val, j = low, js[pick]
            if row4col[j] == -1:
                sink = j
            else:
                i = row4col[j]
            sc[j] = True
            nrem -= 1
            remaining[pick] = remaining[nrem]
            if sink >= 0:
                break
        assert sink >= 0
        u[cur] += min_val
        sr[cur] = False
        rows = np.nonzero(sr)[0]
        u[rows] += min_val - spc[col4row[rows]]
        cols = np.nonzero(sc)[0]
        v[cols] -= min_val - spc[cols]
        j = sink
        while True:
            i = path[j]
            row4col[j] = i
            col4row[i], j = j, col4row[i]
            if i == cur:
                break
    if transposed:
        order = np.argsort(col4row, kind="stable")
        return col4row[order], order, rounds
    return np.arange(nr), col4row, rounds


def cost_matrix(p, q, dl, tl, max_diff, invalid=INVALID):
    """pub_tracker.py:119-128: float32 distances, every operation rounded once, as float64 where the pair is valid (same label, not beyond the gate, a number)
    and ``invalid`` elsewhere -> (cost (N, M) float64, valid (N, M) bool)."""
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy = q[None, :, 0] - p[:, None, 0], q[None, :, 1] - p[:, None, 1]
        d = np.sqrt(dx * dx + dy * dy)
        assert d.dtype == np.float32
        valid = (tl[None, :] == dl[:, None]) & (d <= max_diff[dl][:, None])
    return np.where(valid, d.astype(np.float64), np.float64(invalid)), valid


def greedy_pairs(cost, valid):
    """track_utils.py:7-11 on the same matrix -> the set of (detection, track)."""
    taken, pairs = np.zeros(cost.shape[1], dtype=bool), set()
    for i in range(cost.shape[0]):
        idx = np.nonzero(valid[i] & ~taken)[0]
        if len(idx):
            j = int(idx[np.argmin(cost[i, idx])])
            taken[j] = True
            pairs.add((i, j))
    return pairs


def has_ties(cost, valid):
    """Two valid pairs of one detection, or of one track, at exactly the same distance."""
    for m in (np.where(valid, cost, np.nan), np.where(valid, cost, np.nan).T):
        s = np.sort(m, axis=1)
        if (s[:, 1:] == s[:, :-1]).any():
            return True
    return False


class Tracker(TC.Tracker):
    """One stream's tracker with ``hungarian=True``, restated: the greedy step with another assignment.  ``seen``: what the last step saw where it had both
    detections and tracks (the matrix, the matches), for the generator's flags; ``None`` otherwise."""
    EXTRA_OUT = dict(rounds=np.int32(0))

    def _assign(self, p, q, dl, state):
        """Points 4h-5h: the solver on the reference's matrix; a detection in a match that costs more than 1e16 is parked -- unmatched and numbered last (quirk B)
        -- and its track is gone (quirk A)."""
        N, M = len(p), len(state["label"])
        match = np.full(N, -1, dtype=np.int64)                              # the track of a detection's valid match
        parked = np.zeros(N, dtype=bool)                                    # the detection is in a match that costs more than 1e16
        taken = np.zeros(M, dtype=bool)                                     # the track is in a match, valid or not
        if not M:
            return match, taken, parked, {}
        cost, valid = cost_matrix(p, q, dl, state["label"], self.max_diff)
        di, tj, rounds = solve(cost)
        taken[tj] = True
        good = cost[di, tj] <= SHOWN_BELOW
        match[di[good]], parked[di[~good]] = tj[good], True
        lost = taken.copy()
        lost[tj[good]] = False                                              # quirk A: the tracks in an invalid match are gone, the young ones too
        self.seen = dict(cost=cost, valid=valid, pairs={(int(a), int(b)) for a, b in zip(di[good], tj[good])}, N=N, M=M, parked=parked.copy(),
                         dropped_young=bool((lost & (state["age"] < self.max_age)).any()))
        return match, taken, parked, dict(rounds=np.int32(rounds))


def run_case(c, streams=None, on_step=None):
    return TC.run_case(c, streams, on_step, Tracker)


def frame_flags(seen, clean_pairs):
    """What a frame is a witness of, from the restatement's view of it (``Tracker.seen``) and the valid matches of the uncontaminated solve."""
    if seen is None:
        return [False] * len(FLAGS)
    parked = np.nonzero(seen["parked"])[0]
    free = np.nonzero(~seen["parked"] & ~np.isin(np.arange(seen["N"]), [a for a, _ in seen["pairs"]]))[0]
    quirk_b = seen["N"] > seen["M"] and len(parked) > 0 and len(free) > 0 and parked.min() < free.max()       # a parked detection numbered after a later unmatched one
    return [seen["pairs"] != greedy_pairs(seen["cost"], seen["valid"]), seen["pairs"] != clean_pairs, bool(quirk_b), seen["dropped_young"], has_ties(seen["cost"], seen["valid"])]


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------------------------------------
def given_case(seed, K, M, nframes, classes, max_age=3, spacing=1.5, nobj=None, **kw):
    """A scene of K surviving detections a frame (tracked classes only, a threshold below every score) continued from a given state of M tracks, so that the first
    frame solves K x M."""
    nobj = int(K * 1.4) + 2 if nobj is None else nobj
    c = TC.scene_case(seed, K, nframes, nobj, max_age, thr=0.01, classes=classes, spacing=spacing, **kw)
    for fr in c["frames"]:
        fr["first"][:] = 0
    c["init"], c["init_last"] = [TC.full_state(seed, M, classes, spacing * np.sqrt(nobj))], [TC.T0 - 0.5]
    return c


def counts_case():
    """N and M in {1, 2}: max_age 0 holds exactly the last frame's detections, so the frames solve 1 x 1, 2 x 1, 2 x 2, 1 x 2 and 1 x 1."""
    a, b = (5.0, 5.0, 0.0, 0.0, CAR, 0.9), (6.0, 5.5, 0.0, 0.0, CAR, 0.8)
    return TC.manual_case(4, 0, [[a], [a], [b, a], [a, b], [b], [a]])


def quirk_a_case():
    """Two tracks and a frame whose second detection is far from both: the second track is parked with it and gone, at age 1 of max_age 3; greedy keeps it."""
    a, b, far = (5.0, 5.0, 0.0, 0.0, CAR, 0.9), (15.0, 5.0, 0.0, 0.0, CAR, 0.8), (95.0, 5.0, 0.0, 0.0, CAR, 0.7)
    return TC.manual_case(4, 3, [[a, b], [a, far], [a, b], [a, far, b], [b, far]])


def quirk_b_case():
    """One track and detections at 10, 20 and 30 m: the solver parks one of them on the track at 1e18, and that one is numbered last (ids 3, 4, 2 in row order)."""
    d = lambda x, s: (x, 0.0, 0.0, 0.0, TRUCK, s)
    return TC.manual_case(4, 0, [[d(0.0, 0.9)], [d(10.0, 0.9), d(20.0, 0.8), d(30.0, 0.7)], [d(10.0, 0.9)], [d(40.0, 0.9), d(10.0, 0.8), d(60.0, 0.7), d(70.0, 0.6)],
                                 [d(10.0, 0.9), d(90.0, 0.8)], [d(91.0, 0.9), d(11.0, 0.8), d(50.0, 0.7)]])


def ties_case():
    """Exact ties among valid pairs: tracks on a line two metres apart and detections half-way between them (each at exactly 1.0 from two tracks), then duplicate
    tracks (two detections at one place make them), then detections on the tracks' other side."""
    on = lambda xs, y=0.0: [(float(x), y, 0.0, 0.0, PEDESTRIAN, 0.9 - 0.01 * k) for k, x in enumerate(xs)]
    return TC.manual_case(16, 3, [on([0, 2, 4, 6, 8]), on([1, 3, 5, 7]), on([2, 2, 4, 4, 6]), on([3, 5, 3]), on([4, 2, 4, 6, 2, 6]), on([3, 3, 5, 5], 0.0), on([4, 4], 1.0)])


def all_invalid_case():
    """Every pair invalid: the same places under another label, then more detections than tracks far from all of them."""
    at = lambda cls, xs: [(float(x), 0.0, 0.0, 0.0, cls, 0.9) for x in xs]
    return TC.manual_case(8, 3, [at(CAR, [0, 10, 20]), at(BUS, [0, 10, 20]), at(CAR, [100, 110, 120, 130, 140, 150, 160, 170]), at(TRUCK, [0, 10])])


MANUAL = {
    "counts_1_2": counts_case, "quirk_a": quirk_a_case, "quirk_b": quirk_b_case, "ties": ties_case, "all_invalid": all_invalid_case,
    "tie_tracks": TC.MANUAL["tie_tracks"], "tie_dets": TC.MANUAL["tie_dets"], "gate_and_labels": TC.MANUAL["gate_and_labels"], "motion": TC.MANUAL["motion"],
}
SCENES = {
    "first_frame_n1": TC.SCENES["first_frame_n1"],
    "empty_twice_age0": TC.SCENES["empty_twice_age0"], "empty_twice_age3": TC.SCENES["empty_twice_age3"], "kept_zero": TC.SCENES["kept_zero"],
    "reset_midway": TC.SCENES["reset_midway"], "n65_mixed": TC.SCENES["n65_mixed"], "n64_age0": TC.SCENES["n64_age0"],            # N = M = K = 64 on every frame but the first
    "streams3": TC.SCENES["streams3"],
    "scene300": lambda: TC.scene_case(31, 300, 4, 400, 3, classes=TRACKED, spacing=1.5),
    # 63, 64 and 65 both ways, one label, crowded; rows are detections when N <= M and tracks when N > M
    **{f"n40_m{m}_one_label": (lambda m=m: given_case(40 + m, 40, m, 2, (CAR,), spacing=1.0)) for m in (63, 64, 65)},
    **{f"n{n}_m40_one_label": (lambda n=n: given_case(50 + n, n, 40, 2, (CAR,), spacing=1.0)) for n in (63, 64, 65)},
    # one below, at and one above the list positions one pass of the workgroup covers, both ways, seven labels
    **{f"n100_m{m}": (lambda m=m: given_case(60 + m, 100, m, 2, TRACKED)) for m in (PASS - 1, PASS, PASS + 1)},
    **{f"n{n}_m100": (lambda n=n: given_case(70 + n, n, 100, 2, TRACKED)) for n in (PASS - 1, PASS, PASS + 1)},
    "n128_m128_one_label": lambda: given_case(81, 128, 128, 2, (PEDESTRIAN,), spacing=0.8),
    # at the caps: 512 rows, 2048 tracks, one label, crowded
    "caps_one_label": lambda: given_case(82, MAX_BOXES, MAX_TRACKS, 1, (CAR,), spacing=0.7),
}
CASES = tuple(MANUAL) + tuple(SCENES)
STREAMS_CASE, CAPS_CASE = "streams3", "caps_one_label"
_BUILT = {}


def build_case(name):
    if name not in _BUILT:
        _BUILT[name] = (MANUAL.get(name) or SCENES[name])()
    return _BUILT[name]


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------------------------------------------
def pack_expected(prefix, outs, states, rounds, flags, arrays):
    """As tracking_cases.pack_expected, with ``rounds`` [frame][stream] and ``flags`` [frame][stream][len(FLAGS)] beside."""
    TC.pack_expected(prefix, outs, states, arrays)
    arrays[f"{prefix}/rounds"] = np.asarray(rounds, dtype=np.int32)
    arrays[f"{prefix}/flags"] = np.asarray(flags, dtype=bool)


def expected(name):
    """-> what tracking_cases.expected returns, read from this fixture, with ``rounds`` [F, B] int32 and ``flags`` [F, B, len(FLAGS)] bool."""
    return TC.expected(name, FIXTURE, ("rounds", "flags"))


compare_state = TC.compare_state
