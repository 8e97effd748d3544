"""The cases of the tracking tests and a numpy restatement of the step (include/toc3d_tracks.h, points 0-6), shared by tests/test_cpu_tracking.py,
tests/test_gpu_tracking.py, tools/gen_golden_tracking.py and tools/tracking_time.py, and the base of tests/tracking_hungarian_cases.py, which replaces the
assignment alone.  Beside them: the bytes of a state (``state_to_bytes``, ``bytes_to_state``), the records of a case and the seam the host class is tested through.

The fixture (tests/golden/tracking_cases.npz, written by tools/gen_golden_tracking.py where the reference tree exists) holds what the REFERENCE's PubTracker
returned and held on these cases: per frame and stream the rows in output order with their ids and active counts, and the tracks after the frame.  The inputs are
made again from seeds here (:func:`build_case`); only the near-tie cases, which come out of a search, are stored.  The tracks after a frame are stored in full where
a case holds few of them and as a SHA-256 of their bytes (:func:`state_digest`) always: equality of the digest is equality of every bit.

THE LARGE CASES.  A stream stepped from empty never holds more than K * max_age tracks (for max_age >= 1): a track is made with age 1 and kept only while
age < max_age, so the ages in a state are 1 .. max_age, and a frame adds at most K tracks of age 1.  K = 2048 with max_age = 3 therefore grows to 6144 rows, not to
the 8192 the capacity K * (max_age + 1) allows; the two large cases reach the full 8192 rows by STARTING from a given state of 8192 tracks (``init``), which the
reference is given as well.
"""
import hashlib
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tracking_cases.npz")
CLASS_NAMES = ("car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle", "pedestrian", "traffic_cone")
TRACKING_NAMES = ("car", "truck", "bus", "trailer", "motorcycle", "bicycle", "pedestrian")
MAX_DIFF = 2.5
REC = 12
OUT_KEYS = ("track_id", "active", "order", "num_out")
HEADER_BYTES = 32                        # TOC3D_TRACKS_HEADER_BYTES
STATE_FIELDS = (("ct", 16), ("tracking", 16), ("label", 4), ("tracking_id", 4), ("age", 4), ("active", 4))      # a state's fields in its byte order, bytes per track
STATE_KEYS = tuple(k for k, _ in STATE_FIELDS)
STATE_DTYPES = dict(ct=np.float64, tracking=np.float64, label=np.int32, tracking_id=np.int32, age=np.int32, active=np.int32)
FULL_STATE_ROWS = 600                    # a case whose frames hold at most this many tracks in all has them stored in full
CAR, TRUCK, CONSTRUCTION, BUS, TRAILER, BARRIER, MOTORCYCLE, BICYCLE, PEDESTRIAN, CONE = range(10)
F32 = np.float32


def track_label_table(class_names=CLASS_NAMES, tracking_names=TRACKING_NAMES):
    return np.array([tracking_names.index(n) if n in tracking_names else -1 for n in class_names], dtype=np.int32)


def max_diff_table(tracking_names=TRACKING_NAMES):
    return np.full(len(tracking_names), MAX_DIFF, dtype=np.float32)


def empty_state():
    return dict(ct=np.zeros((0, 2)), tracking=np.zeros((0, 2)), label=np.zeros(0, np.int32), tracking_id=np.zeros(0, np.int32), age=np.zeros(0, np.int32),
                active=np.zeros(0, np.int32), id_count=0)


def state_digest(state):
    """SHA-256 over count, id_count and the live rows' bytes, field by field."""
    h = hashlib.sha256()
    h.update(np.array([len(state["label"]), state["id_count"]], dtype=np.int64).tobytes())
    for k in STATE_KEYS:
        h.update(np.ascontiguousarray(state[k], dtype=STATE_DTYPES[k]).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8).copy()


class Tracker:
    """One stream's tracker, restated: one vector operation over the tracks per detection.  The float32 distance is made of numpy float32 array operations, each
    rounded once (numpy fuses nothing)."""
    EXTRA_OUT = {}                           # outputs beyond OUT_KEYS, with the values an empty frame leaves them at

    def __init__(self, max_age, track_label=None, max_diff=None):
        self.max_age = int(max_age)
        self.track_label = track_label_table() if track_label is None else np.asarray(track_label, dtype=np.int32)
        self.max_diff = max_diff_table() if max_diff is None else np.asarray(max_diff, dtype=np.float32)
        self.last = 0.0
        self.state = empty_state()

    def set_state(self, state, last):
        self.state = {k: (np.array(v, dtype=STATE_DTYPES[k]) if k in STATE_DTYPES else int(v)) for k, v in state.items()}
        self.last = float(last)

    def step(self, rec, score, name, kept, timestamp, first, score_thr):
        """The step in the three parts csrc/tracks_steps.h has: the filter, the assignment, the state write."""
        self.seen = None                                                    # what an assignment that records its view of the frame leaves behind
        out, found = self._filter(rec, score, name, kept, timestamp, first, score_thr)
        if found is None:
            return out
        match, taken, late, extras = self._assign(found["p"], found["q"], found["dl"], self.state)
        out.update(extras)
        self._write(out, found, match, taken, late)
        return out

    def _filter(self, rec, score, name, kept, timestamp, first, score_thr):
        """Points 0-2: the scene start, the time lag, the rows that survive -> (blank outputs, None on an empty frame, else the surviving rows ``rows``, their
        centres ``ct``, displacements ``tracking`` and labels ``dl``, and the float32 positions the distance is taken between: ``p`` predicted, ``q`` held)."""
        K = len(score)
        if first:
            self.state, self.last = empty_state(), float(timestamp)
        lag = np.float64(timestamp) - np.float64(self.last)
        self.last = float(timestamp)
        s = self.state
        n = int(min(max(int(kept), 0), K))
        lab = np.full(K, -1, dtype=np.int64)
        nm = np.asarray(name[:n], dtype=np.int64)
        ok = (nm >= 0) & (nm < len(self.track_label))
        lab[:n][ok] = self.track_label[nm[ok]]
        lab[(lab < 0) | (lab >= len(self.max_diff))] = -1
        keep = lab >= 0
        keep[:n] &= ~(np.asarray(score[:n], dtype=np.float32).astype(np.float64) < np.float64(score_thr))
        rows = np.nonzero(keep)[0]
        N = len(rows)
        out = dict(track_id=np.zeros(K, np.int32), active=np.zeros(K, np.int32), order=np.full(K, -1, np.int32), num_out=np.int64(N), **self.EXTRA_OUT)
        if N == 0:                                                          # the empty-frame quirk: nothing is dropped, the old tracks are left as they are
            young = s["age"] < self.max_age
            s["ct"][young] = s["ct"][young] + s["tracking"][young] * -1.0
            s["age"][young] += 1
            s["active"][young] = 0
            return out, None
        ct = np.asarray(rec, dtype=np.float64)[rows, 0:2]
        tracking = (np.asarray(rec, dtype=np.float64)[rows, 10:12] * -1.0) * lag
        p = (ct + tracking.astype(np.float32).astype(np.float64)).astype(np.float32)
        return out, dict(rows=rows, ct=ct, tracking=tracking, p=p, q=s["ct"].astype(np.float32), dl=lab[rows].astype(np.int32))

    def _assign(self, p, q, dl, state):
        """Points 3-4, greedy: a detection takes the nearest free track of its label within the gate -> (the track of each detection or -1, the tracks taken, the
        unmatched detections that are numbered last -- none here --, further outputs)."""
        N, M = len(p), len(state["label"])
        match = np.full(N, -1, dtype=np.int64)
        taken = np.zeros(M, dtype=bool)
        if M:
            with np.errstate(invalid="ignore", over="ignore"):
                for i in range(N):
                    dx, dy = q[:, 0] - p[i, 0], q[:, 1] - p[i, 1]
                    d = np.sqrt(dx * dx + dy * dy)
                    assert d.dtype == np.float32
                    idx = np.nonzero((state["label"] == dl[i]) & (d <= self.max_diff[dl[i]]) & ~taken)[0]
                    if len(idx):
                        j = idx[np.argmin(d[idx])]                          # the first of the smallest: the lowest track index
                        match[i], taken[j] = j, True
        return match, taken, np.zeros(N, dtype=bool), {}

    def _write(self, out, found, match, taken, late):
        """Points 5-6: the new state -- matches in detection order, then the unmatched detections, those in ``late`` behind the others, then the old tracks that
        stay -- and the outputs."""
        s, rows, ct, tracking, dl = self.state, found["rows"], found["ct"], found["tracking"], found["dl"]
        N = len(rows)
        hit = match >= 0
        seq = np.concatenate([np.nonzero(hit)[0], np.nonzero(~hit & ~late)[0], np.nonzero(late)[0]])
        nu = N - int(hit.sum())
        ids, act = np.empty(N, np.int32), np.empty(N, np.int32)
        ids[hit], act[hit] = s["tracking_id"][match[hit]], s["active"][match[hit]] + 1
        ids[seq[N - nu:]], act[~hit] = s["id_count"] + 1 + np.arange(nu, dtype=np.int32), 1
        stay = ~taken & (s["age"] < self.max_age)
        self.state = dict(ct=np.concatenate([ct[seq], s["ct"][stay] + s["tracking"][stay] * -1.0]), tracking=np.concatenate([tracking[seq], s["tracking"][stay]]),
                          label=np.concatenate([dl[seq], s["label"][stay]]), tracking_id=np.concatenate([ids[seq], s["tracking_id"][stay]]),
                          age=np.concatenate([np.ones(N, np.int32), s["age"][stay] + 1]), active=np.concatenate([act[seq], np.zeros(int(stay.sum()), np.int32)]),
                          id_count=int(s["id_count"]) + nu)
        out["track_id"][rows], out["active"][rows], out["order"][:N] = ids, act, rows[seq]


def run_case(c, streams=None, on_step=None, tracker=Tracker):
    """The restatement ``tracker`` over a case -> (outputs [frame][stream], states after [frame][stream]).  ``on_step(f, b, tracker)`` sees a stream's tracker
    after each step."""
    B = c["B"]
    streams = range(B) if streams is None else streams
    trackers = {b: tracker(c["max_age"]) for b in streams}
    if c.get("init") is not None:
        for b in streams:
            trackers[b].set_state(c["init"][b], c["init_last"][b])
    outs, states = [], []
    for f, fr in enumerate(c["frames"]):
        outs.append([trackers[b].step(fr["rec"][b], fr["score"][b], fr["name"][b], fr["kept"][b], fr["timestamp"][b], fr["first"][b], c["thr"]) for b in streams])
        states.append([{k: (v.copy() if hasattr(v, "copy") else v) for k, v in trackers[b].state.items()} for b in streams])
        if on_step is not None:
            for b in streams:
                on_step(f, b, trackers[b])
    return outs, states


def restated(tracker, restatement=Tracker):
    """The seam: PubTracker._step_host, the one place where the host half of ``tracker`` meets the device, replaced by the restatement."""
    streams = [restatement(tracker.max_age, tracker.track_label, [tracker.NUSCENE_CLS_VELOCITY_ERROR[n] for n in tracker.tracking_names]) for _ in range(tracker.num_streams)]
    started = [False] * tracker.num_streams

    def step_host(rec, score, name, kept, timestamps, first, thr):
        outs, first = [], [False] * len(streams) if first is None else first
        for b, s in enumerate(streams):
            outs.append(s.step(rec[b], score[b], name[b], kept[b], timestamps[b], bool(first[b]) or not started[b], thr))
            started[b] = True
        return {k: np.stack([o[k] for o in outs]) for k in OUT_KEYS + tuple(restatement.EXTRA_OUT)}
    tracker._step_host = step_host
    return tracker


# ---- the state's bytes (include/toc3d_tracks.h) ---------------------------------------------------------------------------------------------------------------------------
def state_bytes(cap):
    return HEADER_BYTES + sum(size for _, size in STATE_FIELDS) * cap


def state_to_bytes(state, last, cap):
    """A state dict -> the bytes of include/toc3d_tracks.h."""
    n = len(state["label"])
    raw = np.zeros(state_bytes(cap), dtype=np.uint8)
    raw[0:8].view(np.int32)[:] = [n, state["id_count"]]
    raw[8:16].view(np.float64)[0] = last
    at = HEADER_BYTES
    for k, size in STATE_FIELDS:
        raw[at:at + size * n] = np.ascontiguousarray(state[k], dtype=STATE_DTYPES[k]).reshape(-1).view(np.uint8)
        at += size * cap
    return raw


def bytes_to_state(raw, cap):
    """-> (state dict of the live rows, last_timestamp, bytes that should be zero and are not: the header's padding and every row at or beyond count)."""
    n, id_count = raw[0:8].view(np.int32).tolist()
    assert 0 <= n <= cap
    dirty = int((raw[16:32] != 0).sum())
    state, at = dict(id_count=id_count), HEADER_BYTES
    for k, size in STATE_FIELDS:
        field = raw[at:at + size * cap]
        live = field[:size * n].view(STATE_DTYPES[k])
        state[k] = live.reshape(-1, 2).copy() if size == 16 else live.copy()
        dirty += int((field[size * n:] != 0).sum())
        at += size * cap
    return state, float(raw[8:16].view(np.float64)[0]), dirty


# ---- records ----------------------------------------------------------------------------------------------------------------------------------------------------------------
def case_annos(c, f, b):
    """The submission records of a case's frame f, stream b: the rows below ``kept``."""
    fr = c["frames"][f]
    return [dict(sample_token=f"s{f}", translation=fr["rec"][b, i, 0:3].tolist(), size=fr["rec"][b, i, 3:6].tolist(), rotation=fr["rec"][b, i, 6:10].tolist(),
                 velocity=fr["rec"][b, i, 10:12].tolist(), detection_name=CLASS_NAMES[int(fr["name"][b, i])], detection_score=float(fr["score"][b, i]),
                 attribute_name="") for i in range(int(fr["kept"][b]))]


def want_annos(annos, e, f, rows):
    """The tracking records the reference makes of frame f's records ``annos`` (stream 0), in its output order ``rows``."""
    return [dict(sample_token=f"s{f}", translation=annos[r]["translation"], size=annos[r]["size"], rotation=annos[r]["rotation"], velocity=annos[r]["velocity"],
                 tracking_id=str(int(e["track_id"][f, 0, r])), tracking_name=annos[r]["detection_name"], tracking_score=annos[r]["detection_score"]) for r in rows]


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------------------------------------
T0 = 1533151603.5                          # seconds: a nuScenes sample's timestamp * 1e-6
ALL_CLASSES = tuple(range(10))
TRACKED = (CAR, TRUCK, BUS, TRAILER, MOTORCYCLE, BICYCLE, PEDESTRIAN)


def blank_frame(B, K, timestamp, first):
    """Rows nothing may read: NaN records and scores, a name outside the class list."""
    return dict(rec=np.full((B, K, REC), np.nan), score=np.full((B, K), np.nan, dtype=np.float32), name=np.full((B, K), 99, dtype=np.int32),
                kept=np.zeros(B, dtype=np.int64), timestamp=np.asarray(timestamp, dtype=np.float64), first=np.asarray(first, dtype=np.int32))


def put(fr, b, dets):
    """dets: (x, y, vx, vy, class, score) in order -> the first rows of stream b."""
    for i, (x, y, vx, vy, cls, sc) in enumerate(dets):
        fr["rec"][b, i] = [x, y, 1.0, 2.0, 4.0, 1.5, 1.0, 0.0, 0.0, 0.0, vx, vy]
        fr["score"][b, i], fr["name"][b, i] = sc, cls
    fr["kept"][b] = len(dets)


def scene_frames(seed, K, nframes, nobj, classes=ALL_CLASSES, B=1, resets=None, empty=(), kept_zero=(), dt=0.5, spacing=2.0, speed=4.0):
    """A seeded scene per stream: nobj objects a few metres apart near a map position far from the origin (float32 rounding of the positions matters), moving at up
    to some 10 m/s (``speed``: the standard deviation of a velocity component); a frame detects nine in ten of them with position and velocity noise, adds false positives, orders by descending score and fills the rows at or
    beyond ``kept`` with NaN.  ``resets[b]``: the frames at which stream b starts a scene (frame 0 always); ``empty``: frames whose scores are all below any
    threshold; ``kept_zero``: frames with kept = 0."""
    frames = [blank_frame(B, K, [T0 + dt * f + 100.0 * b for b in range(B)], [1 if f == 0 or (resets and f in resets[b]) else 0 for b in range(B)])
              for f in range(nframes)]
    for b in range(B):
        rng = np.random.default_rng([seed, b])
        side = spacing * max(1.0, np.sqrt(nobj))
        origin = rng.uniform(300.0, 1500.0, 2)
        pos = origin + rng.uniform(0.0, side, (nobj, 2))
        vel = rng.normal(0.0, speed, (nobj, 2))
        cls = rng.choice(np.asarray(classes), nobj)
        for f, fr in enumerate(frames):
            seen = rng.random(nobj) < 0.9
            nfp = int(rng.integers(0, max(1, nobj // 10) + 1))
            n = min(K, int(seen.sum()) + nfp)
            xy = np.concatenate([(pos + vel * (dt * f))[seen] + rng.normal(0.0, 0.3, (int(seen.sum()), 2)), origin + rng.uniform(0.0, side, (nfp, 2))])
            v = np.concatenate([vel[seen] + rng.normal(0.0, 0.5, (int(seen.sum()), 2)), rng.normal(0.0, 4.0, (nfp, 2))])
            cl = np.concatenate([cls[seen], rng.choice(np.asarray(classes), nfp)])
            pick = rng.permutation(len(xy))[:n]
            sc = np.sort(rng.uniform(0.05, 1.0, n).astype(np.float32))[::-1]
            if f in empty:
                sc = (sc * np.float32(0.01)).astype(np.float32)
            rec = rng.normal(0.0, 1.0, (n, REC))
            rec[:, 0:2], rec[:, 10:12] = xy[pick], v[pick]
            if f not in kept_zero:
                fr["rec"][b, :n], fr["score"][b, :n], fr["name"][b, :n], fr["kept"][b] = rec, sc, cl[pick], n
            else:                                                           # readable rows behind kept = 0: they must not be read all the same
                fr["rec"][b, :n], fr["score"][b, :n], fr["name"][b, :n] = rec, sc, cl[pick]
    return frames


def scene_case(seed, K, nframes, nobj, max_age, thr=0.25, **kw):
    B = kw.get("B", 1)
    return dict(B=B, K=K, max_age=max_age, thr=thr, frames=scene_frames(seed, K, nframes, nobj, **kw))


def full_state(seed, M, classes, side):
    """A given state of M tracks (ages 1 .. 3, ids 1 .. M in a seeded order) around the position scene_frames(seed, ...) of stream 0 uses."""
    rng = np.random.default_rng([seed, 0])
    origin = np.random.default_rng([seed, 0]).uniform(300.0, 1500.0, 2)
    table = track_label_table()
    tracked = np.array([c for c in classes if table[c] >= 0])
    return dict(ct=origin + rng.uniform(0.0, side, (M, 2)), tracking=rng.normal(0.0, 2.0, (M, 2)), label=table[rng.choice(tracked, M)].astype(np.int32),
                tracking_id=(rng.permutation(M) + 1).astype(np.int32), age=rng.integers(1, 4, M).astype(np.int32), active=rng.integers(0, 5, M).astype(np.int32),
                id_count=M)


def large_case(seed, classes):
    c = scene_case(seed, 2048, 3, 2300, 3, thr=0.01, classes=classes)                 # (nine in ten of 2300 objects and the false positives fill all 2048 rows)
    for fr in c["frames"]:
        fr["first"][:] = 0                                                  # the given state is continued, not reset
    side = 2.0 * np.sqrt(2300)
    c["init"], c["init_last"] = [full_state(seed, 8192, classes, side)], [T0 - 0.5]
    return c


def manual_case(K, max_age, frames_dets, thr=0.25, classes_note=None):
    frames = []
    for f, dets in enumerate(frames_dets):
        fr = blank_frame(1, K, [T0 + 0.5 * f], [1 if f == 0 else 0])
        put(fr, 0, dets)
        frames.append(fr)
    return dict(B=1, K=K, max_age=max_age, thr=thr, frames=frames)


def next_up(x):
    return np.nextafter(F32(x), F32(np.inf))


def gate_y_above():
    """A float32 y > 2 for which sqrt(1.5 * 1.5 + y * y), every operation rounded once in float32, is the next float above 2.5."""
    y = F32(2.0)
    for _ in range(64):
        y = next_up(y)
        if np.sqrt(F32(1.5) * F32(1.5) + y * y) == next_up(2.5):
            return float(y)
    raise AssertionError("no float32 y gives the float above 2.5")


def d_once(qx, qy, px, py):
    """The header's distance: float32, every operation rounded once."""
    dx, dy = F32(qx) - F32(px), F32(qy) - F32(py)
    return np.sqrt(dx * dx + dy * dy)


def d_fused(qx, qy, px, py):
    """What a compiler that contracts would compute: sqrt(fma(dx, dx, dy * dy)).  dx * dx is exact in float64 (48 bits); its sum with the rounded dy * dy is
    rounded to float64 and then to float32 -- a double rounding that differs from the true fma only on float64 half-way cases, which the search has no use for."""
    dx, dy = np.asarray(F32(qx) - F32(px)), np.asarray(F32(qy) - F32(py))
    s = (dx.astype(np.float64) * dx.astype(np.float64) + (dy * dy).astype(np.float64)).astype(np.float32)
    return np.sqrt(s)


NEAR_CHOICE, NEAR_GATE = 6, 6              # how many of each the search collects (the issue asks for at least 4)


def search_near_ties(seed=2024):
    """Seeded search -> (choice, gate): ``choice`` rows (px, py, q1x, q1y, q2x, q2y): two tracks at nearly the same distance from p, in track order, for which the
    once-rounded distances and the fused ones pick different tracks (the lower index wins a tie); ``gate`` rows (px, py, qx, qy): one track whose once-rounded
    distance is on one side of 2.5 and whose fused distance on the other.  All coordinates are float32 values; stationary detections put p exactly there."""
    rng = np.random.default_rng(seed)
    choice, gate = [], []
    while len(choice) < NEAR_CHOICE or len(gate) < NEAR_GATE:
        p = rng.uniform(-400.0, 400.0, 2).astype(np.float32)
        ang = rng.uniform(0.0, 2 * np.pi, 256)
        if len(choice) < NEAR_CHOICE:
            r = rng.uniform(0.5, 2.4)
            q = (p.astype(np.float64) + r * np.stack([np.cos(ang), np.sin(ang)], 1)).astype(np.float32)
            a, b = d_once(q[:, 0], q[:, 1], p[0], p[1]), d_fused(q[:, 0], q[:, 1], p[0], p[1])
            first_once = (a[:-1] <= a[1:])                                  # of the neighbours (k, k + 1): does k win?
            flip = np.nonzero((first_once != (b[:-1] <= b[1:])) & (np.maximum(a[:-1], a[1:]) < 2.45))[0]
            if len(flip):
                k = int(flip[0])
                choice.append([p[0], p[1], q[k, 0], q[k, 1], q[k + 1, 0], q[k + 1, 1]])
        if len(gate) < NEAR_GATE:
            q = (p.astype(np.float64) + 2.5 * np.stack([np.cos(ang), np.sin(ang)], 1)).astype(np.float32)
            a, b = d_once(q[:, 0], q[:, 1], p[0], p[1]), d_fused(q[:, 0], q[:, 1], p[0], p[1])
            flip = np.nonzero((a <= F32(2.5)) != (b <= F32(2.5)))[0]
            if len(flip):
                k = int(flip[0])
                gate.append([p[0], p[1], q[k, 0], q[k, 1]])
    return np.array(choice, dtype=np.float32), np.array(gate, dtype=np.float32)


def near_tie_case(choice, gate):
    """Frame 0 makes the tracks (two per choice row, one per gate row, far apart from one another); frame 1's stationary detections stand on the p's; frame 2 moves
    nothing, so every pair is decided once more with the tracks in the new state's order."""
    choice, gate = np.asarray(choice, dtype=np.float32), np.asarray(gate, dtype=np.float32)
    tracks = [(float(r[2 + 2 * k]), float(r[3 + 2 * k]), 0.0, 0.0, CAR, 0.9) for r in choice for k in (0, 1)] + [(float(r[2]), float(r[3]), 0.0, 0.0, CAR, 0.9) for r in gate]
    dets = [(float(r[0]), float(r[1]), 0.0, 0.0, CAR, 0.8) for r in choice] + [(float(r[0]), float(r[1]), 0.0, 0.0, CAR, 0.8) for r in gate]
    return manual_case(64, 3, [tracks, dets, dets])


def check_near_ties(choice, gate):
    """What the generator asserts where it makes the fixture, and the CPU test on what it reads: the counts, and that every row is what it is said to be."""
    assert len(choice) >= 4 and len(gate) >= 4
    for r in choice:
        a = [d_once(r[2 + 2 * k], r[3 + 2 * k], r[0], r[1]) for k in (0, 1)]
        b = [d_fused(r[2 + 2 * k], r[3 + 2 * k], r[0], r[1]) for k in (0, 1)]
        assert (a[0] <= a[1]) != (b[0] <= b[1]) and max(a) < 2.5 and max(b) < 2.5
    for r in gate:
        assert (d_once(r[2], r[3], r[0], r[1]) <= F32(2.5)) != (d_fused(r[2], r[3], r[0], r[1]) <= F32(2.5))


THR_F32 = float(F32(0.3))                  # a threshold that IS a float32, for the scores exactly at it and one float below it
Y_UP = gate_y_above()

MANUAL = {
    # the lower track index wins: two tracks at one position, one detection; then the other track is taken by a second detection
    "tie_tracks": lambda: manual_case(4, 3, [[(5.0, 5.0, 0.0, 0.0, CAR, 0.9), (5.0, 5.0, 0.0, 0.0, CAR, 0.8)], [(6.0, 5.0, 0.0, 0.0, CAR, 0.9)],
                                             [(6.0, 5.0, 0.0, 0.0, CAR, 0.9), (5.0, 5.0, 0.0, 0.0, CAR, 0.8), (5.0, 5.0, 0.0, 0.0, CAR, 0.7)]]),
    # the earlier detection wins: two detections equidistant from one track
    "tie_dets": lambda: manual_case(4, 0, [[(0.0, 0.0, 0.0, 0.0, BUS, 0.9)], [(1.0, 0.0, 0.0, 0.0, BUS, 0.9), (-1.0, 0.0, 0.0, 0.0, BUS, 0.8)],
                                           [(-1.0, 0.0, 0.0, 0.0, BUS, 0.9), (1.0, 0.0, 0.0, 0.0, BUS, 0.8), (0.0, 0.0, 0.0, 0.0, BUS, 0.7)]]),
    # d exactly 2.5 is valid, the next float above is not; the same position under another label does not match
    "gate_and_labels": lambda: manual_case(8, 3, [[(1.5, 2.0, 0.0, 0.0, CAR, 0.9), (101.5, Y_UP, 0.0, 0.0, CAR, 0.9), (200.0, 0.0, 0.0, 0.0, CAR, 0.9),
                                                   (300.0, 0.0, 0.0, 0.0, PEDESTRIAN, 0.9)],
                                                  [(0.0, 0.0, 0.0, 0.0, CAR, 0.9), (100.0, 0.0, 0.0, 0.0, CAR, 0.9), (200.0, 0.0, 0.0, 0.0, TRUCK, 0.9),
                                                   (300.0, 0.0, 0.0, 0.0, BICYCLE, 0.9), (300.0, 0.0, 0.0, 0.0, CONE, 0.9), (300.0, 0.0, 0.0, 0.0, PEDESTRIAN, 0.9)],
                                                  [(200.0, 0.0, 0.0, 0.0, CAR, 0.9), (200.0, 0.0, 0.0, 0.0, TRUCK, 0.9)]]),
    # the comparison is (double)score < thr: at the threshold kept, one float below dropped
    "score_at_f32_thr": lambda: manual_case(4, 3, [[(0.0, 0.0, 0.0, 0.0, CAR, THR_F32), (10.0, 0.0, 0.0, 0.0, CAR, float(np.nextafter(F32(0.3), F32(0))))],
                                                   [(0.0, 0.0, 0.0, 0.0, CAR, float(np.nextafter(F32(0.3), F32(0)))), (10.0, 0.0, 0.0, 0.0, CAR, THR_F32)],
                                                   [(0.0, 0.0, 0.0, 0.0, CAR, THR_F32), (10.0, 0.0, 0.0, 0.0, CAR, THR_F32)]], thr=THR_F32),
    # 0.3 is no float32: float32(0.3) = 0.30000001192... is above it and kept, the float below is dropped
    "score_at_f64_thr": lambda: manual_case(4, 3, [[(0.0, 0.0, 0.0, 0.0, CAR, float(F32(0.3))), (10.0, 0.0, 0.0, 0.0, CAR, float(np.nextafter(F32(0.3), F32(0))))],
                                                   [(0.0, 0.0, 0.0, 0.0, CAR, float(F32(0.3))), (10.0, 0.0, 0.0, 0.0, CAR, float(F32(0.3)))]] * 2, thr=0.3),
    # a moving object: the velocity times the time lag brings the detection back onto its track, and an unmatched track moves on by its own
    "motion": lambda: manual_case(4, 3, [[(700.0, 900.0, 6.0, -2.0, CAR, 0.9), (720.0, 900.0, 0.0, 7.0, TRUCK, 0.9)], [(703.1, 899.0, 6.0, -2.0, CAR, 0.9)],
                                         [(706.0, 898.1, 6.0, -2.0, CAR, 0.9), (720.0, 907.0, 0.0, 7.0, TRUCK, 0.9)], [(720.0, 910.5, 0.0, 7.0, TRUCK, 0.9)]]),
}

SCENES = {
    "first_frame_n1": lambda: scene_case(1, 1, 3, 1, 3, classes=(CAR,)),
    # slow objects: an old track, which the empty frames leave where it was, is still within the gate of its object afterwards
    "empty_twice_age0": lambda: scene_case(2, 16, 5, 12, 0, empty=(1, 2), speed=0.2),      # max_age 0: every track is old, none is dropped by the empty frames, all can match after them
    "empty_twice_age3": lambda: scene_case(3, 16, 5, 12, 3, empty=(1, 2), speed=0.2),      # the tracks reach age 3 = max_age in the empty frames and match on the fourth
    "empty_thrice_age1": lambda: scene_case(4, 16, 5, 12, 1, empty=(1, 2, 3), speed=0.2),
    "kept_zero": lambda: scene_case(5, 16, 4, 10, 3, kept_zero=(0, 2)),
    "reset_midway": lambda: scene_case(6, 32, 5, 24, 3, resets=[(2,)]),
    # N = M = K exactly (every row survives: tracked classes only, a threshold below every score; max_age 0 holds exactly the frame's detections)
    "n63_age0": lambda: scene_case(7, 63, 3, 90, 0, thr=0.01, classes=TRACKED),
    "n64_age0": lambda: scene_case(8, 64, 3, 90, 0, thr=0.01, classes=TRACKED),
    "n65_age0": lambda: scene_case(9, 65, 3, 90, 0, thr=0.01, classes=TRACKED),
    "n64": lambda: scene_case(17, 64, 4, 90, 3, thr=0.01, classes=TRACKED),
    "n65_mixed": lambda: scene_case(18, 65, 4, 70, 3),                          # some rows filtered out by class and by score
    "n65_one_label": lambda: scene_case(10, 65, 4, 90, 3, thr=0.01, classes=(CAR,), spacing=1.0),
    "n256_age0": lambda: scene_case(11, 256, 3, 340, 0, thr=0.01, classes=TRACKED, spacing=1.5),
    "n257": lambda: scene_case(12, 257, 4, 340, 3, thr=0.01, classes=TRACKED, spacing=1.5),
    "n257_mixed": lambda: scene_case(19, 257, 4, 280, 3, spacing=1.5),
    "n257_one_label_age0": lambda: scene_case(13, 257, 3, 340, 0, thr=0.01, classes=(PEDESTRIAN,), spacing=1.0),
    "streams3": lambda: scene_case(14, 48, 5, 40, 3, B=3, resets=[(), (2,), (1, 3)], empty=(3,)),
    "large_one_label": lambda: large_case(15, (CAR,)),
    "large_spread": lambda: large_case(16, ALL_CLASSES),
}
NEAR_TIES = "near_ties"
CASES = tuple(MANUAL) + tuple(SCENES) + (NEAR_TIES,)
STREAMS_CASE = "streams3"
_BUILT = {}


def build_case(name, fixture=None):
    """The inputs of a case; the near-tie case reads its rows from the fixture (``fixture``: an open archive, else the file) instead of searching again."""
    if name not in _BUILT:
        if name == NEAR_TIES:
            z = np.load(FIXTURE) if fixture is None else fixture
            _BUILT[name] = near_tie_case(z["near_choice"], z["near_gate"])
        else:
            _BUILT[name] = (MANUAL.get(name) or SCENES[name])()
    return _BUILT[name]


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------------------------------------------
def pack_expected(prefix, outs, states, arrays):
    """[frame][stream] outputs and states -> flat arrays under ``prefix``."""
    F, B = len(outs), len(outs[0])
    for k in ("track_id", "active", "order"):
        arrays[f"{prefix}/{k}"] = np.stack([np.stack([outs[f][b][k] for b in range(B)]) for f in range(F)]).astype(np.int32)
    arrays[f"{prefix}/num_out"] = np.array([[outs[f][b]["num_out"] for b in range(B)] for f in range(F)], dtype=np.int64)
    arrays[f"{prefix}/count"] = np.array([[len(states[f][b]["label"]) for b in range(B)] for f in range(F)], dtype=np.int64)
    arrays[f"{prefix}/id_count"] = np.array([[states[f][b]["id_count"] for b in range(B)] for f in range(F)], dtype=np.int64)
    arrays[f"{prefix}/digest"] = np.stack([np.stack([state_digest(states[f][b]) for b in range(B)]) for f in range(F)])
    if arrays[f"{prefix}/count"].sum() <= FULL_STATE_ROWS:
        for k in STATE_KEYS:
            arrays[f"{prefix}/state_{k}"] = np.concatenate([np.asarray(states[f][b][k], dtype=STATE_DTYPES[k]) for f in range(F) for b in range(B)])


_EXPECTED = {}


def expected(name, fixture=FIXTURE, extra=()):
    """What the reference returned and held -> dict(track_id, active, order [F, B, K], num_out, count, id_count [F, B], digest [F, B, 32], states [f][b] or None),
    and the arrays ``extra`` names, as the fixture has them."""
    if (fixture, name) not in _EXPECTED:
        z = np.load(fixture)
        e = {k: z[f"{name}/{k}"] for k in ("track_id", "active", "order", "num_out", "count", "id_count", "digest") + tuple(extra)}
        e["states"] = None
        if f"{name}/state_ct" in z.files:
            F, B = e["count"].shape
            flat = {k: z[f"{name}/state_{k}"] for k in STATE_KEYS}
            at, e["states"] = 0, []
            for f in range(F):
                e["states"].append([])
                for b in range(B):
                    m = int(e["count"][f, b])
                    e["states"][f].append(dict({k: flat[k][at:at + m] for k in STATE_KEYS}, id_count=int(e["id_count"][f, b])))
                    at += m
        _EXPECTED[(fixture, name)] = e
    return _EXPECTED[(fixture, name)]


def compare_state(tag, got, e, f, b):
    """A state (dict of live rows and id_count) against the fixture's, every bit: in full where the fixture has the rows, and by the digest always."""
    assert len(got["label"]) == e["count"][f, b] and got["id_count"] == e["id_count"][f, b], f"{tag}: {len(got['label'])} tracks, id_count {got['id_count']}"
    if e["states"] is not None:
        want = e["states"][f][b]
        for k in STATE_KEYS:
            g = np.ascontiguousarray(got[k], dtype=STATE_DTYPES[k])
            assert np.array_equal(g.view(np.uint8), np.ascontiguousarray(want[k]).view(np.uint8)), f"{tag}: {k}, bit for bit"
    assert np.array_equal(state_digest(got), e["digest"][f, b]), f"{tag}: the digest of the tracks held"
