"""Centre-distance tracking of the submission records, on the device: greedy assignment (``toc3d_tracks_step``, include/toc3d_tracks.h) and the reference's
``hungarian=True`` (``toc3d_tracks_step_hungarian``, include/toc3d_assign.h).

The reference tracks after the run, on the host: ``nusc_tracking/pub_tracker.py:26-186`` (``PubTracker.step_centertrack``) with ``track_utils.py:3-12``
(``greedy_assignment``), driven by ``nusc_tracking/pub_test.py:77-153``, which reads ``results_nusc.json`` and writes ``tracking_result.json`` -- per frame an
N x M float64 distance matrix, a deep copy of it and a Python loop with one ``argmin`` per detection, the tracks a list of dicts mutated in place.  Here
:meth:`PubTracker.step_fixed` does a step for every camera stream in one launch, from the tensors :meth:`NuScenesResults.format_fixed` leaves on the device; each
stream's tracks stay in device memory from frame to frame, and a stream is reset by a flag the kernel reads, without a host round trip.  :meth:`PubTracker.step`
takes the reference's lists of dicts, :meth:`PubTracker.track_file` restates ``pub_test.py:main``.  Neither scipy nor the nuScenes devkit is needed.

The reference's quirks are reproduced, not mended (include/toc3d_tracks.h states the arithmetic): a frame none of whose detections survives the filter leaves
every track in place, the old ones (``age >= max_age``) untouched and able to match later; the positions are compared in float32, each operation rounded once; the
lowest track index wins a tie, the earlier detection takes first.  Differences, by design: a distance that is not a number is no match; the unmatched tracks the
reference returns in its list with ``active == 0`` (``pub_test.py:116`` skips them) are state here, not output.  No CPU path for the matching.

HUNGARIAN ASSIGNMENT (``pub_tracker.py:27`` ``hungarian=False``, ``pub_test.py:28,81`` ``--hungarian``) is reached through :func:`build_tracker`, which takes the
reference's keywords: ``build_tracker(hungarian=True, max_age=3)`` returns a :class:`HungarianPubTracker`, whose step replays scipy's
``linear_sum_assignment`` operation for operation on the reference's matrix (1e18 for an invalid pair), tie-breaking included, and so reproduces what the
reference does there and an exact optimum would not: a track parked in an invalid match is dropped at once whatever its age, and the detections parked on tracks
get their new ids after the unmatched ones (include/toc3d_assign.h).  It holds up to 512 rows a stream and 2048 tracks.  ``PubTracker(hungarian=True)`` itself
keeps refusing.
"""
from __future__ import annotations

import ctypes
import json
import math
import os

import numpy as np
import torch

from . import lib
from .nusc_results import CLASS_NAMES

__all__ = ["PubTracker", "HungarianPubTracker", "build_tracker", "NUSCENES_TRACKING_NAMES", "NUSCENE_CLS_VELOCITY_ERROR", "TRACK_ANNO_KEYS", "TRACKING_META"]
_NAME = "toc3d_amd.PubTracker"

NUSCENES_TRACKING_NAMES = ("car", "truck", "bus", "trailer", "motorcycle", "bicycle", "pedestrian")       # pub_tracker.py:9-12: the index is the tracking label
NUSCENE_CLS_VELOCITY_ERROR = dict(car=2.5, truck=2.5, bus=2.5, trailer=2.5, pedestrian=2.5, motorcycle=2.5, bicycle=2.5)      # :15-23, metres
TRACK_ANNO_KEYS = ("sample_token", "translation", "size", "rotation", "velocity", "tracking_id", "tracking_name", "tracking_score")     # pub_test.py:118-127, in order
TRACKING_META = dict(use_camera=False, use_lidar=True, use_radar=False, use_map=False, use_external=False)                           # pub_test.py:139-145, as it is
_STATE_FIELDS = (("ct", torch.float64, 16), ("tracking", torch.float64, 16), ("label", torch.int32, 4), ("tracking_id", torch.int32, 4), ("age", torch.int32, 4),
                 ("active", torch.int32, 4))                                # include/toc3d_tracks.h: the rows of a state, field by field, bytes a track


def capacity_for(K: int, max_age: int) -> int:
    """``K * (max_age + 1)``: the tracks a step of K rows can hold (include/toc3d_tracks.h)."""
    return int(K) * (int(max_age) + 1)


def state_bytes(capacity: int) -> int:
    """TOC3D_TRACKS_STATE_BYTES(capacity)."""
    return lib.TRACKS_HEADER_BYTES + lib.TRACKS_ROW_BYTES * int(capacity)


def _fields(buf, capacity):
    """A state buffer uint8 ``(B, state_bytes)`` -> views: ``header`` int32 (B, 8), ``last_timestamp`` f64 (B, 1) and the six fields."""
    out = dict(header=buf[:, :lib.TRACKS_HEADER_BYTES].view(torch.int32), last_timestamp=buf[:, 8:16].view(torch.float64))
    at = lib.TRACKS_HEADER_BYTES
    for key, dtype, size in _STATE_FIELDS:
        out[key] = buf[:, at:at + size * capacity].view(dtype)
        at += size * capacity
    return out


class PubTracker:
    """``results_nusc.json`` records -> tracking ids, one tracker per camera stream.

    >>> res, trk = toc3d_amd.NuScenesResults(), toc3d_amd.PubTracker(max_age=3, num_streams=B)
    >>> fixed = res.format_fixed(boxes, scores, labels, counts, poses)
    >>> out = trk.step_fixed(fixed["rec"], fixed["score"], fixed["name"], fixed["kept"], timestamps, first)      # on the device, one launch
    >>> toc3d_amd.PubTracker(max_age=3).track_file("results_nusc.json", frames, "./work_dir")                    # pub_test.py:main
    """

    _ENTRY, _MAX_BOXES, _MAX_TRACKS, _CAPS = "toc3d_tracks_step", lib.TRACKS_MAX_BOXES, lib.TRACKS_MAX_TRACKS, ("TOC3D_TRACKS_MAX_BOXES", "TOC3D_TRACKS_MAX_TRACKS")
    _EXTRA_OUT = ()                                                         # outputs of the entry point behind num_out: (key, dtype), one value a stream

    def __init__(self, hungarian=False, max_age=0, class_names=CLASS_NAMES, tracking_names=NUSCENES_TRACKING_NAMES, cls_velocity_error=None, num_streams=1):
        if hungarian:
            raise NotImplementedError(f"{_NAME}: hungarian=True (scipy's linear_sum_assignment) is not implemented: the greedy assignment "
                                      "(track_utils.greedy_assignment, the reference's default) is the path built")
        if int(max_age) != max_age or max_age < 0:
            raise ValueError(f"{_NAME}: max_age must be a non-negative integer, got {max_age!r}")
        names, tracked = tuple(class_names), tuple(tracking_names)
        if not 1 <= len(names) <= lib.TRACKS_MAX_CLASSES or not 1 <= len(tracked) <= lib.TRACKS_MAX_CLASSES:
            raise ValueError(f"{_NAME}: 1 to {lib.TRACKS_MAX_CLASSES} class names and tracking names, got {len(names)} and {len(tracked)}")
        for n in names:
            if n not in CLASS_NAMES:
                raise ValueError(f"{_NAME}: unknown class name {n!r} (the nuScenes detection classes are {', '.join(CLASS_NAMES)})")
        for n in tracked:
            if n not in NUSCENES_TRACKING_NAMES:
                raise ValueError(f"{_NAME}: unknown tracking name {n!r} (the nuScenes tracking classes are {', '.join(NUSCENES_TRACKING_NAMES)})")
        if len(set(names)) != len(names) or len(set(tracked)) != len(tracked):
            raise ValueError(f"{_NAME}: a name is listed twice")
        err = dict(NUSCENE_CLS_VELOCITY_ERROR if cls_velocity_error is None else cls_velocity_error)
        missing = [n for n in tracked if n not in err]
        if missing:
            raise ValueError(f"{_NAME}: cls_velocity_error has no entry for {missing}")
        if not all(float(err[n]) >= 0 for n in tracked):                    # (NaN fails too)
            raise ValueError(f"{_NAME}: cls_velocity_error must be non-negative numbers of metres, got {err}")
        if int(num_streams) != num_streams or num_streams < 1:
            raise ValueError(f"{_NAME}: num_streams must be a positive integer, got {num_streams!r}")
        self.hungarian, self.max_age, self.num_streams = False, int(max_age), int(num_streams)
        self.class_names, self.tracking_names = names, tracked
        self.NUSCENE_CLS_VELOCITY_ERROR = {n: float(err[n]) for n in tracked}
        self.track_label = tuple(tracked.index(n) if n in tracked else -1 for n in names)
        self.capacity = 0
        self._state = None                                                  # [read next, written next]: uint8 (num_streams, state_bytes(capacity)) each
        self._tables = {}                                                   # device -> (track_label i32, max_diff f32)
        self._pending = [True] * self.num_streams                           # streams whose next step starts them, whatever ``first`` says

    # ---- state -----------------------------------------------------------------------------------------------------------------------------------------------
    def reset(self, streams=None):
        """``tracker.reset()`` (pub_tracker.py:37-39) for the streams ``streams`` (default: all): their next step starts from no tracks, ``id_count = 0`` and a zero
        time lag.  Nothing is launched: the step's ``first`` flag does it on the device."""
        for b in range(self.num_streams) if streams is None else streams:
            self._pending[b] = True
        return self

    def _tables_on(self, dev):
        key = str(dev)
        if key not in self._tables:
            lab = torch.tensor(self.track_label, dtype=torch.int32)
            gate = torch.tensor([self.NUSCENE_CLS_VELOCITY_ERROR[n] for n in self.tracking_names], dtype=torch.float32)
            self._tables[key] = (lab.to(dev), gate.to(dev))
        return self._tables[key]

    def _ensure_state(self, K, dev):
        """The two state buffers on ``dev`` with room for a step of K rows; grown (the tracks copied field by field, on the device) when K asks for more."""
        need = capacity_for(K, self.max_age)
        if need > self._MAX_TRACKS:
            raise ValueError(f"{_NAME}: {K} rows a stream with max_age {self.max_age} need {need} tracks, more than {self._MAX_TRACKS} ({self._CAPS[1]})")
        if self._state is not None and self._state[0].device == dev and need <= self.capacity:
            return
        cap = max(need, self.capacity if self._state is not None and self._state[0].device == dev else 0)
        new = [torch.zeros(self.num_streams, state_bytes(cap), dtype=torch.uint8, device=dev) for _ in range(2)]
        if self._state is not None and self._state[0].device == dev:
            old, fresh = _fields(self._state[0], self.capacity), _fields(new[0], cap)
            fresh["header"].copy_(old["header"])
            for key, _, size in _STATE_FIELDS:
                width = old[key].shape[1]
                fresh[key][:, :width].copy_(old[key])
        else:
            self._pending = [True] * self.num_streams                       # another device: nothing is carried over
        self._state, self.capacity = new, cap

    def tracks(self, stream=0):
        """The tracks stream ``stream`` holds, copied to the host (this synchronises: for inspection and tests) -> dict of numpy arrays ``ct``, ``tracking`` (n, 2)
        float64, ``label``, ``tracking_id``, ``age``, ``active`` int32, and ``id_count``, ``last_timestamp``."""
        if self._state is None or self._pending[stream]:
            return dict(ct=np.zeros((0, 2)), tracking=np.zeros((0, 2)), label=np.zeros(0, np.int32), tracking_id=np.zeros(0, np.int32), age=np.zeros(0, np.int32),
                        active=np.zeros(0, np.int32), id_count=0, last_timestamp=None)
        f = {k: v[stream].cpu().numpy() for k, v in _fields(self._state[0], self.capacity).items()}
        n = int(f["header"][0])
        out = {k: (f[k].reshape(-1, 2)[:n] if k in ("ct", "tracking") else f[k][:n]).copy() for k, _, _ in _STATE_FIELDS}
        out.update(id_count=int(f["header"][1]), last_timestamp=float(f["last_timestamp"][0]))
        return out

    # ---- the device half ---------------------------------------------------------------------------------------------------------------------------------
    def step_fixed(self, rec, score, name, kept, timestamps, first=None, score_threshold=0.25):
        """``rec`` f64 ``(B, K, 12)``, ``score`` f32 ``(B, K)``, ``name`` int32 ``(B, K)``, ``kept`` int64 ``(B,)``: what :meth:`NuScenesResults.format_fixed`
        returns, on the device, B = ``num_streams``.  ``timestamps``: a device float64 ``(B,)`` tensor, or B host numbers (seconds; finite, else ``ValueError``).
        ``first``: a device int32 ``(B,)`` tensor, B bools, or ``None``; a stream is started when its flag is set, on its first step and after :meth:`reset`.
        -> ``dict(track_id, active (B, K) int32 per input row, order (B, K) int32: the rows in the reference's output order, -1 from num_out on, num_out (B,) int64)``
        on the device (a :class:`HungarianPubTracker` adds ``rounds (B,) int32``).  One launch, no host synchronisation."""
        for t, what in ((rec, "rec"), (score, "score"), (name, "name"), (kept, "kept")):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise RuntimeError(f"{_NAME}: {what} must be a CUDA/HIP tensor -- the HIP extension is the only compute path")
        B = self.num_streams
        if rec.dim() != 3 or rec.shape[0] != B or rec.shape[2] != lib.TRACKS_REC or rec.dtype != torch.float64:
            raise ValueError(f"{_NAME}: rec must be float64 ({B}, K, {lib.TRACKS_REC}) for {B} stream(s), got {rec.dtype} {tuple(rec.shape)}")
        K = rec.shape[1]
        if (tuple(score.shape), tuple(name.shape), tuple(kept.shape)) != ((B, K), (B, K), (B,)) or score.dtype != torch.float32 or name.dtype != torch.int32 or kept.dtype != torch.int64:
            raise ValueError(f"{_NAME}: float32 score ({B}, {K}), int32 name ({B}, {K}) and int64 kept ({B},) expected, got {score.dtype} {tuple(score.shape)}, "
                             f"{name.dtype} {tuple(name.shape)}, {kept.dtype} {tuple(kept.shape)}")
        if K > self._MAX_BOXES:
            raise ValueError(f"{_NAME}: {K} rows a stream exceed {self._MAX_BOXES} ({self._CAPS[0]})")
        thr = float(score_threshold)
        if not math.isfinite(thr):
            raise ValueError(f"{_NAME}: score_threshold must be finite, got {score_threshold!r}")
        dev = rec.device
        with torch.cuda.device(dev):
            if isinstance(timestamps, torch.Tensor):
                if not timestamps.is_cuda or timestamps.dtype != torch.float64 or tuple(timestamps.shape) != (B,):
                    raise ValueError(f"{_NAME}: timestamps as a tensor must be float64 ({B},) on the device, got {timestamps.dtype} {tuple(timestamps.shape)} on {timestamps.device}")
                ts = timestamps.contiguous()
            else:
                host = np.asarray(timestamps, dtype=np.float64).reshape(-1)
                if host.shape != (B,) or not np.isfinite(host).all():
                    raise ValueError(f"{_NAME}: {B} finite timestamps (seconds) expected, got {host.tolist()}")
                ts = torch.from_numpy(host).pin_memory().to(dev, non_blocking=True)
            self._ensure_state(K, dev)
            pending = list(self._pending)
            if isinstance(first, torch.Tensor):
                if not first.is_cuda or first.dtype != torch.int32 or tuple(first.shape) != (B,):
                    raise ValueError(f"{_NAME}: first as a tensor must be int32 ({B},) on the device, got {first.dtype} {tuple(first.shape)} on {first.device}")
                flags = first.contiguous()
                if any(pending):
                    flags = flags | torch.tensor(pending, dtype=torch.int32).pin_memory().to(dev, non_blocking=True)
            else:
                host = [False] * B if first is None else [bool(f) for f in first]
                if len(host) != B:
                    raise ValueError(f"{_NAME}: {B} first flags expected, got {len(host)}")
                flags = torch.tensor([int(f or p) for f, p in zip(host, pending)], dtype=torch.int32).pin_memory().to(dev, non_blocking=True)
            self._pending = [False] * B
            rec, score, name, kept = rec.contiguous(), score.contiguous(), name.contiguous(), kept.contiguous()
            lab, gate = self._tables_on(dev)
            out = dict(track_id=torch.empty(B, K, dtype=torch.int32, device=dev), active=torch.empty(B, K, dtype=torch.int32, device=dev),
                       order=torch.empty(B, K, dtype=torch.int32, device=dev), num_out=torch.empty(B, dtype=torch.int64, device=dev))
            out.update({key: torch.empty(B, dtype=dtype, device=dev) for key, dtype in self._EXTRA_OUT})
            lib.call(self._ENTRY, rec, score, name, kept, B, K, lab, len(self.class_names), gate, len(self.tracking_names), thr, self.max_age, ts, flags,
                     self._state[0], self._state[1], self.capacity, out["track_id"], out["active"], out["order"], out["num_out"], *[out[key] for key, _ in self._EXTRA_OUT],
                     lib.stream_ptr())
            self._state.reverse()                                           # what was written is read next
        return out

    # ---- the host half -----------------------------------------------------------------------------------------------------------------------------------
    def pack_annos(self, annos_per_stream):
        """Per stream the list of detection dicts of ``results_nusc.json`` -> numpy ``rec (B, K, 12)`` f64, ``score (B, K)`` f32, ``name (B, K)`` int32 (-1 for a
        name outside ``class_names``: the reference passes those over, :64-65), ``kept (B,)`` int64, K the longest list.  The score becomes the float32 the
        detector made it from."""
        B, K = len(annos_per_stream), max([len(a) for a in annos_per_stream], default=0)
        rec, score = np.zeros((B, K, lib.TRACKS_REC), dtype=np.float64), np.zeros((B, K), dtype=np.float32)
        name, kept = np.full((B, K), -1, dtype=np.int32), np.zeros(B, dtype=np.int64)
        index = {n: i for i, n in enumerate(self.class_names)}
        for b, annos in enumerate(annos_per_stream):
            kept[b] = len(annos)
            for i, a in enumerate(annos):
                rec[b, i, 0:3], rec[b, i, 3:6], rec[b, i, 6:10], rec[b, i, 10:12] = a["translation"], a["size"], a["rotation"], a["velocity"][:2]
                score[b, i], name[b, i] = a["detection_score"], index.get(a["detection_name"], -1)
        return rec, score, name, kept

    def _step_host(self, rec, score, name, kept, timestamps, first, score_threshold):
        """numpy in, numpy out around :meth:`step_fixed`: the one place where :meth:`step` meets the device."""
        dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
        if dev is None:
            raise RuntimeError(f"{_NAME}: no CUDA/HIP device -- the HIP extension is the only compute path")
        put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        out = self.step_fixed(put(rec), put(score), put(name), put(kept), timestamps, first, score_threshold)
        return {k: v.cpu().numpy() for k, v in out.items()}

    def step(self, annos_per_stream, timestamps, first=None, score_threshold=0.25):
        """``annos_per_stream``: per stream the list of detection dicts of one sample (``results_nusc.json``'s).  -> per stream the list the reference's
        ``step_centertrack`` returns for the frame, without its ``active == 0`` entries: a copy of each surviving detection's dict with ``tracking_id`` (int) and
        ``active``, matches first and then the new tracks, each group in detection order."""
        if len(annos_per_stream) != self.num_streams:
            raise ValueError(f"{_NAME}: {self.num_streams} stream(s) need {self.num_streams} lists of detections, got {len(annos_per_stream)}")
        out = self._step_host(*self.pack_annos(annos_per_stream), timestamps, first, score_threshold)
        ret = []
        for b, annos in enumerate(annos_per_stream):
            rows = out["order"][b, :int(out["num_out"][b])].tolist()
            ret.append([dict(annos[r], tracking_id=int(out["track_id"][b, r]), active=int(out["active"][b, r])) for r in rows])
        return ret

    def records_to_annos(self, rec, score, name, track_id, order, num_out, tokens):
        """numpy in, dicts out: the arrays of :meth:`NuScenesResults.format_fixed` and :meth:`step_fixed` -> per stream the ``pub_test.py:115-128`` dicts of the
        frame, in output order: ``sample_token``, ``translation``, ``size``, ``rotation``, ``velocity``, ``tracking_id`` (a ``str``), ``tracking_name``,
        ``tracking_score``."""
        rec, score, name, track_id, order, num_out = (np.asarray(a) for a in (rec, score, name, track_id, order, num_out))
        B = rec.shape[0]
        if len(tokens) != B:
            raise ValueError(f"{_NAME}: {B} stream(s) need {B} sample tokens, got {len(tokens)}")
        out = []
        for b in range(B):
            annos = []
            for i in order[b, :int(num_out[b])].tolist():
                r = rec[b, i].tolist()
                annos.append(dict(sample_token=tokens[b], translation=r[0:3], size=r[3:6], rotation=r[6:10], velocity=r[10:12], tracking_id=str(int(track_id[b, i])),
                                  tracking_name=self.class_names[int(name[b, i])], tracking_score=float(score[b, i])))
            out.append(annos)
        return out

    @staticmethod
    def items_to_annos(items, token):
        """One stream's list from :meth:`step` -> its ``pub_test.py:115-128`` dicts."""
        return [dict(sample_token=token, translation=x["translation"], size=x["size"], rotation=x["rotation"], velocity=x["velocity"], tracking_id=str(x["tracking_id"]),
                     tracking_name=x["detection_name"], tracking_score=x["detection_score"]) for x in items if x["active"] != 0]

    def track_file(self, results_json, frames, work_dir, score_threshold=0.25):
        """``pub_test.py:main``: ``results_json`` (the path of a ``results_nusc.json``, or its dict) tracked along ``frames`` -- the list ``frames_meta.json`` holds
        under ``'frames'`` (or that file's path, or its dict): ``{token, timestamp, first}`` per sample, in order, the timestamp in seconds (the sample's
        ``timestamp * 1e-6``, pub_test.py:54) -- and written to ``{work_dir}/tracking_result.json`` with the reference's ``meta`` -> the path.  The tracker starts
        afresh; one stream."""
        if self.num_streams != 1:
            raise ValueError(f"{_NAME}: track_file walks one sequence of frames: num_streams must be 1, got {self.num_streams}")
        if isinstance(results_json, (str, os.PathLike)):
            with open(results_json, "rb") as fh:
                results_json = json.load(fh)
        predictions = results_json["results"]
        if isinstance(frames, (str, os.PathLike)):
            with open(frames, "rb") as fh:
                frames = json.load(fh)
        if isinstance(frames, dict):
            frames = frames["frames"]
        self.reset()
        results = {}
        for fr in frames:
            token = fr["token"]
            items = self.step([predictions[token]], [fr["timestamp"]], [bool(fr["first"])], score_threshold)[0]
            results[token] = self.items_to_annos(items, token)
        os.makedirs(work_dir, exist_ok=True)
        path = os.path.join(work_dir, "tracking_result.json")
        with open(path, "w") as fh:
            json.dump(dict(results=results, meta=dict(TRACKING_META)), fh)
        return path


class HungarianPubTracker(PubTracker):
    """:class:`PubTracker` with the reference's ``hungarian=True``: ``toc3d_tracks_step_hungarian`` (include/toc3d_assign.h) in place of the greedy step.  Made by
    :func:`build_tracker`.  :meth:`step_fixed` returns ``rounds (B,) int32`` -- the scan rounds the solver made per stream -- beside the other outputs; ``step``,
    ``records_to_annos``, ``track_file``, ``reset``, the growth of the state and the streams are inherited.  At most 512 rows a stream (TOC3D_ASSIGN_MAX_BOXES)
    and 2048 tracks (TOC3D_ASSIGN_MAX_TRACKS): more is a ``ValueError``."""
    _ENTRY, _MAX_BOXES, _MAX_TRACKS, _CAPS = "toc3d_tracks_step_hungarian", lib.ASSIGN_MAX_BOXES, lib.ASSIGN_MAX_TRACKS, ("TOC3D_ASSIGN_MAX_BOXES", "TOC3D_ASSIGN_MAX_TRACKS")
    _EXTRA_OUT = (("rounds", torch.int32),)

    def __init__(self, max_age=0, **kwargs):
        super().__init__(hungarian=False, max_age=max_age, **kwargs)
        self.hungarian = True


def build_tracker(hungarian=False, max_age=0, classes=(PubTracker, HungarianPubTracker), **kwargs):
    """The reference's ``PubTracker(hungarian=False, max_age=0)`` (``pub_tracker.py:27``; ``pub_test.py --hungarian --max_age``): a :class:`PubTracker`, or with
    ``hungarian=True`` a :class:`HungarianPubTracker`; ``kwargs`` go to the class.  ``classes``: the (greedy, Hungarian) pair to build from."""
    return classes[1 if hungarian else 0](max_age=max_age, **kwargs)


def library_state_bytes(capacity: int) -> int:
    """``toc3d_tracks_state_bytes`` of the built library (what :func:`state_bytes` restates)."""
    n = ctypes.c_int64(0)
    lib.call("toc3d_tracks_state_bytes", int(capacity), ctypes.byref(n))
    return n.value
