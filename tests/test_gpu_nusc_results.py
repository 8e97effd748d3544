"""GPU: toc3d_boxes_to_global and toc3d_amd.NuScenesResults against the fixture of tests/nusc_results_cases.py (tests/golden/nusc_results_cases.npz: the seeded
inputs and the float64 restatement's outputs) -- kept, src, name, attr and the score bits exactly, the size bit for bit, every other record element within the
bound derived in that module, at 0, 1, 63 / 64 / 65, 256 / 257 and 2048 boxes a sample with every keep pattern; row and sample strides; guard bytes around every
output; the same call twice; the class on top of it; and the detector with the records switched on against one without, bit for bit, in both precisions and for a
step of two streams.  Every test prints the figures it asserts on (run with -s)."""
import functools
import math
import os

import numpy as np
import pytest
import torch

import detector_cases as DC
import nusc_results_cases as NC
import toc3d_amd
from support import DEV, S, guarded, to_dev, touched, worst_report
from toc3d_amd import lib, synth

pytestmark = pytest.mark.gpu
ENTRY = "toc3d_boxes_to_global"
OUT_DTYPES = dict(rec=np.float64, score=np.float32, name=np.int32, attr=np.int32, src=np.int32, kept=np.int64)
note, _report = worst_report("nuScenes records", 44)
dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def launch(c, box_stride=9, sample_pad=0, with_velocity=None, poses=None):
    """One call of the entry point on a case -> (outputs as numpy, guard bytes written).  The boxes lie in a NaN-filled buffer with rows ``box_stride`` and samples
    ``K * box_stride + sample_pad`` elements apart; every output lies between guard bytes."""
    B, K = c["scores"].shape
    vel = c["with_velocity"] if with_velocity is None else with_velocity
    width = min(box_stride, 9)
    sample_stride = K * box_stride + sample_pad
    flat = np.full((B, sample_stride), np.nan, dtype=np.float32)
    for b in range(B):
        flat[b, :K * box_stride].reshape(K, box_stride)[:, :width] = c["boxes"][b, :, :width]          # (a view: one sample's rows are contiguous)
    rng, mov, still = NC.tables()
    shapes = dict(rec=(B, K, 12), score=(B, K), name=(B, K), attr=(B, K), src=(B, K), kept=(B,))
    bufs = {k: guarded(int(np.prod(shapes[k])) * np.dtype(OUT_DTYPES[k]).itemsize) for k in NC.OUT_KEYS}
    lib.call(ENTRY, dv(flat), box_stride, sample_stride, dv(c["scores"]), dv(c["labels"]), dv(c["counts"]), B, K, int(vel), dv(c["poses"] if poses is None else poses), dv(rng),
             dv(mov), dv(still), len(NC.CLASS_NAMES), NC.SPEED_THR, *[bufs[k][1] for k in NC.OUT_KEYS], S())
    torch.cuda.synchronize()
    out = {k: bufs[k][1].cpu().numpy().view(OUT_DTYPES[k]).reshape(shapes[k]) for k in NC.OUT_KEYS}
    g = sum(touched(bufs[k][0], bufs[k][1].numel()) for k in NC.OUT_KEYS)
    return out, g


_TRIG = {}


def trig_error():
    """E of tests/nusc_results_cases.py: the largest difference between the device's float64 sin / cos and Python's math.sin / math.cos on the half angles of the
    fixture's own kept boxes.  MEASURED, because the accuracy table of the HIP math library is not at hand where the tests run: boxes at the origin under identity
    poses leave exactly (cos, 0, 0, sin) in the record's orientation (1 * c - 0 * s and 1 * s + 0 * c are exact).  Sanity ceiling: 4 ulp, OpenCL's own bound for
    double sin and cos."""
    if "E" not in _TRIG:
        yaws = np.concatenate([c["boxes"][b, c["src"][b, :c["kept"][b]], 6] for c in map(NC.load_case, NC.CASES) for b in range(len(c["kept"]))]).astype(np.float32)
        B = -(-len(yaws) // 2048)
        boxes = np.zeros((B, 2048, 9), dtype=np.float32)
        boxes[:, :, 3:6] = 1.0
        boxes.reshape(-1, 9)[:len(yaws), 6] = yaws
        case = dict(boxes=boxes, scores=np.full((B, 2048), 0.5, dtype=np.float32), labels=np.zeros((B, 2048), dtype=np.int64),
                    counts=np.full(B, 2048, dtype=np.int64), poses=np.array([[NC.IDENTITY_POSE, NC.IDENTITY_POSE]] * B), with_velocity=True)
        out, g = launch(case)
        assert g == 0 and (out["kept"] == 2048).all()
        q = out["rec"].reshape(-1, 12)[:len(yaws), 6:10]
        half = yaws.astype(np.float64) / 2
        E = max(max(abs(q[i, 0] - math.cos(h)), abs(q[i, 3] - math.sin(h))) for i, h in enumerate(half.tolist()))
        assert (q[:, 1:3] == 0).all()
        print(f"device float64 sin / cos against math.sin / math.cos on {len(yaws)} half angles in [{half.min():.3f}, {half.max():.3f}]: at most {E:.3e} = {E / 2 ** -53:.2f} ulp of 1")
        assert E <= 4 * 2.0 ** -52
        _TRIG["E"] = E
    return _TRIG["E"]


def compare(tag, out, c):
    """The exact checks and the bound -> the worst fraction of the bound."""
    B, K = c["scores"].shape
    for k in ("kept", "src", "name", "attr"):
        assert np.array_equal(out[k], c[k]), f"{tag}: {k}"
    assert np.array_equal(out["score"].view(np.int32), c["score"].view(np.int32)), f"{tag}: score, bit for bit"
    assert np.array_equal(out["rec"][..., 3:6].view(np.int64), c["rec"][..., 3:6].view(np.int64)), f"{tag}: size, bit for bit"
    live = np.arange(K)[None] < c["kept"][:, None]
    src = np.where(live, c["src"], 0)
    promoted = np.take_along_axis(c["boxes"], src[..., None], axis=1)[..., [4, 3, 5]].astype(np.float64)
    assert np.array_equal(out["rec"][..., 3:6][live], promoted[live]), f"{tag}: size is columns [4, 3, 5] of the input row, promoted"
    assert (out["rec"][~live].view(np.int64) == 0).all() and (out["score"][~live].view(np.int32) == 0).all(), f"{tag}: the tail is zeros"
    if not live.any():
        return 0.0
    bound = c["bound"].copy()
    bound[..., 6:10] += 4 * trig_error()
    err = np.abs(out["rec"] - c["rec"])[live]
    cols = [0, 1, 2, 6, 7, 8, 9, 10, 11]
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.where(bound[live][:, cols] > 0, err[:, cols] / bound[live][:, cols], np.where(err[:, cols] == 0, 0.0, np.inf))
    assert bound.max() < 1e-10, f"{tag}: the bound itself is small (largest {bound.max():.2e})"
    return float(frac.max())


# ---- the entry point against the fixture --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NC.CASES)
def test_records_equal_the_restatement(name):
    """THE BOUND (tests/nusc_results_cases.py, u = 2^-53): a translation within (e_0 + e_1 + e_2) + 18 u S' + 8 u |t'_i| with e_i = 18 u S + 8 u |t_i| and S the
    sum of the centre's magnitudes before each pose; a velocity within 54 u V + 18 u V'; an orientation component within 26 u + 4 E, E the device's sin / cos error
    measured by trig_error(); size and score exact.  Written down before the first run on a device, not fitted; the test prints the worst fraction of it."""
    c = NC.load_case(name)
    out, g = launch(c, box_stride=9 if c["with_velocity"] else 7)
    frac = compare(name, out, c)
    note(f"rec / bound, {name}", frac)
    kept, n = c["kept"].tolist(), c["counts"].tolist()
    print(f"{name}: kept {kept} of {n} (K = {c['scores'].shape[1]}): kept, src, name, attr, score and size equal; worst record element {frac:.3f} of its bound; {g} guard bytes written")
    assert g == 0 and frac <= 1.0


def test_exact_cases_by_name():
    c = NC.load_case(NC.EXACT_CASE)
    out, _ = launch(c)
    annos = toc3d_amd.NuScenesResults().records_to_annos(out["rec"], out["score"], out["name"], out["attr"], out["kept"])[0]
    want = [r for r in NC.EXACT_ROWS if r[4] is not None]
    got = [(a["detection_name"], a["translation"][0], a["translation"][1], a["velocity"][0], a["attribute_name"]) for a in annos]
    print(f"exact cases: {got}")
    assert got == want and out["src"][0, :len(want)].tolist() == [0] + list(range(2, len(NC.EXACT_ROWS)))
    assert np.array_equal(out["rec"][0].view(np.int64), c["rec"][0].view(np.int64)), "identity poses, yaw 0: every bit of every record"


@pytest.mark.parametrize("name,stride,pad,vel", [("wave_random", 11, 0, True), ("wave_random", 9, 5, True), ("wave_mixed", 11, 13, True), ("wave_novel", 9, 0, False),
                                                 ("wave_novel", 11, 7, False), ("chunk_random", 11, 1, True)])
def test_row_and_sample_strides(name, stride, pad, vel):
    """Rows 7 (without the velocity), 9 and 11 elements apart and samples further apart than K rows: the same bytes as the dense layout; what lies between the
    rows is NaN and is not read."""
    c = NC.load_case(name)
    assert c["with_velocity"] == vel
    dense, _ = launch(c, box_stride=9 if vel else 7)
    out, g = launch(c, box_stride=stride, sample_pad=pad)
    same = all(np.array_equal(out[k].view(np.uint8), dense[k].view(np.uint8)) for k in NC.OUT_KEYS)
    print(f"{name}: box_stride {stride}, sample_stride K * {stride} + {pad}, with_velocity {int(vel)}: the same bytes as the dense layout: {same}; {g} guard bytes written")
    assert same and g == 0
    assert compare(name, out, c) <= 1.0


def test_the_same_call_twice_gives_identical_bytes():
    c = NC.load_case("full")
    a, ga = launch(c)
    b, gb = launch(c)
    assert ga == gb == 0 and all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in NC.OUT_KEYS)
    print(f"2048 boxes, {int(a['kept'][0])} kept: two calls, identical bytes in all six outputs")


# ---- the class -------------------------------------------------------------------------------------------------------------------------------------------------------
def test_format_fixed_and_format():
    c = NC.load_case("wave_mixed")
    res = toc3d_amd.NuScenesResults()
    fixed = res.format_fixed(dv(c["boxes"]), dv(c["scores"]), dv(c["labels"]), dv(c["counts"]), c["poses"])
    torch.cuda.synchronize()
    host = {k: fixed[k].cpu().numpy() for k in NC.OUT_KEYS}
    assert [host[k].dtype for k in NC.OUT_KEYS] == [OUT_DTYPES[k] for k in NC.OUT_KEYS] and all(fixed[k].is_cuda for k in NC.OUT_KEYS)
    raw, _ = launch(c)
    assert all(np.array_equal(host[k].view(np.uint8), raw[k].view(np.uint8)) for k in NC.OUT_KEYS), "the class passes the case through unchanged"
    records = NC.pose_records(c["poses"])
    tokens = ["a", "b", "c"]
    fixed = res.format_fixed(dv(c["boxes"]), dv(c["scores"]), dv(c["labels"]), dv(c["counts"]), records)           # (normalised again: may move a pose by an ulp)
    want = res.records_to_annos(*[fixed[k].cpu().numpy() for k in ("rec", "score", "name", "attr", "kept")], tokens)
    n = c["counts"].tolist()
    lists = [[dv(c["boxes"][b, :n[b]]), dv(c["scores"][b, :n[b]]), dv(c["labels"][b, :n[b]])] for b in range(3)]
    got = res.format(lists, records, tokens)
    print(f"format on lists of {n} boxes: {[len(a) for a in got]} records, equal to format_fixed + records_to_annos: {got == want}")
    assert got == want and [len(a) for a in got] == c["kept"].tolist() and sum(map(len, got)) > 0

    class Boxes:                                                            # boxes as an object with .tensor, and the empty list
        tensor = lists[1][0]
    assert res.format([[Boxes(), lists[1][1], lists[1][2]]], records[1:2], ["b"]) == [want[1]]
    none = [torch.zeros(0, 9, device=DEV), torch.zeros(0, device=DEV), torch.zeros(0, dtype=torch.int64, device=DEV)]
    assert res.format([none], records[:1]) == [[]] and res.format([], []) == []
    # without the velocity: seven columns suffice
    novel = NC.load_case("wave_novel")
    r7 = toc3d_amd.NuScenesResults(with_velocity=False).format_fixed(dv(novel["boxes"][..., :7]), dv(novel["scores"]), dv(novel["labels"]), dv(novel["counts"]), novel["poses"])
    assert np.array_equal(r7["kept"].cpu().numpy(), novel["kept"]) and np.array_equal(r7["attr"].cpu().numpy(), novel["attr"]) and (r7["rec"][..., 10:].cpu().numpy() == 0).all()
    with pytest.raises(ValueError, match=r"\(B, K, >= 9\)"):
        res.format_fixed(dv(novel["boxes"][..., :7]), dv(novel["scores"]), dv(novel["labels"]), dv(novel["counts"]), novel["poses"])


# ---- the detector ------------------------------------------------------------------------------------------------------------------------------------------------
TINY = synth.DETECTOR_TINY
build_detector = functools.partial(DC.build_detector, TINY)
run, assert_same_bits, with_pose = DC.run, DC.assert_same_bits, DC.with_pose


def independent(dec, meta, token):
    """The records of one sample's decoded lists from a NuScenesResults of its own: a B = 1 run."""
    boxes = torch.as_tensor(getattr(dec["boxes_3d"], "tensor", dec["boxes_3d"])).to(DEV)
    return toc3d_amd.NuScenesResults().format([[boxes, torch.as_tensor(dec["scores_3d"]).to(DEV), torch.as_tensor(dec["labels_3d"]).to(DEV)]], [meta], [token])[0]


@pytest.mark.parametrize("precision", ["fp32x3", "bf16"])
def test_detector_keeps_its_bits_and_gathers_the_records(precision):
    frames = []
    for f, fr in enumerate(synth.detector_inputs(TINY)[:3]):
        frames.append(dict(img_metas=[with_pose(fr["img_metas"][0], f"sample{f}", 40 + f)], gumbel=fr["gumbel"], dev=to_dev(fr)))
    plain = run(build_detector(precision), frames)
    det = build_detector(precision).enable_nusc_results()
    got = run(det, frames)
    assert_same_bits(got, plain)
    assert list(det.nusc_results.results) == ["sample0", "sample1", "sample2"]
    counts = []
    for f, fr in enumerate(frames):
        want = independent(plain[f][0]["dec"], fr["img_metas"][0], f"sample{f}")
        assert det.nusc_results.results[f"sample{f}"] == want, f"frame {f}"
        counts.append((len(torch.as_tensor(plain[f][0]["dec"]["scores_3d"])), len(want)))
    print(f"{precision}: three frames equal a detector without the records bit for bit; (decoded, inside their class range) per frame: {counts}")
    assert sum(n for n, _ in counts) > 0
    det.disable_nusc_results()
    run(det, frames[:1])
    assert list(det.nusc_results.results) == ["sample0", "sample1", "sample2"]


def test_detector_streams_step_with_a_pose_per_stream(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    steps, _ = synth.detector_stream_steps(TINY, seeds=(0, 1), new_scene_at=(3, 2))
    st = steps[0]
    metas = [with_pose(m, f"stream{b}", 50 + b) for b, m in enumerate(st["img_metas"])]
    assert metas[0]["ego2global_translation"] != metas[1]["ego2global_translation"]
    frames = [dict(img_metas=metas, gumbel=st["gumbel"], dev=to_dev(st))]
    plain = run(build_detector("fp32x3"), frames, streams=True)
    det = build_detector("fp32x3").enable_nusc_results().enable_box_vis(num_sample=1, out_path="box_vis", score_thr=0.0)       # alongside the box overlays
    got = run(det, frames, streams=True)
    assert_same_bits(got, plain)
    assert sorted(os.listdir(tmp_path / "box_vis" / "0")) == ["stream0", "stream1"]
    assert list(det.nusc_results.results) == ["stream0", "stream1"]
    for b in range(2):
        want = independent(plain[0][b]["dec"], metas[b], f"stream{b}")
        n = len(torch.as_tensor(plain[0][b]["dec"]["scores_3d"]))
        print(f"stream {b}: {n} decoded boxes, {len(want)} records, equal to a B = 1 run on its own pose: {det.nusc_results.results[f'stream{b}'] == want}")
        assert det.nusc_results.results[f"stream{b}"] == want and n > 0
    path = det.nusc_results.dump(str(tmp_path / "res"))
    assert os.path.getsize(path) > 0
