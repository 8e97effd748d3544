"""GPU: toc3d_token_alpha, toc3d_token_vis_render and toc3d_amd.TokenVis against the reference's arrays -- every case of tests/golden/token_vis_cases.npz (the
REAL reference function) in both source forms, further shapes against the numpy restatement (tests/token_vis_cases.py; tests/test_cpu_token_vis.py holds it to the
fixture), in six layouts with guard bytes around every output; pixel values that leave [0, 255] and the values on which a fused multiply-add would round
differently; keep lists with out-of-range and duplicate entries; the same call twice; 6 x 320 x 800 with three stages; and the detector with the visualisation
switched on against one without it, bit for bit, with the files it writes decoded and compared.  Every comparison is an equality of bytes.  Every test prints the
figures it asserts on (run with -s)."""
import json
import os

import numpy as np
import pytest
import torch

import detector_cases as DC
import toc3d_amd
import token_vis_cases as TC
from support import DEV, S, guarded, to_dev, touched
from toc3d_amd import lib, synth

pytestmark = pytest.mark.gpu

# (source offset, source row padding, destination offset) in bytes.  Contiguous; source rows padded by 4 (dwords still) and by 5 (bytes); a source base off by 1
# byte (an f32 source: off by 4, which leaves the 16-byte form); a destination base off by 4 (one pixel a thread, a dword per RGBA pixel); everything odd (bytes)
LAYOUTS = ((0, 0, 0), (0, 4, 0), (0, 5, 0), (1, 0, 0), (0, 0, 4), (1, 5, 1))


def pipeline(inp, c, form, layout=(0, 0, 0), with_keep=True):
    """Both entry points on the inputs of a case: the alphas of every stage, then one render.  -> (ori, rgba (A, V, H, W, 4), guard bytes that changed)."""
    src_off, src_pad, dst_off = layout
    V, (H0, W0), (hp, wp), p = c["V"], c["raw"], c["grid"], c["patch"]
    H, W, T, L = hp * p, wp * p, hp * wp, len(inp["masks"])
    with_keep = with_keep and inp["keeps"] is not None
    A = 2 * L if with_keep else L
    abuf, alpha = guarded(A * V * T)
    alpha = alpha.view(A, V, T)
    for l, m in enumerate(inp["masks"]):
        k = inp["keeps"][l] if with_keep else None
        K = 0 if k is None else k.shape[1]
        # the keep rows as the backbone hands them: the first K columns of a (V, T) order
        order = torch.full((V, T), -1, dtype=torch.int64, device=DEV)
        if K:
            order[:, :K] = torch.from_numpy(np.ascontiguousarray(k)).to(DEV)
        lib.call("toc3d_token_alpha", torch.from_numpy(m).to(DEV).contiguous(), order if K else None, T, K, V, T, 0.3, 1.0, alpha[l], alpha[L + l] if with_keep else None, S())
    n = c["norm"]
    if form == "u8":
        stride = W0 * 3 + src_pad
        sbuf = torch.full((src_off + V * H0 * stride,), 0x5A, dtype=torch.uint8, device=DEV)
        rows = sbuf[src_off:].view(V * H0, stride)
        rows[:, :W0 * 3] = torch.from_numpy(inp["raw"].reshape(V * H0, W0 * 3)).to(DEV)
        src, h0, w0 = sbuf[src_off:], H0, W0
    else:
        off = 4 * min(src_off, 1)
        sbuf = torch.zeros(off + V * 3 * H * W * 4, dtype=torch.uint8, device=DEV)
        sbuf[off:] = torch.from_numpy(inp["img"].reshape(-1).view(np.uint8)).to(DEV)
        src, stride, h0, w0 = sbuf[off:], 0, H, W
    obuf, ori = guarded(V * H * W * 3, dst_off)
    rbuf, rgba = guarded(A * V * H * W * 4, dst_off)
    lib.call("toc3d_token_vis_render", src, int(form == "u8"), stride, V, h0, w0, H, W, p, alpha, A, *n["mean"], *n["std"], int(n["to_rgb"]), ori, rgba, S())
    torch.cuda.synchronize()
    t = touched(abuf, A * V * T) + touched(obuf, V * H * W * 3, dst_off) + touched(rbuf, A * V * H * W * 4, dst_off)
    return ori.cpu().numpy().reshape(V, H, W, 3), rgba.cpu().numpy().reshape(A, V, H, W, 4), t


def expected(inp, c, form="f32"):
    if form == "u8":
        files = TC.restated_u8(inp["raw"], inp["masks"], inp["keeps"], inp["drops"], c["norm"], c["patch"])
    else:
        files = TC.restated(inp["img"], inp["masks"], inp["keeps"], inp["drops"], c["norm"], c["patch"])
    return files, TC.planes(files, c["V"], len(inp["masks"]), inp["keeps"] is not None)


def differing(got_ori, got_rgba, want):
    ori, masks, keep = want
    planes = masks if keep is None else np.concatenate([masks, keep])
    return int((got_ori != ori).sum()) + int((got_rgba != planes).sum())


def check_layouts(tag, inp, c, want_by_form, forms=("f32", "u8")):
    for form in forms:
        for layout in LAYOUTS:
            ori, rgba, t = pipeline(inp, c, form, layout)
            diff = differing(ori, rgba, want_by_form[form])
            print(f"{tag} {form} layout {layout}: {diff} of {ori.size + rgba.size} bytes differ, {t} guard bytes written")
            assert diff == 0 and t == 0, (tag, form, layout)


def render_class(inp, c, form):
    """toc3d_amd.TokenVis.render on the backbone's own types -> numpy (ori, masks, keepidx)."""
    vis = toc3d_amd.TokenVis(c["patch"])
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    masks = [dv(m) for m in inp["masks"]]
    keeps = None if inp["keeps"] is None else [dv(k) for k in inp["keeps"]]
    drops = None if inp["drops"] is None else [dv(k) for k in inp["drops"]]
    r = vis.render(dv(inp["raw"] if form == "u8" else inp["img"]), masks, keeps, drops, c["norm"])
    torch.cuda.synchronize()
    cpu = lambda t: None if t is None else t.cpu().numpy()
    return vis, r, (cpu(r["ori"]), cpu(r["masks"]), cpu(r["keepidx"]))


@pytest.fixture(scope="module")
def golden():
    return np.load(TC.FIXTURE), json.load(open(TC.FIXTURE_META))


def golden_planes(z, meta, case):
    c = TC.CASES[case]

    def key(name):
        base = name[:-4]
        return f"{case}_b_" + (base.split("_layer")[0] + "_ori" if base.endswith("_ori") else base)
    files = [(n, z[key(n)]) for n in meta["cases"][case]["files"]]
    L = len(c["K"]) if c["K"] is not None else 2
    return TC.planes(files, c["V"], L, c["K"] is not None)                  # (to_bytes of a uint8 array is the array)


@pytest.mark.parametrize("case", sorted(TC.CASES))
def test_fixture_cases_in_both_source_forms(golden, case):
    z, meta = golden
    c = TC.CASES[case]
    inp = TC.inputs(c, TC.case_seed(case))
    fixture = golden_planes(z, meta, case)
    for form in ("f32", "u8"):
        _, want = expected(inp, c, form)
        assert differing(want[0], want[1] if want[2] is None else np.concatenate([want[1], want[2]]), fixture) == 0, "the restatement is the fixture"
        _, r, got = render_class(inp, c, form)
        assert r["ori"].dtype == torch.uint8 and (got[2] is None) == (c["K"] is None)
        diff = differing(got[0], got[1] if got[2] is None else np.concatenate([got[1], got[2]]), fixture)
        print(f"case {case} {form}: TokenVis.render differs from the fixture in {diff} bytes")
        assert diff == 0
    check_layouts(f"case {case}", inp, c, dict(f32=fixture, u8=fixture))


@pytest.mark.parametrize("name", sorted(TC.SHAPES))
def test_shapes_and_layouts(name):
    c = TC.SHAPES[name]
    inp = TC.inputs(c, TC.case_seed(name))
    want = {form: expected(inp, c, form)[1] for form in ("f32", "u8")}
    assert differing(want["f32"][0], np.concatenate(want["f32"][1:]), want["u8"]) == 0, "both forms of a case come to the same bytes"
    check_layouts(name, inp, c, want)
    for form in ("f32", "u8"):
        _, _, got = render_class(inp, c, form)
        assert differing(got[0], np.concatenate(got[1:]), want[form]) == 0
    if 0 in c["K"]:
        stage = c["K"].index(0)
        assert (want["f32"][2][stage][..., 3] == 76).all(), "a stage that kept nothing: every token dropped"


def test_pixel_values_beyond_the_byte_range_and_the_fma_sensitive_set():
    """Float pixels that denormalise below 0 and above 255 (clipped), soft masks, and the values on which a fused multiply-add rounds to another byte."""
    x, ch = TC.fma_sensitive()
    c = dict(V=2, raw=(16, 96), grid=(1, 6), patch=16, K=(2,), soft=True, norm=TC.SHIPPED_NORM)
    inp = TC.inputs(c, 99)
    img = inp["img"]
    for k in range(3):
        xs = x[ch == k]
        img[0, k].reshape(-1)[:len(xs)] = xs
    rng = np.random.default_rng(3)
    img[1] = rng.uniform(-5.0, 5.0, img[1].shape).astype(np.float32)       # (-5 .. 5) * 57 + 104 .. 124: well beyond both ends
    img[1, :, 0, :6] = np.float32([-1e30, 1e30, -0.0, 2.65, -2.2, 1e-40])[None]
    files, want = expected(inp, c)
    low, high = int((want[0][1] == 0).sum()), int((want[0][1] == 255).sum())
    n = TC.SHIPPED_NORM
    fu, _ = TC.fused(x, TC.f32(n["std"])[ch], TC.f32(n["mean"])[ch])
    assert low > 1000 and high > 1000 and (TC.to_bytes(fu) != TC.to_bytes(TC.two_roundings(x, TC.f32(n["std"])[ch], TC.f32(n["mean"])[ch]))).all()
    for layout in ((0, 0, 0), (1, 0, 0), (0, 0, 4)):                        # 16-byte loads, single loads, the one-pixel form
        ori, rgba, t = pipeline(inp, c, "f32", layout)
        diff = differing(ori, rgba, want)
        sens = sum(int((ori[0].reshape(-1, 3)[:int((ch == k).sum()), k] != TC.to_bytes(TC.two_roundings(x[ch == k], n["std"][k], n["mean"][k]))).sum()) for k in range(3))
        print(f"layout {layout}: {diff} bytes differ; {len(x)} fma-sensitive values, {sens} off; {low} bytes clipped at 0, {high} at 255; {t} guard bytes written")
        assert diff == 0 and sens == 0 and t == 0


def test_keep_lists_with_out_of_range_and_duplicate_entries():
    V, T = 3, 39
    rng = np.random.default_rng(8)
    mask = rng.choice(TC.f32([0.0, 0.25, 0.5, 1.0]), size=(V, T))
    keep = np.stack([rng.permutation(T)[:12] for _ in range(V)]).astype(np.int64)
    bad = keep.copy()
    bad[0, 3], bad[0, 5], bad[1, 0], bad[1, 11], bad[2, 7] = -1, T, 2 ** 40, -(2 ** 62), T + 100
    bad[2, 8] = bad[2, 9]                                                   # a duplicate
    results = {}
    for tag, k in (("clean", keep), ("bad", bad)):
        abuf, out = guarded(2 * V * T)
        out = out.view(2, V, T)
        lib.call("toc3d_token_alpha", torch.from_numpy(mask).to(DEV), torch.from_numpy(k).to(DEV), 12, 12, V, T, 0.3, 1.0, out[0], out[1], S())
        torch.cuda.synchronize()
        results[tag] = (out.cpu().numpy(), touched(abuf, 2 * V * T))
    member = np.zeros((V, T), dtype=np.float32)
    for v in range(V):
        ok = bad[v][(bad[v] >= 0) & (bad[v] < T)]
        member[v, ok] = 1
    clean = np.zeros((V, T), dtype=np.float32)
    np.put_along_axis(clean, keep, 1.0, axis=1)
    print(f"guard bytes written: clean {results['clean'][1]}, with bad entries {results['bad'][1]}; kept tokens {int(clean.sum())} / {int(member.sum())}")
    assert np.array_equal(results["clean"][0][0], TC.to_bytes(TC.token_alpha(mask))) and np.array_equal(results["bad"][0][0], results["clean"][0][0])
    assert np.array_equal(results["clean"][0][1], TC.to_bytes(TC.token_alpha(clean))) and np.array_equal(results["bad"][0][1], TC.to_bytes(TC.token_alpha(member)))
    assert results["clean"][1] == 0 and results["bad"][1] == 0 and int(member.sum()) == int(clean.sum()) - 6
    assert set(np.unique(results["bad"][0][1]).tolist()) == {76, 255}


@pytest.fixture(scope="module")
def big():
    inp = TC.inputs(TC.BIG, TC.case_seed("big"))
    return inp, expected(inp, TC.BIG)[1]


def test_six_views_at_the_shipped_size(big):
    inp, want = big
    vis, r, got = render_class(inp, TC.BIG, "f32")
    assert tuple(r["masks"].shape) == (3, 6, 320, 800, 4) and tuple(r["keepidx"].shape) == (3, 6, 320, 800, 4) and tuple(r["ori"].shape) == (6, 320, 800, 3)
    diff = differing(got[0], np.concatenate(got[1:]), want)
    print(f"6 x 320 x 800, three stages: {diff} of {got[0].size + 2 * got[1].size} bytes differ")
    assert diff == 0
    _, _, got8 = render_class(inp, TC.BIG, "u8")
    assert differing(got8[0], np.concatenate(got8[1:]), want) == 0


def test_the_same_call_twice_gives_the_same_bytes(big):
    inp, want = big
    vis, r, first = render_class(inp, TC.BIG, "f32")
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    ptr = r["ori"].data_ptr()
    r2 = vis.render(dv(inp["img"]), [dv(m) for m in inp["masks"]], [dv(k) for k in inp["keeps"]], [dv(k) for k in inp["drops"]], TC.BIG["norm"])
    assert r2["ori"].data_ptr() == ptr, "the per-shape workspace is reused"
    assert np.array_equal(r2["ori"].cpu().numpy(), first[0]) and np.array_equal(r2["masks"].cpu().numpy(), first[1]) and np.array_equal(r2["keepidx"].cpu().numpy(), first[2])


# ---- the detector ------------------------------------------------------------------------------------------------------------------------------------------------
TINY = synth.DETECTOR_TINY
assert_same_bits = DC.assert_same_bits


def build_detector(precision, norm=None):
    return DC.build_detector(TINY, precision, norm=norm, builder=toc3d_amd.build_vis_detector)


def run(det, frames, at=None):
    """simple_test over the frames -> per frame what must keep its bits; ``at``: the frame whose last_frame tensors and image are brought to the host."""
    kept = {}

    def on_frame(f, det, data, results):
        if f == at:
            last, cpu = det.last_frame, lambda ts: [t.cpu().numpy() for t in ts]
            kept.update(img=data["img"].cpu().numpy(), masks=cpu(last["token_masks"]), keeps=cpu(last["keep_idxes"]), drops=cpu(last["drop_idxes"]))
    return DC.run(det, frames, on_frame=on_frame), kept or None


def check_files(tmp_path, files, V, L):
    assert sorted(os.listdir(tmp_path / "token_vis")) == ["1"], "exactly the directory of frame 1"
    out = tmp_path / "token_vis" / "1"
    assert sorted(os.listdir(out)) == sorted(n for n, _ in files) and len(files) == V * L * 3
    bad = 0
    for n, arr in files:
        want = TC.to_bytes(arr)
        want = np.concatenate([want[..., 2::-1], want[..., 3:]], axis=-1)   # cv2.imwrite: array channel 0 is blue
        bad += int((TC.decode_png(open(out / n, "rb").read()) != want).sum())
    return bad


@pytest.mark.parametrize("precision", ["fp32x3", "bf16"])
def test_detector_keeps_its_bits_and_writes_frame_one(tmp_path, monkeypatch, precision):
    monkeypatch.chdir(tmp_path)
    frames = []
    for fr in synth.detector_inputs(TINY)[:3]:
        metas = [dict(fr["img_metas"][0], img_norm_cfg=TC.SHIPPED_NORM)]
        frames.append(dict(img_metas=metas, gumbel=fr["gumbel"], dev=to_dev(fr)))
    plain, _ = run(build_detector(precision), frames)
    assert not os.path.exists(tmp_path / "token_vis"), "off: nothing is written"
    det = build_detector(precision).enable_token_vis(vis_num_sample=1, vis_start_id=1, vis_out_path="token_vis")
    got, kept = run(det, frames, at=1)
    assert_same_bits(got, plain)
    assert det.cur_id == 2 and det.vis_num_sample == 0
    files = TC.restated(kept["img"][0], kept["masks"], kept["keeps"], kept["drops"], TC.SHIPPED_NORM, 16)
    bad = check_files(tmp_path, files, 6, 3)
    print(f"{precision}: three frames equal a detector without the visualisation bit for bit; {len(files)} files of frame 1, {bad} bytes differ from the restatement")
    assert bad == 0


def test_detector_on_uint8_frames(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(21)
    frames = []
    for f, fr in enumerate(synth.detector_inputs(TINY)[:3]):
        dev = to_dev(fr)
        dev["img"] = torch.from_numpy(rng.integers(0, 256, (1, 6, 318, 796, 3), dtype=np.uint8)).to(DEV)
        frames.append(dict(img_metas=fr["img_metas"], gumbel=fr["gumbel"], dev=dev))                       # no img_norm_cfg in the metas: the backbone's is taken
    norm = dict(TC.RGB_NORM)
    plain, _ = run(build_detector("fp32x3", norm), frames)
    det = build_detector("fp32x3", norm).enable_token_vis(vis_num_sample=1, vis_start_id=1, vis_out_path="token_vis")
    got, kept = run(det, frames, at=1)
    assert_same_bits(got, plain)
    files = TC.restated_u8(kept["img"][0], kept["masks"], kept["keeps"], kept["drops"], norm, 16)
    bad = check_files(tmp_path, files, 6, 3)
    pad = TC.decode_png(open(tmp_path / "token_vis" / "1" / "view0_layer0_ori.png", "rb").read())[319, 799]
    print(f"uint8 frames 318 x 796 padded to 320 x 800: {len(files)} files, {bad} bytes differ; padding pixel in the file (R, G, B) = {pad.tolist()}")
    assert bad == 0 and pad.tolist() == [104, 116, 124], "rint(mean), array channel 0 (red after to_rgb) stored as blue"
