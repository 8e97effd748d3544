"""GPU: several camera streams per step.

(a) toc3d_score_head_frames against toc3d_score_head: the rows of flagged frames bit for bit, every other row still the sentinel the buffers were filled with,
    and (F32) the flagged rows against the f64 tail of tests/scorer_cases.py at ITS bar (``tail_ref64``: per element, from the logits' bound and the measured libm
    allowance -- the bar tests/test_gpu_scorer_kernels.py holds toc3d_score_head to; it is tighter than a flat 1e-5 on ordinary rows and wider on the rows whose
    logits are spread to |l0 - l1| ~ 100).  F = 3 frames of 74 rows (two views of 37 tokens: no multiple of 4 or 64, workgroups straddle frame boundaries) and
    F = 1; kdim 64 and 256 with a padded ld whose padding holds NaN; BF16 and F32; noise given and NULL; flags 000, 111, 010, 101.
(b) the backbone with a per-frame ``prev_exists`` list (toc3d_tiny, two views per frame): B = 2 with [True, False] and [False, True], B = 3 with
    [True, False, True].  Every frame's kept sets and ``last_feat`` equal, BIT FOR BIT, a B = 1 forward of the same model on that frame's inputs with that frame's
    bool -- fp32, fp32x3 and bf16, view_groups 1 and 2 (and 4: groups that hold part of a frame), plan and eager; in fp32 (the precision
    tests/test_gpu_e2e.py::test_two_frames_batch_matches_oracle runs) every frame is also held to the oracle run per frame at that test's bar: rel max < 1e-3,
    kept-set IoU > 0.995.  [True, True] is ``True`` and [False, False] is ``False``, bit for bit.  GEMM tiles are not autotuned (every tile variant accumulates in
    the same order), so no launch choice depends on the batch.
(c) the detector (DETECTOR_TINY): two streams, seeds 0 and 1, scene changes at frames 3 and 2 -- the four steps are all new, both continuing, mixed, mixed --
    against two separate B = 1 detectors with the same weights stepped through their stream with ``simple_test``: kept sets, ``img_feats``, both head outputs, each
    sample's bank after every step and the decoded lists, bit for bit, in fp32x3 and bf16, plan and eager; the same streams run twice give the same bits, and
    ``reset_streams([1])`` makes stream 1's next step a first frame.
Every test prints the figures it asserts on (run with -s)."""
import pytest
import torch

import detector_cases as DC
import scorer_cases as SC
import toc3d_amd
from oracle import toc3d_oracle as O
from support import DEV, iou, rel_max
from toc3d_amd import configs, lib, synth

pytestmark = pytest.mark.gpu
S = lambda: torch.cuda.current_stream().cuda_stream
SENTINEL = 0x7FC0BEEF                         # a NaN no kernel produces: the buffers are compared as bits


# ---- (a) the kernel ----------------------------------------------------------------------------------------------------------------------------------------------
RPF = 74                                      # two views of 37 tokens


def sentinel_bufs(M):
    mk = lambda *s: torch.full(s, SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
    return mk(M, 2), mk(M), mk(M)


bits = lambda t: t.contiguous().view(torch.int32)


@pytest.mark.parametrize("with_noise", [True, False], ids=["noise", "null"])
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("kdim", [64, 256])
@pytest.mark.parametrize("F", [3, 1])
def test_a_score_head_frames_against_score_head(F, kdim, bf16, with_noise):
    M, ld, dt = F * RPF, kdim + 8, lib.BF16 if bf16 else lib.F32
    i = SC.head_inputs(kdim, ld, M, bf16)
    g = SC.gumbel_rows(M, 11 + F) if with_noise else None
    fd, wd, bd, gd = i["f"].to(DEV), i["w"].to(DEV), i["b"].to(DEV), None if g is None else g.to(DEV)
    want = sentinel_bufs(M)
    lib.call("toc3d_score_head", dt, fd, ld, kdim, wd, bd, gd, M, *want, S())
    logits, delta = SC.head_logits64(i)
    ref = SC.tail_ref64(logits, delta, g)
    for pattern in (["000", "111", "010", "101"] if F == 3 else ["0", "1"]):
        flags = torch.tensor([float(c) for c in pattern], device=DEV)
        got = sentinel_bufs(M)
        lib.call("toc3d_score_head_frames", dt, fd, ld, kdim, wd, bd, gd, flags, RPF, M, *got, S())
        torch.cuda.synchronize()
        rows = torch.tensor([c == "1" for c in pattern]).repeat_interleave(RPF)
        n_new = int(rows.sum())
        for name, a, b in zip(("pred", "score", "mask_out"), got, want):
            a, b = bits(a).cpu(), bits(b).cpu()
            assert torch.equal(a[rows], b[rows]), f"{name} {pattern}: flagged rows differ from toc3d_score_head"
            assert bool((a[~rows] == SENTINEL).all()), f"{name} {pattern}: a row of a frame that is not new was written"
        if n_new:
            assert bool((bits(got[0]).cpu()[rows] != SENTINEL).all()), "flagged rows were written"
        worst_p = worst_m = 0.0
        if not bf16 and n_new:
            ep = (got[0].cpu().double() - ref["pred"])[rows].abs() / ref["pred_tol"][rows]
            em = (got[2].cpu().double() - ref["mask"])[rows].abs() / ref["mask_tol"][rows]
            worst_p, worst_m = float(ep.max()), float(em.max())
            assert worst_p <= 1.0 and worst_m <= 1.0, (pattern, worst_p, worst_m)
        print(f"[score_head_frames F={F} kdim={kdim} ld={ld} {'bf16' if bf16 else 'f32'} noise={with_noise} flags={pattern}] {n_new} flagged rows equal bit for bit, "
              f"{M - n_new} rows keep the sentinel; worst error / f64 bound: pred {worst_p:.3f}, mask {worst_m:.3f} (k_pred {ref['k_pred']:.2f})")


# ---- (b) the backbone --------------------------------------------------------------------------------------------------------------------------------------------
PATTERNS = [(True, False), (False, True), (True, False, True)]
_FRAMES, _ORACLE = {}, {}


def frame_inputs(cfg, f):
    if f not in _FRAMES:
        _FRAMES[f] = synth.make_inputs(cfg, n_frames=1, views_per_frame=2, seed=f)
    return _FRAMES[f]


def oracle_frame(cfg, f, prev):
    """The oracle on frame f alone with that frame's bool: computed once, shared, never changed."""
    if (f, prev) not in _ORACLE:
        inp = frame_inputs(cfg, f)
        with torch.no_grad():
            _ORACLE[(f, prev)] = O.forward_toc3d(synth.make_state_dict(cfg), cfg, inp["x"], inp["temp_queries"], inp["temp_ref_points"], inp["temp_vel"],
                                                 inp["temp_timestamp"], inp["temp_ego_pose"], inp["ego_pose_inv"], prev, inp["gumbel"])
    return _ORACLE[(f, prev)]


def build_backbone(precision, groups, launch_mode):
    cfg = configs.get("toc3d_tiny")
    m = toc3d_amd.build_backbone(dict(cfg, precision=precision))
    m.load_state_dict(synth.make_state_dict(cfg), strict=True)
    m = m.to(DEV).eval()
    m.view_groups, m.launch_mode, m.autotune = groups, launch_mode, False
    return cfg, m


def run_backbone(m, inp, prev, times=3):
    """``times`` forwards (eager warm-up, the recording of the plan, its replay): the last one is what is compared."""
    d = lambda t: t.to(DEV)
    for _ in range(times):
        out = m(d(inp["x"]), temp_queries=d(inp["temp_queries"]), prev_exists=prev, temp_ref_points=d(inp["temp_ref_points"]), temp_vel=d(inp["temp_vel"]),
                temp_timestamp=d(inp["temp_timestamp"]), temp_ego_pose=d(inp["temp_ego_pose"]), ego_pose_inv=d(inp["ego_pose_inv"]), gumbel_noise=inp["gumbel"])
    torch.cuda.synchronize()
    return dict(keep=[k.clone() for k in out.keep_idx], mask=[t.clone() for t in out.token_masks], feat=out.img_feats["last_feat"].clone())


BACKBONE_CASES = [(p, g, lm) for p in ("fp32", "fp32x3", "bf16") for g in (1, 2) for lm in ("plan", "eager")] + [("fp32x3", 4, "plan"), ("bf16", 4, "eager")]


@pytest.mark.parametrize("precision,groups,launch_mode", BACKBONE_CASES)
def test_b_backbone_mixed_step_is_each_frame_alone(precision, groups, launch_mode):
    cfg, m = build_backbone(precision, groups, launch_mode)
    single = {}
    for pattern in PATTERNS:
        B = len(pattern)
        got = run_backbone(m, synth.stack_frames([frame_inputs(cfg, f) for f in range(B)]), list(pattern))
        assert tuple(got["feat"].shape) == (2 * B, 128, 20, 50)
        for f, prev in enumerate(pattern):
            if (f, prev) not in single:
                single[(f, prev)] = run_backbone(m, frame_inputs(cfg, f), prev)
            one, v = single[(f, prev)], slice(2 * f, 2 * f + 2)
            for s in range(3):
                assert torch.equal(got["keep"][s][v], one["keep"][s]), f"{pattern} frame {f} stage {s}: kept set differs from the B = 1 forward"
                assert torch.equal(got["mask"][s][v], one["mask"][s]), f"{pattern} frame {f} stage {s}: soft mask differs from the B = 1 forward"
            assert torch.equal(got["feat"][v], one["feat"]), f"{pattern} frame {f}: last_feat differs from the B = 1 forward"
            line = f"[{precision} groups={groups} {launch_mode} {pattern}] frame {f} (prev_exists={prev}): kept sets, masks and last_feat equal the B = 1 forward bit for bit"
            if precision == "fp32":
                ref = oracle_frame(cfg, f, prev)
                err = rel_max(got["feat"][v], ref["last_feat"])
                ious = [iou(got["keep"][s][v], ref["keep_idx"][s].numpy()) for s in range(3)]
                line += f"; vs the oracle: rel max {err:.3e}, kept-set IoU {min(ious):.4f}"
                assert err < 1e-3 and min(ious) > 0.995, (pattern, f, err, ious)
            print(line)
    # the mixed steps ran the third mode -- in the plan launch mode as ONE recorded plan per batch size, whatever the pattern
    states = [st for gp in m._plans.values() for k, st in gp.get("launch", {}).items() if k[0] == "mixed"]
    print(f"[{precision} groups={groups} {launch_mode}] mixed launch states: {len(states)}, recorded: {[st.get('cplan') is not None for st in states]}")
    assert len(states) == 2 and all((st.get("cplan") is not None) == (launch_mode == "plan") for st in states)
    # a new frame and a continuing one really take different scorers: frame 0's kept set as a new frame is not its set as a continuing one
    if (0, False) not in single:
        single[(0, False)] = run_backbone(m, frame_inputs(cfg, 0), False)
    assert not torch.equal(single[(0, True)]["keep"][0], single[(0, False)]["keep"][0])


@pytest.mark.parametrize("launch_mode", ["plan", "eager"])
@pytest.mark.parametrize("precision", ["fp32x3", "bf16"])
def test_b_uniform_lists_are_the_single_bool(precision, launch_mode):
    cfg, m = build_backbone(precision, 2, launch_mode)
    inp = synth.stack_frames([frame_inputs(cfg, f) for f in range(2)])
    for flag in (True, False):
        a, b, c = run_backbone(m, inp, flag), run_backbone(m, inp, [flag, flag]), run_backbone(m, inp, (flag, flag))
        for other in (b, c):
            assert all(torch.equal(x, y) for x, y in zip(a["keep"], other["keep"])) and all(torch.equal(x, y) for x, y in zip(a["mask"], other["mask"]))
            assert torch.equal(a["feat"], other["feat"])
        modes = sorted(str(k[0]) for gp in m._plans.values() for k in gp.get("launch", {}))
        print(f"[{precision} {launch_mode}] prev_exists=[{flag}, {flag}] equals {flag} bit for bit; recorded modes so far: {modes}")
        assert "mixed" not in modes, "a uniform list takes the existing path, not the mixed one"
    with pytest.raises(ValueError, match="3 entries for 2 frames"):
        run_backbone(m, inp, [True, False, True], times=1)


# ---- (c) the detector --------------------------------------------------------------------------------------------------------------------------------------------
TINY = synth.DETECTOR_TINY
BANK = DC.BANK


def build_detector(precision, launch_mode="plan"):
    return DC.build_detector(TINY, precision, launch_mode)


def check_results(f, det, data, results):
    B = data["img"].shape[0]
    assert isinstance(results, list) and len(results) == B and all(set(r) == {"pts_bbox"} for r in results)


def run_streams(det, steps):
    return DC.run(det, steps, streams=True, on_frame=check_results)


def run_single(det, frames):
    return [r[0] for r in DC.run(det, frames)]


def assert_same(tag, x, y):
    assert len(x["keep"]) == len(y["keep"]) == 3 and all(torch.equal(p, q) for p, q in zip(x["keep"], y["keep"])), f"{tag}: kept token sets differ"
    assert torch.equal(x["img_feats"], y["img_feats"]), f"{tag}: img_feats differ"
    for k in ("all_cls_scores", "all_bbox_preds"):
        assert torch.equal(x["out"][k], y["out"][k]), f"{tag}: {k} differs"
    for k in BANK:
        assert torch.equal(x["bank"][k], y["bank"][k]), f"{tag}: {k} differs"
    for k in ("boxes_3d", "scores_3d", "labels_3d"):
        assert torch.equal(torch.as_tensor(x["dec"][k]), torch.as_tensor(y["dec"][k])), f"{tag}: decoded {k} differ"
    print(f"[{tag}] kept sets, img_feats, outputs, bank and {x['dec']['labels_3d'].shape[0]} decoded boxes equal bit for bit")


@pytest.mark.parametrize("launch_mode", ["plan", "eager"])
@pytest.mark.parametrize("precision", ["fp32x3", "bf16"])
def test_c_two_streams_are_two_single_stream_detectors(precision, launch_mode):
    steps, streams = synth.detector_stream_steps(TINY, seeds=(0, 1), new_scene_at=(3, 2))
    scenes = [[m["scene_token"] for m in st["img_metas"]] for st in steps]
    assert scenes == [["a", "a"], ["a", "a"], ["a", "b"], ["b", "b"]], scenes           # all new, both continuing, mixed, mixed
    det = build_detector(precision, launch_mode)
    calls = []
    fwd = det.img_backbone.forward
    det.img_backbone.forward = lambda *a, **k: (calls.append(k["prev_exists"]), fwd(*a, **k))[1]
    got = run_streams(det, steps)
    assert calls == [[False, False], [True, True], [True, False], [False, True]], calls
    assert tuple(det.last_frame["img_feats"].shape) == (2, 6, 32, 20, 50) and tuple(det.pts_bbox_head.memory_embedding.shape) == (2, 160 + 64, 256)
    del det
    for b in range(2):
        want = run_single(build_detector(precision, launch_mode), streams[b])
        for f in range(len(steps)):
            assert_same(f"{precision} {launch_mode} stream {b} step {f} ({'new' if not calls[f][b] else 'continuing'})", got[f][b], want[f])
        assert torch.isfinite(got[-1][b]["out"]["all_bbox_preds"]).all()


def test_c_state_determinism_and_reset_streams():
    steps, streams = synth.detector_stream_steps(TINY, seeds=(0, 1), new_scene_at=(3, 2))
    det = build_detector("fp32x3")
    first = run_streams(det, steps)
    assert det.prev_scene_tokens == ["b", "b"]
    # the same streams again: step 0 carries scene "a" in both, so every stream starts over by itself
    again = run_streams(det, steps)
    for f in range(len(steps)):
        for b in range(2):
            assert_same(f"again step {f} stream {b}", first[f][b], again[f][b])
    # two steps, then stream 1 is forgotten: its next step is a first frame although its token has not changed, and stream 0 continues undisturbed
    run_streams(det, steps[:2])
    det.reset_streams([1])
    assert det.prev_scene_tokens == ["a", None]
    mixed = synth.stack_detector_frames([streams[0][2], streams[1][1]])
    got = run_streams(det, [mixed])[0]
    assert_same("stream 0 beside a forgotten stream", got[0], first[2][0])
    alone = run_single(build_detector("fp32x3"), [streams[1][1]])[0]
    assert_same("forgotten stream 1 = a first frame", got[1], alone)
    assert not torch.equal(got[1]["img_feats"], first[1][1]["img_feats"]), "the same frame as a continuing one is another result"
