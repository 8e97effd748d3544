"""Generates the fixture of the assembled detector from the REAL reference: tests/golden/detector_tiny.npz.

The reference's own ``Petr3D.extract_img_feat``, ``prepare_location``, ``forward_roi_head``, ``simple_test_pts`` and ``simple_test``
(``detectors/petr3d.py:84-243, 311-323, 521-594``) run, unbound, on a holder object whose ``img_backbone`` and ``img_neck`` are the reference's modules as
``oracle.ref_harness`` builds them and whose ``pts_bbox_head`` is the holder of tools/gen_golden_head_e2e.py -- the reference's ``StreamPETRHead.forward`` on the
reference's layers, decoder and box coder.  The LIMITATION stated there carries over word for word: mmcv is not installed, so mmcv's ``FFN`` and
``MultiheadAttention`` are stood in by the stand-ins of tools/gen_golden_decoder.py; every other line that computes is the reference's.  ``Petr3D.__init__`` cannot
run under the stubs (``MVXTwoStageDetector`` builds through mmdet3d), so the holder carries the attributes it would set.  Stubs that only this file needs
(``DETECTORS``, ``bbox3d2result``, ``MVXTwoStageDetector``, the timer, the visualiser) live here; nothing under oracle/ changes.

Four frames of one sample at the sizes of ``toc3d_amd.synth.DETECTOR_TINY`` (the tiny backbone at 6 x 320 x 800, the tiny neck, a two-layer head whose
``topk_proposals`` equals the backbone's ``pruning_num_queries``): a scene start, two continuations -- the backbone reads the head's own proposals --, then a new
scene token.  ``oracle.ref_harness.deterministic_reference`` runs with zero Gumbel noise, ``torch.sort`` / ``topk`` are stable.  Two runs: f32, and f64 as the
arbiter (``Tensor.float`` is the identity while it is on).

The near-tie condition is a condition of the fixture: at EVERY cut of the f64 run -- every call of the selectors' ``sample`` (the three image-level selections and
every per-window selection of the accelerated blocks), the proposals' top-k and the coder's ``max_num`` -- the gap between the last kept and the first dropped
score must be at least 100 x the largest |f32 - f64| over the scores of that cut (pad scores of -1e6 and cuts that keep everything have an infinite gap).  The
first seed, counting from 0, that meets it over all four frames is taken and stored with the gaps; at most MAX_SEEDS are searched.  If none meets it, frame 0 alone
is written under the same condition (``detector_tiny_frame0.npz``), as ``head_full_frame0.npz`` was; a fixture that misses its condition is not written.

Per frame the archive holds: the kept token indices of the three stages (sorted per view), the last-level scores and boxes, the proposal set, the bank
(``memory_embedding``: every BANK_STEP-th row, the other four whole), the decoded lists with their query order, every ROW_STEP-th token row of neck level 0 --
f32; the f64 run's outputs, bank and neck rows under ``f64_`` --, then the seed and the margins.  Fixed zip timestamps: a second run reproduces it byte for byte.
Runs only where the reference tree exists; nothing of it is copied.

Outcome with the seeded weights of ``toc3d_amd.synth`` (seeds 0 .. 63, 7 s a seed): NO seed meets the condition, neither over four frames nor on frame 0 alone, so
neither archive is written and tests/test_gpu_detector.py has no test against a reference fixture.  A frame has 14 cuts (three image-level selections of 500 / 400 /
300 of 1000 tokens in each of six views, nine calls of per-window selections, the 64 proposals of 96, the 30 decoded of 960): with random weights the token scores
around a cut lie ~1e-5 .. 1e-4 apart while f32 differs from f64 by ~1e-6 .. 1e-5 on them, and behind the first cut that falls the other way the scores of the two
runs part altogether.  The best seed reaches a smallest gap of 0.23 x the error on frame 0 (100 x required) and 2.6e-5 x over four frames, and on all 64 seeds
the reference's own f32 and f64 runs keep different token sets -- on this input the reference does not agree with itself.  What holds the detector instead: it equals the chain of
the separately built backbone, neck and head bit for bit (tests/test_gpu_detector.py, tiny and shipped sizes), and each of those is held to the reference by its own
fixtures (tiny_toc3d_*.npz, tiny_neck.npz, head_tiny.npz, head_full_frame0.npz).
"""
import importlib
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_decoder as GD                  # noqa: E402
import gen_golden_head_e2e as GE                 # noqa: E402
import gen_golden_head_outputs as GO             # noqa: E402
from oracle import ref_harness as R              # noqa: E402
from toc3d_amd import configs, synth             # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
BANK = GE.BANK
MARGIN, MAX_SEEDS, ROW_STEP, BANK_STEP = 100.0, 64, 8, 4
SIZES = synth.DETECTOR_TINY


def load_petr3d():
    """The reference's Petr3D class, imported where it lies, on the stubs of the harness plus the ones only the detector file needs."""
    R.load_reference()
    head, Coder = GO.load()
    _, TR = GD.load_petr_transformer()
    sys.modules["mmdet.models"].DETECTORS = R._Registry()
    sys.modules["mmdet3d.core"].bbox3d2result = lambda bboxes, scores, labels: dict(boxes_3d=bboxes, scores_3d=scores, labels_3d=labels)   # what mmdet3d's builds, less .cpu()

    class MVXTwoStageDetector(nn.Module):
        pass

    class Timer:                                                       # utils/gpu_timer.py GLOBAL_TIMER: measures, computes nothing
        def __getattr__(self, name):
            return lambda *a, **k: None

    R._mod("mmdet3d.models.detectors")
    R._mod("mmdet3d.models.detectors.mvx_two_stage", MVXTwoStageDetector=MVXTwoStageDetector)
    R._mod("projects.mmdet3d_plugin.models.utils.gpu_timer", GLOBAL_TIMER=Timer())
    R._mod("projects.mmdet3d_plugin.models.utils.token_select_vis", token_selection_vis=None)
    R._mod("projects.mmdet3d_plugin.models.utils.grid_mask", GridMask=None)          # built by __init__ only, which does not run
    R._mod("projects.mmdet3d_plugin.models.detectors").__path__ = [f"{R.REF}/projects/mmdet3d_plugin/models/detectors"]
    mod = importlib.import_module("projects.mmdet3d_plugin.models.detectors.petr3d")
    return mod.Petr3D, head, Coder, TR


class HeadProxy:
    """``self.pts_bbox_head`` of the holder: calls go to the reference's unbound ``forward`` / ``reset_memory`` on the head holder, attributes come from it."""

    def __init__(self, head, m):
        self.__dict__.update(_head=head, _m=m, outs=None)

    def __call__(self, *a, **k):
        self.__dict__["outs"] = self._head.forward(self._m, *a, **k)
        return self.outs

    def reset_memory(self):
        self._head.reset_memory(self._m)

    def __getattr__(self, name):
        return getattr(self._m, name)


class Detector:
    """What ``self`` is while the reference's methods run: the attributes ``Petr3D.__init__`` (:56-82) and ``MVXTwoStageDetector`` would have set."""
    training = use_grid_mask = token_select_vis = test_time_print = with_img_roi_head = False
    query_backbone_selection = with_img_neck = aux_2d_only = True
    position_level, stride, vis_num_sample, cur_id, vis_start_id = 0, 16, 0, 0, 0

    def __init__(self, P, backbone, neck, head):
        self.img_backbone, self.img_neck, self.pts_bbox_head, self.prev_scene_token = backbone, neck, head, None
        for name in ("extract_img_feat", "prepare_location", "forward_roi_head", "simple_test_pts", "simple_test"):
            setattr(self, name, types.MethodType(getattr(P, name), self))


def build(ref, seed):
    P, head, Coder, TR = ref
    bcfg = configs.get(SIZES["backbone"])
    backbone = R.build_reference_toc3d(bcfg)
    backbone.load_state_dict(synth.make_state_dict(bcfg, seed=seed), strict=True)
    neck = R.build_reference_cpfpn(configs.CPFPN_TINY)
    neck.load_state_dict(synth.neck_state_dict(configs.CPFPN_TINY, seed=seed), strict=True)
    m, holder = GE.build(head, Coder, TR, SIZES["head"], seed)
    return P, head, backbone, neck, m, holder


def run_stream(parts, seed, dtype, frames=None):
    """The reference's simple_test over the frames of synth.detector_inputs -> (per frame a dict of tensors, per frame the cuts [(scores, k), ...])."""
    P, head, backbone, neck, m, holder = parts
    ref = R.load_reference()
    backbone.to(dtype), neck.to(dtype), holder.to(dtype)
    head.reset_memory(m)
    proxy = HeadProxy(head, m)
    det = Detector(P, backbone, neck, proxy)
    sizes = SIZES["head"]
    K, max_num, NC = sizes["topk_proposals"], sizes["max_num"], 10
    cast = lambda t: t.to(dtype) if t.dtype == torch.float32 else t               # (the timestamps are f64 in both runs)
    Sel = ref.toc3d_utils.ScoreBasedTokenSelector
    cuts = []

    def sample(self, pred_score, override_ratio=None):
        out = orig_sample(self, pred_score, override_ratio)
        score = pred_score.flatten(1, 2) if pred_score.dim() == 4 else pred_score
        cuts.append((score[:, :, 0].detach().clone(), out[2].shape[1]))
        return out

    orig_sample = Sel.sample
    orig = (torch.topk, torch.Tensor.topk, torch.Tensor.to, torch.Tensor.float)
    torch.topk = torch.Tensor.topk = GE.stable_topk
    torch.Tensor.to = lambda self, *a, **k: self if (a and a[0] in ("cuda", "cpu")) else orig[2](self, *a, **k)      # position_embeding hops cpu -> cuda (:407)
    if dtype == torch.float64:
        torch.Tensor.float = lambda t, *a, **k: t
    torch.set_default_dtype(dtype)                  # extract_img_feat's zero queries of a scene start (:126-130) are torch.zeros of the default dtype
    Sel.sample = sample
    res, all_cuts, last = [], [], {}
    hk = neck.register_forward_hook(lambda mod, args, out: last.__setitem__("rows", out[0].permute(0, 2, 3, 1).reshape(-1, out[0].shape[1])[::ROW_STEP].clone()))
    try:
        with torch.no_grad(), R.deterministic_reference(None):
            for fr in synth.detector_inputs(SIZES, seed)[:frames]:
                del cuts[:]
                metas = [dict(meta, box_type_3d=lambda t, d: t) for meta in fr["img_metas"]]
                data = {k: cast(v.clone()) for k, v in fr["data"].items()}
                (result,) = det.simple_test(metas, **data)
                outs = proxy.outs
                cls, box = outs["all_cls_scores"], outs["all_bbox_preds"]
                assert outs["dn_mask_dict"] is None and cls.dtype == dtype
                f = dict(cls_last=cls[-1].clone(), box_last=box[-1].clone(), **{k: getattr(m, k).clone() for k in BANK})
                score = cls[-1].sigmoid().max(-1).values                                  # rec_score of post_update_memory (:359)
                flat = cls[-1].sigmoid().flatten(1)
                f["proposal_set"] = GE.stable_topk(score, K, dim=1)[1].sort(1).values
                dec = result["pts_bbox"]
                top_v, top_i = GE.stable_topk(flat[0], min(max_num, flat.shape[1]))
                assert bool((top_v[:-1] > top_v[1:]).all()), "ties among the decoded scores: another seed"
                pos = torch.searchsorted(-top_v, -dec["scores_3d"])                        # the survivors are a subsequence of the top max_num
                assert pos.numel() == 0 or (int(pos.max()) < top_v.numel() and torch.equal(top_v[pos], dec["scores_3d"]) and torch.equal(top_i[pos] % NC, dec["labels_3d"])), \
                    "the decoded list is not a subsequence of the stable top max_num: another seed"
                f["bboxes"], f["scores"], f["labels"] = dec["boxes_3d"], dec["scores_3d"], dec["labels_3d"]
                f["query"] = torch.div(top_i[pos], NC, rounding_mode="floor")
                # what extract_img_feat left: the backbone's kept lists went through the holder's backbone; read them off the cuts (the three image-level ones have T columns)
                T = (SIZES["hw"][0] // 16) * (SIZES["hw"][1] // 16)
                img_cuts = [c for c in cuts if c[0].shape[1] == T]
                assert len(img_cuts) == 3
                for s, (sc, k) in enumerate(img_cuts):
                    f[f"keep{s}"] = torch.sort(sc, dim=1, descending=True, stable=True)[1][:, :k].sort(1).values
                f["neck_rows"] = last["rows"]                                                # every ROW_STEP-th token row of neck level 0, as rows [V*h*w, C]
                res.append(f)
                all_cuts.append(list(cuts) + [(score.clone(), K), (flat.clone(), max_num)])
    finally:
        torch.topk, torch.Tensor.topk, torch.Tensor.to, torch.Tensor.float = orig
        Sel.sample = orig_sample
        torch.set_default_dtype(torch.float32)
        hk.remove()
    return res, all_cuts


def margins(c32, c64):
    """Per frame the smallest gap / error ratio over all cuts, and its (gap, error); a cut that keeps everything, or cuts among pads, has an infinite gap."""
    rows = []
    for f32, f64 in zip(c32, c64):
        assert len(f32) == len(f64)
        worst = (float("inf"), float("inf"), 0.0)
        for (a, ka), (b, kb) in zip(f32, f64):
            assert ka == kb and a.shape == b.shape
            if kb == 0 or kb >= b.shape[1]:
                continue
            s = torch.sort(b, dim=1, descending=True).values
            gap = s[:, kb - 1] - s[:, kb]
            gap = torch.where(s[:, kb] > -1e5, gap, torch.full_like(gap, float("inf")))     # the first dropped score is a pad (toc3d_eva_vit.py:415): no real cut
            real = b > -1e5
            err = ((a.double() - b).abs() * real).amax(1).clamp_min(1e-300)
            ratio = gap / err
            i = int(ratio.argmin())
            if float(ratio[i]) < worst[0]:
                worst = (float(ratio[i]), float(gap[i]), float(err[i]))
        rows.append(worst)
    return np.asarray(rows, dtype=np.float64)                  # [frame, (ratio, gap, error)]


def attempt(ref, seed, frames=None):
    parts = build(ref, seed)
    f32, c32 = run_stream(parts, seed, torch.float32, frames)
    f64, c64 = run_stream(parts, seed, torch.float64, frames)
    mg = margins(c32, c64)
    same = all(all(torch.equal(a[k], b[k]) for k in ("keep0", "keep1", "keep2", "proposal_set", "labels", "query")) for a, b in zip(f32, f64))
    return f32, f64, mg, same, sum(len(c) for c in c64)


def pack(f32, f64):
    out = {}
    for f, (a, b) in enumerate(zip(f32, f64)):
        for k, v in a.items():
            if k.startswith("keep"):
                v = v.to(torch.int16)
            elif k == "memory_embedding":
                v = v[:, ::BANK_STEP]
            out[f"f{f}_{k}"] = v.numpy()
        for k in ("cls_last", "box_last", "neck_rows") + BANK:
            v = b[k][:, ::BANK_STEP] if k == "memory_embedding" else b[k]
            out[f"f64_f{f}_{k}"] = v.numpy().astype(np.float32) if k not in ("memory_timestamp",) else v.numpy()
    return out


def write(name, seed, f32, f64, mg):
    for k in ("cls_last", "box_last", "neck_rows", "memory_embedding"):
        print(f"    {k}: f32 vs f64 max-abs / max-abs "
              f"{max(float((a[k].double() - b[k]).abs().max() / b[k].abs().max().clamp_min(1e-30)) for a, b in zip(f32, f64)):.2e}")
    path = os.path.join(GOLDEN, name)
    GO.save_npz(path, seed=np.array(seed), margins=mg, margin_required=np.array(MARGIN), row_step=np.array(ROW_STEP), bank_step=np.array(BANK_STEP),
                frames=np.array(len(f32)), **pack(f32, f64))
    size = os.path.getsize(path)
    print(name, size, "bytes")
    assert size < 1 << 20


def main():
    ref = load_petr3d()
    frame0_seed = None
    for seed in range(MAX_SEEDS):
        try:
            f32, f64, mg, same, ncuts = attempt(ref, seed)
        except AssertionError as e:
            print(f"  seed {seed}: {e}")
            continue
        print(f"  seed {seed}: smallest gap / error per frame {[f'{v:.2g}' for v in mg[:, 0]]} over {ncuts} cuts (need {MARGIN:.0f}); f32 and f64 keep the same sets: {same}",
              flush=True)
        if bool((mg[:, 0] >= MARGIN).all()):
            assert same, "the margin holds and the sets differ: the condition does not mean what it should"
            write("detector_tiny.npz", seed, f32, f64, mg)
            return
        if frame0_seed is None and mg[0, 0] >= MARGIN:
            frame0_seed = seed                      # (frame 0 of the stream is the stream of one frame)
    names = ("detector_tiny.npz", "detector_tiny_frame0.npz")
    print(f"  no seed below {MAX_SEEDS} meets the near-tie condition over four frames: {names[0]} is NOT written")
    if frame0_seed is not None:
        f32, f64, mg, same, _ = attempt(ref, frame0_seed, 1)
        assert same and bool((mg[:, 0] >= MARGIN).all())
        write(names[1], frame0_seed, f32, f64, mg)
        names = names[:1]
    else:
        print(f"  ... nor on frame 0 alone: {names[1]} is NOT written")
    stale = [n for n in names if os.path.exists(os.path.join(GOLDEN, n))]
    assert not stale, f"{stale} exist without a generator that stands behind them: remove them"


if __name__ == "__main__":
    main()
