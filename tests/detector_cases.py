"""What the tests of the assembled detector (toc3d_amd.Petr3D) and of its output stages share: the synthetic detector with seeded weights, autotune off and the
shipped tile table; the bit-identity check -- ``snapshot``, ``run``, ``assert_same_bits``: "a detector with a stage switched on keeps every bit of one without" --
and the stand-ins the CPU tests of the detector's hooks put in place of the backbone and the head.  A plain module beside the other ``*_cases.py``: importing it
needs no GPU, and it imports nothing from a ``test_*`` module.

As in support.py, two helpers are one here only where they return the same value for every argument: the stand-ins that take a ``log`` (test_cpu_detector.py,
test_cpu_streams.py, test_cpu_detector_sampling.py, test_cpu_token_vis.py, test_cpu_box_vis.py) record different things and stay where they are, and so does
every file's own FakeResults."""
import json
import os

import numpy as np
import torch
import torch.nn as nn

import nusc_results_cases as NC
import toc3d_amd
from head_queries_cases import BANK
from support import DEV, FakeNeck, to_dev
from toc3d_amd import lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD_OUTPUTS = ("all_cls_scores", "all_bbox_preds")
DECODED = ("boxes_3d", "scores_3d", "labels_3d")
_SD = {}


# ---- the detector ------------------------------------------------------------------------------------------------------------------------------------------------
def weights(sizes):
    """synth.detector_state_dict(sizes), made once per size set for the whole session (load_state_dict copies it; nobody changes it)."""
    key = json.dumps(sizes, sort_keys=True)
    if key not in _SD:
        _SD[key] = synth.detector_state_dict(sizes)
    return _SD[key]


def tuning(sizes, precision):
    return os.path.join(ROOT, "toc3d_amd", "tuned", f"{sizes['backbone']}_320x800_{precision}.json")


def schedule(backbone, neck, sizes, precision, launch_mode=None):
    """No autotune (every tile variant accumulates in the same order) and the shipped table where there is one; ``launch_mode=None`` leaves the parts' launch mode
    as built."""
    if launch_mode is not None:
        backbone.launch_mode = neck.launch_mode = launch_mode
    backbone.autotune = neck.autotune = False
    if os.path.exists(tuning(sizes, precision)):
        backbone.load_tuning(tuning(sizes, precision))
        neck._tuned.update(backbone._tuned)


def build_detector(sizes, precision, launch_mode=None, norm=None, cfg=None, builder=toc3d_amd.build_detector):
    """The detector at ``sizes`` with the seeded weights, on the device, scheduled.  ``cfg``: a config block of the caller's in place of synth.detector_cfg(sizes);
    ``norm``: the backbone's img_norm_cfg; ``launch_mode``: the head's and the parts' launch mode; ``builder``: toc3d_amd.build_vis_detector for the subclass."""
    cfg = synth.detector_cfg(sizes) if cfg is None else cfg
    if launch_mode is not None:
        cfg["pts_bbox_head"]["launch_mode"] = launch_mode
    if norm is not None:
        cfg["img_backbone"] = dict(cfg["img_backbone"], img_norm_cfg=norm)
    det = builder(cfg, precision=precision)
    det.load_state_dict(weights(sizes), strict=True)
    det = det.to(DEV)
    schedule(det.img_backbone, det.img_neck, sizes, precision, launch_mode)
    return det


# ---- the bit-identity check --------------------------------------------------------------------------------------------------------------------------------------
def snapshot(det, head_out, results, B, extra=None):
    """Per sample of the step the detector just ran: kept sets, token masks (both None on a dense backbone), img_feats, the two head outputs, the bank, the decoded
    lists, and sample b of every tensor in ``extra`` under its name."""
    last, N = det.last_frame, det.last_frame["img_feats"].shape[1]
    per = lambda ts, b: None if ts is None else [t[b * N:(b + 1) * N].clone() for t in ts]
    return [dict(keep=per(last["keep_idxes"], b), masks=per(last["token_masks"], b), img_feats=last["img_feats"][b].clone(),
                 out={k: head_out[k][:, b].clone() for k in HEAD_OUTPUTS}, bank={k: getattr(det.pts_bbox_head, k)[b].clone() for k in BANK}, dec=results[b]["pts_bbox"],
                 **{k: v[b].clone() for k, v in (extra or {}).items()}) for b in range(B)]


def run(det, frames, streams=False, on_frame=None):
    """simple_test (``streams``: simple_test_streams) over the frames -> [frame][sample] snapshots; the head's outputs come from a forward hook, and a
    ``topk_indexes`` the head was given goes in as ``topk``.  A frame carries its device tensors under "dev", or its host tensors under "data".
    ``on_frame(f, det, data, results)`` sees each frame right after its step."""
    seen, res = [], []
    hook = det.pts_bbox_head.register_forward_hook(lambda m, a, k, out: seen.append((a[2] if len(a) > 2 else k.get("topk_indexes"), out)), with_kwargs=True)
    try:
        for f, fr in enumerate(frames):
            data = fr["dev"] if "dev" in fr else to_dev(fr)
            step = det.simple_test_streams if streams else det.simple_test
            results = step(fr["img_metas"], gumbel_noise=fr["gumbel"], **data)
            topk, out = seen[-1]
            res.append(snapshot(det, out, results, len(fr["img_metas"]), None if topk is None else dict(topk=topk)))
            if on_frame is not None:
                on_frame(f, det, data, results)
    finally:
        hook.remove()
    return res


def _equal_lists(p, q):
    if p is None or q is None:
        return p is None and q is None
    return len(p) == len(q) and all(torch.equal(x, y) for x, y in zip(p, q))


def assert_same_bits(a, b):
    """Two runs' snapshots, every key both carry, bit for bit."""
    assert len(a) == len(b)
    for f, (xs, ys) in enumerate(zip(a, b)):
        assert len(xs) == len(ys)
        for x, y in zip(xs, ys):
            assert _equal_lists(x["keep"], y["keep"]) and _equal_lists(x["masks"], y["masks"]), f"frame {f}: kept sets"
            assert torch.equal(x["img_feats"], y["img_feats"]), f"frame {f}: img_feats"
            assert all(torch.equal(x["out"][k], y["out"][k]) for k in x["out"]) and all(torch.equal(x["bank"][k], y["bank"][k]) for k in BANK), f"frame {f}: head outputs, bank"
            assert all(torch.equal(torch.as_tensor(x["dec"][k]), torch.as_tensor(y["dec"][k])) for k in DECODED), f"frame {f}: decoded lists"
            for k in sorted((set(x) & set(y)) - {"keep", "masks", "img_feats", "out", "bank", "dec"}):
                assert torch.equal(x[k], y[k]), f"frame {f}: {k}"


def with_pose(meta, token, seed):
    """A frame's meta with the four keys of a nuScenes info record (any rotations; the vehicle a few hundred metres from the map's origin) and its sample token."""
    p = NC.random_poses(np.random.default_rng(seed), 1)
    return dict(meta, sample_idx=token, **NC.pose_records(p)[0])


# ---- stand-ins for the detector's parts (CPU) ------------------------------------------------------------------------------------------------------------------------
class FakeBackbone(nn.Module):
    pruning_loc, pruning_num_queries, patch_size, img_norm_cfg = [3, 6, 9], 64, 16, None

    def forward(self, x, **kw):
        return toc3d_amd.ToC3DViTReturnType({"last_feat": torch.zeros(x.shape[0], 8, 2, 5)}, ["m0", "m1", "m2"], None, ["k0", "k1", "k2"], ["d0", "d1", "d2"])


class FakeHead(nn.Module):
    embed_dims = 256

    def backbone_queries(self, n, prev_exists, batch_size=1):
        return dict(temp_queries=torch.zeros(batch_size, n, 256), temp_ref_points=None, temp_timestamp=None, temp_ego_pose=None, temp_vel=None, prev_exists=False)

    def img_feats_rows_buffer(self, B, N, h, w, device=None):
        return "rows", 64, lib.F32X3P

    def reset_memory(self):
        pass

    def forward(self, memory_center, img_metas, topk_indexes=None, img_feats_rows=False, **data):
        return dict(all_cls_scores="cls", all_bbox_preds="box", dn_mask_dict=None)

    def get_bboxes(self, outs, img_metas, rescale=False):
        return [[torch.full((3, 9), float(i)), torch.arange(3.0) + i, torch.arange(3) + i] for i, _ in enumerate(img_metas)]


def fake_detector():
    det = toc3d_amd.build_detector(synth.detector_cfg(synth.DETECTOR_TINY))
    det.img_backbone, det.img_neck, det.pts_bbox_head = FakeBackbone(), FakeNeck([]), FakeHead()
    return det


def posed_meta(token, scene="a"):
    return dict(scene_token=scene, pad_shape=[(32, 80, 3)], sample_idx=token, lidar2ego_rotation=[1.0, 0, 0, 0], lidar2ego_translation=[0.0, 0, 0],
                ego2global_rotation=[1.0, 0, 0, 0], ego2global_translation=[0.0, 0, 0])


def frame(det, metas, t=None):
    """One step of the stand-in detector on blank tensors: simple_test for one sample, simple_test_streams for more.  Timestamps t + 7 b, or zeros."""
    B = len(metas)
    timestamp = torch.zeros(B, dtype=torch.float64) if t is None else torch.tensor([t + 7.0 * b for b in range(B)], dtype=torch.float64)
    data = dict(img=torch.zeros(B, 6, 3, 32, 80), intrinsics=torch.zeros(B, 6, 4, 4), lidar2img=torch.zeros(B, 6, 4, 4), timestamp=timestamp,
                ego_pose=torch.eye(4)[None].repeat(B, 1, 1), ego_pose_inv=torch.eye(4)[None].repeat(B, 1, 1))
    return det.simple_test(metas, **data) if B == 1 else det.simple_test_streams(metas, **data)
