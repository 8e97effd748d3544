"""Generates the fixtures of the 2-D auxiliary head from the REAL reference: tests/golden/focal_head_tiny.npz, focal_head_full.npz and
focal_head_state_dict_spec.json.

Starting from ``oracle.ref_harness.load_reference_head()`` (which installs the stand-in packages and the ``dense_heads`` path), the reference's own
``dense_heads/focal_head.py`` is imported where it lies, and ``FocalHead._init_layers`` (:119-134) and ``FocalHead.forward`` (:140-193) are called unbound on a
plain namespace in eval mode, on the seeded weights and inputs of ``toc3d_amd.synth`` (``focal_head_state_dict``, ``focal_head_inputs``).  The names the module
imports at top level and never calls at eval are stand-ins defined here (``bbox_cxcywh_to_xyxy``, ``bbox_overlaps``, ``clip_sigmoid``, ``build_loss``: empty).
The only ARITHMETIC stand-ins are the two mmdet functions ``models/utils/misc.py`` imports, set to mmdet's formulas: ``misc.bbox_xyxy_to_cxcywh``
(``[(x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1]``) and ``misc.inverse_sigmoid`` (clamp to [0, 1], eps 1e-5).  ``torch.topk`` is wrapped while the forward
runs: it records its input -- ``sample_weight``, which the reference computes and does not return -- and pins the tie order it leaves open to
stable-descending (ties to the lower index), as ``oracle.ref_harness.ReferenceMemory`` does for the memory bank.  Runs only where the reference tree exists;
nothing of it is copied.  Outputs only are stored: the tests regenerate weights and inputs from ``synth``.

The restatement (tests/focal_head_cases.py) is run here as well, in f64: for each sample, the band of half-width 2 x max |f32 reference - f64| of
``sample_weight`` around the K-th reference value must hold at most 0.5 % of the tokens, and the K-th and (K+1)-th f32 values must differ -- the premises of the
index tests.  If an assert fails, change the seed, not the assert.

The archives are written with fixed zip timestamps, so a second run reproduces them byte for byte.
"""
import importlib
import io
import json
import os
import sys
import types
import zipfile

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import focal_head_cases as FC                    # noqa: E402
from oracle import ref_harness as R              # noqa: E402
from toc3d_amd import synth                      # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
SEEDS = dict(tiny=0, full=0)                     # change a seed, not the asserts of main(), if one of them fails
BAND_MAX_SHARE = 0.005


def save_npz(path, **arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k, v in arrays.items():
            buf = io.BytesIO()
            v = np.asarray(v)
            np.lib.format.write_array(buf, v if v.flags.c_contiguous else v.copy(order="C"), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def bbox_xyxy_to_cxcywh(bbox):                   # mmdet/core/bbox/transforms.py
    x1, y1, x2, y2 = bbox.split((1, 1, 1, 1), dim=-1)
    return torch.cat([(x1 + x2) / 2, (y1 + y2) / 2, (x2 - x1), (y2 - y1)], dim=-1)


def inverse_sigmoid(x, eps=1e-5):                # mmdet/models/utils/transformer.py
    x = x.clamp(min=0, max=1)
    x1 = x.clamp(min=eps)
    x2 = (1 - x).clamp(min=eps)
    return torch.log(x1 / x2)


def load():
    R.load_reference_head()
    unused = lambda *a, **k: None
    core = sys.modules["mmdet.core"]
    core.bbox_cxcywh_to_xyxy, core.bbox_overlaps, core.bbox_xyxy_to_cxcywh = unused, unused, bbox_xyxy_to_cxcywh
    sys.modules["mmdet.models"].build_loss = unused
    R._mod("mmdet3d.models.utils", clip_sigmoid=unused)
    misc = R.load_reference().misc
    misc.bbox_xyxy_to_cxcywh, misc.inverse_sigmoid = bbox_xyxy_to_cxcywh, inverse_sigmoid
    return importlib.import_module("projects.mmdet3d_plugin.models.dense_heads.focal_head").FocalHead


def build(Head, sizes, sd):
    """The reference's _init_layers on a namespace -> (namespace, an nn.Module that holds its layers for the state dict)."""
    ns = types.SimpleNamespace(num_classes=sizes["num_classes"], in_channels=sizes["in_channels"], embed_dims=sizes["embed_dims"], stride=sizes["stride"],
                               use_hybrid_tokens=False, train_ratio=1.0, infer_ratio=sizes["infer_ratio"], training=False)
    Head._init_layers(ns)
    holder = nn.Module()
    for name in ("cls", "shared_reg", "shared_cls", "centerness", "ltrb", "center2d"):
        setattr(holder, name, getattr(ns, name))
    holder.load_state_dict(sd, strict=True)
    holder.eval()
    return ns, holder


def run(Head, ns, inp):
    orig, seen = torch.topk, []

    def stable_topk(input, k, dim=-1, largest=True, sorted=True):
        seen.append(input)
        v, i = torch.sort(input, dim=dim, descending=largest, stable=True)
        return v.narrow(dim, 0, k), i.narrow(dim, 0, k)
    torch.topk = stable_topk
    try:
        with torch.no_grad():
            out = Head.forward(ns, inp["location"], img_feats=inp["img_feats"])
    finally:
        torch.topk = orig
    assert len(seen) == 1
    return dict(out, sample_weight=seen[0])


def main():
    Head = load()
    spec = {}
    for tag, (sizes, shape) in FC.SIZES.items():
        seed = SEEDS[tag]
        sd = synth.focal_head_state_dict(sizes, seed=seed)
        ns, holder = build(Head, sizes, sd)
        spec[tag] = {k: list(v.shape) for k, v in holder.state_dict().items()}
        assert len(spec[tag]) == 16
        inp = synth.focal_head_inputs(sizes, shape, seed=seed)
        out = run(Head, ns, inp)
        B, n = out["sample_weight"].shape[:2]
        K = out["topk_indexes"].shape[1]
        assert K == int(n * sizes["infer_ratio"]) and 0 < K < n and out["topk_indexes"].dtype == torch.int64
        assert all(torch.isfinite(out[k]).all() for k in FC.ARITH)
        # the restatement: f32 against the reference (printed; tests/test_cpu_focal_head.py asserts it), f64 for the band
        r32 = FC.restated_forward(sd, inp, sizes["infer_ratio"])
        r64 = FC.restated_forward(sd, inp, sizes["infer_ratio"], dtype=torch.float64)
        print(f"{tag}: restatement f32 vs reference", {k: f"{v:.2e}" for k, v in FC.group_errors(r32, out).items()},
              "indices equal:", torch.equal(r32["topk_indexes"], out["topk_indexes"]))
        print(f"{tag}: reference f32 vs restatement f64", {k: f"{v:.2e}" for k, v in FC.group_errors(out, r64).items()})
        w32, w64 = out["sample_weight"].reshape(B, n), r64["sample_weight"].reshape(B, n)
        half = 2.0 * (w32.double() - w64).abs().max(1).values
        _, share = FC.index_band(w32, K, half)
        srt = torch.sort(w32, dim=1, descending=True).values
        print(f"{tag}: K = {K} of {n}, K-th weight {srt[:, K - 1].tolist()}, gap to the next {(srt[:, K - 1] - srt[:, K]).tolist()}, "
              f"band half-width {half.tolist()} holds {share.tolist()} of the tokens; weights span [{float(w32.min()):.4f}, {float(w32.max()):.4f}]")
        assert bool((share <= BAND_MAX_SHARE).all()), "the f32-error band around the K-th weight holds more than 0.5 % of the tokens: change the seed"
        assert bool((srt[:, K - 1] > srt[:, K]).all()), "the K-th and (K+1)-th reference weights are equal: change the seed"
        save_npz(os.path.join(GOLDEN, f"focal_head_{tag}.npz"), **{k: out[k].numpy() for k in FC.ARITH}, topk_indexes=out["topk_indexes"].numpy(),
                 band_half_width_f64=half.numpy(), infer_ratio=np.array(sizes["infer_ratio"]), seed=np.array(seed))
    json.dump(spec, open(os.path.join(GOLDEN, "focal_head_state_dict_spec.json"), "w"), indent=1)
    for f in ("focal_head_tiny.npz", "focal_head_full.npz", "focal_head_state_dict_spec.json"):
        size = os.path.getsize(os.path.join(GOLDEN, f))
        print(f, size, "bytes")
        assert size < 1 << 20


if __name__ == "__main__":
    main()
