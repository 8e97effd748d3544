"""CPU: bench.py --dump-outputs writes the step's outputs as float32 / float64 .npy files, within its byte budget, the same on every call."""
import os

import numpy as np
import torch

import bench
from toc3d_amd.backbone import ToC3DViTReturnType


def _outputs():
    g = torch.Generator().manual_seed(0)
    order = torch.stack([torch.randperm(200, generator=g) for _ in range(6)])
    feat = torch.randperm(6 * 64 * 10 * 20, generator=g).float().view(6, 64, 10, 20).permute(0, 1, 3, 2)   # distinct values; a strided view like last_feat
    masks = [torch.rand(6, 10, 20, 1, generator=g) for _ in range(3)]
    bb = ToC3DViTReturnType({"last_feat": feat}, masks, None, keep_idx=[order[:, :100]] * 3, drop_idx=[order[:, 100:]] * 3)
    return {"backbone": bb, "neck": torch.randn(6, 16, 10, 20, generator=g).to(torch.bfloat16)}


def test_dump_outputs_dtypes_budget_and_repeatability(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 200_000)
    outs = _outputs()
    bench.dump_outputs(str(tmp_path / "a"), outs)
    bench.dump_outputs(str(tmp_path / "b"), outs)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(["neck_features.npy", "last_feat.npy"] + [f"{k}_stage{s}.npy" for k in ("token_masks", "keep_idx", "drop_idx") for s in range(3)])
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), n
        total += a.nbytes
    assert total <= 200_000
    # what fits is written whole and exact: bf16 -> float32, int64 indices -> float64
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "neck_features.npy"), outs["neck"].float().numpy())
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "keep_idx_stage0.npy"), outs["backbone"].keep_idx[0].double().numpy())
    # the 307 KB feature map does not fit its share: a sample of its own elements, in flattened order
    full = outs["backbone"].img_feats["last_feat"].numpy().reshape(-1)
    s = np.load(tmp_path / "a" / "last_feat.npy")
    assert s.ndim == 1 and 0 < s.size < full.size
    pos = {v: i for i, v in enumerate(full.tolist())}
    idx = [pos[v] for v in s.tolist()]
    assert idx == sorted(idx)
