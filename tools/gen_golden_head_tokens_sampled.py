"""Generates tests/golden/head_tokens_sampled.npz from the REAL reference: the token side of ``StreamPETRHead.forward`` with ``topk_indexes``.

As oracle/gen_golden_head.py does for ``head_tokens.npz``: the reference's ``position_embeding`` (``dense_heads/streampetr_head.py:378-422``, unbound, on an
object holding the same sub-modules) -- here WITH an index list, so its own ``topk_gather`` (``models/utils/misc.py:13-23``) picks the per-token geometry --,
``topk_gather`` on the feature rows (:632), and the reference's ``MLN`` / ``SELayer_Linear`` modules composed as ``forward`` :627-639 composes them.

Sizes: ``synth.HEAD_TOKENS_TINY`` weights and inputs, B = 2, N = 2, 3 x 4 tokens a view: LEN = 24 tokens a sample, K = 7 of them.  The list is seeded, unsorted,
different per sample, and stored.  The reference also runs with ``None``; the full outputs are stored beside the sampled ones, and the generator asserts what was
found when this was first tried: at these sizes the reference's sampled rows equal its gathered full rows bit for bit.  Fixed zip timestamps: a second run
reproduces the archive byte for byte.  Runs only where the reference tree exists; nothing of it is copied."""
import os
import sys
import types

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gen_golden_head_outputs import save_npz     # noqa: E402
from oracle import ref_harness as R              # noqa: E402
from oracle import head_tokens_oracle as HO      # noqa: E402
from toc3d_amd import synth                      # noqa: E402

CFG, B, N, H, W, K, LIST_SEED = synth.HEAD_TOKENS_TINY, 2, 2, 3, 4, 7, 3
NAMES = ("pos_raw", "cone", "memory", "pos_embed")


def index_list():
    g = torch.Generator().manual_seed(LIST_SEED)
    return torch.stack([torch.randperm(N * H * W, generator=g)[:K] for _ in range(B)]).view(B, K, 1)


def main():
    ref = R.load_reference()
    head = R.load_reference_head()
    sd = synth.head_tokens_state_dict(CFG)
    inp = synth.head_tokens_inputs(CFG, B, N, H, W)
    pad_h, pad_w = H * CFG["stride"], W * CFG["stride"]
    E, C, LEN = CFG["embed_dims"], CFG["in_channels"], N * H * W
    obj = types.SimpleNamespace()
    obj.coords_d = HO.coords_d(CFG["position_range"], CFG["depth_num"], CFG["depth_start"], CFG["LID"])
    obj.position_range = torch.tensor(CFG["position_range"])
    obj.position_encoder = nn.Sequential(nn.Linear(CFG["depth_num"] * 3, 4 * E), nn.ReLU(), nn.Linear(4 * E, E))
    memory_embed = nn.Sequential(nn.Linear(C, E), nn.ReLU(), nn.Linear(E, E))
    mln = ref.misc.MLN(8, f_dim=E)
    se = ref.misc.SELayer_Linear(E)
    for mod, pre in ((obj.position_encoder, "position_encoder."), (memory_embed, "memory_embed."), (mln, "spatial_alignment."), (se, "featurized_pe.")):
        mod.load_state_dict({k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}, strict=True)
    sys.modules[head.__module__].inverse_sigmoid = HO.inverse_sigmoid            # mmdet's, stubbed as None in the harness
    topk = index_list()
    idx = topk.view(B, K)
    assert all(len(set(r.tolist())) == K and r.tolist() != sorted(r.tolist()) for r in idx) and idx[0].tolist() != idx[1].tolist(), "unsorted, different per sample"

    def run(tk):
        with torch.no_grad():
            centers = ref.misc.locations(inp["feats"].flatten(0, 1), CFG["stride"], pad_h, pad_w)[None].repeat(B * N, 1, 1, 1)
            data = dict(intrinsics=inp["intrinsics"], lidar2img=inp["lidar2img"])
            pos, cone = head.position_embeding(obj, data, centers, tk, [dict(pad_shape=[(pad_h, pad_w, 3)])])
            memory = inp["feats"].permute(0, 1, 3, 4, 2).reshape(B, LEN, C)
            memory = ref.misc.topk_gather(memory, tk)
            memory = mln(memory_embed(memory), cone)
            return pos, cone, memory, se(pos, memory)

    orig_to = torch.Tensor.to
    torch.Tensor.to = lambda self, *a, **k: self if (a and a[0] in ("cuda", "cpu")) else orig_to(self, *a, **k)   # :404 hops cpu -> cuda
    try:
        full, sampled = run(None), run(topk)
    finally:
        torch.Tensor.to = orig_to
    out = dict(topk_indexes=topk.numpy())
    for name, f, s in zip(NAMES, full, sampled):
        assert tuple(s.shape) == (B, K, f.shape[-1]) and tuple(f.shape[:2]) == (B, LEN)
        gathered = torch.gather(f, 1, idx[..., None].expand(-1, -1, f.shape[-1]))
        assert torch.equal(gathered, s), f"{name}: the reference's sampled rows are not its gathered full rows bit for bit"
        out[name], out["full_" + name] = s.numpy(), f.numpy()
    path = os.path.join(ROOT, "tests", "golden", "head_tokens_sampled.npz")
    save_npz(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", idx.tolist())
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
