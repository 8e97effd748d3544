"""What the tests of the sampled token side share (test_cpu_head_sampled.py, test_gpu_head_sampled_kernels.py, test_gpu_head_tokens_sampled.py,
test_gpu_head_sampled.py): the sizes of tests/golden/head_tokens_sampled.npz restated, the index-list families of the kernel tests, and the module's build / run
helpers.  Importing it needs no GPU."""
import os

import torch

import toc3d_amd
from toc3d_amd import synth

from support import DEV

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# tools/gen_golden_head_tokens_sampled.py: synth.HEAD_TOKENS_TINY, B = 2, N = 2, 3 x 4 tokens a view -> LEN = 24 a sample, K = 7 of them
CFG, B, N, H, W, K = synth.HEAD_TOKENS_TINY, 2, 2, 3, 4, 7
TOKENS = {1: (1, 1, 1, 1), 5: (1, 1, 1, 5), 24: (2, 2, 2, 3)}          # tokens -> (B, N, h, w), the shapes of tests/test_gpu_head_tokens_x3.py


def index_families(B, LEN, seed=0):
    """{name: int64 (B, K)}: K = 1; K = LEN as a permutation (another one per sample); and -- where LEN allows a strict subset -- K = (LEN + 2) // 2 listed
    tokens in random order, of which the last repeats the first (the planted duplicate).  An index list has ONE K for all samples, so the 24-token shape
    (B = 2, LEN = 12) takes 7 rows from each of its two samples; 5 tokens take 3."""
    g = torch.Generator().manual_seed(100 + seed)
    perm = torch.stack([torch.randperm(LEN, generator=g) for _ in range(B)])
    fam = {"one": torch.stack([torch.randint(0, LEN, (1,), generator=g) for _ in range(B)]), "permutation": perm}
    if LEN > 2:
        sub = torch.stack([torch.randperm(LEN, generator=g)[:(LEN + 2) // 2] for _ in range(B)])
        sub[-1, -1] = sub[-1, 0]
        fam["subset"] = sub
    return fam


def gather_rows(t, index):
    """torch's form of topk_gather: t (B, LEN, C), index (B, K) -> (B, K, C)."""
    return torch.gather(t, 1, index[..., None].expand(-1, -1, t.shape[-1]))


def build_tokens(precision, cfg=CFG, seed=0):
    m = toc3d_amd.HeadTokenEmbedding(precision=precision, **cfg)
    m.load_state_dict(synth.head_tokens_state_dict(cfg, seed=seed), strict=True)
    return m.to(DEV).eval()


def run_tokens(m, inp, h, w, stride, topk=None):
    return m(inp["feats"].to(DEV), inp["intrinsics"].to(DEV), inp["lidar2img"].to(DEV), (h * stride, w * stride, 3), topk_indexes=None if topk is None else topk.to(DEV))
