"""Cases and references shared by tests/test_gpu_token_kernels.py (the kernels on the GPU) and tests/test_cpu_token_abi.py (the references' own invariants,
without a GPU).

`layout_reference` is the compact layout of toc3d_window_topk written from the rule in the kernel's header comment (toc3d_amd/csrc/tokens.hip,
window_topk_kernel), as lists: for window i with real_i real tokens, r_w real tokens among its k best slots, cap = min(k, real_i) + 1 and
e_w = cap - 1 - r_w, the window's key list is

    kept real tokens (rank order) | the first e_w kept pads (rank order; explicit zero rows, crow_tok = -1) | representative (crow_tok = -2, slot k)
    | the remaining kept pads (virtual keys: arows = -1, aslots = their slot)

and the first cap entries own the compact rows [off_i, off_i + cap).  e_w > 0 needs a real token that loses against a pad, i.e. a score <= -1e6 in a window
that HAS pads: a full window has no pad to lose against, so there e_w = 0 whatever the scores are.
"""
import torch

from oracle import toc3d_oracle as O

GRIDS = {3: (2, 4, 7), 7: (2, 8, 15), 8: (1, 9, 17), 4: (1, 7, 9), 32: (1, 33, 40)}     # (V, h, w) per window side: edge windows with one real row / column / token
KS = {3: (0, 1, 4, 8), 7: (0, 1, 6, 20, 48), 8: (0, 1, 47, 48, 49, 63)}                 # 0, 1, N - 1, k above a ragged window's real count, N - k in {15, 16, 17}


def topk_rows(V, h, w, L, k):
    return V * sum(min(k, min(L, h - r) * min(L, w - c)) + 1 for r in range(0, h, L) for c in range(0, w, L))


def window_tokens(V, h, w, L):
    """[nW, N] int64: token row of every window slot, -1 for a padded slot."""
    idx = torch.arange(V * h * w, dtype=torch.float64).reshape(V, h, w, 1)
    return O.window_partition(idx, L, pad_value=-1)[0].reshape(-1, L * L).long()


def window_scores(scores, L):
    """f32 [V, h, w] -> [nW, N] with the pad score."""
    return O.window_partition(scores[..., None], L, pad_value=O.PAD_SCORE)[0].reshape(-1, L * L)


def make_scores(V, h, w, L, seed=0, planted=True):
    """Log-probability-like scores, all < 0.  planted: ties among real tokens, and -- on about a fifth of the tokens of ragged windows and a few of full
    ones -- scores of -2e6 (a real token that loses against every pad) and of exactly -1e6 (a real token that ties with the pads: the slot decides)."""
    g = torch.Generator().manual_seed(seed)
    s = -torch.rand(V, h, w, generator=g) * 4 - 0.01
    if not planted:
        return s
    s[0, :2, : min(w, 5)] = s[0, 0, 0]
    s[-1, -1, :] = torch.minimum(s[-1, -1, :], s[-1, -1, :1])        # (ties in a ragged window too)
    u = torch.rand(V, h, w, generator=g)
    ragged = torch.zeros(V, h, w, dtype=torch.bool)
    if h % L:
        ragged[:, h - h % L:, :] = True
    if w % L:
        ragged[:, :, w - w % L:] = True
    s[ragged & (u < 0.22)] = -2e6
    s[ragged & (u > 0.88)] = -1e6
    s[~ragged & (u < 0.04)] = -2e6
    s[~ragged & (u > 0.97)] = -1e6
    if h % L and w % L:
        s[0, h - 1, w - 1] = -2e6                                     # the corner window's last (for a remainder of 1: only) real token loses against its pads
    return s


def layout_reference(scores, V, h, w, L, k):
    """The outputs of toc3d_window_topk as int64 tensors (wgt: f64, from the f32 scores), plus cap / e_w / r_w / real per window."""
    N = L * L
    tokw, sw = window_tokens(V, h, w, L), window_scores(scores.float(), L)
    nW = tokw.shape[0]
    s_sorted, order = O.sort_desc_stable(sw)
    tok = torch.gather(tokw, 1, order)
    fast = s_sorted[:, k:].double()
    wgt = torch.zeros(nW, N, dtype=torch.float64)
    wgt[:, k:] = fast / fast.sum(dim=1, keepdim=True)
    ms = topk_rows(V, h, w, L, k)
    out = dict(order=order, tok=tok, wgt=wgt, prow=torch.full((nW, N), -1), crow_tok=torch.full((ms,), -9), rep_index=torch.full((ms,), -9),
               crow_rc=torch.full((ms,), -9), rep_row=torch.zeros(nW, dtype=torch.long), arows=torch.full((nW, k + 1), -9),
               aslots=torch.full((nW, k + 1), -9), acount_q=torch.zeros(nW, dtype=torch.long), acount_k=torch.full((nW,), k + 1),
               cap=[], e_w=[], r_w=[], real=[], ms=ms)
    rc = lambda slot: ((slot // L) << 16) | (slot % L)
    off = 0
    for i in range(nW):
        real = int((tokw[i] >= 0).sum())
        kept_real = [p for p in range(k) if tok[i, p] >= 0]
        kept_pads = [p for p in range(k) if tok[i, p] < 0]
        r_w, cap = len(kept_real), min(k, real) + 1
        e_w = cap - 1 - r_w
        explicit = kept_real + kept_pads[:e_w]                           # positions that own a compact row, in key order
        for j, p in enumerate(explicit):
            slot = int(order[i, p])
            out["prow"][i, p] = off + j
            out["crow_tok"][off + j] = int(tok[i, p]) if tok[i, p] >= 0 else -1
            out["rep_index"][off + j] = -1
            out["crow_rc"][off + j] = rc(slot)
            out["arows"][i, j], out["aslots"][i, j] = off + j, slot
        rr = off + cap - 1
        out["crow_tok"][rr], out["rep_index"][rr], out["crow_rc"][rr], out["rep_row"][i] = -2, i, rc(k), rr
        out["arows"][i, cap - 1], out["aslots"][i, cap - 1] = rr, k
        for j, p in enumerate(kept_pads[e_w:]):
            out["arows"][i, cap + j], out["aslots"][i, cap + j] = -1, int(order[i, p])
        out["acount_q"][i] = cap
        for key, val in (("cap", cap), ("e_w", e_w), ("r_w", r_w), ("real", real)):
            out[key].append(val)
        off += cap
    assert off == ms
    return out


# ---------------------------------------------------------------------------------------------------
# Row-block -> XCD remap sweeps (csrc/common.h xcd_remap / xcd_remap_off).  The kept-row blocks of the gather are permuted by xcd_remap_off(block, offset,
# count): what can go wrong depends on (offset mod 8, count mod 8) and on count < 8 (the early-out).  toc3d_gather_merge_ln_ex: offset = nW, count =
# ceil(rows / 16); toc3d_gather_merge_ln_split with s workgroups per window: offset = 8 s ceil(nW / 8) (always 0 mod 8), count = ceil(rows / (16 / s)).
# ---------------------------------------------------------------------------------------------------
SPLITS = (0, 2, 8, 16)
WAVES_PER_BLOCK = {None: 16, 0: 4, 2: 8, 8: 2, 16: 1}                 # None = toc3d_gather_merge_ln_ex


def remap_sweep_cases(L=4):
    """[(V, h, w, k)]: for _ex every pair (nW mod 8, blocks mod 8) with blocks >= 8, every blocks < 8 that this L reaches, nW < 8 and nW >= 8; for each
    split every blocks mod 8, below and above 8 where reachable.  Greedy over a small candidate grid, in a fixed order."""
    need, cases = {}, []
    cands = [(V, h, w, k) for V in (1, 2, 3) for h in (3, 4, 7, 9) for w in range(1, 37) for k in (1, 3, 5, 8, 11, 15)]

    def keys(c):
        V, h, w, k = c
        nW, rows = V * -(-h // L) * -(-w // L), topk_rows(V, h, w, L, k)
        ks = []
        for form, wpb in WAVES_PER_BLOCK.items():
            blocks = -(-rows // wpb)
            ks.append((form, nW % 8 if form is None else 0, blocks % 8, blocks < 8))
        ks.append(("nW<8", nW < 8))
        return ks

    for c in cands:
        for key in keys(c):
            need.setdefault(key, None)
    for c in cands:
        new = [key for key in keys(c) if need[key] is None]
        if new:
            cases.append(c)
            for key in new:
                need[key] = c
    return cases, need
