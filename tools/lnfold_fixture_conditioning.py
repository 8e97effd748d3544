"""Where the shipped fixtures stand against the accuracy envelope of the folded LayerNorms (profiles/lnfold_conditioning.txt): runs the oracle backbone on the
CPU in fp32 and records, for every row that enters a `norm2` or an `ffn_ln`, cond = (mean^2 + var) / (var + eps) and |mean| / sigma -- what the one-pass statistics and
the raw-row GEMM of EPI_SWIGLU_STATS_LN / EPI_RESIDUAL_LN are sensitive to (tests/lnfold_cases.py).  Prints the largest value per LayerNorm and stage of the backbone.

    python tools/lnfold_fixture_conditioning.py [tiny] [vitl] [vitl_stress] [--blocks N]

Inputs and weights are the fixtures' own (toc3d_amd.synth: SEEDED RANDOM weights; the token selection of the ViT-L run is the one recorded in tests/golden/); nobody has
measured a trained checkpoint's rows.  Not a test; needs no GPU."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import toc3d_oracle as O            # noqa: E402
from toc3d_amd import configs, synth           # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
ARGS = ("x", "temp_queries", "temp_ref_points", "temp_vel", "temp_timestamp", "temp_ego_pose", "ego_pose_inv")


class Done(Exception):
    pass


def run(tag, name, views, hw, fixture, stress, max_blocks):
    cfg = configs.get(name)
    sd = synth.make_state_dict(cfg, stress=True) if stress else synth.make_state_dict(cfg)
    inp = synth.make_inputs(cfg, views_per_frame=views, hw=hw) if hw else synth.make_inputs(cfg, views_per_frame=views)
    names = {id(v): k for k, v in sd.items() if k.endswith("norm2.weight") or k.endswith("ffn_ln.weight")}
    rec = {}                                                    # (block, kind) -> [max cond, max |mean| / sigma, rows]
    plain = O.layer_norm

    def hooked(x, w, b, eps=O.LN_EPS):
        key = names.get(id(w))
        if key is not None:
            parts = key.split(".")
            blk, kind = int(parts[1]), parts[-2]
            if max_blocks and blk >= max_blocks:
                raise Done
            r = x.reshape(-1, x.shape[-1]).double()
            mean, var = r.mean(1), r.var(1, unbiased=False)
            cond, ratio = (mean * mean + var) / (var + eps), mean.abs() / var.sqrt().clamp_min(1e-300)
            e = rec.setdefault((blk, kind), [0.0, 0.0, 0])
            e[0], e[1], e[2] = max(e[0], float(cond.max())), max(e[1], float(ratio.max())), e[2] + r.shape[0]
        return plain(x, w, b, eps)

    forced = None
    if fixture:
        g = np.load(os.path.join(GOLDEN, fixture + ".npz"))
        forced = [(torch.from_numpy(g[f"stage{s}.score"]), torch.from_numpy(g[f"token_mask{s}"]).reshape(g[f"stage{s}.score"].shape)) for s in range(3)]
    t0 = time.time()
    O.layer_norm = hooked
    try:
        with torch.no_grad():
            O.forward_toc3d(sd, cfg, *[inp[k] for k in ARGS], True, inp["gumbel"], **({"forced": forced} if forced else {}))
    except Done:
        pass
    finally:
        O.layer_norm = plain
    print(f"[{tag}] config {name}, {views} views{' of %d x %d' % hw if hw else ''}, blocks {'0-%d' % (max_blocks - 1) if max_blocks else 'all'}, {time.time() - t0:.0f} s on the CPU (fp32 oracle)")
    print(f"[{tag}] {'block':>5s} {'LayerNorm':>9s} {'rows':>8s} {'max cond':>10s} {'max |mean|/sigma':>17s}")
    for (blk, kind), (c, r, n) in sorted(rec.items()):
        print(f"[{tag}] {blk:>5d} {kind:>9s} {n:>8d} {c:>10.3g} {r:>17.3g}")
    for kind in ("norm2", "ffn_ln"):
        sel = [(v[0], v[1], k[0]) for k, v in rec.items() if k[1] == kind]
        if sel:
            c = max(sel)
            r = max(sel, key=lambda t: t[1])
            print(f"[{tag}] {kind}: largest cond {c[0]:.3g} (block {c[2]}), largest |mean| / sigma {r[1]:.3g} (block {r[2]})")


def main(argv):
    max_blocks = int(argv[argv.index("--blocks") + 1]) if "--blocks" in argv else 0
    which = [a for a in argv if a in ("tiny", "vitl", "vitl_stress")] or ["tiny", "vitl"]
    if "tiny" in which:
        run("tiny", "toc3d_tiny", 2, None, None, False, max_blocks)
    if "vitl" in which:
        run("vitl 320x800", "toc3d_faster", 6, (320, 800), "vitl_toc3d_faster", False, max_blocks)
    if "vitl_stress" in which:
        run("vitl stress", "toc3d_faster", 6, (320, 800), None, True, max_blocks)


if __name__ == "__main__":
    main(sys.argv[1:])
