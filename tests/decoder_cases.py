"""The decoder's plain-torch restatement and module builders (shared by test_cpu_decoder.py, test_gpu_decoder.py, test_gpu_decoder_kernels.py and the head's GPU
tests; importing this needs no GPU).  ``restated_decoder`` pins tests/golden/decoder_tiny.npz -- output of the REAL reference (tools/gen_golden_decoder.py) -- to
something checkable where the reference does not exist, and is the GPU tests' control."""
import torch

import toc3d_amd
from support import DEV, layer_norm
from toc3d_amd import synth


def restated_decoder(sd, sizes, inp, dtype=torch.float32, contract=None, capture=None):
    """PETRTemporalTransformer.forward at eval from the formulas: per layer self_attn, norm, cross_attn, norm, ffn, norm (post-norm, identity = the
    attention's / FFN's own input), the shared post_norm on every layer's output.  ``contract`` = dtype the operands of every contraction (projections, q.k,
    p.v, FFN) are rounded to (None: none), accumulation and everything else in ``dtype``: contract=torch.bfloat16 is the torch-bf16 control."""
    E, H, L = sizes["embed_dims"], sizes["num_heads"], sizes["num_layers"]
    c = lambda t: t if contract is None else t.to(contract).to(dtype)
    mm = lambda a, b: c(a) @ c(b)
    p = {k: v.to(inp["memory"].device, dtype) for k, v in sd.items()}
    t = lambda k: None if inp[k] is None else inp[k].to(dtype)
    memory, qpos, pos, tmem, tpos = t("memory"), t("query_pos"), t("pos_embed"), t("temp_memory"), t("temp_pos")
    x = torch.zeros_like(qpos) if inp["tgt"] is None else t("tgt")

    def mha(pre, q_in, k_in, v_in):
        w, b = p[pre + "attn.in_proj_weight"], p[pre + "attn.in_proj_bias"]
        q, k, v = mm(q_in, w[:E].T) + b[:E], mm(k_in, w[E:2 * E].T) + b[E:2 * E], mm(v_in, w[2 * E:].T) + b[2 * E:]
        heads = lambda a: a.view(a.shape[0], a.shape[1], H, E // H).transpose(1, 2)
        s = mm(heads(q), heads(k).transpose(-1, -2)) * (E // H) ** -0.5
        s = s - s.max(-1, keepdim=True).values
        e = torch.exp(s)
        o = mm(e / e.sum(-1, keepdim=True), heads(v)).transpose(1, 2).reshape(q.shape)
        return mm(o, p[pre + "attn.out_proj.weight"].T) + p[pre + "attn.out_proj.bias"]

    outs = []
    for i in range(L):
        pre = f"decoder.layers.{i}."
        n = lambda j, y: layer_norm(y, p[pre + f"norms.{j}.weight"], p[pre + f"norms.{j}.bias"])
        keys, kpos = (x, qpos) if tmem is None else (torch.cat([x, tmem], 1), torch.cat([qpos, tpos], 1))
        x1 = n(0, x + mha(pre + "attentions.0.", x + qpos, keys + kpos, keys))
        x2 = n(1, x1 + mha(pre + "attentions.1.", x1 + qpos, memory + pos, memory))
        h = torch.relu(mm(x2, p[pre + "ffns.0.layers.0.0.weight"].T) + p[pre + "ffns.0.layers.0.0.bias"])
        x = n(2, x2 + mm(h, p[pre + "ffns.0.layers.1.weight"].T) + p[pre + "ffns.0.layers.1.bias"])
        if capture is not None:
            capture.update({f"l{i}_norm0": x1, f"l{i}_norm1": x2, f"l{i}_norm2": x})
        outs.append(layer_norm(x, p["decoder.post_norm.weight"], p["decoder.post_norm.bias"]))
    return torch.stack(outs)


def build(sizes, precision="fp32x3", launch_mode="plan", seed=0):
    m = toc3d_amd.build_transformer(dict(synth.decoder_cfg(**sizes), precision=precision, launch_mode=launch_mode))
    m.load_state_dict(synth.decoder_state_dict(sizes, seed=seed), strict=True)
    return m.to(DEV).eval()


def run(m, inp):
    d = lambda t: None if t is None else t.to(DEV)
    return m(d(inp["memory"]), d(inp["tgt"]), d(inp["query_pos"]), d(inp["pos_embed"]), None, d(inp["temp_memory"]), d(inp["temp_pos"]))


def _heads(t, H):
    return t.view(t.shape[0], t.shape[1], H, 32).transpose(1, 2)
