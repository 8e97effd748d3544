"""GPU: toc3d_mha_attention and toc3d_amd.PETRTemporalTransformer against the REAL reference's fixtures (tests/golden/decoder_*.npz, written by
tools/gen_golden_decoder.py) and against f64 torch.  Error measure as in tests/test_gpu_e2e.py: max-abs error over max-abs reference; the bf16 bounds are
relative to a torch-bf16 control on the same card (tests/test_gpu_parity_bf16.py).

Measured on MI355X (profiles/decoder_parity.txt): fp32x3 against the f32 reference, worst layer: tiny 4.1e-5 / 3.0e-5 (with / without temp_memory), shipped
sizes 1.5e-5; bf16 relative L2 of the last layer against the f64 arbiter 6.8e-3 next to the control's 6.7e-3; toc3d_mha_attention alone: fp32x3 <= 2.5e-5,
bf16 <= 3.0e-3 (control 6.7e-3 ... 2.6e-2: torch's eager bf16 ops round the scores too)."""
import os

import numpy as np
import pytest
import torch

import toc3d_amd
from decoder_cases import _heads, build, restated_decoder, run
from support import DEV, rel_l2, rel_max
from toc3d_amd import lib, synth

pytestmark = pytest.mark.gpu


# ---- the kernel alone ------------------------------------------------------------------------------------------------------------------
def _attention(q, k, v, H):
    """softmax(q.k^T / sqrt(32)).v per head in the dtype of the operands (f64: the arbiter; bf16: torch's eager bf16 ops, the control)."""
    p = torch.softmax(_heads(q, H) @ _heads(k, H).transpose(-1, -2) * 32 ** -0.5, -1)
    return (p @ _heads(v, H)).transpose(1, 2).reshape(q.shape)


@pytest.mark.parametrize("precision", ["fp32x3", "bf16"])
@pytest.mark.parametrize("H", [2, 8])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("Nq,Nk", [(1, 1), (15, 17), (16, 64), (900, 1668), (900, 6000), (33, 6001)])
def test_mha_attention_against_f64(Nq, Nk, B, H, precision):
    g = torch.Generator().manual_seed(Nq * 7 + Nk + B + H)
    W = H * 32
    dt, tdt = (lib.F32X3, torch.float32) if precision == "fp32x3" else (lib.BF16, torch.bfloat16)
    q, k, v = ((torch.randn(B, n, W, generator=g) * s).to(DEV).to(tdt) for n, s in ((Nq, 1.5), (Nk, 1.5), (Nk, 1.0)))
    ref = _attention(q.double(), k.double(), v.double(), H)
    outs = []
    for _ in range(2):
        out = torch.full((B * Nq + 5, W), 777.0, dtype=tdt, device=DEV)             # over-allocated: rows past B * Nq must stay untouched
        lib.call("toc3d_mha_attention", dt, q, W, k, W, v, W, out, W, B, Nq, Nk, H, 32, 32 ** -0.5, lib.stream_ptr())
        torch.cuda.synchronize()
        outs.append(out)
    assert torch.equal(outs[0], outs[1]), "two runs differ"
    assert bool((outs[0][B * Nq:] == 777.0).all()), "rows past B * Nq were written"
    err = rel_max(outs[0][:B * Nq].view(B, Nq, W), ref)
    if precision == "fp32x3":
        print(f"[mha fp32x3 Nq={Nq} Nk={Nk} B={B} H={H}] rel max err {err:.2e}")
        assert err < 1e-3 / 10                                                      # one op gets a tenth of the end-to-end budget
    else:
        ctl = rel_max(_attention(q, k, v, H), ref)
        print(f"[mha bf16 Nq={Nq} Nk={Nk} B={B} H={H}] rel max err {err:.2e}   torch-bf16 control {ctl:.2e}")
        assert err <= 1.2 * ctl


def test_mha_attention_refuses_other_head_dims_and_dtypes():
    q = torch.zeros(16, 64, device=DEV)
    l = lib.load()
    args = lambda dt, hd: (dt, q.data_ptr(), 64, q.data_ptr(), 64, q.data_ptr(), 64, q.data_ptr(), 64, 1, 16, 16, 1, hd, 0.125, None)
    assert l.toc3d_mha_attention(*args(lib.F32X3, 64)) == -2 and b"head_dim must be 32" in l.toc3d_last_error()
    assert l.toc3d_mha_attention(*args(lib.F32, 32)) == -2


def test_mha_attention_two_key_segments_equal_one():
    """The decoder's self-attention reads its keys from two buffers ([query; temp_memory], the second projected once per frame for all layers)."""
    g = torch.Generator().manual_seed(5)
    B, H, Nq, Nk, W = 2, 8, 900, 1668, 256
    for dt, tdt in ((lib.F32X3, torch.float32), (lib.BF16, torch.bfloat16)):
        q, k, v = (torch.randn(B, n, W, generator=g).to(DEV).to(tdt) for n in (Nq, Nk, Nk))
        one, two = torch.empty(B * Nq, W, dtype=tdt, device=DEV), torch.empty(B * Nq, W, dtype=tdt, device=DEV)
        lib.call("toc3d_mha_attention_ex", dt, q, W, k, W, v, W, None, 0, None, 0, one, W, B, Nq, Nk, 0, H, 32, 32 ** -0.5, lib.stream_ptr())
        k1, k2, v1, v2 = k[:, :900].contiguous(), k[:, 900:].contiguous(), v[:, :900].contiguous(), v[:, 900:].contiguous()
        lib.call("toc3d_mha_attention_ex", dt, q, W, k1, W, v1, W, k2, W, v2, W, two, W, B, Nq, 900, Nk - 900, H, 32, 32 ** -0.5, lib.stream_ptr())
        assert torch.equal(one, two)


# ---- the module against the reference's fixtures --------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,with_temp", [("temp", True), ("notemp", False)])
def test_decoder_tiny_matches_reference_golden(golden_dir, tag, with_temp):
    """fp32x3 (the default) < 1e-3, the project's parity bar, on every layer of outs_dec -- replayed plan -- and, through eager
    launches, on the three post-norm intermediates of every layer."""
    g = np.load(os.path.join(golden_dir, "decoder_tiny.npz"))
    sizes, shape = synth.DECODER_TINY, synth.DECODER_TINY_SHAPE
    inp = synth.decoder_inputs(sizes, shape, with_temp=with_temp)
    m = build(sizes)
    assert m.precision == "fp32x3"
    for _ in range(3):                                  # eager, recorded, replayed
        outs, mem, attn = run(m, inp)
    assert attn is None and outs.shape == (2, 2, 32, 64) and torch.equal(mem.cpu(), inp["memory"])
    errs = [rel_max(outs[l], g[f"{tag}_outs_dec"][l]) for l in range(2)]
    m.capture = {}
    outs_e, _, _ = run(m, inp)
    assert torch.equal(outs_e, outs), "eager launches and the replayed plan differ"
    mids = {k: rel_max(v, g[f"{tag}_{k}"]) for k, v in m.capture.items()}
    print(f"[decoder tiny {tag} fp32x3] rel max err per layer {[f'{e:.2e}' for e in errs]}   intermediates max {max(mids.values()):.2e}")
    assert len(mids) == 6 and max(errs) < 1e-3 and max(mids.values()) < 1e-3


def _full(golden_dir):
    g = np.load(os.path.join(golden_dir, "decoder_full.npz"))
    return g, torch.from_numpy(g["rows"]).long(), synth.decoder_inputs(synth.DECODER_FULL, synth.DECODER_FULL_SHAPE)


def test_decoder_full_size_fp32x3_matches_reference_golden(golden_dir):
    """Shipped sizes (E 256, 8 heads, FFN 2048, 6 layers, 900 queries, 768 memory entries, 6000 image tokens): every layer of outs_dec < 1e-3 on the
    fixture's rows (every 8th query; committed files are capped at 1 MiB)."""
    g, rows, inp = _full(golden_dir)
    m = build(synth.DECODER_FULL)
    for _ in range(3):
        outs, _, _ = run(m, inp)
    assert outs.shape == (6, 1, 900, 256) and outs.dtype == torch.float32
    errs = [rel_max(outs[l][:, rows], g["outs_dec"][l]) for l in range(6)]
    print(f"[decoder full fp32x3] rel max err per layer {[f'{e:.2e}' for e in errs]}")
    assert max(errs) < 1e-3


def test_decoder_full_size_bf16_within_control(golden_dir):
    """bf16: relative L2 of outs_dec[-1] at most 1.2 x that of the torch-bf16 control (the restatement with bf16 contraction operands, f32 accumulation, on the
    same card), both against the f64 run of the reference's modules."""
    g, rows, inp = _full(golden_dir)
    m = build(synth.DECODER_FULL, precision="bf16")
    for _ in range(3):
        outs, _, _ = run(m, inp)
    with torch.no_grad():
        ctl = restated_decoder(synth.decoder_state_dict(synth.DECODER_FULL), synth.DECODER_FULL, {k: None if v is None else v.to(DEV) for k, v in inp.items()},
                               contract=torch.bfloat16)
    e_hip, e_ctl = rel_l2(outs[-1][:, rows], g["last_f64"]), rel_l2(ctl[-1][:, rows], g["last_f64"])
    print(f"[decoder full bf16] rel l2 of the last layer vs f64: hip {e_hip:.3e}   torch-bf16 control {e_ctl:.3e}")
    assert torch.isfinite(outs).all()
    assert e_hip <= 1.2 * e_ctl


@pytest.mark.parametrize("precision", ["fp32x3", "bf16"])
def test_replayed_plan_equals_eager_launches_bit_for_bit(precision):
    sizes, shape = synth.DECODER_FULL, synth.DECODER_FULL_SHAPE
    a, b = synth.decoder_inputs(sizes, shape, seed=0), synth.decoder_inputs(sizes, shape, seed=1)
    b["tgt"] = None                                     # tgt=None means zeros: the staged buffer must not keep frame a's rows
    eager, plan = build(sizes, precision, "eager"), build(sizes, precision, "plan")
    ea, eb = run(eager, a)[0], run(eager, b)[0]
    assert not torch.equal(ea, eb)
    for _ in range(3):
        pa = run(plan, a)[0]
    state = plan._states[(1, 900, 6000, 768)]
    assert state.get("cplan") is not None and state["cplan"].num_launches > 70
    assert torch.equal(pa, ea)
    pb = run(plan, b)[0]                                # other inputs through the SAME recorded plan
    assert plan._states[(1, 900, 6000, 768)]["cplan"] is state["cplan"]
    assert torch.equal(pb, eb) and torch.equal(pa, ea), "an output aliases a workspace"


def test_chain_head_tokens_decoder_memory_two_frames():
    """HeadTokenEmbedding -> PETRTemporalTransformer -> (seeded cls / bbox) -> TemporalMemory.post_update_memory, tensors handed over as they come (no copies,
    no layout change); the second frame equals a run that clones every tensor in between: nothing handed out aliases a workspace."""
    hcfg, sizes = synth.HEAD_TOKENS_CFG, synth.DECODER_FULL
    B, N, h, w, NQ, NCLS = 1, 6, 20, 50, 900, 10
    mcfg = dict(memory_len=640, topk_proposals=128, num_propagated=128, embed_dims=256)
    minp = synth.memory_inputs(mcfg, B, NQ - mcfg["num_propagated"], NCLS, 2, seed=3)
    head = toc3d_amd.HeadTokenEmbedding(precision="fp32", **hcfg)
    head.load_state_dict(synth.head_tokens_state_dict(hcfg))
    head = head.to(DEV).eval()
    d = lambda t: t.to(DEV)

    def sequence(clone):
        c = (lambda t: t.clone()) if clone else (lambda t: t)
        dec = build(sizes)
        mem = toc3d_amd.TemporalMemory(pseudo_reference_points=minp["pseudo"], **mcfg)
        res = []
        for f in range(2):
            hin = synth.head_tokens_inputs(hcfg, B, N, h, w, seed=f)
            qin = synth.decoder_inputs(sizes, synth.DECODER_FULL_SHAPE, seed=10 + f)
            fr = minp["frames"][f]
            data = {k: d(v) for k, v in fr["data"].items()}
            mem.pre_update_memory(data)
            memory, pos_embed, _ = head(d(hin["feats"]), d(hin["intrinsics"]), d(hin["lidar2img"]), (320, 800, 3))
            temp_memory = mem.memory_embedding
            outs_dec, _, _ = dec(c(memory), d(qin["tgt"]), d(qin["query_pos"]), c(pos_embed), None, c(temp_memory), d(qin["temp_pos"])[:, :temp_memory.shape[1]])
            mem.post_update_memory(data, d(fr["rec_ego_pose"]), d(fr["cls"])[None], d(fr["bbox"])[None], c(outs_dec))
            res.append((outs_dec, mem.memory_embedding.clone(), mem.memory_reference_point.clone()))
        return res
    plain, cloned = sequence(False), sequence(True)
    assert plain[0][0].shape == (6, 1, 900, 256) and plain[1][1].shape == (1, 768, 256)
    for p, q in zip(plain[1], cloned[1]):
        assert torch.isfinite(p).all() and torch.equal(p, q)
    assert not torch.equal(plain[0][0], plain[1][0])
