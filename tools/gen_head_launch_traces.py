"""Records what the head's four modules hand to the library: tests/golden/head_launch_traces.json, the ``lib.call`` list of ``PETRTemporalTransformer``,
``HeadOutputs``, ``HeadQueries`` and ``HeadTokenEmbedding`` at the tiny sizes of ``toc3d_amd.synth``, in every precision each supports, launched eagerly.

Per case two lists: the first forward (weight packing, the learned queries' half, the frame) and the second one (the frame alone).  A call is written as
``[entry name, argument, ...]`` with tensors as ``[dtype, shape]``, pointer lists element by element, integers of magnitude >= 2^32 (device and host addresses)
as ``"ptr"`` and everything else as it is: dtype codes, epilogues, tile variants, M / N / K, leading dimensions, eps.  Only public constructors and ``synth`` are
used, so the file can be recorded on any commit; tests/test_gpu_head_launch_trace.py replays the cases and compares the lists.  A change that alters the launches
on purpose regenerates the file (needs the GPU) and says so.

  python tools/gen_head_launch_traces.py
"""
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import toc3d_amd                                  # noqa: E402
from toc3d_amd import lib, synth                  # noqa: E402

DEV = "cuda:0"
PATH = os.path.join(ROOT, "tests", "golden", "head_launch_traces.json")


def _decoder(precision, with_temp):
    m = toc3d_amd.build_transformer(synth.decoder_cfg(**synth.DECODER_TINY), precision=precision, launch_mode="eager")
    m.load_state_dict(synth.decoder_state_dict(synth.DECODER_TINY))
    m = m.to(DEV).eval()
    i = {k: None if v is None else v.to(DEV) for k, v in synth.decoder_inputs(synth.DECODER_TINY, synth.DECODER_TINY_SHAPE, with_temp=with_temp).items()}
    return lambda: m(i["memory"], i["tgt"], i["query_pos"], i["pos_embed"], None, i["temp_memory"], i["temp_pos"])


def _outputs(precision, levels):
    m = toc3d_amd.HeadOutputs(**synth.HEAD_OUTPUTS_TINY, precision=precision, launch_mode="eager", levels=levels)
    m.load_state_dict(synth.head_outputs_state_dict(synth.HEAD_OUTPUTS_TINY))
    m = m.to(DEV).eval()
    i = synth.head_outputs_inputs(synth.HEAD_OUTPUTS_TINY, synth.HEAD_OUTPUTS_TINY_SHAPE)
    outs, ref = i["outs_dec"].to(DEV), i["reference_points"].to(DEV)
    return lambda: m(outs, ref)


def _queries(precision, with_ego_pos):
    m = toc3d_amd.HeadQueries(**synth.HEAD_QUERIES_TINY, with_ego_pos=with_ego_pos, precision=precision, launch_mode="eager")
    m.load_state_dict(synth.head_queries_state_dict(synth.HEAD_QUERIES_TINY, with_ego_pos=with_ego_pos))
    m = m.to(DEV).eval()
    bank = {k: v.to(DEV) for k, v in synth.head_queries_bank(synth.HEAD_QUERIES_TINY, 2, 1).items()}
    return lambda: m(bank["memory_embedding"], bank["memory_reference_point"], bank["memory_timestamp"], bank["memory_egopose"], bank["memory_velo"])


def _tokens(precision):
    cfg, (B, N, h, w) = synth.HEAD_TOKENS_TINY, (2, 2, 2, 3)
    m = toc3d_amd.HeadTokenEmbedding(precision=precision, **cfg)
    m.load_state_dict(synth.head_tokens_state_dict(cfg))
    m = m.to(DEV).eval()
    i = {k: v.to(DEV) for k, v in synth.head_tokens_inputs(cfg, B, N, h, w).items()}
    return lambda: m(i["feats"], i["intrinsics"], i["lidar2img"], (h * cfg["stride"], w * cfg["stride"], 3))


def cases():
    """{case name: a function that builds the module and its inputs and returns the forward to trace}."""
    out = {}
    for p in ("bf16", "fp32x3"):
        for with_temp in (True, False):
            out[f"decoder {p} {'with' if with_temp else 'without'} temp memory"] = lambda p=p, t=with_temp: _decoder(p, t)
        for levels in ("all", "last"):
            out[f"head_outputs {p} levels={levels}"] = lambda p=p, l=levels: _outputs(p, l)
    for p in ("bf16", "fp32x3", "fp32"):
        for ego in (True, False):
            out[f"head_queries {p} with_ego_pos={ego}"] = lambda p=p, e=ego: _queries(p, e)
        out[f"head_tokens {p}"] = lambda p=p: _tokens(p)
    return out


def _norm(a):
    if isinstance(a, torch.Tensor):
        return [str(a.dtype), list(a.shape)]
    if isinstance(a, ctypes.Array):
        return [_norm(v) for v in a]
    if isinstance(a, int) and not isinstance(a, bool) and abs(a) >= 2 ** 32:
        return "ptr"
    return a


def trace(make):
    """[calls of the first forward, calls of the second forward] of one case."""
    calls, real = [], lib.call

    def recorder(name, *args):
        calls.append([name] + [_norm(a) for a in args])
        return real(name, *args)
    lib.call = recorder                     # (the modules reach the library through ``lib.call`` alone)
    try:
        forward = make()
        del calls[:]                        # (what building the module and its inputs issued is not the module's frame)
        out = []
        for _ in range(2):
            forward()
            out.append(list(calls))
            del calls[:]
        torch.cuda.synchronize()
    finally:
        lib.call = real
    return json.loads(json.dumps(out))      # (what the file holds: tuples as lists)


def main():
    res = {name: trace(make) for name, make in cases().items()}
    one = lambda calls: "[\n" + ",\n".join(json.dumps(c, separators=(",", ":")) for c in calls) + "\n]"        # a call per line: a diff names the launch
    with open(PATH, "w") as fh:
        fh.write("{\n" + ",\n".join(f"{json.dumps(k)}: [{one(t[0])}, {one(t[1])}]" for k, t in sorted(res.items())) + "\n}\n")
    print(f"{PATH}: {len(res)} cases, {sum(len(t[0]) + len(t[1]) for t in res.values())} calls, {os.path.getsize(PATH)} bytes")


if __name__ == "__main__":
    main()
