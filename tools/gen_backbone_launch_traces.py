"""Records what the backbones and the neck hand to the library: tests/golden/backbone_launch_traces.json, the ``lib.call`` list of ``ToC3DEVAViT``, ``EVA_ViT`` and
``CPFPN`` at the tiny configs (2 views per frame, 320 x 800), with ``autotune = False`` and ``launch_mode = "plan"``.

Per case three lists, one per forward, on the inputs of seeds 0, 1, 2: weight packing and the eager warm-up, the recording, the replay.  While a plan is recorded
the ``stream`` argument of a launch is its lane's handle (0x70c3d000 + lane, below 2^32, so it stays a number): the second list pins every launch's lane and every
``toc3d_plan_wait`` edge, not just the order.  Calls are normalised as tools/gen_head_launch_traces.py does it (addresses as ``"ptr"``), with a tensor written
``f32[2000,128]``.  The twelve blocks of a frame repeat a few launches on a few lanes, so the file holds every distinct call without its last argument (the
stream of a launch) once, one per line, and a forward as runs ``[last argument, line, line, ...]`` of consecutive calls that end on the same one.
Only public constructors, ``configs`` and ``synth`` are used, so the file can be recorded on any commit; tests/test_gpu_backbone_launch_trace.py replays the cases
and compares the lists.  A change that alters the launches on purpose regenerates the file (needs the GPU) and says so.

  python tools/gen_backbone_launch_traces.py
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import toc3d_amd                                  # noqa: E402
from toc3d_amd import configs, lib, synth         # noqa: E402
from tools.gen_head_launch_traces import _norm    # noqa: E402

DEV = "cuda:0"
PATH = os.path.join(ROOT, "tests", "golden", "backbone_launch_traces.json")
FORWARDS = 3
IMG_NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)


def _backbone(name, precision, groups=1, **kw):
    cfg = configs.get(name)
    m = toc3d_amd.build_backbone(dict(cfg, precision=precision, **kw))
    m.load_state_dict(synth.make_state_dict(cfg))
    m = m.to(DEV).eval()
    m.autotune, m.launch_mode, m.view_groups = False, "plan", groups
    return cfg, m


def _toc3d(precision="bf16", groups=1, prev=True, frames=1, noise=True, f32_ts=False, u8=False, **kw):
    cfg, m = _backbone("toc3d_tiny", precision, groups, **kw)
    m.gumbel_seed = 1234                           # (the key of the device-side draw is an argument of its launch: not left to torch's seed of the moment)

    def forward(seed):
        i = synth.make_inputs(cfg, n_frames=frames, views_per_frame=2, seed=seed, device=DEV)
        x = i["x"]
        if u8:                                     # raw camera images, HWC, of a size that the padding rounds up to 320 x 800
            g = torch.Generator().manual_seed(seed)
            x = torch.randint(0, 256, (x.shape[0], 310, 790, 3), dtype=torch.uint8, generator=g).to(DEV)
        o = m(x, temp_queries=i["temp_queries"], prev_exists=prev, temp_ref_points=i["temp_ref_points"], temp_vel=i["temp_vel"],
              temp_timestamp=i["temp_timestamp"].float() if f32_ts else i["temp_timestamp"], temp_ego_pose=i["temp_ego_pose"],
              ego_pose_inv=i["ego_pose_inv"], gumbel_noise=i["gumbel"] if noise else None)
        return [o.img_feats["last_feat"], *o.token_masks, *o.keep_idx, *o.drop_idx]
    return forward


def _eva(precision, groups, neck=None):
    cfg, m = _backbone("eva_tiny", precision, groups)
    if neck is None:
        return lambda seed: [m(synth.make_inputs(cfg, views_per_frame=2, seed=seed, device=DEV)["x"])["last_feat"]]
    m.alias_outputs = True                         # the neck records a plan only on an input at a fixed address
    n = toc3d_amd.build_neck(dict(configs.CPFPN_TINY, precision=precision))
    n.load_state_dict(synth.neck_state_dict(configs.CPFPN_TINY))
    n = n.to(DEV).eval()
    n.autotune = False
    rows = torch.zeros(2 * 20 * 50, 64, dtype=torch.bfloat16, device=DEV)

    def forward(seed):
        feats = [m(synth.make_inputs(cfg, views_per_frame=2, seed=seed, device=DEV)["x"])["last_feat"]]
        outs = n(feats) if neck == "forward" else n.forward_fanout(feats, rows, rows.shape[1], lib.BF16)
        return [*outs] + ([] if neck == "forward" else [rows])
    return forward


def cases():
    """{case name: a function that builds the modules and returns ``forward(seed)`` -> the list of returned tensors}."""
    out = {}
    for p in ("bf16", "fp32x3", "fp32"):
        for g in (1, 2):
            out[f"toc3d_tiny {p} view_groups={g}"] = lambda p=p, g=g: _toc3d(p, g)
    for tag, kw in (("prev_exists=False", dict(prev=False)), ("mixed step", dict(prev=[True, False], frames=2)), ("device-drawn noise", dict(noise=False)),
                    ("f32 timestamps", dict(f32_ts=True)), ("side_lanes=False", dict(schedule=dict(side_lanes=False))),
                    ("gather_split=True", dict(schedule=dict(gather_split=True))), ("attn_rot=False", dict(schedule=dict(attn_rot=False))),
                    ("uint8 HWC input", dict(u8=True, img_norm_cfg=IMG_NORM))):
        out[f"toc3d_tiny bf16 {tag}"] = lambda kw=kw: _toc3d(**kw)
    for p in ("bf16", "fp32x3"):
        for g in (1, 2):
            out[f"eva_tiny {p} view_groups={g}"] = lambda p=p, g=g: _eva(p, g)
    for neck in ("forward", "forward_fanout"):
        out[f"eva_tiny bf16 aliased -> CPFPN_TINY {neck}"] = lambda neck=neck: _eva("bf16", 1, neck)
    return out


def _short(a):
    """``_norm``'s ``[dtype, shape]`` of a tensor as one word: f32[2000,128], bf16[..], i32[..], ui8[..]."""
    if isinstance(a, list) and len(a) == 2 and isinstance(a[0], str) and a[0].startswith("torch."):
        return a[0][6:].replace("bfloat", "bf").replace("float", "f").replace("int", "i") + json.dumps(a[1], separators=(",", ":"))
    return [_short(v) for v in a] if isinstance(a, list) else a


def trace(make):
    """[calls of the first, second, third forward] of one case."""
    calls, real = [], lib.call

    def recorder(name, *args):
        calls.append([name] + [_short(_norm(a)) for a in args])
        return real(name, *args)
    lib.call = recorder                     # (the modules reach the library through ``lib.call`` alone)
    try:
        forward = make()
        out = []
        for seed in range(FORWARDS):
            del calls[:]                    # (what building the modules and the inputs issued is not the modules' frame)
            forward(seed)
            out.append(list(calls))
        torch.cuda.synchronize()
    finally:
        lib.call = real
    return json.loads(json.dumps(out))      # (what the file holds: tuples as lists)


def load(path=PATH):
    """{case: [calls, calls, calls]} of the file: the runs put back into calls."""
    with open(path) as fh:
        d = json.load(fh)
    return {k: [[d["calls"][i] + [run[0]] for run in f for i in run[1:]] for f in t] for k, t in d["cases"].items()}


def dump(res, path=PATH):
    """Write {case: [calls, calls, calls]}; -> the number of distinct lines."""
    line = lambda c: json.dumps(c[:-1], separators=(",", ":"))
    lines = sorted({line(c) for t in res.values() for f in t for c in f})            # a distinct call per line: a diff names the launch
    at = {l: i for i, l in enumerate(lines)}
    cases = {}
    for k, t in res.items():
        cases[k] = []
        for f in t:
            runs = []
            for c in f:
                if runs and runs[-1][0] == c[-1]:
                    runs[-1].append(at[line(c)])
                else:
                    runs.append([c[-1], at[line(c)]])
            cases[k].append(runs)
    with open(path, "w") as fh:
        fh.write('{"calls": [\n' + ",\n".join(lines) + '\n],\n"cases": {\n' +
                 ",\n".join(f"{json.dumps(k)}: {json.dumps(t, separators=(',', ':'))}" for k, t in sorted(cases.items())) + "\n}}\n")
    return len(lines)


def main():
    res = {name: trace(make) for name, make in cases().items()}
    n = dump(res)
    print(f"{PATH}: {len(res)} cases, {sum(len(f) for t in res.values() for f in t)} calls, {n} distinct lines, {os.path.getsize(PATH)} bytes")


if __name__ == "__main__":
    main()
