"""CPU: toc3d_amd.staged.StagedModule, the base of the head's four modules, on a toy subclass -- no device.

Derived / instance state over load_state_dict, _apply, deepcopy and pickle (for the base's sets and for a subclass that extends both); the replay helper's
per-key states and oldest-first eviction; the two refusals; and _linear: the positional tuple that reaches lib.call for every form the four modules' own closures
had before the base existed, written out from those closures (lib.call is a recorder and the recording lane makes lib.stream_ptr() a lane handle, as in
tests/test_cpu_abi.py)."""
import contextlib
import copy
import pickle
import threading

import pytest
import torch
import torch.nn as nn

import toc3d_amd
from toc3d_amd import lib, plan
from toc3d_amd.staged import StagedModule, require_cuda


class Toy(StagedModule):
    _NAME, _RUNS, _SUPPORTED = "toc3d_amd.Toy", "the toy runs", ("bf16", "fp32x3", "fp32")

    def __init__(self, precision="bf16", launch_mode="plan"):
        super().__init__()
        self.fc = nn.Linear(4, 4)
        self._init_staged(precision, launch_mode)


class ToyMore(Toy):                       # extends both tiers, as HeadQueries (_fresh) and the decoder (capture) do
    _DERIVED = dict(Toy._DERIVED, _fresh=None)
    _INSTANCE = dict(Toy._INSTANCE, capture=None)

    def __init__(self):
        super().__init__()
        self.capture = None


@pytest.mark.parametrize("cls", [Toy, ToyMore])
def test_derived_and_instance_state(cls):
    assert set(StagedModule._DERIVED) == {"_packed", "_ws", "_states", "_sk_ws", "_sk_ws_old"} and set(StagedModule._INSTANCE) == {"_pool"}
    assert set(ToyMore._DERIVED) == set(Toy._DERIVED) | {"_fresh"} and set(ToyMore._INSTANCE) == {"_pool", "capture"}
    m = cls()
    every = {**cls._DERIVED, **cls._INSTANCE}
    assert all(getattr(m, k) == empty for k, empty in every.items()), "a new module starts with both tiers empty"
    assert all(getattr(m, k) is not empty for k, empty in every.items() if empty is not None), "... on containers of its own"
    mark = threading.Lock()                # neither copyable nor picklable: a copy that carried it over would raise

    def plant():
        for k, empty in every.items():
            setattr(m, k, [mark] if isinstance(empty, list) else {"k": mark})
    empties = lambda x, names: all(getattr(x, k) == every[k] for k in names)
    planted = lambda x, names: all(getattr(x, k) in ([mark], {"k": mark}) for k in names)
    for invalidate in (lambda: m.load_state_dict(m.state_dict()), lambda: m._apply(lambda t: t), lambda: m.double(),
                       lambda: nn.ModuleDict(dict(part=m)).load_state_dict({"part." + k: v for k, v in m.state_dict().items()})):
        plant()
        invalidate()
        assert empties(m, cls._DERIVED) and planted(m, cls._INSTANCE), "new weights or a move empty _DERIVED and keep _INSTANCE"
    m.float()
    plant()
    for c in (copy.deepcopy(m), pickle.loads(pickle.dumps(m))):
        assert empties(c, every) and c.precision == m.precision and c.launch_mode == m.launch_mode
        assert all(torch.equal(a, b) and a.data_ptr() != b.data_ptr() for a, b in zip(c.state_dict().values(), m.state_dict().values()))
    assert planted(m, every), "the original keeps its own"


class _Ex:
    def __init__(self):
        self.lanes = []

    @contextlib.contextmanager
    def lane(self, i):
        self.lanes.append(i)
        yield


def test_replay_helper_states_and_eviction(monkeypatch):
    seen = []

    def run_frame(state, mode, n_lanes, frame_fn, pool):
        ex = _Ex()
        frame_fn(ex)
        seen.append((state, mode, n_lanes, pool, ex.lanes))
    monkeypatch.setattr(plan, "run_frame", run_frame)
    m, ran = Toy(launch_mode="plan"), []
    m._run("a", lambda: ran.append("a"))
    m._run("a", lambda: ran.append("a again"), mode="eager")
    assert ran == ["a", "a again"] and list(m._states) == ["a"]
    assert seen[0][0] is m._states["a"] and seen[1][0] is m._states["a"], "one state per key, handed to plan.run_frame"
    assert [s[1:] for s in seen] == [("plan", 1, m._pool, [0]), ("eager", 1, m._pool, [0])] and seen[0][3] is m._pool
    # without max_states nothing is dropped
    for k in range(20):
        m._run(k, lambda: None)
    assert len(m._states) == 21
    # with it: the oldest goes first, and only when a NEW key arrives at the bound
    m = Toy()
    for k in range(8):
        m._run(k, lambda: None, max_states=8)
    m._states[0]["cplan"] = "recorded"
    assert list(m._states) == list(range(8))
    m._run(0, lambda: None, max_states=8)                                  # the oldest key, in use again at the bound: nothing is evicted
    assert list(m._states) == list(range(8)) and m._states[0] == {"cplan": "recorded"} and seen[-1][0] is m._states[0]
    m._run(8, lambda: None, max_states=8)
    assert list(m._states) == list(range(1, 9)) and seen[-1][0] is m._states[8], "the new key is in, the oldest is out"
    m._run(9, lambda: None, max_states=8)
    assert list(m._states) == list(range(2, 10))
    m._run(10, lambda: None, max_states=3)                                 # a smaller bound drops down to it, oldest first, never the key in use
    assert list(m._states) == [8, 9, 10]


def test_refusals_carry_the_name():
    with pytest.raises(NotImplementedError, match=r"toc3d_amd\.Toy: precision 'fp16' is not implemented; the toy runs in 'bf16' or 'fp32x3' or 'fp32'"):
        Toy(precision="fp16")
    with pytest.raises(AssertionError):
        Toy(launch_mode="lazy")
    for match in (r"^toc3d_amd\.Toy: inputs must be", "CUDA/HIP", "no CPU"):
        with pytest.raises(RuntimeError, match=match):
            require_cuda(Toy._NAME, torch.zeros(2))
        with pytest.raises(RuntimeError, match=match):
            require_cuda(Toy._NAME, None, on_device=False)
    require_cuda(Toy._NAME, torch.zeros(2), torch.zeros(3), on_device=False)         # tensors, wherever they live
    # the token module, which used to assert: the same refusals under its own name
    cfg = dict(toc3d_amd.synth.HEAD_TOKENS_TINY)
    with pytest.raises(NotImplementedError, match=r"toc3d_amd\.HeadTokenEmbedding: precision 'fp16' is not implemented; the token side runs in"):
        toc3d_amd.HeadTokenEmbedding(precision="fp16", **cfg)
    with pytest.raises(NotImplementedError, match=r"toc3d_amd\.HeadTokenEmbedding: .*depth_num=8"):
        toc3d_amd.HeadTokenEmbedding(**dict(cfg, depth_num=8))
    tok = toc3d_amd.HeadTokenEmbedding(with_position=True, **cfg)                    # (unknown keys of the head's config block are still swallowed)
    assert tok.precision == "fp32" and tok._states == {} and tok._pool == []
    inp = toc3d_amd.synth.head_tokens_inputs(cfg, 1, 1, 2, 3)
    for match in (r"^toc3d_amd\.HeadTokenEmbedding: ", "CUDA/HIP", "no CPU"):
        with pytest.raises(RuntimeError, match=match):
            tok(inp["feats"], inp["intrinsics"], inp["lidar2img"], (32, 48, 3))


def test_linear_reaches_the_launcher_as_the_four_closures_did():
    L, z = lib, torch.zeros
    plain = L.NO_FUSED
    calls = []
    real_call, lib.call = lib.call, lambda name, *a: calls.append((name, a))
    lib.set_rec_lane(1)

    def one(precision, *a, **kw):
        m = Toy(precision)
        del calls[:]
        m._linear(*a, **kw)
        assert len(calls) == 1 and len(calls[0][1]) == len(lib._SIGS[calls[0][0]])
        return m, calls[0][0], calls[0][1]
    same = lambda got, want: len(got) == len(want) and all(g is w if isinstance(w, torch.Tensor) else (g == w and type(g) is type(w)) for g, w in zip(got, want))
    try:
        s = lib.stream_ptr()
        b = z(2048)
        # ---- the decoder's closure: linear(a, wb, out, M, N, K, residual=None) -- EPI_BIAS, or EPI_RESIDUAL onto f32 rows; plain A rows; lda / ldo = row lengths
        A, W, out, x = z(90, 64), z(128, 64), z(90, 128), z(90, 64)
        for precision, dt in (("bf16", L.BF16), ("fp32x3", L.F32X3W)):
            _, name, got = one(precision, A, (W, b), out, 90, 128, 64)                                    # self-attention q | k
            assert name == "toc3d_linear_fused" and same(got, (dt, L.EPI_BIAS, 14, A, 64, W, 64, b, out, 128, None, 0, 0, None, None, 90, 128, 64, 0, *plain, s))
            _, name, got = one(precision, A, (W, b), x, 90, 64, 64, residual=x)                            # an output projection, added to the stream
            assert name == "toc3d_linear_fused" and same(got, (dt, L.EPI_RESIDUAL, 14, A, 64, W, 64, b, x, 64, x, 64, 0, None, None, 90, 64, 64, 0, *plain, s))
            # the FFN's second layer at the shipped width, K = 2048 into N = 256 with the residual: the four-way split-K, on its workspace
            A2, W2, y, x2 = z(90, 2048), z(256, 2048), z(90, 256), z(90, 256)
            m, name, got = one(precision, A2, (W2, b), y, 90, 256, 2048, residual=x2)
            ws = m._sk_ws[(None, s)]
            assert ws.numel() * 4 == lib.load().toc3d_linear_splitk_workspace_bytes(4014, 90, 256) > 0
            assert name == "toc3d_linear_fused_ws" and same(got, (dt, L.EPI_RESIDUAL, 4014, A2, 2048, W2, 2048, b, y, 256, x2, 256, 0, None, None, 90, 256, 2048, 0, *plain,
                                                                  ws, ws.numel() * 4, s))
            # ... and without one (the FFN's first layer the other way round): no split
            _, name, got = one(precision, A2, (W2, b), y, 90, 256, 2048)
            assert name == "toc3d_linear_fused" and same(got, (dt, L.EPI_BIAS, 14, A2, 2048, W2, 2048, b, y, 256, None, 0, 0, None, None, 90, 256, 2048, 0, *plain, s))
            # the keys of all six layers from 6000 image tokens: 47 x 12 default tiles >= 256 -> the library's heuristic
            A3, W3, o3 = torch.empty(6000, 256), z(1536, 256), torch.empty(6000, 1536)
            _, name, got = one(precision, A3, (W3, b), o3, 6000, 1536, 256)
            assert name == "toc3d_linear_fused" and same(got, (dt, L.EPI_BIAS, 0, A3, 256, W3, 256, b, o3, 1536, None, 0, 0, None, None, 6000, 1536, 256, 0, *plain, s))
        # ---- HeadOutputs' closure: linear(a, wb, out, N, lda, ldo) -- always f32 rows out (EPI_RESIDUAL, no residual), A in planes on fp32x3, columns of wider buffers
        a1, Wc, h2 = z(128, 128), z(128, 64), z(128, 128)
        for precision, planes, dt in (("bf16", False, L.BF16), ("fp32x3", True, L.F32X3WA)):
            _, name, got = one(precision, a1, (Wc, b), h2, 128, 64, 64, f32_out=True, lda=128, ldo=128, a_planes=planes)
            assert name == "toc3d_linear_fused" and same(got, (dt, L.EPI_RESIDUAL, 14, a1, 128, Wc, 64, b, h2, 128, None, 0, 0, None, None, 128, 64, 64, 0, *plain, s))
            pa, po = a1.data_ptr() + 256, h2.data_ptr() + 256                                             # the box tower's half: pointers into both
            _, name, got = one(precision, pa, (Wc, b), po, 128, 64, 64, f32_out=True, lda=128, ldo=128, a_planes=planes)
            assert name == "toc3d_linear_fused" and same(got, (dt, L.EPI_RESIDUAL, 14, pa, 128, Wc, 64, b, po, 128, None, 0, 0, None, None, 128, 64, 64, 0, *plain, s))
        # ---- HeadQueries' closure: linear(a, wb, out, N, K, lda, ldo, f32_out, planes) -- act rows (EPI_BIAS) or f32 rows; A in planes = planes and fp32x3
        pos, Wq, h1, qe = z(54, 384), z(256, 384), z(54, 256), z(54, 256)
        for precision, dt_plain, dt_planes in (("bf16", L.BF16, L.BF16), ("fp32", L.F32, L.F32), ("fp32x3", L.F32X3W, L.F32X3WA)):
            x3p = precision == "fp32x3"
            _, name, got = one(precision, pos, (Wq, b), h1, 54, 256, 384, f32_out=False, lda=384, ldo=256, a_planes=True and x3p)      # query_embedding.0
            assert name == "toc3d_linear_fused" and same(got, (dt_planes, L.EPI_BIAS, 14, pos, 384, Wq, 384, b, h1, 256, None, 0, 0, None, None, 54, 256, 384, 0, *plain, s))
            _, name, got = one(precision, h1, (Wq, b), qe, 54, 256, 256, f32_out=True, lda=256, ldo=256, a_planes=False and x3p)       # query_embedding.2
            assert name == "toc3d_linear_fused" and same(got, (dt_plain, L.EPI_RESIDUAL, 14, h1, 256, Wq, 384, b, qe, 256, None, 0, 0, None, None, 54, 256, 256, 0, *plain, s))
        # ---- HeadTokenEmbedding's fp32x3 closure: linear(x, wb, out, n, k, f32_out, relu) -- K = the packed weight's row length; the ReLU in the epilogue on
        # A in planes, f32 rows from plain A behind it
        pin, Wp, hh, pe = torch.empty(6000, 192), z(1024, 192), torch.empty(6000, 1024), torch.empty(6000, 256)
        _, name, got = one("fp32x3", pin, (Wp, b), hh, 6000, 1024, 192, relu=True, a_planes=True)          # position_encoder.0 at the shipped size: 47 x 8 tiles -> 0
        assert name == "toc3d_linear_fused" and same(got, (L.F32X3WA, L.EPI_BIAS_RELU, 0, pin, 192, Wp, 192, b, hh, 1024, None, 0, 0, None, None, 6000, 1024, 192, 0, *plain, s))
        Wp2 = z(256, 1024)
        _, name, got = one("fp32x3", hh, (Wp2, b), pe, 6000, 256, 1024, f32_out=True, a_planes=False)      # position_encoder.2: 47 x 2 tiles, no residual -> 64x64
        assert name == "toc3d_linear_fused" and same(got, (L.F32X3W, L.EPI_RESIDUAL, 14, hh, 1024, Wp2, 1024, b, pe, 256, None, 0, 0, None, None, 6000, 256, 1024, 0, *plain, s))
        _, name, got = one("fp32x3", A, (W, b), out, 24, 128, 64, relu=False, a_planes=False)              # (neither flag: what EPI_BIAS took)
        assert name == "toc3d_linear_fused" and same(got, (L.F32X3W, L.EPI_BIAS, 14, A, 64, W, 64, b, out, 128, None, 0, 0, None, None, 24, 128, 64, 0, *plain, s))
    finally:
        lib.call = real_call
        lib.set_rec_lane(None)
