"""CPU: the C-ABI library loads without a GPU, exports every symbol include/toc3d.h declares, the ctypes
signatures agree with the header, and the host-side modules mirror the reference interface."""
import ctypes
import json
import os
import re

import pytest
import torch

import toc3d_amd
from support import OldLibrary, header_sigs
from toc3d_amd import configs, lib


def test_library_exports_every_declared_symbol():
    assert os.path.exists(lib.LIB_PATH), "build first: make -C toc3d_amd/csrc"
    dll = ctypes.CDLL(lib.LIB_PATH)
    names = lib.header_functions()
    assert len(names) >= 50
    for n in names:
        assert hasattr(dll, n), f"{n} declared in include/toc3d.h but not exported"
    l = lib.load()
    hdr = int(re.search(r"#define\s+TOC3D_ABI_VERSION\s+(\d+)", open(lib.HEADER_PATH).read()).group(1))
    assert l.toc3d_abi_version() == hdr == lib.ABI_VERSION
    assert l.toc3d_motion_weights_floats() > 500000


def test_ctypes_signatures_match_header():
    sigs = dict(lib._SIGS)
    seen = 0
    for name, sig in header_sigs(lib.header_text(), sigs).items():        # (toc3d_abi_version and the helpers bound by hand in lib.load() are not in the table)
        assert sigs[name] == sig, name
        seen += 1
    assert seen == len(sigs)
    assert lib.load().toc3d_window_topk_rows(6, 20, 50, 16, 128) == 6 * (3 * 129 + 33 + 3 * 65 + 9)


@pytest.mark.parametrize("key", list(lib.SIDES))
def test_side_header_table_and_binder_agree(key, monkeypatch):
    """What each side header's own file checks, once over lib.SIDES: no name in two tables, the header declares the table's names and its ABI symbol and nothing
    else, the parsed signatures are the table, and a library without the symbols is told to rebuild by the one binder, naming that header."""
    path, abi_fn, abi, sigs = lib.SIDES[key]
    assert abi_fn == f"toc3d_{key}_abi" and os.path.basename(path) == f"toc3d_{key}.h" and abi == getattr(lib, f"{key.upper()}_ABI")
    assert sigs is getattr(lib, f"_{key.upper()}_SIGS") and path == getattr(lib, f"{key.upper()}_HEADER_PATH") and sigs
    for other, row in lib.SIDES.items():
        assert other == key or not set(sigs) & set(row[3]), f"a name of {key} is also in {other}"
    assert not set(sigs) & set(lib._SIGS)
    assert all(lib._SIDE_OF[n] == key for n in sigs) and len(lib._SIDE_OF) == sum(len(row[3]) for row in lib.SIDES.values())
    txt = lib.header_text(path)
    assert set(re.findall(r"\b(toc3d_\w+)\s*\(", txt)) == set(sigs) | {abi_fn}
    assert header_sigs(txt, sigs) == sigs
    first = next(iter(sigs))
    monkeypatch.setattr(lib, "_lib", OldLibrary())
    with pytest.raises(RuntimeError, match=rf"reports {key} ABI None, this package binds {abi} \(include/toc3d_{key}\.h\): rebuild the library \(`make -C toc3d_amd/csrc`\)$"):
        lib.call(first, *[None] * len(sigs[first]))


def test_argument_validation_reports_errors_without_gpu():
    l = lib.load()
    rc = l.toc3d_linear(lib.BF16, 0, None, 0, None, 0, None, None, 0, None, 0, 0, None, None, 4, 4, 64, 0, None)
    assert rc == -1 and b"null buffer" in l.toc3d_last_error()
    with pytest.raises(RuntimeError, match="toc3d_rank_desc failed"):
        lib.call("toc3d_rank_desc", None, 1, 10, None, None)


def test_module_surface_matches_reference(golden_dir):
    spec = json.load(open(os.path.join(golden_dir, "state_dict_spec.json")))
    for name in ("toc3d_tiny", "eva_tiny"):
        m = toc3d_amd.build_backbone(configs.get(name))
        assert {k: list(v.shape) for k, v in m.state_dict().items()} == spec[name]
    m = toc3d_amd.build_backbone(configs.get("toc3d_tiny"))
    assert m.pruning_loc == [3, 6, 9] and m.pruning_num_queries == 64          # read by Petr3D (petr3d.py:73-74,123)
    assert set(toc3d_amd.BACKBONES.module_dict) >= {"ToC3DEVAViT", "EVA_ViT"} and "CPFPN" in toc3d_amd.NECKS.module_dict
    with pytest.raises(AssertionError):                                            # toc3d_eva_vit.py:141-142
        toc3d_amd.build_backbone(dict(configs.get("toc3d_tiny"), pruning_loc=[2, 6, 9]))
    with pytest.raises(NotImplementedError):
        toc3d_amd.build_backbone(dict(configs.get("toc3d_tiny"), use_rel_pos=True))
    n = toc3d_amd.build_neck(configs.CPFPN_TINY)
    assert list(n.state_dict()) == ["lateral_convs.0.conv.weight", "lateral_convs.0.conv.bias", "fpn_convs.0.conv.weight", "fpn_convs.0.conv.bias"]


def test_no_cpu_fallback():
    m = toc3d_amd.build_backbone(configs.get("eva_tiny"))
    with pytest.raises(RuntimeError, match="no CPU"):
        m(torch.zeros(2, 3, 320, 800))
    n = toc3d_amd.build_neck(configs.CPFPN_TINY)
    with pytest.raises(RuntimeError, match="no CPU"):
        n([torch.zeros(2, 128, 20, 50)])


def test_launch_plan_api_validates_without_gpu():
    """toc3d_plan_*: handles, lane handles and the recording state machine work (and fail loudly) without a GPU."""
    l = lib.load()
    h = ctypes.c_void_p()
    assert l.toc3d_plan_create(ctypes.addressof(h)) == 0 and h.value
    assert l.toc3d_plan_lane_stream(0) and l.toc3d_plan_lane_stream(3) and not l.toc3d_plan_lane_stream(64)
    assert l.toc3d_plan_num_launches(h.value) == 0
    assert l.toc3d_plan_wait(h.value, 1, 0) == -1 and b"not recording" in l.toc3d_last_error()
    assert l.toc3d_plan_run(h.value, None) == -1 and b"not finalized" in l.toc3d_last_error()
    assert l.toc3d_plan_begin(h.value) == 0
    h2 = ctypes.c_void_p()
    assert l.toc3d_plan_create(ctypes.addressof(h2)) == 0
    assert l.toc3d_plan_begin(h2.value) == -1 and b"already recording" in l.toc3d_last_error()
    assert l.toc3d_plan_wait(h.value, 1, 0) == 0 and l.toc3d_plan_wait(h.value, 1, 99) == -1
    assert l.toc3d_plan_end(h.value, 0) == -1 and b"nothing was recorded" in l.toc3d_last_error()
    assert l.toc3d_plan_destroy(h.value) == 0 and l.toc3d_plan_destroy(h2.value) == 0
    assert l.toc3d_plan_begin(None) == -1


def test_return_type_binds_to_the_plugin_class_when_the_plugin_is_imported():
    """petr3d.py:159 does isinstance(out, ToC3DViTReturnType) with the plugin's class (petr3d.py:17): once that module is in
    sys.modules the backbone returns the plugin's class, no manual re-binding."""
    import sys
    import types
    from toc3d_amd import backbone as bb
    name = "projects.mmdet3d_plugin.models.backbones.toc3d_utils"
    assert name not in sys.modules and bb._return_type() is bb.ToC3DViTReturnType

    class PluginReturnType:                                    # stands in for toc3d_utils.py:10-25 (same constructor signature)
        def __init__(self, img_feats=None, token_masks=None, attn_scores=None, keep_idx=None, drop_idx=None, aux_outputs=None):
            self.img_feats, self.token_masks, self.keep_idx, self.drop_idx = img_feats, token_masks, keep_idx, drop_idx
    mod = types.ModuleType(name)
    mod.ToC3DViTReturnType = PluginReturnType
    sys.modules[name] = mod
    try:
        assert bb._return_type() is PluginReturnType
        out = bb._return_type()({"last_feat": 1}, None, None, keep_idx=None, drop_idx=None, aux_outputs=None)
        assert isinstance(out, PluginReturnType) and out.img_feats == {"last_feat": 1}
    finally:
        del sys.modules[name]


def test_registration_on_an_mmcv_style_registry():
    """The HAVE_MMDET branch of toc3d_amd/registry.py: with mmdet.models.builder importable, the classes are registered on ITS
    registries under the reference's type names (force=True shadows the plugin's own registration) and built through them."""
    import importlib
    import sys
    import types

    class Registry:                                            # the slice of mmcv.utils.Registry the plugin relies on
        def __init__(self, name):
            self.name, self._module_dict = name, {}

        @property
        def module_dict(self):
            return self._module_dict

        def register_module(self, name=None, force=False, module=None):
            def _register(cls):
                key = name or cls.__name__
                if not force and key in self._module_dict:
                    raise KeyError(f"{key} is already registered in {self.name}")
                self._module_dict[key] = cls
                return cls
            return _register(module) if module is not None else _register

        def get(self, key):
            return self._module_dict.get(key)

        def build(self, cfg):
            cfg = dict(cfg)
            return self._module_dict[cfg.pop("type")](**cfg)

    class RefBackbone:                                         # what the plugin registered first
        pass
    fake = {n: types.ModuleType(n) for n in ("mmdet", "mmdet.models", "mmdet.models.builder")}
    fake["mmdet.models.builder"].BACKBONES, fake["mmdet.models.builder"].NECKS = Registry("backbone"), Registry("neck")
    fake["mmdet.models.builder"].BACKBONES.register_module(name="ToC3DEVAViT", module=RefBackbone)
    saved = {n: sys.modules.get(n) for n in fake}
    sys.modules.update(fake)
    from toc3d_amd import registry
    try:
        reg = importlib.reload(registry)
        assert reg.HAVE_MMDET and reg.BACKBONES is fake["mmdet.models.builder"].BACKBONES
        reg.register_all()
        assert reg.BACKBONES.get("ToC3DEVAViT") is toc3d_amd.ToC3DEVAViT and reg.BACKBONES.get("EVA_ViT") is toc3d_amd.EVA_ViT
        assert reg.NECKS.get("CPFPN") is toc3d_amd.CPFPN
        m = reg.build_backbone(configs.get("toc3d_tiny"), precision="fp32")
        assert isinstance(m, toc3d_amd.ToC3DEVAViT) and m.precision == "fp32"
        assert isinstance(reg.build_neck(configs.CPFPN_TINY), toc3d_amd.CPFPN)
    finally:
        for n, v in saved.items():
            if v is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = v
        importlib.reload(registry)
        registry.register_all()
    assert not registry.HAVE_MMDET


def test_copies_of_modules_drop_recorded_plans_and_packed_weights():
    """A LaunchPlan's launches carry baked device pointers of the module that recorded it: plans are not copyable, and copies /
    pickles of the modules start without plans, workspaces and packed weights (they re-pack and re-record)."""
    import copy
    import pickle

    from toc3d_amd.plan import LaunchPlan
    lp = LaunchPlan()
    with pytest.raises(TypeError):
        copy.deepcopy(lp)
    with pytest.raises(TypeError):
        copy.copy(lp)
    with pytest.raises(TypeError):
        pickle.dumps(lp)
    m = toc3d_amd.build_backbone(configs.get("toc3d_tiny"))
    m._plans = {"k": {"launch": {None: {"cplan": lp}}, "x": torch.zeros(2)}}
    m._packed = {"dev": "cuda", "blocks": [lp]}
    m._tuned[(0, 1, 2, 3)] = 16
    for c in (copy.deepcopy(m), pickle.loads(pickle.dumps(m))):
        assert c._plans == {} and c._packed is None and c._stream_pool == []
        assert c._tuned == {(0, 1, 2, 3): 16} and c.pruning_loc == m.pruning_loc
        assert all(torch.equal(a, b) for a, b in zip(c.state_dict().values(), m.state_dict().values()))
        assert c.blocks[0].attn.q_proj.weight.data_ptr() != m.blocks[0].attn.q_proj.weight.data_ptr()
    n = toc3d_amd.build_neck(configs.CPFPN_TINY)
    n._ws = {(1, 2, 3): {"launch": {7: {"cplan": lp}}}}
    n._packed = {"w": lp}
    c = copy.deepcopy(n)
    assert c._ws == {} and c._packed is None
    # weights arriving through a parent module (mmcv load_checkpoint on the detector) invalidate the neck's packed state too
    parent = torch.nn.Module()
    parent.neck = n
    parent.load_state_dict({"neck." + k: v for k, v in n.state_dict().items()})
    assert n._ws == {} and n._packed is None
    # the decoder and the head-token module keep the same protocol (toc3d_amd.plan.DerivedState): copies and pickles start without packed weights, workspaces,
    # recorded plans, streams and the capture instrument; configuration is copied
    from toc3d_amd import synth
    dec = toc3d_amd.build_transformer(synth.decoder_cfg(**synth.DECODER_TINY))
    tok = toc3d_amd.HeadTokenEmbedding(in_channels=64, embed_dims=64, depth_num=32)

    def plant(mod):
        mod._packed, mod._ws = {"w": lp}, {(1, 2, 3): {"buf": torch.zeros(2), "cplan": lp}}
        if mod is dec:
            dec._states, dec._pool, dec.capture = {(1, 2, 3, 0): {"cplan": lp, "warm": True}}, [lp], {"l0_norm0": torch.zeros(2)}
            dec._sk_ws, dec._sk_ws_old = {(0, 0): torch.zeros(2)}, [torch.zeros(2)]
    for mod in (dec, tok):
        plant(mod)
        for c in (copy.deepcopy(mod), pickle.loads(pickle.dumps(mod))):
            assert c._packed is None and c._ws == {} and c.precision == mod.precision
            assert all(torch.equal(a, b) and a.data_ptr() != b.data_ptr() for a, b in zip(c.state_dict().values(), mod.state_dict().values()))
            if mod is dec:
                assert c._states == {} and c._pool == [] and c.capture is None and c._sk_ws == {} and c._sk_ws_old == [] and c.launch_mode == dec.launch_mode
    assert dec._pool == [lp] and dec.capture is not None and tok._ws != {}, "the originals keep theirs"
    # new weights, loaded into the module itself, leave every derived attribute empty -- and keep what belongs to the instance (streams, the instrument)
    m._stream_pool, m._sk_ws, m._sk_ws_old = [lp], {(0, 0): torch.zeros(2)}, [torch.zeros(2)]
    n._ws, n._packed, n._stream_pool = {(1, 2, 3): {"launch": {7: {"cplan": lp}}}}, {"w": lp}, [lp]
    for mod in (m, n, dec, tok):
        mod.load_state_dict(mod.state_dict())
        assert mod._packed is None and all(getattr(mod, k) == empty for k, empty in type(mod)._DERIVED.items()), type(mod).__name__
    assert m._plans == {} and m._sk_ws == {} and m._sk_ws_old == [] and n._ws == {} and dec._ws == {} and dec._states == {} and dec._sk_ws == {} and tok._ws == {}
    assert m._stream_pool == [lp] and n._stream_pool == [lp] and dec._pool == [lp] and dec.capture is not None


def test_recording_lane_is_thread_local():
    """lib.stream_ptr() hands out lane handles only on the thread that records (the C side's recording flag is thread_local)."""
    import threading
    lib.set_rec_lane(2)
    try:
        assert lib.recording() and lib.stream_ptr() == lib.load().toc3d_plan_lane_stream(2)
        seen = {}
        t = threading.Thread(target=lambda: seen.update(rec=lib.recording(), lane=lib.rec_lane()))
        t.start(); t.join()
        assert seen == {"rec": False, "lane": None}
    finally:
        lib.set_rec_lane(None)
    assert not lib.recording()


def test_product_forward_has_no_test_switches():
    """forced_scores / block_hook live in toc3d_amd.testing (a test-only subclass), not in the product forward."""
    import inspect

    from toc3d_amd.backbone import ToC3DEVAViT
    from toc3d_amd.testing import InstrumentedToC3DEVAViT, instrument
    sig = inspect.signature(ToC3DEVAViT.forward)
    assert "forced_scores" not in sig.parameters and "gumbel_noise" in sig.parameters
    m = toc3d_amd.build_backbone(configs.get("toc3d_tiny"))
    assert not hasattr(m, "block_hook") and m._instrumented is False
    with pytest.raises(TypeError, match="test instrument"):
        ToC3DEVAViT.forward(m, torch.zeros(2, 3, 320, 800), forced_scores=[])
    im = instrument(m)
    assert im is m and isinstance(m, InstrumentedToC3DEVAViT) and m._instrumented is True and "forced_scores" in inspect.signature(type(m).forward).parameters


def test_launch_schedule_switches_are_attributes_not_environment():
    """The schedule switches of the product forward (toc3d_amd.backbone.schedule_defaults) are constructor kwargs / attributes with shipped defaults per
    precision; no module of the product package reads an environment variable to pick a code path (TOC3D_LIB, the library file name, is the one
    environment hook: it selects WHICH build is loaded, not what the host code does)."""
    from toc3d_amd.backbone import schedule_defaults
    assert set(schedule_defaults("bf16")) == {"carry_compact", "fold_ffn_ln", "fold_norm2", "gathered_residual", "prefetch_weights", "attn_rot", "side_lanes",
                                              "big_windows_first", "launch_mode", "gather_split", "x3_planes", "x3_attention"}
    d16, d32, dx3 = schedule_defaults("bf16"), schedule_defaults("fp32"), schedule_defaults("fp32x3")
    assert d16["fold_norm2"] and d16["carry_compact"] and d16["attn_rot"] and d16["prefetch_weights"] > 0
    assert not (d32["fold_ffn_ln"] or d32["fold_norm2"] or d32["carry_compact"] or d32["attn_rot"]), "the strict-parity path keeps the reference's sequence"
    assert dx3["fold_ffn_ln"] and dx3["fold_norm2"] and dx3["carry_compact"] and dx3["attn_rot"], "fp32x3: the folds, the carried compact set and (round 6) the pre-rotated attention on (hi, lo) planes"
    assert dx3["x3_planes"] and dx3["x3_attention"] and not (d16["x3_planes"] or d32["x3_planes"] or d16["x3_attention"] or d32["x3_attention"]), "(hi, lo) planes are the fp32x3 path's operand layout only"
    m = toc3d_amd.build_backbone(dict(configs.get("toc3d_tiny"), schedule=dict(fold_norm2=False, side_lanes=False)))
    assert m.fold_norm2 is False and m.side_lanes is False and m.fold_ffn_ln is True
    with pytest.raises(TypeError, match="unknown schedule"):
        toc3d_amd.build_backbone(dict(configs.get("toc3d_tiny"), schedule=dict(ln_self=True)))
    pkg = os.path.dirname(os.path.abspath(toc3d_amd.__file__))
    for fn in sorted(os.listdir(pkg)):
        if fn.endswith(".py"):
            src = open(os.path.join(pkg, fn)).read()
            reads = set(re.findall(r"environ[^\n]*?[\"'](TOC3D_\w+)[\"']", src))
            assert reads <= ({"TOC3D_LIB"} if fn == "lib.py" else set()), (fn, reads)


def test_frame_timeline_cuts_frames_and_counts_idle_time():
    """tools/frame_timeline.py (the tool behind profiles/r03_where_time_goes*.txt): frames are cut at the copy_segments launches, overlapping side-lane
    kernels do not count as idle time, mangled and plain kernel names land in one family, torch / runtime kernels are counted as foreign."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("frame_timeline", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "frame_timeline.py"))
    ft = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ft)
    g1 = "_ZN12_GLOBAL__N_111gemm_kernelIDF16bLi4ELi128ELi128ELi1ELi128ELi2ELi4ELi6ELi0EEEv8GemmArgs"
    g2 = "void (anonymous namespace)::gemm_kernel<__bf16, 5, 64, 64, 2, 128, 2, 2, 1, 0>(GemmArgs)"
    rows = []
    for f in range(3):
        t = f * 10000
        rows += [(t, t + 100, "(anonymous namespace)::copy_segments_kernel(void const*)", "0"), (t + 100, t + 1100, g1, "0"),
                 (t + 300, t + 900, "(anonymous namespace)::motion_queries_kernel<float>(int)", "3"),      # another stream, inside the GEMM: no idle time
                 (t + 1150, t + 2150, g2, "0"),                                                             # 50 ns gap
                 (t + 2150, t + 2200, "void at::native::vectorized_elementwise_kernel<4, at::native::FillFunctor<float>>(int)", "0")]
    frames = ft.cut_frames(list(reversed(rows)))
    assert len(frames) == 2                                                                                # the open last frame is dropped
    r = ft.summarize(frames[0])
    assert r["launches"] == 5 and r["span"] == 2200 and r["idle"] == 50 and r["foreign"] == 1
    assert r["families"]["gemm_kernel (all toc3d_linear* launches)"] == [2, 2000]
    assert r["families"]["motion_queries_kernel (side lane)"] == [1, 600]


def test_header_constants_match_the_python_binding():
    """dtype / epilogue codes of include/toc3d.h and their twins in toc3d_amd/lib.py (what the host passes through ctypes) and csrc/common.h (what the library
    compares against) are one table."""
    txt = open(lib.HEADER_PATH).read()
    hdr = {m[1]: int(m[2]) for m in re.finditer(r"#define\s+(TOC3D_(?:DTYPE|EPI)_\w+)\s+(\d+)\b", txt)}
    py = {"TOC3D_DTYPE_F32": lib.F32, "TOC3D_DTYPE_BF16": lib.BF16, "TOC3D_DTYPE_F32X3": lib.F32X3, "TOC3D_DTYPE_F32X6": lib.F32X6,
          "TOC3D_DTYPE_F32X3W": lib.F32X3W, "TOC3D_DTYPE_F32X3P": lib.F32X3P, "TOC3D_DTYPE_F32X3WO": lib.F32X3WO, "TOC3D_DTYPE_F32X3WA": lib.F32X3WA,
          "TOC3D_EPI_BIAS": lib.EPI_BIAS, "TOC3D_EPI_RESIDUAL": lib.EPI_RESIDUAL, "TOC3D_EPI_SWIGLU": lib.EPI_SWIGLU, "TOC3D_EPI_GELU": lib.EPI_GELU,
          "TOC3D_EPI_SWIGLU_STATS": lib.EPI_SWIGLU_STATS, "TOC3D_EPI_RESIDUAL_LN": lib.EPI_RESIDUAL_LN, "TOC3D_EPI_RESIDUAL_STATS": lib.EPI_RESIDUAL_STATS,
          "TOC3D_EPI_SWIGLU_STATS_LN": lib.EPI_SWIGLU_STATS_LN, "TOC3D_EPI_CONV3X3": lib.EPI_CONV3X3, "TOC3D_EPI_QKV_ROPE": lib.EPI_QKV_ROPE}
    for k, v in py.items():
        assert hdr.get(k) == v, (k, hdr.get(k), v)
    common = open(os.path.join(os.path.dirname(os.path.abspath(toc3d_amd.__file__)), "csrc", "common.h")).read()
    enum = dict((m[1], int(m[2])) for m in re.finditer(r"(TOC3D_(?:F32|BF16)\w*)\s*=\s*(\d+)", common))
    for k, v in py.items():
        if k.startswith("TOC3D_DTYPE_"):
            assert enum.get("TOC3D_" + k[len("TOC3D_DTYPE_"):]) == v, (k, enum)
    # the q scale of the pre-rotated attention path is the LIBRARY's convention (exp2-based softmax): the Python constant must be what it reports
    assert abs(lib.load().toc3d_attn_rot_q_scale(64) - lib.ATTN_ROT_Q_SCALE) < 1e-7 * lib.ATTN_ROT_Q_SCALE


def test_python_tile_table_matches_the_cpp_tile_table():
    """The GEMM tiles are one table on each side: TOC3D_GEMM_TILES in csrc/gemm_kernels.h (what the three dispatchers and the split-K workspace are generated
    from) and lib.TILES (what PRODUCT_VARIANTS and the tuner's geometric exclusions are read from).  The C++ rows are parsed out of the source, as the header's
    constants are above: same ids, shapes and family membership; what the C++ serves on planes only is inside X3_PLANES_ONLY_VARIANTS (which stays the wider,
    literal policy: it also holds 59); every tuning candidate names a tile its dtype's family has; the split-K ids the error text spells are the table's."""
    from toc3d_amd import gemm
    csrc = os.path.join(os.path.dirname(os.path.abspath(toc3d_amd.__file__)), "csrc")
    rows = [[f.strip() for f in m.group(1).split(",")] for m in re.finditer(r"\bROW\(\s*(\d+,[^)]*)\)", open(os.path.join(csrc, "gemm_kernels.h")).read())]
    assert len(rows) == 37 and all(len(r) == 14 for r in rows)
    cpp, planes_only = {}, set()
    for ident, bm, bn, stages, rb, wm, wn, form, main, _, xf, _, skf, _ in rows:
        bm, bn, rb, wm, wn = int(bm), int(bn), int(rb), int(wm), int(wn)
        assert form in ("F_RING", "F_PHASED", "F_PIPE") and main in ("S_ALL", "S_BF16") and xf in ("S_NONE", "S_X3", "S_X36") and skf in ("S_NONE", "S_SK", "S_SK_NOX")
        assert int(ident) not in cpp, f"tile {ident} has two rows"
        cpp[int(ident)] = (bm, bn, wm, wn, (main[2:], xf[2:], skf[2:]))
        partial_round = (bm * (rb // 16)) % (64 * wm * wn) != 0 or (bn * (rb // 16)) % (64 * wm * wn) != 0          # launch_cfg's rule: 96- / 160-row tiles
        if xf != "S_NONE" and (partial_round or form == "F_PHASED"):
            planes_only.add(int(ident))
    assert cpp == lib.TILES
    assert lib.PRODUCT_VARIANTS == tuple(sorted(cpp)) and all(0 < v < 100 for v in cpp)
    assert planes_only == {54, 55, 56, 57, 58, 60, 61, 62, 63} and planes_only <= set(lib.X3_PLANES_ONLY_VARIANTS)
    x3 = (lib.F32X3, lib.F32X3W, lib.F32X3P, lib.F32X3WO, lib.F32X3WA)
    assert set(gemm._VARIANTS) == {lib.BF16, lib.F32, lib.F32X6, *x3}
    for dt, cands in gemm._VARIANTS.items():
        for v in cands:
            assert lib.has_variant(v) and v < 400, (dt, v)
            main, xf, _ = lib.TILES[v % 100][4]
            # (F32X6 shares the bf16 x 3 tuple: the tiles only x3 has are refused by the library and drop out of the timing)
            assert dt == lib.BF16 or (main == "ALL" if dt == lib.F32 else xf != "NONE"), (dt, v)
            if v % 100 in planes_only:
                assert dt in (lib.BF16, lib.F32X3P), (dt, v)
    sk = sorted(v for v, t in lib.TILES.items() if t[4][2] != "NONE")
    assert gemm.SPLITK_VARIANT % 1000 in sk
    assert f"tile variants {', '.join(map(str, sk))})" in open(os.path.join(csrc, "gemm.hip")).read()
    L = lib.load()
    for v, (bm, bn, _, _, fam) in lib.TILES.items():
        assert L.toc3d_linear_splitk_workspace_bytes(2000 + v, 1, 1) == (65536 + 2 * bm * bn * 4 if fam[2] != "NONE" else -1), v


def test_backbone_survives_pickles_written_before_gumbel_seed_became_a_property():
    """a whole-module pickle from before the property carries `gumbel_seed` in __dict__ and no `_gumbel_seed`; reading the property then raised through
    nn.Module.__getattr__.  __setstate__ migrates the entry; the class carries defaults."""
    import copy
    import pickle
    m = toc3d_amd.build_backbone(dict(configs.get("toc3d_tiny")))
    m.gumbel_seed = 1234
    st = m.__getstate__()
    st["gumbel_seed"] = st.pop("_gumbel_seed")                 # the old layout
    del st["_forward_pre_hooks_with_kwargs"]                   # ... written by a torch that did not have this hook dictionary yet
    old = m.__class__.__new__(m.__class__)
    old.__setstate__(st)
    assert old.gumbel_seed == 1234 and "gumbel_seed" not in old.__dict__
    assert old._forward_pre_hooks_with_kwargs == {}, "nn.Module.__setstate__ back-fills what old pickles lack (ADVICE.md, fourth item)"
    assert pickle.loads(pickle.dumps(m)).gumbel_seed == 1234 and copy.deepcopy(m).gumbel_seed == 1234


def test_unchanged_reference_config_builds_the_parity_grade_precision():
    """A config without a `precision` key (a reference config dropped in unchanged) builds the path that meets the reference's 1e-3 tolerance, not the bf16
    headline path (INTEGRATION.md "Precision"); backbone and neck agree."""
    from toc3d_amd.backbone import DEFAULT_PRECISION
    assert DEFAULT_PRECISION == "fp32x3"
    for name in ("toc3d_tiny", "eva_tiny"):
        assert toc3d_amd.build_backbone(configs.get(name)).precision == "fp32x3"
        assert toc3d_amd.build_backbone(dict(configs.get(name), precision="bf16")).precision == "bf16"
    assert toc3d_amd.build_neck(configs.CPFPN_TINY).precision == "fp32x3"


def test_splitk_workspace_is_sized_from_the_launched_tile_shape():
    """toc3d_linear_splitk_workspace_bytes inferred (BM, BN) from BM * BN, which cannot tell variant 9's 128x64 tile from the 64x128 tile of
    variants 10 / 26 -- the host then counted too few tiles when N % 128 is in 1..64 and accepted a workspace the kernel writes past.  The size now comes from the launch
    table's own tile shape (csrc/gemm_kernels.h, sk_tile_dims): checked here for every split-K tile variant on shapes with ragged N, without a GPU (a host function)."""
    L = lib.load()
    dims = {1: (128, 128), 9: (128, 64), 10: (64, 128), 14: (64, 64), 16: (128, 128), 17: (128, 128), 19: (256, 128), 22: (128, 128), 26: (64, 128), 28: (128, 128),
            29: (128, 128), 55: (96, 128), 56: (96, 128)}
    for v, (bm, bn) in dims.items():
        for split in (2, 3, 4):
            for M, N in ((128, 192), (128, 64), (300, 1024), (6000, 1024), (97, 130)):
                tiles = -(-M // bm) * -(-N // bn)
                want = 65536 + tiles * split * bm * bn * 4
                got = L.toc3d_linear_splitk_workspace_bytes(1000 * split + v, M, N)
                assert got == want, (v, split, M, N, got, want)
    assert L.toc3d_linear_splitk_workspace_bytes(2060, 128, 128) < 0 and L.toc3d_linear_splitk_workspace_bytes(16, 128, 128) < 0      # no split-K form / not a split variant


def test_gemm_launcher_hands_the_library_its_arguments_in_header_order():
    """toc3d_amd.gemm.linear, the one launcher of the fused GEMM family: for every epilogue form the product uses, the exact positional tuple that reaches lib.call,
    written out in the order of include/toc3d.h.  The expected tuples are what the launcher this one replaced (backbone.tuned_linear with its ten-slot `fused=`
    tuple) passed for the same inputs -- recorded from that code, not from this one.  No device: lib.call is a recorder, the recording lane makes
    lib.stream_ptr() a lane handle and sends an untabled shape down the "first seen while recording" branch (variant 0, no timing, nothing tabled)."""
    import types

    from toc3d_amd import gemm
    L = lib
    z = torch.zeros
    A, W, bias, out, res, rep_out, act = z(4, 64), z(128, 64), z(128), z(4, 128), z(4, 128), z(2, 128), z(4, 128)
    rep_index, ridx, rc = (z(4, dtype=torch.int32) for _ in range(3))
    st, st2, c1, zeros, tab = z(64), z(64), z(128), z(256, dtype=torch.uint8), z(2, 2, 8, 16)
    calls = []
    real_call, lib.call = lib.call, lambda name, *a: calls.append((name, a))
    lib.set_rec_lane(1)

    def run(precision, epi, tuned=None, x3_planes=True, twice=False, **kw):
        owner = types.SimpleNamespace(_tuned=dict(tuned or {}), autotune=True, precision=precision, x3_planes=x3_planes)
        del calls[:]
        for _ in range(2 if twice else 1):
            gemm.linear(owner, epi, A, W, bias, out, 4, 128, 64, **kw)
        assert owner._tuned == (tuned or {})                        # nothing is tabled while recording; EPI_QKV_ROPE never records a key of its own
        for name, args in calls:
            assert len(args) == len(lib._SIGS[name]), name
        return owner, calls[0] if not twice else list(calls)
    try:
        stream = lib.stream_ptr()
        q = L.ATTN_ROT_Q_SCALE
        plain = (None, 0, None, 0, None, 0, 0.0, None, 0, None)      # the ten epilogue arguments at their neutral values
        same = lambda got, want: len(got) == len(want) and all(g is w if isinstance(w, torch.Tensor) else (g == w and type(g) is type(w)) for g, w in zip(got, want))

        def fused(got, *want):
            assert got[0] == "toc3d_linear_fused" and same(got[1], want + (stream,)), (got, want)

        def roped(got, *want):
            assert got[0] == "toc3d_linear_qkv_rope" and same(got[1], want + (stream,)), (got, want)
        fused(run("bf16", L.EPI_BIAS)[1], 1, 0, 0, A, 64, W, 64, bias, out, 128, None, 0, 0, None, None, 4, 128, 64, 0, *plain)
        fused(run("fp32", L.EPI_GELU)[1], 0, 3, 0, A, 64, W, 64, bias, out, 128, None, 0, 0, None, None, 4, 128, 64, 0, *plain)
        fused(run("fp32x6", L.EPI_RESIDUAL, residual=res, ldr=128, residual_row_mod=2)[1],
              3, 1, 0, A, 64, W, 64, bias, out, 128, res, 128, 2, None, None, 4, 128, 64, 0, *plain)
        fused(run("bf16", L.EPI_RESIDUAL, residual=res, ldr=128, rep_out=rep_out, rep_index=rep_index, residual_index=ridx)[1],
              1, 1, 0, A, 64, W, 64, bias, out, 128, res, 128, 0, rep_out, rep_index, 4, 128, 64, 0, None, 0, None, 0, None, 0, 0.0, None, 0, ridx)
        fused(run("bf16", L.EPI_SWIGLU, n_valid=50)[1], 1, 2, 0, A, 64, W, 64, bias, out, 128, None, 0, 0, None, None, 4, 128, 64, 50, *plain)
        fused(run("bf16", L.EPI_SWIGLU_STATS, n_valid=50, stats_out=(st, 2))[1],
              1, 4, 0, A, 64, W, 64, bias, out, 128, None, 0, 0, None, None, 4, 128, 64, 50, st, 2, None, 0, None, 0, 0.0, None, 0, None)
        fused(run("bf16", L.EPI_RESIDUAL_LN, residual=out, ldr=128, rep_out=rep_out, rep_index=rep_index, stats_in=(st, 2, 1), col_sums=c1, ln_n=50, ln_eps=1e-6)[1],
              1, 5, 0, A, 64, W, 64, bias, out, 128, out, 128, 0, rep_out, rep_index, 4, 128, 64, 0, None, 0, st, 4294967298, c1, 50, 1e-06, None, 0, None)
        fused(run("bf16", L.EPI_RESIDUAL_STATS, residual=res, ldr=128, rep_out=rep_out, rep_index=rep_index, stats_out=(st2, 2), out_act=act, ld_act=128, residual_index=ridx)[1],
              1, 6, 0, A, 64, W, 64, bias, out, 128, res, 128, 0, rep_out, rep_index, 4, 128, 64, 0, st2, 2, None, 0, None, 0, 0.0, act, 128, ridx)
        fused(run("bf16", L.EPI_SWIGLU_STATS_LN, n_valid=50, stats_out=(st, 2), stats_in=(st2, 2, 1), col_sums=c1, ln_n=64, ln_eps=1e-6)[1],
              1, 7, 0, A, 64, W, 64, bias, out, 128, None, 0, 0, None, None, 4, 128, 64, 50, st, 2, st2, 4294967298, c1, 64, 1e-06, None, 0, None)
        fused(run("bf16", L.EPI_CONV3X3, conv=(zeros, 2, 2))[1],
              1, 8, 0, A, 64, W, 64, bias, out, 128, None, 0, 0, None, None, 4, 128, 64, 0, None, 0, None, 0, None, 0, 0.0, zeros, 8589934594, None)
        # EPI_QKV_ROPE looks its tile up under the EPI_BIAS key
        roped(run("bf16", L.EPI_QKV_ROPE, tuned={(L.EPI_BIAS, 4, 128, 64): 14}, rope=(rc, tab, 8, q))[1],
              1, 14, A, 64, W, 64, bias, out, 128, 4, 128, 64, rc, tab, 8, 0.18033688011112042)
        # fp32x3 with the weights in planes (TOC3D_DTYPE_F32X3W): every (a_planes, o_planes) -> F32X3W / WO / WA / P; the rotating epilogue always writes planes
        for ap, op, dt, dt_rope in ((False, False, 4, 6), (False, True, 6, 6), (True, False, 7, 5), (True, True, 5, 5)):
            fused(run("fp32x3", L.EPI_BIAS, a_planes=ap, o_planes=op)[1], dt, 0, 0, A, 64, W, 64, bias, out, 128, None, 0, 0, None, None, 4, 128, 64, 0, *plain)
            roped(run("fp32x3", L.EPI_QKV_ROPE, a_planes=ap, o_planes=op, rope=(rc, tab, 8, q))[1],
                  dt_rope, 0, A, 64, W, 64, bias, out, 128, 4, 128, 64, rc, tab, 8, 0.18033688011112042)
        # ... and with x3_planes off the flags mean nothing: plain TOC3D_DTYPE_F32X3
        fused(run("fp32x3", L.EPI_BIAS, x3_planes=False, a_planes=True, o_planes=True)[1], 2, 0, 0, A, 64, W, 64, bias, out, 128, None, 0, 0, None, None, 4, 128, 64, 0, *plain)
        # a tabled variant; a variant the caller decides (the decoder) needs no table at all
        fused(run("bf16", L.EPI_RESIDUAL, tuned={(L.EPI_RESIDUAL, 4, 128, 64): 16}, residual=out, ldr=128)[1],
              1, 1, 16, A, 64, W, 64, bias, out, 128, out, 128, 0, None, None, 4, 128, 64, 0, *plain)
        fused(run("bf16", L.EPI_RESIDUAL, residual=out, ldr=128, variant=14)[1], 1, 1, 14, A, 64, W, 64, bias, out, 128, out, 128, 0, None, None, 4, 128, 64, 0, *plain)
        # a tabled split-K variant goes to toc3d_linear_fused_ws with a zeroed workspace of the size the library asks for, reused by the second launch
        owner, (c0, c1_) = run("bf16", L.EPI_RESIDUAL, tuned={(L.EPI_RESIDUAL, 4, 128, 64): 2014}, twice=True, residual=out, ldr=128)
        ws = c0[1][-3]
        assert lib.load().toc3d_linear_splitk_workspace_bytes(2014, 4, 128) == 131072
        assert ws.dtype == torch.int32 and ws.numel() * 4 == 131072 and not ws.any() and c1_[1][-3] is ws and owner._sk_ws == {(None, stream): ws}
        for c in (c0, c1_):
            assert c[0] == "toc3d_linear_fused_ws" and same(c[1], (1, 1, 2014, A, 64, W, 64, bias, out, 128, out, 128, 0, None, None, 4, 128, 64, 0, *plain, ws, 131072, stream))
    finally:
        lib.call = real_call
        lib.set_rec_lane(None)
