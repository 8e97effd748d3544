"""ctypes binding of ``libtoc3d_gfx950.so`` (the C ABI declared in ``include/toc3d.h``).

There is deliberately no fallback: if the shared library is missing the import of any compute entry
point raises, so a GPU box can never silently run a CPU / eager path.
"""
from __future__ import annotations

import ctypes
import os
import re
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, os.environ.get("TOC3D_LIB", "libtoc3d_gfx950.so"))       # TOC3D_LIB: a development build beside the shipped one (library A/B runs)
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "toc3d.h")

ABI_VERSION = 11                # == TOC3D_ABI_VERSION of include/toc3d.h (tests/test_cpu_abi.py cross-checks): moves on a changed or removed entry point
ABI_MINOR = 1                   # == TOC3D_ABI_MINOR: moves on an added entry point (1: toc3d_neck_rows_fanout); a library with a higher minor still binds
F32, BF16, F32X3, F32X6, F32X3W, F32X3P, F32X3WO, F32X3WA = 0, 1, 2, 3, 4, 5, 6, 7          # F32X3: linear layers only -- f32 buffers, products as three bf16 MFMAs (include/toc3d.h)
EPI_BIAS, EPI_RESIDUAL, EPI_SWIGLU, EPI_GELU, EPI_SWIGLU_STATS, EPI_RESIDUAL_LN, EPI_RESIDUAL_STATS, EPI_SWIGLU_STATS_LN, EPI_CONV3X3, EPI_QKV_ROPE = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9
EPI_BIAS_RELU = 10              # relu(A.W^T + bias): served wherever EPI_BIAS is (a new value of an existing argument: the ABI version does not move)
# q scale of the pre-rotated attention path (toc3d_linear_qkv_rope -> toc3d_window_attention_rot, head_dim 64): head_dim^-0.5 (eva_vit.py:104-109) times log2(e) --
# that kernel's softmax is exp2-based (include/toc3d.h), so the conversion factor rides on the multiply the epilogue does anyway
ATTN_ROT_Q_SCALE = 64 ** -0.5 * 1.4426950408889634
NO_FUSED = (None, 0, None, 0, None, 0, 0.0, None, 0, None)     # the ten extra arguments of toc3d_linear_fused for epilogues 0-3
# GEMM tiles: id -> (BM, BN, WM, WN, (bf16|f32, x3|x6, split-K family code)) -- the host's twin of the one tile table, TOC3D_GEMM_TILES in csrc/gemm_kernels.h (the
# family codes are that table's, without the S_ prefix; tests/test_cpu_abi.py parses the C++ rows and holds the two together).  A NEW TILE IS ONE NEW ROW HERE.
# The id is a variant mod 100: + 100 / 200 / 300 select the XCD order at run time, + 1000 * split the split-K form.
TILES = {
    1: (128, 128, 2, 2, ("ALL", "X36", "SK")),
    8: (128, 128, 2, 2, ("ALL", "X36", "NONE")),
    9: (128, 64, 2, 2, ("ALL", "X36", "SK")),
    10: (64, 128, 2, 2, ("ALL", "X36", "SK")),
    13: (128, 64, 2, 2, ("ALL", "NONE", "NONE")),
    14: (64, 64, 2, 2, ("ALL", "X36", "SK")),
    15: (128, 128, 2, 2, ("ALL", "NONE", "NONE")),
    16: (128, 128, 2, 4, ("ALL", "X36", "SK")),
    17: (128, 128, 2, 4, ("ALL", "X36", "SK")),
    19: (256, 128, 4, 2, ("ALL", "X36", "SK")),
    22: (128, 128, 2, 4, ("ALL", "X36", "SK")),
    24: (64, 128, 2, 4, ("ALL", "NONE", "NONE")),
    26: (64, 128, 2, 4, ("ALL", "X36", "SK")),
    27: (64, 64, 2, 2, ("ALL", "NONE", "NONE")),
    28: (128, 128, 2, 4, ("ALL", "X36", "SK")),
    29: (128, 128, 2, 4, ("ALL", "X3", "SK_NOX")),
    30: (128, 128, 2, 4, ("BF16", "NONE", "NONE")),
    33: (128, 64, 2, 4, ("ALL", "X3", "NONE")),
    45: (128, 192, 2, 4, ("ALL", "X3", "NONE")),
    47: (128, 192, 4, 2, ("ALL", "X3", "NONE")),
    49: (192, 128, 2, 4, ("ALL", "X36", "NONE")),
    51: (128, 128, 2, 4, ("ALL", "NONE", "NONE")),
    52: (192, 192, 2, 4, ("ALL", "X3", "NONE")),
    53: (192, 192, 2, 4, ("ALL", "X3", "NONE")),
    54: (96, 128, 2, 4, ("ALL", "X3", "NONE")),
    55: (96, 128, 2, 4, ("ALL", "X3", "SK_NOX")),
    56: (96, 128, 2, 4, ("ALL", "X3", "SK_NOX")),
    57: (160, 128, 2, 4, ("ALL", "X3", "NONE")),
    58: (160, 128, 2, 4, ("ALL", "X3", "NONE")),
    59: (192, 128, 2, 4, ("ALL", "X3", "NONE")),
    60: (256, 256, 2, 4, ("BF16", "X3", "NONE")),
    61: (256, 128, 4, 2, ("BF16", "X3", "NONE")),
    62: (128, 256, 2, 4, ("BF16", "X3", "NONE")),
    63: (128, 128, 2, 4, ("BF16", "X3", "NONE")),
    64: (128, 128, 2, 4, ("BF16", "NONE", "NONE")),
    65: (128, 128, 2, 4, ("BF16", "NONE", "NONE")),
    66: (128, 128, 2, 2, ("BF16", "NONE", "NONE")),
}
PRODUCT_VARIANTS = tuple(TILES)    # every tile the autotuner may pick or a shipped table names
# ... of which the tuner and the shipped tables treat the bf16 x 3 forms as existing only with BOTH operands as (hi, lo) planes (TOC3D_DTYPE_F32X3P / F32X3WA): the 96- / 160-row tiles and the phased big tiles
X3_PLANES_ONLY_VARIANTS = (54, 55, 56, 57, 58, 59, 60, 61, 62, 63)


def has_variant(v: int) -> bool:
    return (v % 100) in PRODUCT_VARIANTS

_P, _I64, _I, _F = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float

# name -> argtypes, in header order.  'p' pointer, 'l' int64, 'i' int, 'f' float
_SIGS = {
    "toc3d_linear": "iiplplpplpllppllllp",
    "toc3d_linear_ex": "iiiplplpplpllppllllp",
    "toc3d_linear_fused": "iiiplplpplpllppllll" + "plplplf" + "pl" + "p" + "p",
    "toc3d_linear_fused_ws": "iiiplplpplpllppllll" + "plplplf" + "pl" + "p" + "pl" + "p",
    "toc3d_pack_swiglu_lnfold": "ippppppllpppllp",
    "toc3d_pack_weight_lnfold": "ippppllpllppp",
    "toc3d_conv3x3_nhwc": "iiplplpplllllpp",
    "toc3d_pack_weight": "ipllpllp",
    "toc3d_x3_planes": "plplllp",
    "toc3d_pack_swiglu": "ippppllppllp",
    "toc3d_im2col_patches": "ippllllllp",
    "toc3d_normalize_images": "plllppipllp",
    "toc3d_im2col_patches_u8": "iplllppipllllp",
    "toc3d_abs_pos_bicubic": "pllpllp",
    "toc3d_layernorm_rows": "iplppppfplllp",
    "toc3d_layernorm_act": "iplppfplllp",
    "toc3d_window_map_dense": "llllppppp",
    "toc3d_window_attention": "iplplppppppllllpplpfp",
    "toc3d_window_attention_pf": "iplplppppppllllpplpf" + "lppl" + "p",
    "toc3d_rank_desc": "pllpp",
    "toc3d_window_topk": "plllllppppppppppppp",
    "toc3d_linear_qkv_rope": "iiplplppllllpplfp",
    "toc3d_window_attention_rot": "iplplppppppllllp" + "lppl" + "p",
    "toc3d_gather_merge_ln": "iplppppllllppfpplp",
    "toc3d_gather_merge_ln_ex": "iplppppllllppfppllp",
    "toc3d_gather_merge_ln_split": "iplppppllllppfppll" + "pll" + "p",
    "toc3d_scatter_update": "plpplllpppppp",
    "toc3d_rebase_layernorm_rows": "iplpppllppppfpllp",
    "toc3d_pack_motion_weights": "p" * 24 + "p",
    "toc3d_motion_queries": "pllppppippllpp",
    "toc3d_collapse_query_scorer": "ppppplllfppp",
    "toc3d_score_tokens": "plpppplllpppp",
    "toc3d_gumbel_noise": "plLpp",
    "toc3d_gumbel_from_bits": "plpp",
    "toc3d_global_mean_half": "ipllllp",
    "toc3d_score_head": "ipllppplpppp",
    "toc3d_nhwc_to_nchw": "pplllp",
    "toc3d_im2col_3x3": "ipplllllp",
    "toc3d_head_frustum_inputs": "ippppllllllllplplpp",
    "toc3d_relu_inplace": "iplp",
    "toc3d_nchw_to_rows": "ippllllp",
    "toc3d_mln_apply": "ipppllpplp",
    "toc3d_neck_rows_fanout": "iplppllllp",
    "toc3d_se_gate": "ppplp",
    "toc3d_memory_pre_update": "pppppppppplllllip",
    "toc3d_memory_scores": "pllpp",
    "toc3d_memory_post_update": "ppppppppppppplpppllllllp",
    "toc3d_mha_attention": "iplplplpllllllfp",
    "toc3d_mha_attention_ex": "iplplplplplplllllllfp",
    "toc3d_add_layernorm_pos": "iplppfplplplplppplllp",
    "toc3d_add_pos_rows": "iplplplplllp",
    "toc3d_head_nan_to_num_rows": "iplplplllp",
    "toc3d_head_ln_relu_rows": "iplppfpllllp",
    "toc3d_head_outputs": "plppfppppplpplplllllp",
    "toc3d_nms_free_decode": "plpllllllpifipppppp",
    "toc3d_head_query_inputs": "iplplplplppp" + "plplpl" + "pl" + "llll" + "p",
    "toc3d_head_query_combine": "plplplppf" + "pllpl" + "plpll" + "ppl" + "llll" + "p",
    "toc3d_copy_bytes": "pplp",
    "toc3d_copy_segments": "lpppp",
    "toc3d_plan_create": "p",
    "toc3d_plan_destroy": "p",
    "toc3d_plan_begin": "p",
    "toc3d_plan_wait": "pll",
    "toc3d_plan_end": "pi",
    "toc3d_plan_run": "pp",
}
_CT = {"p": _P, "l": _I64, "i": _I, "f": _F, "L": ctypes.c_uint64}
# include/toc3d_streams.h (several camera streams per step), in a table of its own: _SIGS is include/toc3d.h one to one, whose minor stays where the tests of
# the 11.1 surface pin it (the header folds into toc3d.h at 11.2).  Bound at first use (call()): a library built before the header existed lacks the symbols.
STREAMS_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "toc3d_streams.h")
STREAMS_ABI = 1                 # == TOC3D_STREAMS_ABI
_STREAMS_SIGS = {
    "toc3d_score_head_frames": "ipllppppllpppp",
}
# include/toc3d_focal.h (the 2-D auxiliary head, toc3d_amd.FocalHead): a side header as toc3d_streams.h is, for the same reason, bound the same way -- every side
# header is its path, its ABI number, its constants and its table here, and one row of SIDES below; nothing else is written per header
FOCAL_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "toc3d_focal.h")
FOCAL_ABI = 1                   # == TOC3D_FOCAL_ABI
_FOCAL_SIGS = {
    "toc3d_focal_gn_stats": "iplllllfpp",
    "toc3d_focal_heads": "iplppppppppllllplppppp",
}
# include/toc3d_sampled.h (the head's token side on FocalHead's sampled tokens, toc3d_amd.HeadTokenEmbedding(topk_indexes=...)): a side header likewise
SAMPLED_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "toc3d_sampled.h")
SAMPLED_ABI = 1                 # == TOC3D_SAMPLED_ABI
_SAMPLED_SIGS = {
    "toc3d_head_frustum_inputs_sampled": "ippppplllllllllplplpp",
    "toc3d_gather_token_rows": "iplpllllplp",
}
# include/toc3d_select.h (FocalHead's selection-only path, toc3d_amd.FocalHead.select_rows): a side header likewise
SELECT_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "toc3d_select.h")
SELECT_ABI = 1                  # == TOC3D_SELECT_ABI
_SELECT_SIGS = {
    "toc3d_focal_sample_weight": "iplpppppllllpp",
}
# include/toc3d_ingest.h (camera ingest: Pillow's resize and crop of raw uint8 frames, toc3d_amd.ResizeCropFlipRotImage): a side header likewise
INGEST_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "toc3d_ingest.h")
INGEST_ABI = 1                  # == TOC3D_INGEST_ABI
INGEST_TILE_W, INGEST_TILE_H, INGEST_LDS_ROWS, INGEST_MAX_KSIZE = 64, 32, 168, 32       # == TOC3D_INGEST_TILE_W, _TILE_H, _LDS_ROWS, _MAX_KSIZE
_INGEST_SIGS = {
    "toc3d_resize_crop_u8": "pllll" + "plll" + "ppl" + "ppl" + "l" + "p",
}
# include/toc3d_vis.h (token selection overlays: the reference's token_selection_vis as uint8 pixels, toc3d_amd.TokenVis): a side header likewise
VIS_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "toc3d_vis.h")
VIS_ABI = 1                     # == TOC3D_VIS_ABI
VIS_MAX_TOKENS = 8192           # == TOC3D_VIS_MAX_TOKENS
_CT["d"] = ctypes.c_double      # 'd' double: min_alpha / max_alpha, whose difference the entry point forms as Python does
_VIS_SIGS = {
    "toc3d_token_alpha": "ppllll" + "dd" + "pp" + "p",
    "toc3d_token_vis_render": "pil" + "llllll" + "pl" + "ffffff" + "i" + "pp" + "p",
}
# include/toc3d_boxes.h (predicted 3-D boxes drawn on the camera views and a top-down panel, toc3d_amd.BoxVis): a side header likewise
BOXES_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "toc3d_boxes.h")
BOXES_ABI = 1                   # == TOC3D_BOXES_ABI
BOXES_CAMERA_EDGES, BOXES_BEV_EDGES, BOXES_MAX_SIDE, BOXES_MAX_GUARD, BOXES_MAX_THICKNESS = 12, 5, 8192, 16, 15     # == TOC3D_BOXES_CAMERA_EDGES, ...
BOXES_TILE_W, BOXES_TILE_H = 64, 16                                                                                  # == TOC3D_BOXES_TILE_W, _TILE_H
_BOXES_SIGS = {
    "toc3d_box_segments": "plpplfl" + "plflll" + "l" + "ppp" + "p",
    "toc3d_box_segments_bev": "plpplfl" + "lfl" + "l" + "ppp" + "p",
    "toc3d_segments_render": "pil" + "lll" + "ffffff" + "i" + "iii" + "ppl" + "pl" + "ll" + "p" + "p",
}
# include/toc3d_results.h (decoded boxes to nuScenes submission records in the global frame, toc3d_amd.NuScenesResults): a side header likewise
RESULTS_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "toc3d_results.h")
RESULTS_ABI = 1                 # == TOC3D_RESULTS_ABI
RESULTS_MAX_BOXES, RESULTS_MAX_CLASSES, RESULTS_REC = 2048, 64, 12      # == TOC3D_RESULTS_MAX_BOXES, _MAX_CLASSES, _REC
_RESULTS_SIGS = {
    "toc3d_boxes_to_global": "pll" + "ppp" + "ll" + "i" + "p" + "ppp" + "l" + "d" + "pppppp" + "p",
}
# include/toc3d_tracks.h (greedy centre-distance tracking of the submission records, toc3d_amd.PubTracker): a side header likewise
TRACKS_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "toc3d_tracks.h")
TRACKS_ABI = 1                  # == TOC3D_TRACKS_ABI
TRACKS_MAX_TRACKS, TRACKS_MAX_BOXES, TRACKS_MAX_CLASSES, TRACKS_REC = 8192, 2048, 64, 12        # == TOC3D_TRACKS_MAX_TRACKS, _MAX_BOXES, _MAX_CLASSES, _REC
TRACKS_HEADER_BYTES, TRACKS_ROW_BYTES = 32, 48                                                   # == TOC3D_TRACKS_HEADER_BYTES, _ROW_BYTES
_TRACKS_SIGS = {
    "toc3d_tracks_state_bytes": "lp",
    "toc3d_tracks_step": "pppp" + "ll" + "pl" + "pl" + "d" + "l" + "pp" + "ppl" + "pppp" + "p",
}
# include/toc3d_assign.h (the tracking step with the reference's hungarian=True: scipy's solver replayed, toc3d_amd.HungarianPubTracker): a side header likewise
ASSIGN_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "toc3d_assign.h")
ASSIGN_ABI = 1                  # == TOC3D_ASSIGN_ABI
ASSIGN_MAX_BOXES, ASSIGN_MAX_TRACKS = 512, 2048                                                  # == TOC3D_ASSIGN_MAX_BOXES, _MAX_TRACKS
_ASSIGN_SIGS = {
    "toc3d_tracks_step_hungarian": "pppp" + "ll" + "pl" + "pl" + "d" + "l" + "pp" + "ppl" + "pppp" + "p" + "p",
}

# The side headers, one row each: key -> (header, the symbol that reports its ABI, the ABI this package binds, its signature table).  _bind_side() and call() read
# nothing else, so A NEW SIDE HEADER IS ONE NEW ROW HERE plus its constants above (tests/test_cpu_abi.py holds every row against its header).
SIDES = {
    "streams": (STREAMS_HEADER_PATH, "toc3d_streams_abi", STREAMS_ABI, _STREAMS_SIGS),
    "focal": (FOCAL_HEADER_PATH, "toc3d_focal_abi", FOCAL_ABI, _FOCAL_SIGS),
    "sampled": (SAMPLED_HEADER_PATH, "toc3d_sampled_abi", SAMPLED_ABI, _SAMPLED_SIGS),
    "select": (SELECT_HEADER_PATH, "toc3d_select_abi", SELECT_ABI, _SELECT_SIGS),
    "ingest": (INGEST_HEADER_PATH, "toc3d_ingest_abi", INGEST_ABI, _INGEST_SIGS),
    "vis": (VIS_HEADER_PATH, "toc3d_vis_abi", VIS_ABI, _VIS_SIGS),
    "boxes": (BOXES_HEADER_PATH, "toc3d_boxes_abi", BOXES_ABI, _BOXES_SIGS),
    "results": (RESULTS_HEADER_PATH, "toc3d_results_abi", RESULTS_ABI, _RESULTS_SIGS),
    "tracks": (TRACKS_HEADER_PATH, "toc3d_tracks_abi", TRACKS_ABI, _TRACKS_SIGS),
    "assign": (ASSIGN_HEADER_PATH, "toc3d_assign_abi", ASSIGN_ABI, _ASSIGN_SIGS),
}
_SIDE_OF = {name: key for key, row in SIDES.items() for name in row[3]}       # entry point -> its side: call()'s one lookup

_lib = None


def header_text(path: str = HEADER_PATH) -> str:
    """include/toc3d.h (or another header of the library) without comments."""
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def header_functions():
    """Names of all functions declared in include/toc3d.h (used by the symbol-export test)."""
    return sorted(set(re.findall(r"\b(toc3d_\w+)\s*\(", header_text())))


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: the HIP extension is not built. Run `make -C toc3d_amd/csrc` "
            "(or `python -c 'import __graft_entry__ as g; g.build()'`). There is no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    try:
        lib.toc3d_abi_version.restype = _I
        abi = lib.toc3d_abi_version()
    except AttributeError:
        abi = None
    try:
        lib.toc3d_abi_minor.restype = _I
        minor = lib.toc3d_abi_minor()
    except AttributeError:
        minor = None                # a build from before the minor existed: it lacks the entry points added since
    if abi != ABI_VERSION or minor is None or minor < ABI_MINOR:
        # checked BEFORE any symbol is bound: an older build (TOC3D_LIB) fails here with a message, not with a bare
        # AttributeError on the first entry point it lacks
        raise RuntimeError(f"{LIB_PATH} reports ABI version {abi}.{'?' if minor is None else minor}, this package binds ABI {ABI_VERSION}.{ABI_MINOR} "
                           "(include/toc3d.h): rebuild the library (`make -C toc3d_amd/csrc`)")
    lib.toc3d_last_error.restype = ctypes.c_char_p
    lib.toc3d_attn_rot_q_scale.restype = _F
    lib.toc3d_attn_rot_q_scale.argtypes = [_I64]
    lib.toc3d_motion_weights_floats.restype = _I64
    lib.toc3d_window_topk_rows.restype = _I64
    lib.toc3d_window_topk_rows.argtypes = [_I64] * 5
    lib.toc3d_linear_splitk_workspace_bytes.restype = _I64
    lib.toc3d_linear_splitk_workspace_bytes.argtypes = [_I, _I64, _I64]
    lib.toc3d_gather_merge_ln_scratch_bytes.restype = _I64
    lib.toc3d_gather_merge_ln_scratch_bytes.argtypes = [_I64, _I64]
    lib.toc3d_plan_lane_stream.restype = _P
    lib.toc3d_plan_lane_stream.argtypes = [_I64]
    lib.toc3d_plan_num_launches.restype = _I64
    lib.toc3d_plan_num_launches.argtypes = [_P]
    for name, sig in _SIGS.items():
        fn = getattr(lib, name)
        fn.restype = _I
        fn.argtypes = [_CT[c] for c in sig]
    _lib = lib
    return lib


def _conv(a):
    import torch
    if a is None:
        return None
    if isinstance(a, torch.Tensor):
        return a.data_ptr()
    return a


def _bind_side(lib, key):
    """The entry points of one side header (a row of SIDES), bound when the first of them is called.  The mark is left on the library object: another object in its
    place (an older build) is asked for its own toc3d_<key>_abi."""
    path, abi_fn, want, sigs = SIDES[key]
    try:
        getattr(lib, abi_fn).restype = _I
        abi = getattr(lib, abi_fn)()
        fns = {name: getattr(lib, name) for name in sigs}
    except AttributeError:
        abi, fns = None, {}
    if abi != want:
        raise RuntimeError(f"{LIB_PATH} reports {key} ABI {abi}, this package binds {want} (include/{os.path.basename(path)}): "
                           "rebuild the library (`make -C toc3d_amd/csrc`)")
    for name, fn in fns.items():
        fn.restype = _I
        fn.argtypes = [_CT[c] for c in sigs[name]]
    setattr(lib, f"_toc3d_{key}_bound", True)


def call(name: str, *args):
    """Invoke a C-ABI entry point; tensors are passed as device pointers; raises on a non-zero return."""
    lib = load()
    key = _SIDE_OF.get(name)
    if key is not None and not getattr(lib, f"_toc3d_{key}_bound", False):
        _bind_side(lib, key)
    rc = getattr(lib, name)(*[_conv(a) for a in args])
    if rc != 0:
        raise RuntimeError(f"{name} failed ({rc}): {lib.toc3d_last_error().decode()}")


def ptr_arrays(tensors, min_len=0):
    """(void* [n], int64 [n]): the device pointers and byte counts of ``tensors``, as the ABI's pointer-list arguments take them (n >= min_len, zero filled)."""
    n = max(min_len, len(tensors))
    return (ctypes.c_void_p * n)(*[t.data_ptr() for t in tensors]), (ctypes.c_int64 * n)(*[t.numel() * t.element_size() for t in tensors])


def copy_segments(pairs, stream):
    """[(dst tensor, src tensor), ...] (same byte sizes) staged with one toc3d_copy_segments launch per 16 pairs."""
    for i in range(0, len(pairs), 16):
        chunk = pairs[i:i + 16]
        d, b = ptr_arrays([t for t, _ in chunk])
        s, _ = ptr_arrays([t for _, t in chunk])
        call("toc3d_copy_segments", len(chunk), d, s, b, stream)


# Lane of the launch plan being recorded by THIS thread (toc3d_amd/plan.py); None = launch on torch's current stream.  Thread-local
# like the C side's recording flag (csrc/plan.cpp, toc3d_tls_recording): another Python thread that calls a toc3d op while this one
# records must get a real stream, not a lane handle the C side would not recognise for that thread.
_tls = threading.local()


def rec_lane():
    return getattr(_tls, "lane", None)


def set_rec_lane(lane):
    _tls.lane = lane


def stream_ptr():
    """The `stream` argument of a C-ABI call: torch's current HIP stream, or -- while a launch plan is being recorded by this
    thread -- the handle of the current lane (include/toc3d.h, toc3d_plan_lane_stream)."""
    lane = rec_lane()
    if lane is not None:
        return load().toc3d_plan_lane_stream(lane)
    import torch
    return torch.cuda.current_stream().cuda_stream


def recording() -> bool:
    return rec_lane() is not None
