"""CPU: several camera streams per step without a GPU -- the header of the entry point it adds (include/toc3d_streams.h) against the ctypes table that binds it, with
include/toc3d.h, its two version numbers and lib._SIGS left where they were; every refusal of toc3d_score_head_frames on made-up host pointers (nothing is launched);
the per-sample form of the bank's ``backbone_queries`` as far as it goes without a device; and -- with the three parts replaced by recording fakes, as
tests/test_cpu_detector.py does -- the sequencing of ``Petr3D.simple_test_streams``: the lists handed to the backbone, the ``prev_exists`` tensor handed to the
head, when ``reset_memory`` is called, ``reset_streams`` and a change of B.  Every test prints the figures it asserts on (run with -s)."""
import ctypes
import re

import pytest
import torch
import torch.nn as nn

import toc3d_amd
from support import A, ERR_ARG, FakeNeck, OldLibrary, header_sigs, raw_call
from toc3d_amd import lib, synth

I31 = (1 << 31) - 1
NAME = "toc3d_score_head_frames"


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_streams_header_and_ctypes_table_agree():
    raw = open(lib.STREAMS_HEADER_PATH).read()
    found = header_sigs(lib.header_text(lib.STREAMS_HEADER_PATH), lib._STREAMS_SIGS)
    print(f"toc3d_streams.h declares {found}")
    assert found == lib._STREAMS_SIGS and list(found) == [NAME]
    assert int(re.search(r"#define\s+TOC3D_STREAMS_ABI\s+(\d+)", raw).group(1)) == lib.STREAMS_ABI == 1
    assert "backbones/toc3d_utils.py:110-129" in raw and ":255-273" in raw, "the header cites the reference lines it serves"
    dll = ctypes.CDLL(lib.LIB_PATH)
    assert hasattr(dll, NAME) and hasattr(dll, "toc3d_streams_abi")
    dll.toc3d_streams_abi.restype = ctypes.c_int
    assert dll.toc3d_streams_abi() == 1


def test_toc3d_h_and_its_table_are_where_they_were():
    raw = open(lib.HEADER_PATH).read()
    assert int(re.search(r"#define\s+TOC3D_ABI_VERSION\s+(\d+)", raw).group(1)) == lib.ABI_VERSION == 11
    assert int(re.search(r"#define\s+TOC3D_ABI_MINOR\s+(\d+)", raw).group(1)) == lib.ABI_MINOR == 1
    l = lib.load()
    l.toc3d_abi_minor.restype = ctypes.c_int
    assert l.toc3d_abi_version() == 11 and l.toc3d_abi_minor() == 1
    assert "toc3d_score_head_frames" not in raw and "toc3d_streams" not in raw
    assert not set(lib._STREAMS_SIGS) & set(lib._SIGS)
    assert header_sigs(lib.header_text(), lib._SIGS) == lib._SIGS, "lib._SIGS is include/toc3d.h one to one"
    print(f"toc3d.h: ABI {lib.ABI_VERSION}.{lib.ABI_MINOR}, {len(lib._SIGS)} signatures; toc3d_streams.h: {len(lib._STREAMS_SIGS)}")


def test_call_binds_the_entry_point_and_an_old_library_is_told_to_rebuild(monkeypatch):
    with pytest.raises(RuntimeError, match=r"toc3d_score_head_frames failed \(-1\).*null buffer"):
        lib.call(NAME, lib.F32, None, 64, 32, None, None, None, None, 74, 148, None, None, None, None)
    fn = getattr(lib.load(), NAME)
    assert fn.argtypes == [lib._CT[c] for c in lib._STREAMS_SIGS[NAME]], "bound with the table's argument types (int64 counts, not C ints)"

    monkeypatch.setattr(lib, "_lib", OldLibrary())
    with pytest.raises(RuntimeError, match="rebuild the library"):
        lib.call(NAME, lib.F32, A, 64, 32, A, A, None, A, 74, 148, A, A, A, None)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------------------
PTRS = ("f", "w", "b", "frame_new", "pred", "score", "mask_out")


def args(dtype=lib.F32, **o):
    a = dict({p: A for p in PTRS}, gumbel=None, ld=64, kdim=32, rpf=74, M=222)
    a.update(o)
    return (dtype, a["f"], a["ld"], a["kdim"], a["w"], a["b"], a["gumbel"], a["frame_new"], a["rpf"], a["M"], a["pred"], a["score"], a["mask_out"], None)


@pytest.mark.parametrize("dtype,over,reason", [
    *[(lib.F32, {p: None}, "null buffer") for p in PTRS],
    (lib.F32, dict(rpf=0), "rows_per_frame must be positive"), (lib.BF16, dict(rpf=-74), "rows_per_frame must be positive"),
    (lib.F32, dict(M=221), "multiple of rows_per_frame"), (lib.BF16, dict(M=75), "multiple of rows_per_frame"), (lib.F32, dict(M=73), "multiple of rows_per_frame"),
    (99, {}, "bad dtype"), (lib.F32X3, {}, "bad dtype"), (lib.F32X3P, {}, "bad dtype"),
    (lib.F32, dict(kdim=12), "multiples of 8"), (lib.F32, dict(ld=68), "multiples of 8"), (lib.BF16, dict(ld=24), "multiples of 8"),
    (lib.F32, dict(kdim=-8), "bad kdim"), (lib.BF16, dict(kdim=1 << 31, ld=1 << 31), "bad kdim"),
    (lib.F32, dict(f=A + 8), "16-byte aligned"), (lib.BF16, dict(f=A + 2), "16-byte aligned"),
    (lib.F32, dict(M=4 * I31 + 4, rpf=4), "too many rows"),
])
def test_score_head_frames_refusals(dtype, over, reason):
    rc, msg = raw_call(lib._STREAMS_SIGS, NAME, args(dtype, **over))
    print(f"{over or dtype}: rc {rc}, {msg!r}")
    assert rc == ERR_ARG and NAME in msg and reason in msg, (rc, msg)


def test_score_head_frames_empty_call_returns_before_the_launch():
    assert raw_call(lib._STREAMS_SIGS, NAME, args(M=0))[0] == 0 and raw_call(lib._STREAMS_SIGS, NAME, args(lib.BF16, M=-74))[0] == 0


# ---- sequencing, on recording fakes (the pattern of tests/test_cpu_detector.py) ----------------------------------------------------------------------------------
class FakeBackbone(nn.Module):
    pruning_loc, pruning_num_queries = [3, 6, 9], 64

    def __init__(self, log):
        super().__init__()
        self.log = log

    def forward(self, x, **kw):
        self.log.append(("backbone", tuple(x.shape), kw["prev_exists"], tuple(kw["temp_queries"].shape), tuple(kw["ego_pose_inv"].shape), kw.get("gumbel_noise")))
        feats = torch.zeros(x.shape[0], 8, 2, 5)
        return toc3d_amd.ToC3DViTReturnType({"last_feat": feats}, ["m0", "m1", "m2"], None, ["k0", "k1", "k2"], ["d0", "d1", "d2"])


class FakeHead(nn.Module):
    """The bank of the real head as far as the sequencing sees it: allocated for a batch size by ``forward``, gone after ``reset_memory``; the per-sample form of
    ``backbone_queries`` answers as ``TemporalMemory.backbone_queries`` does."""
    embed_dims = 256

    def __init__(self, log):
        super().__init__()
        self.log, self.bank, self.rows = log, None, {}

    def backbone_queries(self, n, prev_exists, batch_size=1):
        self.log.append(("queries", n, prev_exists, batch_size, self.bank))
        assert isinstance(prev_exists, list) and len(prev_exists) == batch_size
        if self.bank is not None:
            assert self.bank[1] == batch_size, "the bank is allocated per batch size: the detector resets it when B changes"
        flags = list(prev_exists) if self.bank is not None else [False] * batch_size
        return dict(temp_queries=torch.zeros(batch_size, n, 256), temp_ref_points=None, temp_timestamp=None, temp_ego_pose=None, temp_vel=None, prev_exists=flags)

    def img_feats_rows_buffer(self, B, N, h, w, device=None):
        return self.rows.setdefault((B, N, h, w), "rows(%d,%d,%d,%d)" % (B, N, h, w)), 64, lib.F32X3P

    def reset_memory(self):
        self.log.append(("reset",))
        self.bank = None

    def forward(self, memory_center, img_metas, topk_indexes=None, img_feats_rows=False, **data):
        self.log.append(("head", topk_indexes, img_feats_rows, sorted(data), data["prev_exists"].tolist(), tuple(data["img_feats"].shape), tuple(data["intrinsics"].shape),
                         tuple(data["timestamp"].shape), data["prev_exists"].dtype, len(img_metas)))
        self.bank = ("bank%d" % len(self.log), data["prev_exists"].shape[0])
        return dict(all_cls_scores="cls", all_bbox_preds="box", dn_mask_dict=None)

    def get_bboxes(self, outs, img_metas, rescale=False):
        self.log.append(("get_bboxes", outs["all_cls_scores"], len(img_metas)))
        return [[torch.zeros(3, 9), torch.arange(3.0) + b, torch.arange(3)] for b in range(len(img_metas))]


def step(det, log, scenes, noise=None):
    del log[:]
    B = len(scenes)
    metas = [dict(scene_token=s, pad_shape=[(32, 80, 3)]) for s in scenes]
    out = det.simple_test_streams(metas, gumbel_noise=noise, img=torch.zeros(B, 6, 3, 32, 80), intrinsics=torch.zeros(B, 6, 4, 4), lidar2img=torch.zeros(B, 6, 4, 4),
                                  timestamp=torch.zeros(B, dtype=torch.float64), ego_pose=torch.eye(4).repeat(B, 1, 1), ego_pose_inv=torch.eye(4).repeat(B, 1, 1))
    return out, [e[0] for e in log]


def test_sequencing_over_four_steps_of_two_streams_with_scene_changes_at_different_frames():
    det, log = toc3d_amd.build_detector(synth.detector_cfg(synth.DETECTOR_TINY)), []
    det.img_backbone, det.img_neck, det.pts_bbox_head = FakeBackbone(log), FakeNeck(log), FakeHead(log)
    # stream 0 changes scene at frame 3, stream 1 at frame 2 (synth.detector_stream_steps): all new, both continuing, mixed, mixed
    scenes = [("a", "a"), ("a", "a"), ("a", "b"), ("b", "b")]
    want = [[False, False], [True, True], [True, False], [False, True]]
    for f, (sc, prev) in enumerate(zip(scenes, want)):
        out, names = step(det, log, sc, "noise" if f == 1 else None)
        print(f"step {f}: scenes {sc} -> {names}, backbone got {log[names.index('backbone')][2]}, head got {log[-2][4]}")
        assert names == (["reset"] if f == 0 else []) + ["queries", "backbone", "neck", "head", "get_bboxes"], (f, names)
        q, bb, nk, hd = log[-5], log[-4], log[-3], log[-2]
        # the bank gets the host-side list, B = 2; the backbone gets the list the bank answers with: Python bools, one per stream, no tensor anywhere
        assert q[1:4] == (64, prev, 2) and all(type(p) is bool for p in q[2]) and (q[4] is not None) == (f > 0)
        assert bb[1] == (12, 3, 32, 80) and bb[2] == prev and type(bb[2]) is list and all(type(p) is bool for p in bb[2])
        assert bb[3] == (2, 64, 256) and bb[4] == (2, 4, 4) and bb[5] == ("noise" if f == 1 else None)
        # the neck fans out into the head's rows buffer of this (B, N, h, w); the head runs on the rows, with the (B,) f32 tensor of the same flags
        assert nk[1:] == ((12, 8, 2, 5), "rows(2,6,2,5)", 64, lib.F32X3P)
        assert hd[1] is None and hd[2] is True and hd[4] == [float(p) for p in prev] and hd[8] == torch.float32 and hd[9] == 2
        assert hd[5] == (2, 6, 4, 2, 5) and hd[6] == (2, 6, 4, 4) and hd[7] == (2,)
        assert hd[3] == sorted(["img", "img_feats", "intrinsics", "lidar2img", "timestamp", "ego_pose", "ego_pose_inv", "prev_exists"])
        assert det.prev_scene_tokens == list(sc)
        assert isinstance(out, list) and len(out) == 2 and all(list(o) == ["pts_bbox"] and set(o["pts_bbox"]) == {"boxes_3d", "scores_3d", "labels_3d"} for o in out)
        assert out[1]["pts_bbox"]["scores_3d"].tolist() == [1.0, 2.0, 3.0], "sample b's list at index b"
        assert det.last_frame["keep_idxes"] == ["k0", "k1", "k2"] and tuple(det.last_frame["img_feats"].shape) == (2, 6, 4, 2, 5)
    # reset_streams: the named stream's next step starts a scene whatever token it carries; the bank is NOT reset (the other stream continues)
    det.reset_streams([1])
    assert det.prev_scene_tokens == ["b", None]
    _, names = step(det, log, ("b", "b"))
    assert "reset" not in names and log[1][2] == [True, False] and log[-2][4] == [1.0, 0.0]
    _, names = step(det, log, ("b", "b"))
    assert "reset" not in names and log[1][2] == [True, True]
    # ... all streams forgotten: every stream is new, so the bank is reset
    det.reset_streams()
    _, names = step(det, log, ("b", "b"))
    assert names[0] == "reset" and log[2][2] == [False, False] and log[-2][4] == [0.0, 0.0]
    # a change of B restarts every stream, tokens that match the old step's included
    _, names = step(det, log, ("b", "b", "b"))
    print(f"B 2 -> 3: {names}, backbone got {log[2][2]}")
    assert names[0] == "reset" and log[2][2] == [False, False, False] and log[2][1] == (18, 3, 32, 80) and log[-2][4] == [0.0, 0.0, 0.0]
    _, names = step(det, log, ("b", "c", "b"))
    assert "reset" not in names and log[1][2] == [True, False, True]
    _, names = step(det, log, ("b",))
    assert names[0] == "reset" and log[2][2] == [False]
    # derived state: dropped with the weights and with a move, like prev_scene_token
    assert det.prev_scene_tokens == ["b"]
    det.to("cpu")
    assert det.prev_scene_tokens is None
    det.reset_streams([0])                                  # nothing to forget: no error
    # simple_test is what it was: one stream, a Python bool
    del log[:]
    FakeHead.backbone_queries = lambda self, n, prev_exists, batch_size=1: (self.log.append(("queries", prev_exists)), dict(
        temp_queries=torch.zeros(batch_size, n, 256), temp_ref_points=None, temp_timestamp=None, temp_ego_pose=None, temp_vel=None, prev_exists=False))[1]
    det.simple_test([dict(scene_token="z", pad_shape=[(32, 80, 3)])], img=torch.zeros(1, 6, 3, 32, 80), intrinsics=torch.zeros(1, 6, 4, 4), lidar2img=torch.zeros(1, 6, 4, 4),
                    timestamp=torch.zeros(1, dtype=torch.float64), ego_pose=torch.eye(4)[None], ego_pose_inv=torch.eye(4)[None])
    assert log[0] == ("queries", False) and [e[0] for e in log] == ["queries", "backbone", "neck", "reset", "head", "get_bboxes"] and det.prev_scene_token == "z"
