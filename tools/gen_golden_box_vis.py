"""Generates the corner fixture of the box overlays from the REAL reference: tests/golden/box_vis_cases.npz.

The vendored mmdet3d's ``core/bbox/structures/utils.py`` (``rotation_3d_in_axis``, :79-106) and ``lidar_box3d.py`` (``LiDARInstance3DBoxes.corners``, :50-90) are
loaded where they lie, by file path, with stand-ins for what they import and do not use here: ``mmdet3d.core.utils.array_converter`` (a decorator that converts
numpy arguments; the tensors handed over need none), ``mmdet3d.core.points.BasePoints`` (only named in ``isinstance`` checks of other methods) and
``.base_box3d.BaseInstance3DBoxes``, of which ``corners`` uses ``tensor``, ``dims`` and ``YAW_AXIS`` -- those three are what the stand-in has.  The property then
runs on the float64 boxes of ``box_vis_cases.geometry_case`` and ``big_case``: the offsets, their order, the rotation and the sum are the reference's.  Runs only
where the reference tree exists; nothing of the reference is copied.

The archive holds, per case, the boxes (float64 of the float32 rows) and the corners (n, 8, 3) in float64; tests/test_cpu_box_vis.py holds the restatement of
tests/box_vis_cases.py to it.  Written with fixed zip timestamps, so a second run reproduces it byte for byte.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import box_vis_cases as BC                       # noqa: E402
from oracle import ref_harness as R              # noqa: E402
from tools.gen_golden_focal_head import save_npz  # noqa: E402

PKG = "toc3d_reference_structures"


def _from_file(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load():
    """The reference's LiDARInstance3DBoxes class, from the files where they lie."""
    assert R.reference_available(), "the reference tree is needed"
    sys.dont_write_bytecode = True               # the reference tree is read-only
    here = os.path.join(R.REF, "mmdetection3d", "mmdet3d", "core", "bbox", "structures")
    for name in ("mmdet3d", "mmdet3d.core"):
        if name not in sys.modules:
            R._mod(name)
    R._mod("mmdet3d.core.utils", array_converter=lambda **kw: (lambda fn: fn))
    R._mod("mmdet3d.core.points", BasePoints=type("BasePoints", (), {}))

    class BaseInstance3DBoxes:                   # what `corners` uses of the base class (base_box3d.py): the tensor, its dims columns, the yaw axis
        YAW_AXIS = 2

        def __init__(self, tensor):
            self.tensor = tensor

        @property
        def dims(self):
            return self.tensor[:, 3:6]
    pkg = R._mod(PKG)
    pkg.__path__ = []
    R._mod(PKG + ".base_box3d", BaseInstance3DBoxes=BaseInstance3DBoxes)
    _from_file(PKG + ".utils", os.path.join(here, "utils.py"))
    return _from_file(PKG + ".lidar_box3d", os.path.join(here, "lidar_box3d.py")).LiDARInstance3DBoxes


def main():
    cls = load()
    arrays = {}
    for name in ("hand", "random_a", "random_b", "big"):
        boxes = (BC.big_case() if name == "big" else BC.geometry_case(name))["boxes"].astype(np.float64)
        got = cls(torch.from_numpy(boxes)).corners.numpy()
        mine = BC.corners64(boxes)
        ok = np.isfinite(got).all(axis=(1, 2))
        assert got.shape == mine.shape == (len(boxes), 8, 3) and np.array_equal(ok, np.isfinite(mine).all(axis=(1, 2)))
        worst = float(np.abs(got[ok] - mine[ok]).max())
        print(f"case {name}: {len(boxes)} boxes ({int((~ok).sum())} not finite), the restatement differs from the reference's corners by at most {worst:.2e}")
        assert worst < 1e-12
        arrays[f"{name}_boxes"], arrays[f"{name}_corners"] = boxes, got
    assert cls(torch.zeros(0, 9, dtype=torch.float64)).corners.shape == (0, 8, 3)
    save_npz(BC.FIXTURE, **arrays)
    print(f"wrote {BC.FIXTURE}: {os.path.getsize(BC.FIXTURE)} bytes")


if __name__ == "__main__":
    main()
