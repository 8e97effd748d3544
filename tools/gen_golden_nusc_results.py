"""Generates tests/golden/nusc_results_cases.npz: per case of tests/nusc_results_cases.py the seeded inputs and the expected outputs of toc3d_boxes_to_global.

WHERE THE EXPECTED OUTPUTS COME FROM.  The reference's own route -- output_to_nusc_box and lidar_nusc_box_to_global of the vendored mmdet3d
(mmdet3d/datasets/nuscenes_dataset.py:576-657) -- needs pyquaternion and the nuScenes devkit (nuscenes.utils.data_classes.Box).  This tool tries to import
both.  Where they are missing (they were where the committed fixture was made) the outputs are the float64 restatement of tests/nusc_results_cases.py, written
from those lines, and the archive says so in ``generated_by``.  Where they import, the same loop runs on their objects (:func:`from_devkit`), the restatement is
held to it within its own bound, and the archive holds the devkit's numbers.  THAT SECOND BRANCH HAS NOT BEEN RUN YET: whoever runs this tool where the packages
exist should read its printout before committing the new archive.

Written with fixed zip timestamps, so a second run reproduces the archive byte for byte.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nusc_results_cases as NC                  # noqa: E402
from tools.gen_golden_focal_head import save_npz  # noqa: E402


def devkit():
    try:
        import pyquaternion
        from nuscenes.utils.data_classes import Box
    except ImportError:
        return None
    return pyquaternion.Quaternion, Box


def from_devkit(Quaternion, Box, c, restated):
    """The records of the boxes the restatement kept, through pyquaternion and the devkit's Box: Quaternion(axis, radians), rotate, translate, rotate, translate."""
    rec = np.zeros_like(restated["rec"])
    for b in range(rec.shape[0]):
        p = c["poses"][b]
        for k in range(int(restated["kept"][b])):
            row = c["boxes"][b, restated["src"][b, k]]
            zg = np.float32(row[2]) + np.float32(row[5]) * np.float32(0.5)
            vel = (float(row[7]), float(row[8]), 0.0) if c["with_velocity"] else (0.0, 0.0, 0.0)
            box = Box([float(row[0]), float(row[1]), float(zg)], [float(row[4]), float(row[3]), float(row[5])], Quaternion(axis=[0, 0, 1], radians=float(row[6])),
                      velocity=vel)
            box.rotate(Quaternion(p[0, :4]))
            box.translate(p[0, 4:])
            box.rotate(Quaternion(p[1, :4]))
            box.translate(p[1, 4:])
            rec[b, k] = (*box.center, *box.wlh, *box.orientation.elements, *box.velocity[:2])
    return rec


def main():
    arrays = NC.fixture_arrays()
    kit = devkit()
    if kit is None:
        arrays["generated_by"] = np.array("restatement: pyquaternion and the nuScenes devkit are not importable here")
        print("pyquaternion / nuscenes are not importable: the expected outputs are the restatement's")
    else:
        for name in NC.CASES:
            c = NC.build_case(name)
            restated = NC.restate(c["boxes"], c["scores"], c["labels"], c["counts"], c["poses"], c["with_velocity"])
            rec = from_devkit(*kit, c, restated)
            bound = restated["bound"] + 1e-15                # (the devkit normalises the pose again and multiplies two 4 x 4 matrices: a few more roundings)
            worst = float((np.abs(rec - restated["rec"]) / bound).max()) if rec.size else 0.0
            print(f"case {name}: the restatement is within {worst:.3f} of its bound of the devkit's records")
            assert worst <= 4.0, name
            arrays[f"{name}_rec"] = rec
        arrays["generated_by"] = np.array("pyquaternion and the nuScenes devkit")
    total = kept = 0
    for name in NC.CASES:
        total, kept = total + int(arrays[f"{name}_counts"].sum()), kept + int(arrays[f"{name}_kept"].sum())
    save_npz(NC.FIXTURE, **arrays)
    print(f"wrote {NC.FIXTURE}: {len(NC.CASES)} cases, {total} boxes of which {kept} are kept, {os.path.getsize(NC.FIXTURE)} bytes")


if __name__ == "__main__":
    main()
