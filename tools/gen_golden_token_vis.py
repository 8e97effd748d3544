"""Generates the fixtures of the token selection overlays from the REAL reference: tests/golden/token_vis_cases.npz and token_vis_cases.json.

The reference's ``models/utils/token_select_vis.py`` is loaded where it lies, by file path, with a stand-in for the one import it cannot make here (``mmcv``):
``imwrite`` captures ``(file name, array)`` instead of encoding a file, and ``imdenormalize`` is the numpy restatement of tests/token_vis_cases.py.  Its own
``token_selection_vis`` then runs on the seeded inputs of ``token_vis_cases.CASES`` (torch tensors on the CPU): the repeats, the alpha arithmetic, the
concatenation, the order and the names of the files are the reference's.  Runs only where the reference tree exists; nothing of the reference is copied.

LIMITATION (written into the .json as well): OpenCV is not installed, so what ``cv2.multiply`` / ``cv2.add`` do in the last bit of a float32 image
(``imdenormalize``) and what ``cv2.imwrite`` does with a float array (taken to be saturate_cast<uchar>: round half to even, clip) are restated, not run.

Per case the archive holds the inputs (raw uint8 frames, the normalised float32 images, masks, index lists), per captured file the float32 array (an ``_ori``
file once per view: the generator asserts that the reference writes the same array for every stage) and its bytes; the .json the file names in the order written.
The archive is written with fixed zip timestamps, so a second run reproduces it byte for byte.
"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import token_vis_cases as TC                     # noqa: E402
from oracle import ref_harness as R              # noqa: E402
from tools.gen_golden_focal_head import save_npz  # noqa: E402

LIMITATION = ("OpenCV and mmcv are not installed where this was generated: mmcv.imdenormalize is the numpy float32 restatement (img * std, then + mean), and "
              "cv2.imwrite's conversion of a float array is taken to be round-half-to-even and clip; OpenCV's own last-bit behaviour for float input was not run")


def load(captured):
    """The reference's token_selection_vis, from the file where it lies, writing into ``captured``."""
    assert R.reference_available(), "the reference tree is needed"
    R._mod("mmcv", imwrite=lambda img, name: captured.append((name, np.array(img, copy=True))), imdenormalize=TC.imdenormalize)
    path = os.path.join(R.REF, "projects", "mmdet3d_plugin", "models", "utils", "token_select_vis.py")
    spec = importlib.util.spec_from_file_location("toc3d_reference_token_select_vis", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.token_selection_vis


def main():
    captured = []
    ref = load(captured)
    arrays, meta = {}, {}
    for case, c in TC.CASES.items():
        inp = TC.inputs(c, TC.case_seed(case))
        t = lambda a: None if a is None else [torch.from_numpy(x) for x in a]
        del captured[:]
        ref(torch.from_numpy(inp["img"]), t(inp["masks"]), t(inp["keeps"]), t(inp["drops"]), c["norm"], "out/", patch_size=c["patch"])
        names = [n for n, _ in captured]
        mine = TC.restated(inp["img"], inp["masks"], inp["keeps"], inp["drops"], c["norm"], c["patch"], prefix="out/")
        assert names == [n for n, _ in mine], (case, names)
        worst = 0
        arrays.update({f"{case}_in_raw": inp["raw"], f"{case}_in_img": inp["img"]})
        for l, m in enumerate(inp["masks"]):
            arrays[f"{case}_in_mask{l}"] = m
            if inp["keeps"] is not None:
                arrays[f"{case}_in_keep{l}"], arrays[f"{case}_in_drop{l}"] = inp["keeps"][l], inp["drops"][l]
        for (name, got), (_, want) in zip(captured, mine):
            assert got.dtype == np.float32 and got.shape == want.shape, (name, got.dtype, got.shape)
            worst = max(worst, int((got.view(np.int32) != want.view(np.int32)).sum()))
            base = os.path.basename(name)[:-4]
            if base.endswith("_ori"):
                base = base.split("_layer")[0] + "_ori"
                if f"{case}_f_{base}" in arrays:
                    assert np.array_equal(arrays[f"{case}_f_{base}"], got), "the same ori image for every stage"
                    continue
            arrays[f"{case}_f_{base}"], arrays[f"{case}_b_{base}"] = got, TC.to_bytes(got)
        u8 = TC.restated_u8(inp["raw"], inp["masks"], inp["keeps"], inp["drops"], c["norm"], c["patch"], prefix="out/")
        diff = sum(int((TC.to_bytes(a) != TC.to_bytes(b)).sum()) for (_, a), (_, b) in zip(u8, mine))
        print(f"case {case}: {len(names)} files, restatement differs in {worst} float32 values; the uint8 form differs in {diff} bytes")
        assert worst == 0 and diff == 0
        meta[case] = dict(files=[os.path.basename(n) for n in names], V=c["V"], raw=list(c["raw"]), grid=list(c["grid"]), patch=c["patch"],
                          K=None if c["K"] is None else list(c["K"]), norm=c["norm"])
    save_npz(TC.FIXTURE, **arrays)
    json.dump(dict(numpy=np.__version__, torch=torch.__version__, source="the reference's token_selection_vis (models/utils/token_select_vis.py), loaded with a stand-in "
                   "mmcv whose imwrite captures and whose imdenormalize is the numpy restatement", LIMITATION=LIMITATION, cases=meta), open(TC.FIXTURE_META, "w"), indent=1)
    for f in (TC.FIXTURE, TC.FIXTURE_META):
        print(f, os.path.getsize(f), "bytes")
        assert os.path.getsize(f) < 512 * 1024


if __name__ == "__main__":
    main()
