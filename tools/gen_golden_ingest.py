"""Generates the fixtures of the camera ingest from the REAL reference: tests/golden/ingest_cases.npz and ingest_cases.json (the Pillow version they hold).

The reference's ``datasets/pipelines/transform_3d.py`` is loaded where it lies, by file path, with stand-ins for the two imports it makes at top level and never
uses at eval (``mmcv``; ``mmdet.datasets.builder.PIPELINES``, an ``oracle.ref_harness._Registry``), and its own ``ResizeCropFlipRotImage(data_aug_conf,
training=False)`` is called on the seeded frames and cameras of tests/ingest_cases.py: Pillow does the resize and the crop, the class its own geometry and camera
update.  Runs only where the reference tree and Pillow exist; nothing of the reference is copied.  Per case and form the archive holds the output images (uint8),
the intrinsics after the update and ``lidar2img`` (the reference's own dtypes), the 3 x 3 matrix ``_img_transform`` returned, and the geometry
``_sample_augmentation`` returned; the inputs are regenerated from seeds by the tests and stored as well (they are small).

The geometry is also checked against the hand-checked table ``ingest_cases.CASES``, and the numpy restatement against the images: zero differing bytes.

The archive is written with fixed zip timestamps, so a second run reproduces it byte for byte.
"""
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ingest_cases as IC                        # noqa: E402
from oracle import ref_harness as R              # noqa: E402
from tools.gen_golden_focal_head import save_npz  # noqa: E402


def load():
    """The reference's ResizeCropFlipRotImage, from the file where it lies."""
    assert R.reference_available(), "the reference tree is needed"
    R._mod("mmcv")
    R._mod("mmdet")
    R._mod("mmdet.datasets")
    R._mod("mmdet.datasets.builder", PIPELINES=R._Registry())
    path = os.path.join(R.REF, "projects", "mmdet3d_plugin", "datasets", "pipelines", "transform_3d.py")
    spec = importlib.util.spec_from_file_location("toc3d_reference_transform_3d", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.ResizeCropFlipRotImage


def main():
    import PIL
    Ref = load()
    arrays = {}
    for case, c in IC.CASES.items():
        conf = IC.case_conf(case)
        ref = Ref(data_aug_conf=conf, training=False)
        resize, resize_dims, crop, flip, rotate = ref._sample_augmentation()
        assert (tuple(resize_dims), tuple(crop), flip, rotate) == (c["resize_dims"], c["crop"], False, 0), (case, resize_dims, crop)
        for form in IC.FORMS:
            img = IC.frames(case, form)
            V = len(img)
            K, E = IC.cameras(case, form, V)
            results = dict(img=[f for f in img], intrinsics=[k.copy() for k in K], extrinsics=[e.copy() for e in E])
            out = ref(results)
            got = np.stack(out["img"])
            assert got.dtype == np.float32 and got.shape == (V,) + tuple(c["final_dim"]) + (3,) and np.array_equal(got, np.round(got)), "integer-valued float32 HWC"
            u8 = got.astype(np.uint8)
            _, ida = ref._img_transform(PIL.Image.fromarray(img[0]), resize=resize, resize_dims=resize_dims, crop=crop, flip=flip, rotate=rotate)
            diff = int((IC.restated_case(conf, img) != u8).sum())
            print(f"case {case} {form}: {img.shape} -> {u8.shape}, resize {resize}, dims {resize_dims}, crop {crop}; restatement differs in {diff} bytes; "
                  f"intrinsics {out['intrinsics'][0].dtype}, lidar2img {out['lidar2img'][0].dtype}")
            assert diff == 0
            tag = f"{case}_{form}_"
            arrays.update({tag + "input": img, tag + "image": u8, tag + "intrinsics_in": K, tag + "extrinsics": E,
                           tag + "intrinsics_out": np.stack(out["intrinsics"]), tag + "lidar2img": np.stack(out["lidar2img"]), tag + "ida_mat": ida.numpy(),
                           tag + "resize": np.array(resize), tag + "resize_dims": np.array(resize_dims), tag + "crop": np.array(crop)})
    save_npz(IC.FIXTURE, **arrays)
    json.dump(dict(pillow=PIL.__version__, numpy=np.__version__, source="the reference's ResizeCropFlipRotImage(training=False), loaded with stand-ins for mmcv and "
                   "mmdet.datasets.builder.PIPELINES", cases={k: dict(v, final_dim=list(v["final_dim"])) for k, v in IC.CASES.items()}),
              open(IC.FIXTURE_META, "w"), indent=1)
    for f in (IC.FIXTURE, IC.FIXTURE_META):
        print(f, os.path.getsize(f), "bytes")
        assert os.path.getsize(f) < 1 << 20


if __name__ == "__main__":
    main()
