"""Writes tests/golden/trivial_augment.npz: the inputs of tests/test_trivial_augment.py (a few images of at most 40
pixels a side), the (image, op, bin, sign, flip) entries and what Pillow makes of each.  Run where Pillow is installed
(the committed file was written with Pillow 12.2.0):

    python tests/golden/make_goldens_trivial_augment.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "vit-inductive-bias-distillation_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main() -> None:
    import PIL
    import test_trivial_augment as T
    from basd_amd import trivial_augment as TA
    images = T.golden_images()
    entries = T.golden_entries(len(images))
    arrays = {"entries": np.asarray(entries, dtype=np.int64), "pillow_version": np.asarray(PIL.__version__)}
    for i, img in enumerate(images):
        arrays[f"image_{i}"] = img
    for k, entry in enumerate(entries):
        img = images[entry[0]]
        rec = T._record(entry, img.shape[1], img.shape[2])
        arrays[f"out_{k}"] = T.pillow_apply(img, rec, TA.magnitude(entry[1], entry[2], bool(entry[3])))
    path = os.path.join(HERE, "trivial_augment.npz")
    np.savez_compressed(path, **arrays)
    print(f"{path}: {len(entries)} entries on {len(images)} images, {os.path.getsize(path)} bytes, Pillow {PIL.__version__}")


if __name__ == "__main__":
    main()
