"""Writes tests/golden/resize_filters.npz: ten small images (at most 40 pixels a side, one and three channels, a third of
them two-level), forty (image, win_x, win_y, win_w, win_h, res_w, res_h) cases and what Pillow's
``Image.crop(box).resize((res_w, res_h), F)`` makes of each for F = BILINEAR, BICUBIC and BOX (``out_<filter>_<case>``):
the fixtures of tests/test_resize_filters.py.  Run where Pillow is installed (the committed file was written with Pillow
12.2.0):

    python tests/golden/make_goldens_resize_filters.py
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FILTERS = ("bilinear", "bicubic", "box")


def golden_images():
    rng = np.random.RandomState(30)
    images = []
    for i, (h, w, c) in enumerate([(40, 33, 3), (17, 40, 3), (9, 9, 3), (1, 23, 3), (31, 1, 3), (37, 29, 1), (12, 35, 1),
                                   (40, 40, 3), (5, 7, 1), (23, 38, 3)]):
        if i % 3 == 2:
            img = np.where(rng.rand(h, w, c) < 0.5, 0, 255)      # two-level: bicubic over- and undershoots on every edge
        else:
            ramp = np.add.outer(np.arange(h) * 3, np.arange(w) * 5)[:, :, None]
            img = (ramp + rng.randint(0, 120, (h, w, c))) % 256
        images.append(img.astype(np.uint8))
    return images


def golden_cases(images):
    """Four cases per image: the whole image reduced, a window enlarged, a window with one axis unchanged, a window
    reduced strongly in one axis (by up to 13: inside bicubic's limit of 16) and enlarged in the other."""
    rng = np.random.RandomState(31)
    cases = []
    for i, img in enumerate(images):
        h, w = img.shape[:2]
        cases.append((i, 0, 0, w, h, max(1, w // 2 + 1), max(1, (2 * h) // 3)))
        for kind in range(3):
            ww, wh = rng.randint(1, w + 1), rng.randint(1, h + 1)
            wx, wy = rng.randint(0, w - ww + 1), rng.randint(0, h - wh + 1)
            if kind == 0:
                rw, rh = ww + rng.randint(1, 30), wh + rng.randint(1, 30)
            elif kind == 1:
                rw, rh = ww, rng.randint(max(1, (wh + 15) // 16), 45)
            else:
                rw, rh = max(1, ww // 7), wh * 3
            cases.append((i, wx, wy, ww, wh, rw, rh))
    return cases


def pillow_resize(img, case, name):
    from PIL import Image
    _, wx, wy, ww, wh, rw, rh = case
    pil = Image.fromarray(img[:, :, 0] if img.shape[2] == 1 else img)
    out = np.asarray(pil.crop((wx, wy, wx + ww, wy + wh)).resize((rw, rh), getattr(Image, name.upper())))
    return out[:, :, None] if out.ndim == 2 else out


def main() -> None:
    import PIL
    images = golden_images()
    cases = golden_cases(images)
    arrays = {"cases": np.asarray(cases, dtype=np.int64), "pillow_version": np.asarray(PIL.__version__),
              "filters": np.asarray(FILTERS)}
    for i, img in enumerate(images):
        arrays[f"image_{i}"] = img
    for name in FILTERS:
        for k, case in enumerate(cases):
            arrays[f"out_{name}_{k}"] = pillow_resize(images[case[0]], case, name)
    path = os.path.join(HERE, "resize_filters.npz")
    np.savez_compressed(path, **arrays)
    print(f"{path}: {len(cases)} cases x {len(FILTERS)} filters on {len(images)} images, {os.path.getsize(path)} bytes, "
          f"Pillow {PIL.__version__}")


if __name__ == "__main__":
    main()
