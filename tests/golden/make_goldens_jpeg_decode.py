"""Writes tests/golden/jpeg_decode.npz: baseline JPEG streams made by Pillow's encoder with Pillow's decoded RGB
(``np.asarray(Image.open(...).convert("RGB"))``) for each, plus one progressive and one CMYK stream for the fallback
route.  Written with Pillow 12.2.0 (libjpeg-turbo); run from the repository root:

    python tests/golden/make_goldens_jpeg_decode.py

Keys: ``names`` (the streams' names, in order), ``stream_<name>`` (uint8), ``rgb_<name>`` (H, W, 3) uint8.
"""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
SIDES = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33)
SUBSAMPLING = {"444": 0, "422": 1, "420": 2}


def picture(rng: np.random.Generator, height: int, width: int, kind: str, gray: bool) -> np.ndarray:
    """``noise``: two-level 0 / 255 noise (the IDCT overshoots into the clamps, the scan is full of FF bytes);
    ``ramp``: a noisy ramp."""
    shape = (height, width) if gray else (height, width, 3)
    if kind == "noise":
        return (rng.integers(0, 2, size=shape) * 255).astype(np.uint8)
    yy, xx = np.mgrid[0:height, 0:width]
    ramp = (xx * 255.0 / max(width - 1, 1) + yy * 128.0 / max(height - 1, 1))
    if not gray:
        ramp = np.stack([ramp, ramp[::-1], 255 - ramp], axis=2)
    return np.clip(ramp + rng.normal(0, 12, size=shape), 0, 255).astype(np.uint8)


def encode(pixels: np.ndarray, **options) -> bytes:
    out = io.BytesIO()
    Image.fromarray(pixels).save(out, format="JPEG", **options)
    return out.getvalue()


def decode(stream: bytes) -> np.ndarray:
    return np.asarray(Image.open(io.BytesIO(stream)).convert("RGB"))


def corpus() -> dict:
    rng = np.random.default_rng(20251019)
    streams = {}
    modes = ("gray", "444", "422", "420")
    qualities = (1, 75, 100)
    n = 0
    # mixed pairs of the sides: every side is a width once and a height once, every mode and quality comes up
    widths = list(SIDES)
    heights = list(SIDES[5:] + SIDES[:5])
    for w, h in zip(widths + [1, 2, 33, 17, 3, 16], heights + [1, 31, 33, 2, 3, 16]):
        mode, quality = modes[n % 4], qualities[(n // 4) % 3]
        kind = "noise" if n % 3 == 0 else "ramp"
        options = dict(quality=quality)
        if mode != "gray":
            options["subsampling"] = SUBSAMPLING[mode]
        if n % 5 == 1:
            options["optimize"] = True
        streams[f"{mode}_{w}x{h}_q{quality}_{kind}" + ("_opt" if options.get("optimize") else "")] = encode(
            picture(rng, h, w, kind, mode == "gray"), **options)
        n += 1
    # restart intervals on one picture per mode, and the same picture without (the two decode alike)
    for mode, (w, h) in zip(modes, ((17, 9), (33, 17), (31, 33), (33, 31))):
        pixels = picture(rng, h, w, "ramp", mode == "gray")
        options = dict(quality=75) if mode == "gray" else dict(quality=75, subsampling=SUBSAMPLING[mode])
        streams[f"{mode}_{w}x{h}_q75_plain"] = encode(pixels, **options)
        streams[f"{mode}_{w}x{h}_q75_rst1"] = encode(pixels, restart_marker_blocks=1, **options)
        streams[f"{mode}_{w}x{h}_q75_rst2"] = encode(pixels, restart_marker_blocks=2, **options)
        streams[f"{mode}_{w}x{h}_q75_rstrow"] = encode(pixels, restart_marker_rows=1, **options)
    streams["420_64x96_q100_noise"] = encode(picture(rng, 96, 64, "noise", False), quality=100, subsampling=2)
    # 81 restart intervals: more segments than a workgroup has lanes, and the marker count wraps modulo 8
    streams["444_72x72_q75_81segments"] = encode(picture(rng, 72, 72, "ramp", False), quality=75, subsampling=0,
                                           restart_marker_blocks=1)
    # the fallback route
    small = picture(rng, 9, 15, "ramp", False)
    streams["fallback_progressive"] = encode(small, quality=75, progressive=True)
    out = io.BytesIO()
    Image.fromarray(small).convert("CMYK").save(out, format="JPEG", quality=75)
    streams["fallback_cmyk"] = out.getvalue()
    return streams


def main() -> None:
    streams = corpus()
    arrays = {"names": np.array(list(streams))}
    for name, stream in streams.items():
        arrays[f"stream_{name}"] = np.frombuffer(stream, dtype=np.uint8)
        arrays[f"rgb_{name}"] = decode(stream)
    path = os.path.join(HERE, "jpeg_decode.npz")
    np.savez_compressed(path, **arrays)
    print(f"{path}: {len(streams)} streams, {os.path.getsize(path)} bytes", file=sys.stderr)


if __name__ == "__main__":
    main()
