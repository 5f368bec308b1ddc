"""The decode of a batch of PNG files on the device (basd_amd.png, two launches) beside Pillow's decode of the same
files in 1 and in 16 processes on the same machine, and beside the path such files took before (pack_jpegs's host
fallback: Pillow in the collate worker, decoded pixels packed), at two corpora:
  cifar   128 files of 32 x 32 RGB (the reference's configs/experiment/basd_cifar100.yaml)
  large   256 files of 500 x 375 RGB (the picture size of tools/jpeg_bench.py)
usage: png_bench.py [--corpus cifar|large|both] [--windows 5] [--per-window 10] [--processes 16] [--device-only]
Where Pillow is importable the files are encoded with it (16 different pictures, repeated); otherwise by the tests' own
PNG writer (filter 4, zlib level 6) and only the device is timed (the output says so).  The windows of the device and
the Pillow runs alternate; the figures are medians over the windows."""
import argparse
import importlib.util
import io
import json
import multiprocessing
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "vit-inductive-bias-distillation_amd"))

CORPORA = {"cifar": (128, 32, 32), "large": (256, 500, 375)}            # batch, width, height


def have_pillow() -> bool:
    try:
        import PIL.Image  # noqa: F401
    except ImportError:
        return False
    return True


def make_files(batch: int, width: int, height: int, distinct: int = 16):
    """(files, pixels of the distinct pictures, how they were made): smooth colour fields, edges and sensor-like noise."""
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float64)
    pictures = []
    for _ in range(distinct):
        planes = []
        for _c in range(3):
            field = sum(rng.uniform(20, 60) * np.sin(xx * rng.uniform(0.005, 0.08) + yy * rng.uniform(0.005, 0.08)
                                                     + rng.uniform(0, 6.3)) for _k in range(4))
            edges = 60.0 * ((xx * rng.uniform(-1, 1) + yy * rng.uniform(-1, 1)) % rng.uniform(40, 160) < 20)
            planes.append(128 + field + edges + rng.normal(0, 3, size=field.shape))
        pictures.append(np.clip(np.stack(planes, axis=2), 0, 255).astype(np.uint8))
    if have_pillow():
        from PIL import Image
        files = []
        for pixels in pictures:
            out = io.BytesIO()
            Image.fromarray(pixels).save(out, format="PNG")
            files.append(out.getvalue())
        how = f"Pillow {__import__('PIL').__version__}: {distinct} pictures of {width} x {height}, RGB, default options"
    else:
        spec = importlib.util.spec_from_file_location(
            "make_goldens_png_decode", os.path.join(ROOT, "tests", "golden", "make_goldens_png_decode.py"))
        writer = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(writer)
        files = [writer.write_png(pixels, 2, [4] * height) for pixels in pictures]
        how = f"no Pillow here: {distinct} pictures of {width} x {height} by the tests' writer (Paeth rows, zlib level 6)"
    return [files[i % distinct] for i in range(batch)], pictures, how


def _pillow_pixels(data: bytes) -> np.ndarray:
    from PIL import Image
    with Image.open(io.BytesIO(data)) as img:
        return np.asarray(img.convert("RGB"))


def _pillow_decode(data: bytes) -> int:
    return _pillow_pixels(data).size


def run(name: str, args, pool) -> None:
    import torch
    from basd_amd.jpeg import pack_jpegs
    from basd_amd.png import PngDecoder, pack_pngs
    batch_size, width, height = CORPORA[name]
    files, pictures, how = make_files(batch_size, width, height)
    timed_pillow = pool is not None
    dev = torch.device("cuda", 0)
    t0 = time.perf_counter()
    packed = pack_pngs(files)
    pack_ms = (time.perf_counter() - t0) * 1e3
    assert packed.fallbacks == 0
    pinned = packed.pin_memory()
    decoder = PngDecoder(dev)
    batch = pinned.to(dev, non_blocking=True)
    for _ in range(3):
        ragged = decoder(batch)
    torch.cuda.synchronize()
    assert decoder.status() == 0
    check = [0, batch_size // 2, batch_size - 1]
    for i in check:                                                     # PNG is lossless: the source pixels
        assert np.array_equal(ragged.image(i).cpu().numpy(), pictures[i % len(pictures)]), i
    print(json.dumps({"case": f"{name}: the batch", "files": how, "batch": batch_size,
                      "stream_bytes": int(packed.records["src_len"].sum()), "decoded_bytes": packed.out_bytes,
                      "workspace_bytes": packed.workspace_bytes, "pack_pngs_ms": round(pack_ms, 2)}))
    launches, calls, uploads, one, many, parent = [], [], [], [], [], []
    for _ in range(args.windows):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        start.record()
        for _ in range(args.per_window):
            decoder(batch)
        stop.record()
        torch.cuda.synchronize()
        calls.append((time.perf_counter() - t0) * 1e3 / args.per_window)
        launches.append(start.elapsed_time(stop) / args.per_window)
        t0 = time.perf_counter()
        for _ in range(args.per_window):
            pinned.to(dev, non_blocking=True)
        torch.cuda.synchronize()
        uploads.append((time.perf_counter() - t0) * 1e3 / args.per_window)
        if timed_pillow:
            t0 = time.perf_counter()
            for f in files:
                _pillow_decode(f)
            one.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            pool.map(_pillow_decode, files, chunksize=max(1, batch_size // (4 * args.processes)))
            many.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            before = pack_jpegs(files)
            parent.append((time.perf_counter() - t0) * 1e3)
            assert before.fallbacks == batch_size
    assert decoder.status() == 0

    def line(case, ms):
        med = statistics.median(ms)
        print(json.dumps({"case": f"{name}: {case}", "ms": [round(v, 3) for v in ms], "median_ms": round(med, 3),
                          "spread_ms": round(max(ms) - min(ms), 3), "images_per_s": round(batch_size / med * 1e3)}))
        return med

    device_ms = line("device decode, two launches (device events)", launches)
    line("PngDecoder.__call__ (table copied, launched, waited for)", calls)
    line("upload of the packed files (pinned, one copy)", uploads)
    if timed_pillow:
        one_ms = line("Pillow, 1 process", one)
        many_ms = line(f"Pillow, {args.processes} processes (results not sent back)", many)
        parent_ms = line("pack_jpegs of the same files (the path before: Pillow in the collate worker, pixels packed)", parent)
        print(f"\n  {name}: device {device_ms:.3f} ms per batch of {batch_size}; Pillow {one_ms:.1f} ms in 1 process, "
              f"{many_ms:.1f} ms in {args.processes}, pack_jpegs {parent_ms:.1f} ms: Pillow's time over the device's is "
              f"{one_ms / device_ms:.2f}, {many_ms / device_ms:.2f} and {parent_ms / device_ms:.2f}; images {check} "
              "compared with the source pixels byte for byte\n")
    else:
        print(f"\n  {name}: device {device_ms:.3f} ms per batch of {batch_size}; Pillow not timed; images {check} compared "
              "with the source pixels byte for byte\n")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--corpus", choices=("cifar", "large", "both"), default="both")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--per-window", type=int, default=10)
    ap.add_argument("--processes", type=int, default=16)
    ap.add_argument("--device-only", action="store_true")
    args = ap.parse_args()
    timed_pillow = have_pillow() and not args.device_only
    # the worker processes exist before this process opens the GPU, and never open it themselves
    pool = multiprocessing.get_context("fork").Pool(args.processes) if timed_pillow else None
    for name in (("cifar", "large") if args.corpus == "both" else (args.corpus,)):
        run(name, args, pool)
    if pool is not None:
        pool.close()
        pool.join()


if __name__ == "__main__":
    main()
