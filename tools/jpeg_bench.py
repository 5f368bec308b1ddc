"""The decode of one batch of 256 JPEG files of 500 x 375 (quality 90, 4:2:0) on the device (basd_amd.jpeg, three
launches) beside Pillow's decode of the same files in 1 and in 16 processes on the same machine.
usage: jpeg_bench.py [--batch 256] [--windows 5] [--per-window 10] [--processes 16] [--device-only]
                     [--entropy serial|parallel|both] [--sub-bytes N] [--progressive]
(--device-only: no worker processes and no Pillow timing, for a run under a profiler; --entropy: the decoder's entropy
stage, JpegDecoder(entropy=...); both: a serial and a parallel window in every round, one after the other, so the two
are measured in the same run; --sub-bytes: JpegDecoder(sub_bytes=...) of the parallel stage, default its own)
Where Pillow is importable the files are encoded with it (16 different pictures, repeated); otherwise the largest
stream of tests/golden/jpeg_decode.npz is repeated and only the device is timed (the output says so).  The windows of
the device and the Pillow runs alternate; the figures are medians over the windows.
--progressive (needs Pillow): the same pictures as progressive files through basd_jpeg_decode_progressive
(pack_jpegs(..., progressive=True)), beside Pillow in 1 and in --processes processes on those files, the path without
the keyword (Pillow inside pack_jpegs, then the raw pixels uploaded and copied into place), the baseline batch again and
a mixed batch with 1 file in 10 progressive (that share is an assumption, not a measurement of any data set), all in
one call with alternating windows."""
import argparse
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


def have_pillow() -> bool:
    try:
        import PIL.Image  # noqa: F401
    except ImportError:
        return False
    return True


def make_streams(batch: int, width: int = 500, height: int = 375, quality: int = 90, distinct: int = 16,
                 progressive: bool = False):
    """(files, how they were made): ``batch`` JPEG files.  With Pillow: ``distinct`` seeded pictures (smooth colour
    fields, edges and sensor-like noise) encoded at ``quality`` with 4:2:0, repeated; without: the largest recorded
    stream repeated."""
    if not have_pillow():
        g = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_decode.npz"), allow_pickle=False)
        name = max((n for n in g["names"] if not str(n).startswith("fallback_")), key=lambda n: g[f"stream_{n}"].size)
        return [g[f"stream_{name}"].tobytes()] * batch, f"no Pillow here: the recorded stream {name} repeated"
    from PIL import Image
    rng = np.random.default_rng(5)
    files = []
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float64)
    for _ in range(distinct):
        planes = []
        for _c in range(3):
            field = sum(rng.uniform(20, 60) * np.sin(xx * rng.uniform(0.005, 0.08) + yy * rng.uniform(0.005, 0.08)
                                                     + rng.uniform(0, 6.3)) for _k in range(4))
            edges = 60.0 * ((xx * rng.uniform(-1, 1) + yy * rng.uniform(-1, 1)) % rng.uniform(40, 160) < 20)
            planes.append(128 + field + edges + rng.normal(0, 11, size=field.shape))
        out = io.BytesIO()
        Image.fromarray(np.clip(np.stack(planes, axis=2), 0, 255).astype(np.uint8)).save(
            out, format="JPEG", quality=quality, subsampling=2, progressive=progressive)
        files.append(out.getvalue())
    return [files[i % distinct] for i in range(batch)], \
        f"Pillow {__import__('PIL').__version__}: {distinct} pictures of {width} x {height}, quality {quality}, 4:2:0" \
        + (", progressive" if progressive else "")


def _pillow_pixels(data: bytes) -> np.ndarray:
    from PIL import Image
    with Image.open(io.BytesIO(data)) as img:
        return np.asarray(img.convert("RGB"))


def _pillow_decode(data: bytes) -> int:
    return _pillow_pixels(data).size


def progressive_main(args) -> None:
    """--progressive: every case in every window, one after the other."""
    if not have_pillow():
        sys.exit("--progressive needs Pillow: it writes the files and is what the device is measured against")
    prog, how = make_streams(args.batch, progressive=True)
    base, _ = make_streams(args.batch)
    mixed = [prog[i] if i % 10 == 0 else base[i] for i in range(args.batch)]
    pool = multiprocessing.get_context("fork").Pool(args.processes) if not args.device_only else None
    import torch
    from basd_amd.jpeg import JpegDecoder, pack_jpegs
    dev = torch.device("cuda", 0)
    entropy = "serial" if args.entropy == "both" else args.entropy
    decoder = JpegDecoder(dev, entropy=entropy, sub_bytes=args.sub_bytes if entropy == "parallel" else None)
    packed = {"progressive files on the device (four launches)": pack_jpegs(prog, progressive=True),
              "baseline files on the device (three launches)": pack_jpegs(base),
              "1 file in 10 progressive (an assumed share) on the device (four launches)":
                  pack_jpegs(mixed, progressive=True),
              "the path without the keyword: raw pixels copied into place (three launches)": pack_jpegs(prog)}
    counts = [(b.progressive, b.fallbacks) for b in packed.values()]
    assert counts == [(args.batch, 0), (0, 0), (len(mixed[::10]), 0), (0, args.batch)], counts
    pinned = {k: b.pin_memory() for k, b in packed.items()}
    on_device = {k: b.to(dev, non_blocking=True) for k, b in pinned.items()}
    check = [0, args.batch // 2, args.batch - 1]
    for (case, batch), files in zip(on_device.items(), (prog, base, mixed, prog)):
        for _ in range(3):
            ragged = decoder(batch)
        torch.cuda.synchronize()
        assert decoder.status() == 0, case
        for i in check:
            assert np.array_equal(ragged.image(i).cpu().numpy(), _pillow_pixels(files[i])), (case, i)
    first = packed["progressive files on the device (four launches)"]
    print(json.dumps({"case": "the batch", "files": how, "batch": args.batch, "entropy": entropy,
                      "stream_bytes": {"progressive": sum(map(len, prog)), "baseline": sum(map(len, base))},
                      "packed_bytes": {k: b.data.numel() for k, b in packed.items()}, "decoded_bytes": first.out_bytes,
                      "scans": first.max_scans, "blocks_per_image": first.max_blocks}))
    launches = {k: [] for k in on_device}
    uploads = {k: [] for k in on_device}
    pack_prog, pack_raw, one, many = [], [], [], []
    for _ in range(args.windows):
        for case, batch in on_device.items():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            start.record()
            for _ in range(args.per_window):
                decoder(batch)
            stop.record()
            torch.cuda.synchronize()
            launches[case].append(start.elapsed_time(stop) / args.per_window)
            t0 = time.perf_counter()
            for _ in range(args.per_window):
                pinned[case].to(dev, non_blocking=True)
            torch.cuda.synchronize()
            uploads[case].append((time.perf_counter() - t0) * 1e3 / args.per_window)
        if pool is not None:
            t0 = time.perf_counter()
            pack_jpegs(prog, progressive=True)
            pack_prog.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            pack_jpegs(prog)
            pack_raw.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            for f in prog:
                _pillow_decode(f)
            one.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            pool.map(_pillow_decode, prog, chunksize=max(1, args.batch // (4 * args.processes)))
            many.append((time.perf_counter() - t0) * 1e3)
    if pool is not None:
        pool.close()
        pool.join()
    assert decoder.status() == 0

    def line(case, ms):
        med = statistics.median(ms)
        print(json.dumps({"case": case, "ms": [round(v, 3) for v in ms], "median_ms": round(med, 3),
                          "spread_ms": round(max(ms) - min(ms), 3), "images_per_s": round(args.batch / med * 1e3)}))
        return med

    device = {case: line(case + " (device events)", ms) for case, ms in launches.items()}
    for case, ms in uploads.items():
        line("upload (pinned, one copy) for: " + case, ms)
    if pool is not None:
        line("pack_jpegs(progressive=True) of the progressive files, 1 process (host)", pack_prog)
        line("pack_jpegs without the keyword: Pillow decodes them, 1 process (host)", pack_raw)
        one_ms = line("Pillow on the progressive files, 1 process", one)
        many_ms = line(f"Pillow on the progressive files, {args.processes} processes (results not sent back)", many)
        ms = device["progressive files on the device (four launches)"]
        print(f"\n  progressive on the device {ms:.3f} ms per batch of {args.batch}; Pillow {one_ms:.1f} ms in 1 process, "
              f"{many_ms:.1f} ms in {args.processes}: factors {one_ms / ms:.2f} and {many_ms / ms:.2f}; images {check} "
              "of every case compared with Pillow byte for byte")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--per-window", type=int, default=10)
    ap.add_argument("--processes", type=int, default=16)
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--entropy", choices=("serial", "parallel", "both"), default="serial")
    ap.add_argument("--sub-bytes", type=int, default=None)
    ap.add_argument("--progressive", action="store_true")
    args = ap.parse_args()
    if args.progressive:
        return progressive_main(args)
    modes = ("serial", "parallel") if args.entropy == "both" else (args.entropy,)
    files, how = make_streams(args.batch)
    pillow = have_pillow()
    timed_pillow = pillow and not args.device_only
    # the worker processes exist before this process opens the GPU, and never open it themselves
    pool = multiprocessing.get_context("fork").Pool(args.processes) if timed_pillow else None
    import torch
    from basd_amd.jpeg import JpegDecoder, decode_reference, pack_jpegs
    dev = torch.device("cuda", 0)
    t0 = time.perf_counter()
    packed = pack_jpegs(files)
    pack_ms = (time.perf_counter() - t0) * 1e3
    assert packed.fallbacks == 0
    pinned = packed.pin_memory()
    decoders = {m: JpegDecoder(dev, entropy=m, sub_bytes=args.sub_bytes if m == "parallel" else None) for m in modes}
    batch = pinned.to(dev, non_blocking=True)
    check = [0, args.batch // 2, args.batch - 1]
    outputs = []
    for decoder in decoders.values():
        for _ in range(3):
            ragged = decoder(batch)
        torch.cuda.synchronize()
        assert decoder.status() == 0
        for i in check:
            want = _pillow_pixels(files[i]) if pillow else decode_reference(files[i])
            assert np.array_equal(ragged.image(i).cpu().numpy(), want), i
        outputs.append(ragged.data)
    assert all(torch.equal(outputs[0], other) for other in outputs[1:])       # every byte of the batch, mode against mode
    del outputs
    stream_bytes = sum(len(f) for f in files)
    info = {"case": "the batch", "files": how, "batch": args.batch, "stream_bytes": stream_bytes,
            "decoded_bytes": packed.out_bytes, "workspace_bytes": packed.workspace_bytes,
            "blocks_per_image": packed.max_blocks, "pack_jpegs_ms": round(pack_ms, 2), "entropy": list(modes),
            "sub_bytes": args.sub_bytes}
    print(json.dumps(info))
    launches, calls = {m: [] for m in modes}, {m: [] for m in modes}
    uploads, one, many = [], [], []
    for _ in range(args.windows):
        for mode, decoder in decoders.items():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            start.record()
            for _ in range(args.per_window):
                decoder(batch)
            stop.record()
            torch.cuda.synchronize()
            calls[mode].append((time.perf_counter() - t0) * 1e3 / args.per_window)
            launches[mode].append(start.elapsed_time(stop) / args.per_window)
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
            pool.map(_pillow_decode, files, chunksize=max(1, args.batch // (4 * args.processes)))
            many.append((time.perf_counter() - t0) * 1e3)
    if pool is not None:
        pool.close()
        pool.join()
    assert all(decoder.status() == 0 for decoder in decoders.values())

    def line(case, ms):
        med = statistics.median(ms)
        row = {"case": case, "ms": [round(v, 3) for v in ms], "median_ms": round(med, 3),
               "spread_ms": round(max(ms) - min(ms), 3), "images_per_s": round(args.batch / med * 1e3)}
        print(json.dumps(row))
        return med

    device = {m: line(f"device decode, {m} entropy stage, three launches (device events)", launches[m]) for m in modes}
    for m in modes:
        line(f"JpegDecoder.__call__, {m} (table copied, launched, waited for)", calls[m])
    line("upload of the packed files (pinned, one copy)", uploads)
    device_ms = device[modes[-1]]
    if len(modes) == 2:
        gain = max(launches["parallel"]) < min(launches["serial"])
        print(json.dumps({"case": "parallel against serial, same run", "serial_over_parallel":
                          round(device["serial"] / device["parallel"], 2), "slowest_parallel_window_ms":
                          round(max(launches["parallel"]), 3), "fastest_serial_window_ms":
                          round(min(launches["serial"]), 3), "every_parallel_window_faster": gain}))
    if timed_pillow:
        one_ms = line("Pillow, 1 process", one)
        many_ms = line(f"Pillow, {args.processes} processes (results not sent back)", many)
        print(f"\n  device ({modes[-1]}) {device_ms:.3f} ms per batch of {args.batch}; Pillow {one_ms:.1f} ms in 1 process, {many_ms:.1f} ms "
              f"in {args.processes}: the device decode is faster by a factor of {one_ms / device_ms:.1f} and "
              f"{many_ms / device_ms:.1f}; images {check} compared byte for byte")
    else:
        print(f"\n  device ({modes[-1]}) {device_ms:.3f} ms per batch of {args.batch}; Pillow not timed; images {check} compared "
              f"with {'Pillow' if pillow else 'decode_reference'} byte for byte")


if __name__ == "__main__":
    main()
