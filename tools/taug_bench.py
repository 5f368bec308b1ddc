"""The flip + TrivialAugmentWide of one uint8 training batch, (B, C, H, W) = (256, 3, 224, 224), on one GPU:
(a) ONE launch of ``trivial_augment_kernel`` (``basd_trivial_augment`` with the record table already on the device) with
the whole batch forced to one op (bin 20, alternating signs and flips), once per op, and with a drawn mix; the drawn mix
also through ``TrivialAugment.__call__`` (the table built on the host, copied, launched);
(b) for scale, the convert-only ``BatchMixer`` launch (uint8 -> bf16, normalised) on the same batch;
(c) Pillow doing the same drawn mix on ``--threads`` host threads (``ImageEnhance`` / ``ImageOps`` / ``Image.transform``
on images that are already decoded: the part of the loader's work that the launch replaces).
The device side: one process, ``--repeats`` windows of ``--iters`` batches after ``--warmup`` batches, device events
around each window, median and spread (max - min) over the windows.  "of copy" = (source once + destination once) at the
rate the convert-only launch reaches on its own bytes.  Writes the report to ``--out`` and prints it.
usage: taug_bench.py [--iters 50] [--warmup 5] [--repeats 5] [--threads 16] [--out profiles/trivial_augment.txt]"""
import argparse, json, os, sys, time
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "vit-inductive-bias-distillation_amd"))
import numpy as np
import torch
from basd_amd import _lib, trivial_augment as TA
from basd_amd.augment import BatchMixer, MixParams

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trivial_augment.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("taug_bench.py measures on a GPU: none found")
dev = torch.device("cuda", 0)
B, C, H, W = 256, 3, 224, 224
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
g = torch.Generator().manual_seed(1)
# images with structure: a smooth ramp per image plus noise, so that histograms and equal neighbours are not those of
# white noise
ramp = torch.linspace(0, 1, W).view(1, 1, 1, W) * torch.rand(B, C, 1, 1, generator=g) * 160
host = (ramp + torch.rand(B, C, H, 1, generator=g) * 40 + torch.rand(B, C, H, W, generator=g) * 55).to(torch.uint8)
images = host.to(dev)
out = torch.empty_like(images)
aug = TA.TrivialAugment(device=dev)
mixer = BatchMixer(1000, mean=MEAN, std=STD, out_dtype=torch.bfloat16, device=dev)
mixed = torch.empty((B, C, H, W), dtype=torch.bfloat16, device=dev)


def forced(op):
    i = torch.arange(B)
    return TA.AugmentParams(torch.full((B,), op), torch.full((B,), 20), i % 2 == 1, (i // 2) % 2 == 1)


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.iters):
        fn()
    e1.record()
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1) / args.iters                # us per batch


def measure(fn):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    us = [window(fn) for _ in range(args.repeats)]
    return sorted(us)[len(us) // 2], max(us) - min(us), us


drawn = TA.draw_augment_params(B, generator=torch.Generator().manual_seed(2))
cases = [(name, forced(op)) for op, name in enumerate(TA.OPS)] + [("drawn mix", drawn)]
rows, report = [], []
conv_med, conv_spread, conv_us = measure(lambda: mixer(images, None, MixParams("none"), out=mixed))
conv_bytes = images.numel() * 3                                   # one byte read, two written
conv_gbps = conv_bytes / (conv_med * 1e-6) / 1e9
rows.append(json.dumps({"case": "BatchMixer convert-only uint8 -> bf16", "us": [round(v, 2) for v in conv_us],
                        "median_us": round(conv_med, 2), "bytes": conv_bytes, "GBps": round(conv_gbps, 1)}))
report.append(f"  {'convert-only mixer':14s} {conv_med:8.2f} us  (spread {conv_spread:.2f})   {conv_gbps:6.0f} GB/s over 3 bytes "
              "per element")
nbytes = images.numel() * 2
copy_us = nbytes / (conv_gbps * 1e9) * 1e6
status = torch.zeros(1, dtype=torch.int32, device=dev)
stream = torch._C._cuda_getCurrentRawStream(dev.index)
for name, params in cases:
    # the kernel alone: the record table is already on the device
    table = torch.from_numpy(TA.make_records(params, H, W).view(np.uint8).copy()).to(dev)
    med, spread, us = measure(lambda: _lib.call("basd_trivial_augment", images.data_ptr(), out.data_ptr(), B, C, H, W,
                                                table.data_ptr(), status.data_ptr(), stream))
    gbps = nbytes / (med * 1e-6) / 1e9
    rows.append(json.dumps({"case": name, "us": [round(v, 2) for v in us], "median_us": round(med, 2),
                            "spread_us": round(spread, 2), "bytes": nbytes, "GBps": round(gbps, 1),
                            "of_copy": round(copy_us / med, 3)}))
    report.append(f"  {name:14s} {med:8.2f} us  (spread {spread:.2f})   {gbps:6.0f} GB/s   {100 * copy_us / med:5.1f} % of copy")
assert int(status.item()) == 0
call_med, call_spread, call_us = measure(lambda: aug(images, drawn, out=out))
assert aug.status() == 0
rows.append(json.dumps({"case": "TrivialAugment.__call__, drawn mix (table built, copied, launched)",
                        "us": [round(v, 2) for v in call_us], "median_us": round(call_med, 2)}))
report.append(f"  {'whole call':14s} {call_med:8.2f} us  (spread {call_spread:.2f})   drawn mix through TrivialAugment.__call__: the "
              "record table built on the host, one copy, one launch")
# the host side of one call (building the record table), without the device
t0 = time.perf_counter()
for _ in range(20):
    TA.make_records(drawn, H, W)
table_us = (time.perf_counter() - t0) / 20 * 1e6

pillow = "Pillow is not installed here: the host side was not measured"
try:
    import PIL
    from PIL import Image, ImageEnhance, ImageOps
except ImportError:
    PIL = None
if PIL is not None:
    rec = TA.make_records(drawn, H, W)
    mags = [TA.magnitude(int(o), int(b), bool(s)) for o, b, s in zip(drawn.op, drawn.bin, drawn.sign)]
    pil_images = [Image.fromarray(np.ascontiguousarray(host[i].permute(1, 2, 0).numpy()), "RGB") for i in range(B)]

    def one(i):
        im, r, op = pil_images[i], rec[i], int(rec[i]["op"])
        if int(r["flip"]):
            im = im.transpose(Image.FLIP_LEFT_RIGHT)
        if op == TA.IDENTITY:
            return im.copy()
        if op in (TA.SHEAR_X, TA.SHEAR_Y, TA.TRANSLATE_X, TA.TRANSLATE_Y):
            return im.transform(im.size, Image.AFFINE, tuple(float(v) for v in r["a"]), Image.NEAREST, fillcolor=0)
        if op == TA.ROTATE:
            return im.rotate(mags[i], Image.NEAREST, expand=False, fillcolor=0)
        if op in (TA.BRIGHTNESS, TA.COLOR, TA.CONTRAST, TA.SHARPNESS):
            cls = {TA.BRIGHTNESS: ImageEnhance.Brightness, TA.COLOR: ImageEnhance.Color,
                   TA.CONTRAST: ImageEnhance.Contrast, TA.SHARPNESS: ImageEnhance.Sharpness}[op]
            return cls(im).enhance(float(r["farg"]))
        if op == TA.POSTERIZE:
            return ImageOps.posterize(im, int(r["iarg"]))
        if op == TA.SOLARIZE:
            return ImageOps.solarize(im, float(r["farg"]))
        return ImageOps.autocontrast(im) if op == TA.AUTOCONTRAST else ImageOps.equalize(im)

    with ThreadPoolExecutor(args.threads) as pool:
        list(pool.map(one, range(B)))                              # warm
        ms = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            list(pool.map(one, range(B)))
            ms.append((time.perf_counter() - t0) * 1e3)
    pil_med = sorted(ms)[len(ms) // 2]
    rows.append(json.dumps({"case": f"Pillow {PIL.__version__}, drawn mix, {args.threads} threads", "ms": [round(v, 2) for v in ms],
                            "median_ms": round(pil_med, 2), "images_per_s": round(B / pil_med * 1e3)}))
    pillow = (f"Pillow {PIL.__version__} on {args.threads} host threads, the same drawn mix on decoded images: {pil_med:.2f} ms "
              f"per batch (spread {max(ms) - min(ms):.2f}), {B / pil_med * 1e3:.0f} images/s")

text = "\n".join(
    ["The flip + TrivialAugmentWide of one uint8 batch (256, 3, 224, 224), one MI355X: tools/taug_bench.py.  One launch of",
     "trivial_augment_kernel per batch (one workgroup per image, the image staged in LDS), its 16 KiB record table already on",
     "the device; every row forces the whole batch to one op at bin 20 with alternating signs and flips, then a drawn mix,",
     f"then the drawn mix through the host class.  One process, {args.repeats} windows of {args.iters} batches after {args.warmup} warm batches, device events around each "
     "window; us per batch,",
     "median over the windows (spread = max - min).  GB/s =",
     "(source once + destination once) over that time; 'of copy' = the time the same bytes take at the rate of the convert-only",
     "BatchMixer launch (uint8 in, bf16 out, first row), over the measured time.",
     "", "$ python tools/taug_bench.py"] + rows + [""] + report
    + ["", f"  building the record table of a drawn batch on the host: {table_us:.0f} us per call (Python, per sample)",
       "  " + pillow]) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text)
print(text)
