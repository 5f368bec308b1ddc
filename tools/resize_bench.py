"""The crops and resizes of one ragged training batch -- B = 256 decoded images of 375 x 500 x 3, both views to 224 with
crop_ratio 0.875 -- on one GPU:
(a) ONE launch of ``resize_crop_kernel`` (``basd_resize_crop`` with the packed images and the record table already on the
device): both views, the clean view alone, the augmented view alone; both views also through ``ResizeCrop.__call__`` (the
crops given, the table built on the host, copied, launched);
(b) for scale, the convert-only ``BatchMixer`` launch (uint8 -> bf16, normalised) on the bytes the launch writes;
(c) Pillow doing the same crops and resizes on ``--threads`` host threads, on images that are already decoded: the part
of the loader's work that the launch replaces.
The device side: one process, ``--repeats`` windows of ``--iters`` batches after ``--warmup`` batches, device events
around each window, median and spread (max - min) over the windows.  "of copy" = (every source byte once + every
destination byte once) at the rate the convert-only launch reaches on its own bytes, over the measured time.  Writes the
report to ``--out`` and prints it.  ``--interpolation`` names the filter of all of it (the records of both views, and
Pillow's, the host yardstick).
``--filters`` measures the filters against each other instead: the launch of both views with bilinear / bilinear,
bicubic (clean) / bilinear (augmented), bicubic / bicubic and box / box records, and -- with ``--parent-lib`` naming a
``libbasd_hip.so`` built from another commit -- that build's launch on the bilinear table, all in this one process with
their windows interleaved (round after round, one window of each), so that a drift of the clocks falls on all of them
alike; then Pillow with ``--interpolation`` on ``--threads`` threads.  A gain or a loss is claimed only where every
window of one side lies beyond every window of the other.
usage: resize_bench.py [--iters 20] [--warmup 3] [--repeats 5] [--threads 16] [--interpolation bilinear]
                       [--filters [--parent-lib PATH]] [--out profiles/resize_crop.txt]"""
import argparse, ctypes, json, os, sys, time
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "vit-inductive-bias-distillation_amd"))
import numpy as np
import torch
from basd_amd import _lib, resize as RZ
from basd_amd.augment import BatchMixer, MixParams

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--interpolation", choices=RZ.INTERPOLATIONS, default="bilinear")
ap.add_argument("--filters", action="store_true")
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if args.out is None:
    args.out = os.path.join(ROOT, "profiles", "resize_filters.txt" if args.filters else "resize_crop.txt")
if args.parent_lib and not args.filters:
    sys.exit("--parent-lib belongs to --filters")
if not torch.cuda.is_available():
    sys.exit("resize_bench.py measures on a GPU: none found")
dev = torch.device("cuda", 0)
B, C, H, W, S, RATIO = 256, 3, 375, 500, 224, 0.875
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
g = torch.Generator().manual_seed(1)
# images with structure: a smooth ramp per image plus noise
ramp = torch.linspace(0, 1, W).view(1, 1, W, 1) * torch.rand(B, 1, 1, C, generator=g) * 160
host = (ramp + torch.rand(B, H, 1, C, generator=g) * 40 + torch.rand(B, H, W, C, generator=g) * 55).to(torch.uint8)
ragged_host = RZ.pack_images([host[i] for i in range(B)])
ragged = ragged_host.to(dev)
crops = RZ.draw_crop_params(ragged.sizes, generator=torch.Generator().manual_seed(2))
rc = RZ.ResizeCrop(S, RATIO, device=dev, interpolation=args.interpolation)
PIL_FILTER = args.interpolation.upper()
mixer = BatchMixer(1000, mean=MEAN, std=STD, out_dtype=torch.bfloat16, device=dev)
out = torch.empty((2 * B, C, S, S), dtype=torch.uint8, device=dev)
mixed = torch.empty((2 * B, C, S, S), dtype=torch.bfloat16, device=dev)


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


def pillow_windows(name):
    """(ms per batch of every window, the first pass's images) of Pillow making both views with filter ``name``, or None."""
    try:
        from PIL import Image
    except ImportError:
        return None
    flt = getattr(Image, name.upper())
    pil_images = [Image.fromarray(host[i].numpy()) for i in range(B)]
    res_h, res_w, top, left = RZ.eval_window(H, W, S, RATIO)
    boxes = [(int(crops.left[i]), int(crops.top[i]), int(crops.left[i] + crops.width[i]),
              int(crops.top[i] + crops.height[i])) for i in range(B)]

    def one(i):
        im = pil_images[i]
        clean = im.resize((res_w, res_h), flt).crop((left, top, left + S, top + S))
        clean.load()
        return clean, im.crop(boxes[i]).resize((S, S), flt)

    with ThreadPoolExecutor(args.threads) as pool:
        first = list(pool.map(one, range(B)))                      # warm
        ms = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            list(pool.map(one, range(B)))
            ms.append((time.perf_counter() - t0) * 1e3)
    return ms, first


def beyond(a, b):
    """'below' / 'above' where every window of a lies below / above every window of b, else None."""
    return "below" if max(a) < min(b) else "above" if min(a) > max(b) else None


def compare_filters():
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    stream = torch._C._cuda_getCurrentRawStream(dev.index)
    n = 2 * B

    def table_of(interpolation):
        rec = RZ.make_records(ragged.sizes, S, RATIO, crops, interpolation=interpolation)
        return torch.from_numpy(rec.view(np.uint8).copy()).to(dev)

    def launcher(fn, table):
        def go():
            code = fn(ragged.data.data_ptr(), ragged.data.numel(), out.data_ptr(), n, C, S, S, table.data_ptr(),
                      status.data_ptr(), 0, stream)
            if code:
                raise RuntimeError(f"basd_resize_crop returned {code}")
        return go

    ours = _lib.load().basd_resize_crop
    tables = {"bilinear / bilinear": table_of("bilinear"),
              "bicubic / bilinear": table_of({"clean": "bicubic", "augmented": "bilinear"}),
              "bicubic / bicubic": table_of("bicubic"), "box / box": table_of("box")}
    configs = {name: launcher(ours, t) for name, t in tables.items()}
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib)).basd_resize_crop
        parent.argtypes, parent.restype = _lib.SIGNATURES["basd_resize_crop"], ctypes.c_int
        configs["parent build, bilinear / bilinear"] = launcher(parent, tables["bilinear / bilinear"])
    # the parent's launch and this build's make the same bytes of the bilinear table
    kept = {}
    for name, go in configs.items():
        out.fill_(0xA5)
        go()
        kept[name] = out.clone()
    assert int(status.item()) == 0
    same = None
    if args.parent_lib:
        same = bool(torch.equal(kept["parent build, bilinear / bilinear"], kept["bilinear / bilinear"]))
        assert same, "the parent build and this one differ on the bilinear table"
    for go in configs.values():
        for _ in range(args.warmup):
            go()
    torch.cuda.synchronize()
    us = {name: [] for name in configs}
    for _ in range(args.repeats):                                  # interleaved: one window of each per round
        for name, go in configs.items():
            us[name].append(window(go))
    med = {name: sorted(v)[len(v) // 2] for name, v in us.items()}
    rows = [json.dumps({"case": name + " (clean / augmented), both views, one launch", "us": [round(x, 2) for x in v],
                        "median_us": round(med[name], 2)}) for name, v in us.items()]
    base = "bilinear / bilinear"
    report = []
    for name, v in us.items():
        line = f"  {name:36s} {med[name]:9.2f} us  (windows {min(v):.2f} .. {max(v):.2f})"
        if name != base:
            side = beyond(v, us[base])
            line += (f"   {med[name] / med[base]:.3f} x bilinear of this build; "
                     + (f"every window {side} every window of it" if side else "the windows overlap: no difference claimed"))
        report.append(line)
    if args.parent_lib:
        side = beyond(us[base], us["parent build, bilinear / bilinear"])
        report.append(f"  bilinear, this build against the parent's: {med[base] / med['parent build, bilinear / bilinear']:.3f} x; "
                      + (f"every window of this build lies {side} every window of the parent's" if side else
                         "the windows overlap: no loss and no gain") + f"; the two builds' bytes are equal: {same}")
    pil = pillow_windows(args.interpolation)
    both = args.interpolation + " / " + args.interpolation
    if pil is None:
        report.append("  Pillow is not installed here: the host side was not measured")
    else:
        import PIL
        ms, first = pil
        flags = kept[both].cpu().numpy()
        for i in (0, B // 2, B - 1):
            assert np.array_equal(flags[i], np.asarray(first[i][0]).transpose(2, 0, 1))
            assert np.array_equal(flags[B + i], np.asarray(first[i][1]).transpose(2, 0, 1))
        pil_med = sorted(ms)[len(ms) // 2]
        rows.append(json.dumps({"case": f"Pillow {PIL.__version__} {PIL_FILTER}, both views, {args.threads} threads",
                                "ms": [round(v, 2) for v in ms], "median_ms": round(pil_med, 2),
                                "images_per_s": round(B / pil_med * 1e3)}))
        report.append(f"  Pillow {PIL.__version__} Image.{PIL_FILTER} on {args.threads} host threads, both views of the same decoded "
                      f"images: {pil_med:.2f} ms per batch (windows {min(ms):.2f} .. {max(ms):.2f}); the {both} launch takes "
                      f"{med[both] / 1e3:.3f} ms: a factor of {pil_med / (med[both] / 1e3):.1f}; three images per view "
                      "compared byte for byte")
    text = "\n".join(
        [f"The filters of the resize launch against each other: {B} decoded images of {H} x {W} x {C}, both views to {S}",
         f"(crop_ratio {RATIO}), one launch of resize_crop_kernel per batch, the packed images and the record table already on",
         f"the device, one MI355X, ONE process and one run series: tools/resize_bench.py --filters.  {args.repeats} rounds; a round is",
         f"one window of {args.iters} batches of every configuration in turn (after {args.warmup} warm batches of each), device events",
         "around each window; us per batch.  'a / b': the filter of the clean view's records / of the augmented view's.",
         "", "$ python tools/resize_bench.py --filters" + (" --parent-lib <the parent commit's libbasd_hip.so>" if args.parent_lib else "")
         + (f" --interpolation {args.interpolation}" if args.interpolation != "bilinear" else "")] + rows + [""] + report) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if args.filters:
    compare_filters()
    sys.exit(0)

rows, report = [], []
conv_med, conv_spread, conv_us = measure(lambda: mixer(out, None, MixParams("none"), out=mixed))
conv_bytes = out.numel() * 3                                      # one byte read, two written
conv_gbps = conv_bytes / (conv_med * 1e-6) / 1e9
rows.append(json.dumps({"case": "BatchMixer convert-only uint8 -> bf16 on the 2 x 256 output images",
                        "us": [round(v, 2) for v in conv_us], "median_us": round(conv_med, 2), "bytes": conv_bytes,
                        "GBps": round(conv_gbps, 1)}))
report.append(f"  {'convert-only mixer':18s} {conv_med:9.2f} us  (spread {conv_spread:.2f})   {conv_gbps:6.0f} GB/s over 3 bytes per "
              "element")
status = torch.zeros(1, dtype=torch.int32, device=dev)
stream = torch._C._cuda_getCurrentRawStream(dev.index)
results = {}
for name, views in (("both views", RZ.VIEWS), ("clean view", ("clean",)), ("augmented view", ("augmented",))):
    rec = RZ.make_records(ragged.sizes, S, RATIO, crops, views=views, interpolation=args.interpolation)
    n = len(rec)
    table = torch.from_numpy(rec.view(np.uint8).copy()).to(dev)
    med, spread, us = measure(lambda: _lib.call("basd_resize_crop", ragged.data.data_ptr(), ragged.data.numel(),
                                                out.data_ptr(), n, C, S, S, table.data_ptr(), status.data_ptr(), 0,
                                                stream))
    nbytes = ragged.data.numel() + n * C * S * S
    copy_us = nbytes / (conv_gbps * 1e9) * 1e6
    gbps = nbytes / (med * 1e-6) / 1e9
    results[name] = med
    rows.append(json.dumps({"case": name, "us": [round(v, 2) for v in us], "median_us": round(med, 2),
                            "spread_us": round(spread, 2), "bytes": nbytes, "GBps": round(gbps, 1),
                            "of_copy": round(copy_us / med, 3)}))
    report.append(f"  {name:18s} {med:9.2f} us  (spread {spread:.2f})   {gbps:6.0f} GB/s   {100 * copy_us / med:5.1f} % of copy")
assert int(status.item()) == 0
call_med, call_spread, call_us = measure(lambda: rc(ragged, crops))
assert rc.status() == 0
rows.append(json.dumps({"case": "ResizeCrop.__call__, both views (table built, copied, launched)",
                        "us": [round(v, 2) for v in call_us], "median_us": round(call_med, 2)}))
report.append(f"  {'whole call':18s} {call_med:9.2f} us  (spread {call_spread:.2f})   both views through ResizeCrop.__call__: the "
              "record table built on the host, one copy, one launch")
t0 = time.perf_counter()
for _ in range(20):
    RZ.make_records(ragged.sizes, S, RATIO, crops)
table_us = (time.perf_counter() - t0) / 20 * 1e6
t0 = time.perf_counter()
for _ in range(20):
    RZ.draw_crop_params(ragged.sizes)
draw_us = (time.perf_counter() - t0) / 20 * 1e6

pillow = "Pillow is not installed here: the host side was not measured"
pil = pillow_windows(args.interpolation)
if pil is not None:
    import PIL
    ms, first = pil
    # the launch and Pillow make the same bytes
    got = rc(ragged, crops)
    for i in (0, B // 2, B - 1):
        assert np.array_equal(got["clean"][i].cpu().numpy(), np.asarray(first[i][0]).transpose(2, 0, 1))
        assert np.array_equal(got["augmented"][i].cpu().numpy(), np.asarray(first[i][1]).transpose(2, 0, 1))
    pil_med = sorted(ms)[len(ms) // 2]
    rows.append(json.dumps({"case": f"Pillow {PIL.__version__} {PIL_FILTER}, both views, {args.threads} threads",
                            "ms": [round(v, 2) for v in ms], "median_ms": round(pil_med, 2),
                            "images_per_s": round(B / pil_med * 1e3)}))
    pillow = (f"Pillow {PIL.__version__} Image.{PIL_FILTER} on {args.threads} host threads, both views of the same decoded images: "
              f"{pil_med:.2f} ms per batch (spread {max(ms) - min(ms):.2f}), {B / pil_med * 1e3:.0f} images/s; the launch of both views "
              f"takes {results['both views'] / 1e3:.2f} ms: {'faster' if results['both views'] / 1e3 < pil_med else 'NOT faster'} "
              f"by a factor of {pil_med / (results['both views'] / 1e3):.1f}; three images compared byte for byte")

text = "\n".join(
    [f"The crops and resizes of one ragged batch, {B} decoded images of {H} x {W} x {C} ({ragged.data.numel()} bytes packed), both",
     f"views to {S} (crop_ratio {RATIO}: the clean view {H} x {W} -> 256 x 341 and its centre, the augmented view a drawn",
     f"RandomResizedCrop window -> 224 x 224), {args.interpolation}, one MI355X: tools/resize_bench.py.  One launch of resize_crop_kernel per batch",
     "(a workgroup per band of output rows and record, the horizontal pass staged in LDS), the packed images and the record",
     f"table already on the device.  One process, {args.repeats} windows of {args.iters} batches after {args.warmup} warm batches, device events around",
     "each window; us per batch, median over the windows (spread = max - min).  GB/s = (every source byte once + every",
     "destination byte once) over that time; 'of copy' = the time the same bytes take at the rate of the convert-only",
     "BatchMixer launch (uint8 in, bf16 out, first row), over the measured time.",
     "", "$ python tools/resize_bench.py" + (f" --interpolation {args.interpolation}" if args.interpolation != "bilinear" else "")]
    + rows + [""] + report
    + ["", f"  on the host per call (Python, per image): drawing the crops {draw_us:.0f} us, building the record table {table_us:.0f} us",
       "  " + pillow]) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text)
print(text)
