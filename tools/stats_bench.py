"""Per-channel sums of uint8 pixels two ways on one GPU: (a) ``basd_amd.stats.ChannelStats.update`` (ONE launch of
``channel_stats_kernel``), (b) torch ops on the device forming the same integers (``x.sum(dims, dtype=int64)`` and
``x.to(int32).square_().sum(dims, dtype=int64)``).  Cases: a (256, 3, 224, 224) batch as CHW, the same bytes as HWC, and
a 64 MiB ragged HWC concatenation (a flat run of whole pixels that starts one byte past a 16-byte boundary).  Each case
runs over ``--buffers`` different buffers in turn, more bytes than the 256 MiB last-level cache holds, so that every
launch reads from HBM ("hbm"), and over one buffer again and again ("resident": served by the caches, a batch that a
previous kernel has just written).  One process, the two sides alternating, ``--repeats`` windows of ``--iters`` calls
after ``--warmup`` calls, device events around each window, median over the windows.  The roofline is the bytes read
once over the datasheet's 8 TB/s; beside it, the share of the 5.75 TB/s that this project's other streaming kernel
reaches (``profiles/schedulefree_step.txt``).
Writes the report to ``--out`` and prints it.
usage: stats_bench.py [--iters 240] [--warmup 12] [--repeats 5] [--buffers 12] [--out profiles/channel_stats.txt]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "vit-inductive-bias-distillation_amd"))
import torch
from basd_amd import _lib
from basd_amd.stats import ChannelStats

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=240)
ap.add_argument("--warmup", type=int, default=12)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--buffers", type=int, default=12)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "channel_stats.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("stats_bench.py measures on a GPU: none found")
dev = torch.device("cuda", 0)
B, C, H, W = 256, 3, 224, 224
RAGGED = (64 << 20) // C * C
HBM_SPEC = 8.0e12
SCHEDULEFREE = 5.746e12                     # profiles/schedulefree_step.txt: this project's other streaming kernel
SWEEP = (64, 128, 256, 384, 0)
CASES = [("batch", "chw", (B, C, H, W), 0), ("batch", "hwc", (B * H * W, C), 0),
         ("ragged-64MiB", "hwc", (RAGGED // C, C), 1)]


def build(layout, shape, offset, count):
    n = 1
    for s in shape:
        n *= s
    g = torch.Generator(device=dev).manual_seed(1)
    views = []
    for _ in range(count):
        raw = torch.randint(0, 256, (n + 16,), generator=g, dtype=torch.uint8, device=dev)
        views.append(raw[offset:offset + n].view(shape))
    stats = ChannelStats(C, device=dev)
    dims = (0, 2, 3) if layout == "chw" else (0,)
    keep = {}

    def kernel(i):
        stats.update(views[i % len(views)], layout)

    def ops(i):
        x = views[i % len(views)]
        keep["ops"] = (x.sum(dims, dtype=torch.int64), x.to(torch.int32).square_().sum(dims, dtype=torch.int64))

    def agreement():
        stats.reset()
        kernel(0)
        ops(0)
        n_px, s1, s2 = stats.sums()
        return {"pixels": n_px, "sums_equal_torch_ops": s1 == keep["ops"][0].tolist() and s2 == keep["ops"][1].tolist()}

    def capped(max_blocks):
        def fn(i):
            x = views[i % len(views)]
            images, pixels = (shape[0], shape[2] * shape[3]) if layout == "chw" else (1, shape[0])
            _lib.call("basd_channel_stats", x.data_ptr(), 1 if layout == "chw" else 0, images, C, pixels,
                      stats.state.data_ptr(), max_blocks, torch._C._cuda_getCurrentRawStream(dev.index))
        return fn
    return {"kernel": kernel, "ops": ops}, agreement, n, capped


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(args.iters):
        fn(i)
    e1.record()
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1) / args.iters                # us per call


lines, report = [], []
for name, layout, shape, offset in CASES:
    for mode, count in (("hbm", args.buffers), ("resident", 1)):
        sides, agreement, nbytes, capped = build(layout, shape, offset, count)
        for fn in sides.values():
            for i in range(args.warmup):
                fn(i)
        torch.cuda.synchronize()
        us = {k: [] for k in sides}
        for _ in range(args.repeats):
            for k, fn in sides.items():
                us[k].append(window(fn))
        med = {k: sorted(v)[len(v) // 2] for k, v in us.items()}
        spread = {k: max(v) - min(v) for k, v in us.items()}
        rate = nbytes / (med["kernel"] * 1e-6)
        row = {"case": name, "layout": layout, "mode": mode, "buffers": count, "buffer_bytes": nbytes,
               "cycled_bytes": nbytes * count, "iters": args.iters, "repeats": args.repeats,
               "kernel_us": [round(v, 2) for v in us["kernel"]], "ops_us": [round(v, 2) for v in us["ops"]],
               "kernel_median_us": round(med["kernel"], 2), "ops_median_us": round(med["ops"], 2),
               "ratio": round(med["ops"] / med["kernel"], 2), "kernel_GBps": round(rate / 1e9, 1),
               "fraction_of_hbm_roofline": round(rate / HBM_SPEC, 3),
               "fraction_of_schedulefree_rate": round(rate / SCHEDULEFREE, 3)}
        row.update(agreement())
        lines.append(json.dumps(row))
        roof = (f"{100.0 * rate / HBM_SPEC:.0f} % of the HBM roofline, {100.0 * rate / SCHEDULEFREE:.0f} % of schedulefree's rate"
                if mode == "hbm"
                else "(cache-resident: not an HBM figure)")
        report.append(f"  {name:13s} {layout} {mode:8s}: {nbytes / 1e6:7.1f} MB  kernel {med['kernel']:8.2f} us (spread "
                      f"{spread['kernel']:.2f})  torch ops {med['ops']:9.2f} us (spread {spread['ops']:.2f})  ratio "
                      f"{med['ops'] / med['kernel']:.1f}x  {rate / 1e9:.0f} GB/s  {roof}")
        if mode == "hbm":
            # the tuning hook: the same launch on fewer workgroups (0 = the entry point's own choice)
            sweep = {}
            for max_blocks in SWEEP:
                fn = capped(max_blocks)
                for i in range(args.warmup):
                    fn(i)
                sweep[max_blocks] = sorted(window(fn) for _ in range(args.repeats))[args.repeats // 2]
            lines.append(json.dumps({"case": name, "layout": layout, "mode": mode, "max_blocks_median_us":
                                     {str(k): round(v, 2) for k, v in sweep.items()}}))
            report.append("      max_blocks " + "  ".join(f"{k}: {v:.2f} us" for k, v in sweep.items()))
        del sides, agreement, capped
        torch.cuda.empty_cache()
text = "\n".join(
    ["Per-channel sums of uint8 pixels, one MI355X: tools/stats_bench.py.  kernel = ChannelStats.update (ONE launch of",
     "channel_stats_kernel: count, sums and sums of squares of every channel, exact 64-bit integers); torch ops = the same",
     "integers as x.sum(dims, dtype=int64) and x.to(int32).square_().sum(dims, dtype=int64).  hbm = the calls cycle over",
     f"{args.buffers} different buffers (more than the 256 MiB last-level cache holds between two uses of a buffer); resident = one",
     f"buffer again and again.  One process, the two sides alternating, {args.repeats} windows of {args.iters} calls after "
     f"{args.warmup} warm calls,",
     "device events around each window; us per call, median over the windows (spread = max - min).  Roofline: the bytes",
     "read once over the datasheet's 8 TB/s; beside it the share of the 5.75 TB/s of profiles/schedulefree_step.txt.",
     "max_blocks lines: the hbm case again through the entry point's tuning hook (a cap on the workgroups; 0 = its own",
     "choice), median of the same windows.",
     "", "$ python tools/stats_bench.py"] + lines + [""] + report) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text)
print(text)
