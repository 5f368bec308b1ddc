"""A real DeiT-S <- ResNet-50 distillation step at batch 256 (stock torch models, random init, synthetic images) around
the HIP loss path: time of the whole step and of its parts, so that the share of the loss is a measured number.
usage: trainer_step_bench.py [--batch 256] [--steps 8] [--dtype bf16|fp32] [--optimizer adamw|schedulefree]
[--mixup torch|fused]  (torch: the op chain of trainer.mixup_cutmix; fused: basd_amd.augment, one launch per batch)
[--teacher resnet50|vit_b] [--attn-capture torch|fused]  (vit_b: a ViT-B/16 teacher, 12 hooked attention layers;
fused: basd_amd.attention on each block's own qkv output, one launch per layer)
[--uint8]  (the loader's contract of mixup="fused" + image_stats: both batches arrive as bytes and are converted and
normalised inside the fused launches)  [--trivial-augment]  (with --uint8: the flip and TrivialAugmentWide of the augmented
batch on the device, basd_amd.trivial_augment, one launch per batch ahead of the mixer)
[--resize-crop]  (with --uint8: the batch is a pinned RaggedBatch of 500 x 375 decoded images, uploaded inside the step;
basd_amd.resize makes both views, one launch)  [--jpeg-decode [serial|parallel]]  (with --resize-crop: the batch is a
pinned JpegBatch of the same pictures as JPEG files (tools/jpeg_bench.make_streams), decoded by basd_amd.jpeg ahead of
the resize launch; parallel: Trainer(jpeg_decode="parallel"), the entropy stage that decodes inside a segment)
[--prefetch V [V ...]] [--windows 1]  (the step is fed from a list of --steps references to the batch through the
trainer's DevicePrefetcher; V is a depth, or DEPTH:lowest for a side stream of the lowest priority; 0, the default, is
the serial path.  Several values: --windows windows of --steps steps for each, alternating in this one process, every
window a host clock around a device synchronise; then the loss alone, timed with events while the side stream holds
the input work of a batch and while it is idle.  Prints GPU_MAX_HW_QUEUES as found in the environment.)
[--teacher-cache]  (resnet50 only: Trainer(teacher_cache=batch) and a batch that carries "index"; the warm steps fill
the cache, then every --prefetch variant is timed twice per round of windows, "uncached" -- the option switched off for
the window: the usual step, the yardstick -- and "cached", in turn in this one process.  "gained" is true only if every
cached window lies below every uncached one.  Also: the loss alone through forward_cached, one store and one load
between events, and the cache's bytes at this batch shape.)"""
import argparse, os, sys, time
from types import SimpleNamespace
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "vit-inductive-bias-distillation_amd"))
import torch
from basd_amd import trainer as T, capture
from tools import stock_models as SM

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--steps", type=int, default=8)
ap.add_argument("--dtype", default="bf16")
ap.add_argument("--optimizer", default="adamw", choices=["adamw", "schedulefree"])
ap.add_argument("--mixup", default="torch", choices=["torch", "fused"])
ap.add_argument("--teacher", default="resnet50", choices=["resnet50", "vit_b"])
ap.add_argument("--attn-capture", default="torch", choices=["torch", "fused"])
ap.add_argument("--uint8", action="store_true")
ap.add_argument("--trivial-augment", action="store_true")
ap.add_argument("--resize-crop", action="store_true")
ap.add_argument("--jpeg-decode", nargs="?", const="serial", choices=("serial", "parallel"), default=None)
ap.add_argument("--prefetch", nargs="+", default=["0"])
ap.add_argument("--windows", type=int, default=1)
ap.add_argument("--teacher-cache", action="store_true")
args = ap.parse_args()


def variant(text):
    depth, _, priority = text.partition(":")
    if not depth.isdigit() or priority not in ("", "default", "lowest"):
        ap.error(f"--prefetch takes DEPTH or DEPTH:lowest (got {text!r})")
    return text, int(depth), priority or "default"


variants = [variant(v) for v in args.prefetch]
if args.uint8 and args.mixup != "fused":
    ap.error("--uint8 needs --mixup fused")
if args.trivial_augment and not args.uint8:
    ap.error("--trivial-augment needs --uint8")
if args.resize_crop and not args.uint8:
    ap.error("--resize-crop needs --uint8")
if args.jpeg_decode and not args.resize_crop:
    ap.error("--jpeg-decode needs --resize-crop")
if args.teacher_cache and args.teacher != "resnet50":
    ap.error("--teacher-cache needs a teacher with one extracted layer (--teacher resnet50)")
files = None
if args.resize_crop:
    # made before the GPU is opened (the pictures are encoded, and for --resize-crop decoded, with Pillow on the host)
    from tools import jpeg_bench
    files, how_made = jpeg_bench.make_streams(args.batch)
dev = torch.device("cuda", 0)
torch.manual_seed(0)
student = SM.StockViT().to(dev)                      # DeiT-S
if args.teacher == "vit_b":
    teacher = SM.make_teacher(SM.StockViT(embed_dim=768, depth=12, num_heads=12, num_classes=0).to(dev), 224)
else:
    teacher = SM.make_teacher(SM.StockResNet().to(dev), 224)
cfg = SimpleNamespace(training=SimpleNamespace(label_smoothing=0.1, learning_rate=1e-3, weight_decay=0.05),
                      basd=SimpleNamespace(num_extraction_points=4),
                      model=SimpleNamespace(num_classes=1000, vit=SimpleNamespace(img_size=224)),
                      data=SimpleNamespace(eval_crop_ratio=0.875))
torch.manual_seed(42)
ac = torch.bfloat16 if args.dtype == "bf16" else None
tr = T.Trainer(student, cfg, teacher, student_info=SM.probe_model(student, 224), autocast_dtype=ac,
               mixup=True if args.mixup == "torch" else "fused", optimizer=args.optimizer,
               attn_capture=args.attn_capture,
               image_stats={"clean": ((0.5,) * 3, (0.25,) * 3), "augmented": ((0.5,) * 3, (0.25,) * 3)} if args.uint8 else None,
               mix_dtype=ac if args.uint8 else None, trivial_augment=args.trivial_augment,
               resize_crop=args.resize_crop,
               jpeg_decode={None: False, "serial": True, "parallel": "parallel"}[args.jpeg_decode],
               teacher_cache=args.batch if args.teacher_cache else None)
g = torch.Generator().manual_seed(1)
B = args.batch
# images with per-image structure (a random colour cast + noise) so that the teacher features are not pure noise
imgs = (torch.randn(B, 3, 1, 1, generator=g) * 2 + torch.randn(B, 3, 224, 224, generator=g)).to(dev)
batch = {"clean": imgs, "augmented": imgs.flip(3), "label": torch.randint(0, 1000, (B,), generator=g).to(dev)}
step_batch = batch
if args.uint8:
    # the same images as bytes (x = 255 (0.5 + 0.25 v), clamped); the parts below keep the float batch
    as_bytes = lambda t: (t * 0.25 + 0.5).clamp_(0, 1).mul_(255).to(torch.uint8)
    step_batch = {"clean": as_bytes(imgs), "augmented": as_bytes(imgs.flip(3)), "label": batch["label"]}
if args.jpeg_decode:
    from basd_amd.jpeg import pack_jpegs
    step_batch = {"images": pack_jpegs(files).pin_memory(), "label": batch["label"]}
elif args.resize_crop:
    from basd_amd.jpeg import pillow_fallback
    from basd_amd.resize import pack_images
    step_batch = {"images": pack_images([pillow_fallback(f) for f in files]).pin_memory(), "label": batch["label"]}
if args.teacher_cache:
    step_batch = dict(step_batch, index=torch.randperm(B, generator=g))      # the "dataset" is this one batch


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


from basd_amd.prefetch import DevicePrefetcher
feed = [step_batch] * args.steps
prefetchers = {name: DevicePrefetcher(tr.prepare_batch, device=dev, depth=depth, priority=priority)
               for name, depth, priority in variants}


# with --teacher-cache every variant runs in two modes; "uncached" switches the option off for the window
modes = ("uncached", "cached") if args.teacher_cache else (None,)
cache = tr.teacher_cache                                    # the capacity, until the first step has built the cache
label = lambda name, mode: name if mode is None else f"{name}/{mode}"


def window(name, mode=None):
    """--steps steps through the trainer's prefetcher, as _train_epoch feeds them (its metrics code aside)."""
    global out
    tr._prefetcher = prefetchers[name]
    tr.teacher_cache = cache if mode == "cached" else None
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for prepared in tr._prefetcher.iterate(feed):
        out = tr.step_prepared(prepared)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / args.steps * 1e3


for name in prefetchers:                                   # warm-up: every variant once (its stream, its events)
    for mode in modes:                                     # (cached: the first step misses and fills, the second hits)
        tr._prefetcher = prefetchers[name]
        tr.teacher_cache = cache if mode == "cached" else None
        for prepared in tr._prefetcher.iterate(feed[:2]):
            out = tr.step_prepared(prepared)
        if mode == "cached":
            cache = tr.teacher_cache
windows = {label(name, mode): [] for name in prefetchers for mode in modes}
losses = {key: [] for key in windows}                      # the last step's loss of every window
for _ in range(args.windows):
    for name in prefetchers:
        for mode in modes:
            windows[label(name, mode)].append(round(window(name, mode), 2))
            losses[label(name, mode)].append(round(float(out["loss"]), 4))
tr.teacher_cache = None
step_ms = sum(windows[label(variants[0][0], modes[0])]) / args.windows
acx = torch.autocast("cuda", dtype=ac, enabled=ac is not None)


def fwd_student():
    with acx:
        return capture._extract_student(tr.model, batch["augmented"], tr.basd_loss.token_layers,
                                        layer_paths=tr._student_layer_paths, has_cls_token=True)


def fwd_teacher():
    with acx:
        return capture.extract_intermediates(teacher, batch["clean"], attn=args.attn_capture)


with torch.no_grad():
    s_ms = timed(fwd_student, args.steps)
t_ms = timed(fwd_teacher, args.steps)
logits, s_tok = fwd_student()
t_tok, t_att = fwd_teacher()
s_leaf = {k: v.detach().requires_grad_(True) for k, v in s_tok.items()}
lg = logits.detach().float().requires_grad_(True)


def loss_only():
    loss = tr.basd_loss(lg, batch["label"], s_leaf, t_tok, t_att)
    loss.backward()


loss_only()
l_ms = timed(loss_only, args.steps)


def loss_by_events(side):
    """The loss alone between two events on its own stream; with ``side`` the input work of one batch is queued on
    that stream ahead of every call, so the loss's four streams share the hardware queues with a fifth busy one."""
    pairs = []
    torch.cuda.synchronize()
    for _ in range(args.steps):
        if side is not None:
            with torch.cuda.stream(side):
                tr.prepare_batch(step_batch)
        pairs.append((torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)))
        pairs[-1][0].record()
        loss_only()
        pairs[-1][1].record()
    torch.cuda.synchronize()
    return round(sum(a.elapsed_time(b) for a, b in pairs) / args.steps, 2)


loss_events = {"side_idle": loss_by_events(None)}
for name, pf in prefetchers.items():
    if pf.stream is not None:
        loss_events[f"side_busy[{name}]"] = loss_by_events(pf.stream)
cache_report = None
if args.teacher_cache:
    from basd_amd.ops import TeacherSide
    loss_only()
    side = TeacherSide(*(t.clone() for t in tr.basd_loss.last_teacher_side()))
    index_host = step_batch["index"]
    index_dev = index_host.to(dev)

    def loss_cached():
        loss = tr.basd_loss.forward_cached(lg, batch["label"], s_leaf, cache.load(index_host, device_index=index_dev))
        loss.backward()

    def by_events(fn):
        pairs = []
        torch.cuda.synchronize()
        for _ in range(args.steps):
            pairs.append((torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)))
            pairs[-1][0].record()
            fn()
            pairs[-1][1].record()
        torch.cuda.synchronize()
        return round(sum(a.elapsed_time(b) for a, b in pairs) / args.steps, 4)

    loss_cached()
    cache_report = {
        "loss_fwd_bwd_cached_ms": round(timed(loss_cached, args.steps), 2),
        "loss_fwd_bwd_cached_ms_by_events": by_events(loss_cached),
        "store_ms_by_events": by_events(lambda: cache.store(index_host, side, device_index=index_dev)),
        "load_ms_by_events": by_events(lambda: cache.load(index_host, device_index=index_dev).tensors()),
        "n": cache.n, "n_s": cache.n_s, "capacity": cache.capacity, "nbytes": cache.nbytes,
        "record_bytes": cache.record_bytes(cache.n, cache.n_s),
        "mean_ms": {key: round(sum(v) / len(v), 2) for key, v in windows.items()},
        # every cached window below every uncached one, per variant
        "gained": {name: max(windows[f"{name}/cached"]) < min(windows[f"{name}/uncached"]) for name in prefetchers}}
print({"batch": B, "dtype": args.dtype, "optimizer": args.optimizer, "mixup": args.mixup, "teacher": args.teacher,
       "attn_capture": args.attn_capture, "uint8": args.uint8, "trivial_augment": args.trivial_augment, "resize_crop": args.resize_crop,
       "jpeg_decode": args.jpeg_decode, "prefetch": args.prefetch, "steps": args.steps, "step_ms": round(step_ms, 2),
       "step_ms_windows": windows, "loss_windows": losses, "images_per_s": round(B / step_ms * 1e3, 1),
       "student_fwd_nograd_ms": round(s_ms, 2), "teacher_fwd_ms": round(t_ms, 2), "loss_fwd_bwd_ms": round(l_ms, 2),
       "loss_fwd_bwd_ms_by_events": loss_events, "GPU_MAX_HW_QUEUES": os.environ.get("GPU_MAX_HW_QUEUES", "unset"),
       "loss_share": round(l_ms / step_ms, 3), "loss": float(out["loss"]), "ranks": dict(tr.basd_loss.layer_selector.subspace_ranks),
       **({"teacher_cache": cache_report} if cache_report is not None else {})})
