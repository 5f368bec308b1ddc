"""The teacher side computed by itself, measured on a DeiT-S <- ResNet-50 trainer (stock torch models, random init,
synthetic uint8 images, bf16, AdamW, mixup="fused"): the fill pass, the call alone, and partly cached steps.
usage: teacher_fill_bench.py [--batch 256] [--images 2048] [--fill-batch 256 1024] [--partial 32] [--missing 1 32 128]
[--steps 20] [--windows 5] [--out profiles/teacher_fill.txt]

1. Trainer.fill_teacher_cache over --images pinned host images at every --fill-batch with as_batch=--batch: images/s of
   the whole pass (host clock around a device synchronise, three passes behind a warm one), and its three stages --
   teacher forward, BASDLoss.teacher_side, TeacherCache.store -- between events on one batch of that size.
2. Steps with teacher_partial=--partial and m of --batch images missing (m in --missing; the rows are marked unseen
   again on the host ahead of every step) against "uncached" (the options switched off: the yardstick) and "cached"
   (every row filled) windows: --windows rounds, every round one window of --steps steps of each mode in turn.  A mode
   has GAINED on another only if every one of its windows lies below every window of the other.
3. ops.procrustes_teacher_side alone at the step's teacher shape beside BASDLoss.forward and forward_cached (forward and
   backward), same process behind the windows, host clock and events.
The report goes to stdout and to --out."""
import argparse, os, sys, time
from types import SimpleNamespace
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "vit-inductive-bias-distillation_amd"))
import torch
from basd_amd import capture, ops, trainer as T
from basd_amd.augment import MixParams
from tools import stock_models as SM

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--images", type=int, default=2048)
ap.add_argument("--fill-batch", type=int, nargs="+", default=[256, 1024])
ap.add_argument("--partial", type=int, default=32)
ap.add_argument("--missing", type=int, nargs="+", default=[1, 32, 128])
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
B, N = args.batch, args.images
if N % B or any(N % fb for fb in args.fill_batch):
    ap.error("--images must be a multiple of --batch and of every --fill-batch")

dev = torch.device("cuda", 0)
torch.manual_seed(0)
student = SM.StockViT().to(dev)                      # DeiT-S
teacher = SM.make_teacher(SM.StockResNet().to(dev), 224)
cfg = SimpleNamespace(training=SimpleNamespace(label_smoothing=0.1, learning_rate=1e-3, weight_decay=0.05),
                      basd=SimpleNamespace(num_extraction_points=4),
                      model=SimpleNamespace(num_classes=1000, vit=SimpleNamespace(img_size=224)),
                      data=SimpleNamespace(eval_crop_ratio=0.875))
torch.manual_seed(42)
stats = {"clean": ((0.5,) * 3, (0.25,) * 3), "augmented": ((0.5,) * 3, (0.25,) * 3)}
tr = T.Trainer(student, cfg, teacher, student_info=SM.probe_model(student, 224), autocast_dtype=torch.bfloat16,
               mixup="fused", image_stats=stats, mix_dtype=torch.bfloat16, teacher_cache=N, teacher_partial=args.partial)
g = torch.Generator().manual_seed(1)
# per-image structure (a colour cast + noise), as bytes, pinned: the fill pass uploads them
images = torch.empty((N, 3, 224, 224), dtype=torch.uint8).pin_memory()
for i in range(0, N, B):
    x = torch.randn(B, 3, 1, 1, generator=g) * 2 + torch.randn(B, 3, 224, 224, generator=g)
    images[i:i + B] = (x * 0.25 + 0.5).clamp_(0, 1).mul_(255).to(torch.uint8)
labels = torch.randint(0, 1000, (N,), generator=g)
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def host_ms(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def event_ms(fn, n):
    pairs = []
    torch.cuda.synchronize()
    for _ in range(n):
        pairs.append((torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)))
        pairs[-1][0].record()
        fn()
        pairs[-1][1].record()
    torch.cuda.synchronize()
    return sum(a.elapsed_time(b) for a, b in pairs) / n


say(f"tools/teacher_fill_bench.py --batch {B} --images {N} --fill-batch {' '.join(map(str, args.fill_batch))} "
    f"--partial {args.partial} --missing {' '.join(map(str, args.missing))} --steps {args.steps} --windows {args.windows}")
say(f"GPU_MAX_HW_QUEUES in effect: {os.environ.get('GPU_MAX_HW_QUEUES', 'unset')} (read from the environment; nothing "
    "here sets it).")

# ---- 1. the fill pass -------------------------------------------------------------------------------------------
acx = torch.autocast("cuda", dtype=torch.bfloat16)
say()
say(f"1. Trainer.fill_teacher_cache over {N} pinned uint8 images, as_batch={B}")
for fb in args.fill_batch:
    loader = [{"clean": images[i:i + fb], "index": torch.arange(i, i + fb)} for i in range(0, N, fb)]
    assert tr.fill_teacher_cache(loader, as_batch=B) == N                  # warm: this shape's convolution search
    passes = [host_ms(lambda: tr.fill_teacher_cache(loader, as_batch=B), 1) for _ in range(3)]
    # the three stages between events, on one batch of this size already on the device
    clean, _ = tr._clean_mixer(loader[0]["clean"].to(dev), None, MixParams("none"))
    index = loader[0]["index"]
    index_dev = index.to(dev)
    state = {}

    def forward():
        with acx:
            state["tokens"], state["attns"] = capture.extract_intermediates(teacher, clean, attn="torch")

    def side():
        state["side"] = tr.basd_loss.teacher_side(state["tokens"], state["attns"], as_batch=B)

    forward(), side()
    parts = (event_ms(forward, 5), event_ms(side, 20),
             event_ms(lambda: tr.teacher_cache.store(index, state["side"], device_index=index_dev), 20))
    say(f"   fill batch {fb:5d}: " + "  ".join(f"{N / p * 1e3:8.0f}" for p in passes) + "  images/s  (passes of "
        + ", ".join(f"{p:.1f}" for p in passes) + " ms)")
    say(f"      per batch between events: teacher forward {parts[0]:.3f} ms, teacher side {parts[1]:.4f} ms, "
        f"store {parts[2]:.4f} ms  ({fb / sum(parts) * 1e3:.0f} images/s for the three alone)")
    del clean, state
cache = tr.teacher_cache
say(f"   cache: n = {cache.n}, n_s = {cache.n_s}, {cache.record_bytes(cache.n, cache.n_s)} bytes per image, "
    f"{cache.nbytes} bytes for {cache.capacity} rows")

order = torch.randperm(B, generator=g)
step_batch = {"clean": images[:B].to(dev), "augmented": images[:B].flip(3).to(dev), "label": labels[:B].to(dev),
              "index": order}

# ---- 2. partly cached steps -------------------------------------------------------------------------------------
modes = ["uncached", "cached"] + [f"partial-{m}" for m in args.missing]
unseen = order[torch.randperm(B, generator=g)]             # which dataset rows a partial mode marks unseen, in this order
teacher_batches = {}
out = None


def feed(mode, steps):
    for _ in range(steps):
        if mode.startswith("partial-"):
            cache._filled[unseen[:int(mode.split("-")[1])].numpy()] = False
        yield step_batch


def window(mode, steps=args.steps):
    global out
    tr.teacher_cache = None if mode == "uncached" else cache
    tr.teacher_partial = args.partial if mode.startswith("partial-") else 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for prepared in tr._prefetcher.iterate(feed(mode, steps)):
        rows = prepared.get("teacher_rows")
        teacher_batches[mode] = 0 if "clean" not in prepared else prepared["clean"].shape[0]
        assert mode == "uncached" or mode == "cached" or (rows is not None and rows.numel() > 0)
        out = tr.step_prepared(prepared)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


assert cache.has(order)
tr.model.train()
for mode in modes:                                         # warm-up: every mode's shapes (the teacher's batch sizes)
    window(mode, 2)
windows = {mode: [] for mode in modes}
losses = {mode: [] for mode in modes}
for _ in range(args.windows):
    for mode in modes:
        windows[mode].append(window(mode))
        losses[mode].append(float(out["loss"]))
tr._finish_loss()
say()
say(f"2. Steps at batch {B}, teacher_partial={args.partial}: {args.windows} rounds, every round one window of {args.steps} "
    "steps of each mode in turn; ms per step (host clock around a device synchronise)")
for mode in modes:
    w = windows[mode]
    say(f"   {mode:12s} " + " ".join(f"{x:6.2f}" for x in w) + f"     mean {sum(w) / len(w):6.2f}   (teacher batch "
        f"{teacher_batches[mode]})")
for mode in modes[2:]:
    for other in ("uncached", "cached"):
        a, b = windows[mode], windows[other]
        if max(a) < min(b):
            verdict = f"GAINED on {other}: every window below every {other} window, by {min(b) - max(a):.2f} to {max(b) - min(a):.2f} ms"
        elif min(a) > max(b):
            verdict = f"slower than {other}: every window above every {other} window, by {min(a) - max(b):.2f} to {max(a) - min(b):.2f} ms"
        else:
            verdict = f"not separated from {other}: the windows overlap"
        say(f"   {mode} {verdict}")
say("   losses of the last step of every window (the model trains on one batch; the modes take turns on the same weights):")
for mode in modes:
    say(f"   {mode:12s} " + " ".join(f"{x:.4f}" for x in losses[mode]))
# ---- 3. the call alone, behind the windows (a warm process: plans, streams and the allocator have settled) ---------
prepared = tr.prepare_batch(dict(step_batch, index=torch.arange(N - B, N)))       # floats for the parts below
with acx, torch.no_grad():
    logits, s_tok = capture._extract_student(tr.model, prepared["augmented"], tr.basd_loss.token_layers,
                                             layer_paths=tr._student_layer_paths, has_cls_token=True)
clean_f, _ = tr._clean_mixer(step_batch["clean"], None, MixParams("none"))
with acx:
    t_tok, t_att = capture.extract_intermediates(teacher, clean_f, attn="torch")
s_leaf = {k: v.detach().requires_grad_(True) for k, v in s_tok.items()}
lg = logits.detach().float().requires_grad_(True)
index_dev = order.to(dev)
tokens = t_tok[0]


def loss_forward():
    tr.basd_loss(lg, step_batch["label"], s_leaf, t_tok, t_att).backward()


def loss_cached():
    tr.basd_loss.forward_cached(lg, step_batch["label"], s_leaf, cache.load(order, device_index=index_dev)).backward()


def side_alone():
    return ops.procrustes_teacher_side(tokens, t_att[0], False, tr.basd_loss.num_student_tokens, as_batch=B)


for _ in range(3):
    loss_forward(), loss_cached(), side_alone()
say()
say(f"3. The call alone, teacher tokens {tuple(tokens.shape)} {tokens.dtype} strides {tokens.stride()}, n_s = "
    f"{tr.basd_loss.num_student_tokens}, g_splits = {ops.teacher_gram_splits(B, tokens.shape[2])}; ms, host clock / "
    f"between events, {args.steps} calls")
for name, fn in (("BASDLoss.forward + backward", loss_forward), ("BASDLoss.forward_cached + backward", loss_cached),
                 ("ops.procrustes_teacher_side", side_alone)):
    say(f"   {name:36s} {host_ms(fn, args.steps):7.3f} / {event_ms(fn, args.steps):7.3f}")
tr._finish_loss()

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
