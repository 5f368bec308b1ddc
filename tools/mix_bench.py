"""One training batch prepared two ways on one GPU: (a) ``basd_amd.augment.BatchMixer`` (ONE launch of
``mix_batch_kernel``), (b) the torch-op chain of ``basd_amd.trainer.mixup_cutmix`` with the same forced draw (MixUp:
``lam * x + (1 - lam) * x.roll(1, 0)``; CutMix: ``clone``, ``roll`` and the box copy; targets: ``one_hot``, ``roll`` and
three elementwise ops), preceded for uint8 batches by ``x.float().div(255).sub(mean).div(std)`` and followed for a bf16
destination by ``.to(torch.bfloat16)``.  Neither side draws random numbers or reads anything back inside the timed
window.  Cases at (B, C, H, W) = (256, 3, 224, 224), K = 1000.  One process, the two alternating, ``--repeats`` windows
of ``--iters`` batches each after ``--warmup`` batches, device events around each window, median over the windows.
GB/s of (a) over the algorithmic bytes: the source read once, the destination written once, B * K * 4 of targets.
Writes the report to ``--out`` and prints it.
usage: mix_bench.py [--iters 100] [--warmup 10] [--repeats 5] [--out profiles/mix_batch.txt]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "vit-inductive-bias-distillation_amd"))
import torch
import torch.nn.functional as F
from basd_amd.augment import BatchMixer, MixParams

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=100)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mix_batch.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("mix_bench.py measures on a GPU: none found")
dev = torch.device("cuda", 0)
B, C, H, W, K = 256, 3, 224, 224, 1000
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SCHEDULEFREE_GBPS = 5750.0                 # profiles/schedulefree_step.txt: this project's other streaming kernel
HALF_BOX = (33, 33, 191, 192)              # (x1, y1, x2, y2): 158 x 159 of 224 x 224, about half the area
MIXUP = MixParams("mixup", 0.3141592653589793, None, 0.3141592653589793)
CUTMIX = MixParams("cutmix", 0.5, HALF_BOX, 1.0 - (HALF_BOX[2] - HALF_BOX[0]) * (HALF_BOX[3] - HALF_BOX[1]) / (W * H))
CASES = [("mixup", MIXUP, torch.float32, torch.float32), ("cutmix-half", CUTMIX, torch.float32, torch.float32),
         ("mixup", MIXUP, torch.float32, torch.bfloat16), ("mixup", MIXUP, torch.uint8, torch.float32),
         ("mixup", MIXUP, torch.uint8, torch.bfloat16)]
NAMES = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.uint8: "uint8"}


def build(params, src, dst):
    g = torch.Generator().manual_seed(1)
    if src == torch.uint8:
        images = torch.randint(0, 256, (B, C, H, W), generator=g, dtype=torch.uint8).to(dev)
    else:
        images = torch.randn(B, C, H, W, generator=g).to(dev)
    labels = torch.randint(0, K, (B,), generator=g).to(dev)
    mixer = BatchMixer(K, mean=MEAN, std=STD, out_dtype=dst, device=dev)
    mean = torch.tensor(MEAN, device=dev).view(1, C, 1, 1)
    std = torch.tensor(STD, device=dev).view(1, C, 1, 1)
    keep = {}

    def fused():
        keep["fused"] = mixer(images, labels, params)

    def chain():
        x = images.float().div(255).sub(mean).div(std) if src == torch.uint8 else images
        onehot = F.one_hot(labels, K).to(torch.float32)
        if params.kind == "mixup":
            lam = params.lam
            mixed = lam * x + (1.0 - lam) * x.roll(1, 0)
        else:
            x1, y1, x2, y2 = params.box
            mixed = x.clone()
            mixed[..., y1:y2, x1:x2] = x.roll(1, 0)[..., y1:y2, x1:x2]
        lam = params.lam_targets
        keep["chain"] = (mixed.to(dst), lam * onehot + (1.0 - lam) * onehot.roll(1, 0))

    def agreement():
        a, b = keep["fused"], keep["chain"]
        return {"max_abs_image_difference": float((a[0].float() - b[0].float()).abs().max()),
                "max_abs_target_difference": float((a[1] - b[1]).abs().max())}
    return {"fused": fused, "chain": chain}, agreement


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.iters):
        fn()
    e1.record()
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1) / args.iters                # us per batch


lines, report, verdicts = [], [], []
for name, params, src, dst in CASES:
    sides, agreement = build(params, src, dst)
    for fn in sides.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in sides}
    for _ in range(args.repeats):
        for k, fn in sides.items():
            us[k].append(window(fn))
    med = {k: sorted(v)[len(v) // 2] for k, v in us.items()}
    spread = {k: max(v) - min(v) for k, v in us.items()}
    n = B * C * H * W
    nbytes = n * torch.empty((), dtype=src).element_size() + n * torch.empty((), dtype=dst).element_size() + B * K * 4
    gbps = nbytes / (med["fused"] * 1e-6) / 1e9
    wins = med["chain"] - med["fused"] > spread["chain"] + spread["fused"]
    verdicts.append(wins)
    row = {"case": name, "src": NAMES[src], "dst": NAMES[dst], "B": B, "K": K, "iters": args.iters,
           "repeats": args.repeats, "fused_us": [round(v, 2) for v in us["fused"]],
           "chain_us": [round(v, 2) for v in us["chain"]], "fused_median_us": round(med["fused"], 2),
           "chain_median_us": round(med["chain"], 2), "ratio": round(med["chain"] / med["fused"], 2),
           "bytes": nbytes, "fused_GBps": round(gbps, 1), "fused_wins_by_more_than_both_spreads": bool(wins)}
    row.update(agreement())
    lines.append(json.dumps(row))
    report.append(f"  {name:11s} {NAMES[src]:>5s} -> {NAMES[dst]}: fused {med['fused']:8.2f} us  (spread {spread['fused']:.2f})   "
                  f"chain {med['chain']:8.2f} us  (spread {spread['chain']:.2f})   ratio {med['chain'] / med['fused']:.1f}x   "
                  f"{gbps:.0f} GB/s")
    if (name, src, dst) == ("mixup", torch.float32, torch.float32):
        report.append(f"      fp32 -> fp32 MixUp: {gbps:.0f} GB/s beside the {SCHEDULEFREE_GBPS:.0f} GB/s of the schedule-free "
                      f"step (profiles/schedulefree_step.txt): {100.0 * gbps / SCHEDULEFREE_GBPS:.0f} %")
    del sides, agreement
    torch.cuda.empty_cache()
text = "\n".join(
    ["One training batch, one MI355X: tools/mix_bench.py.  fused = BatchMixer (ONE launch of mix_batch_kernel: mixing,",
     "soft targets, uint8 conversion and normalisation); chain = the torch ops of trainer.mixup_cutmix with the same forced",
     "draw (for uint8 after x.float().div(255).sub(mean).div(std), for bf16 followed by .to(bfloat16)).  One process, the two",
     f"alternating, {args.repeats} windows of {args.iters} batches after {args.warmup} warm batches, device events around "
     "each window;",
     "us per batch, median over the windows (spread = max - min).  GB/s = (source once + destination once + B * K * 4 of",
     "targets) over the fused launch's time.  The max_abs_*_difference fields compare the two sides' last outputs (the chain",
     "is free to contract and to reorder; the bit-exact checks are tests/test_mix_batch.py).",
     "", "$ python tools/mix_bench.py"] + lines + [""] + report
    + ["", "  the fused launch beats the chain by more than the two spreads combined in "
       f"{sum(verdicts)} of {len(verdicts)} cases"]) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text)
print(text)
