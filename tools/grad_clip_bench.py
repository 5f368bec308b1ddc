"""What global-norm clipping and the non-finite guard cost around the schedule-free step, on the parameter list of DeiT-S
(the set-up of ``optim_bench.py``: ``stock_models.StockViT()``, 22 050 664 elements in ~150 tensors, plus the selector's 4
temperatures as a second group; ``zero_grad_in_step=True``):
(a) ``plain``: ``AdamWScheduleFree.step()``, one launch;
(b) ``torch_clip``: ``torch.nn.utils.clip_grad_norm_(params, 1.0, foreach=True)`` followed by (a);
(c) ``clipped``: ``AdamWScheduleFree(max_grad_norm=1.0, skip_nonfinite=True).step()``, two launches.
One process, the three alternating, ``--repeats`` windows of ``--steps`` steps each after ``--warmup`` steps, timed with
device events.  As in ``optim_bench.py`` the first step zeroes the gradients and they stay zero: none of the three does
less for that (the multiplication by the coefficient is unconditional in ``clip_grad_norm_`` and in the kernel, and no
kernel branches on a value).  (c) counts as faster than (b) only if EVERY window of (c) is below EVERY window of (b).
usage: grad_clip_bench.py [--steps 50] [--warmup 10] [--repeats 5]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "vit-inductive-bias-distillation_amd"))
import torch
from basd_amd.optim import AdamWScheduleFree
from tools import stock_models as SM

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--repeats", type=int, default=5)
args = ap.parse_args()
dev = torch.device("cuda", 0)
LR, WD = 1e-3, 0.05

with torch.device("meta"):
    shapes = [p.shape for p in SM.StockViT().parameters()] + [torch.Size([4])]
numel = sum(s.numel() for s in shapes)


def build(kind):
    """``step()`` of one variant over its own parameters and gradients."""
    g = torch.Generator().manual_seed(0)
    params = [torch.nn.Parameter((0.02 * torch.randn(s, generator=g)).to(dev)) for s in shapes]
    for p in params:
        p.grad = (1e-3 * torch.randn(p.shape, generator=g)).to(dev)
    kw = dict(max_grad_norm=1.0, skip_nonfinite=True) if kind == "clipped" else {}
    opt = AdamWScheduleFree(params[:-1], lr=LR, weight_decay=WD, zero_grad_in_step=True, **kw)
    opt.add_param_group({"params": params[-1:]})
    opt.train()
    if kind != "torch_clip":
        return opt.step

    def step():
        torch.nn.utils.clip_grad_norm_(params, 1.0, foreach=True)
        opt.step()
    return step


kinds = ["plain", "torch_clip", "clipped"]
steps = {k: build(k) for k in kinds}
for k in kinds:
    for _ in range(args.warmup):
        steps[k]()
torch.cuda.synchronize()
ms = {k: [] for k in kinds}
for _ in range(args.repeats):
    for k in kinds:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            steps[k]()
        e1.record()
        e1.synchronize()
        ms[k].append(e0.elapsed_time(e1) / args.steps)
out = {"elements": numel, "tensors": len(shapes), "steps": args.steps, "repeats": args.repeats}
for k in kinds:
    out[k] = {"ms_per_step": [round(v, 4) for v in ms[k]], "median_ms": round(sorted(ms[k])[len(ms[k]) // 2], 4),
              "spread_ms": round(max(ms[k]) - min(ms[k]), 4)}
out["clipped_every_window_faster_than_torch_clip"] = max(ms["clipped"]) < min(ms["torch_clip"])
out["clipped_over_plain_ms"] = round(out["clipped"]["median_ms"] - out["plain"]["median_ms"], 4)
out["torch_clip_over_plain_ms"] = round(out["torch_clip"]["median_ms"] - out["plain"]["median_ms"], 4)
print(json.dumps(out))
