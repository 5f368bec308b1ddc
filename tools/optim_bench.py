"""The optimizer step alone on the parameter list of DeiT-S (``stock_models.StockViT()``: 22 050 664 elements in ~150
tensors, plus the selector's 4 temperatures as a second group): (a) ``torch.optim.AdamW`` as the trainer builds it +
``zero_grad(set_to_none=False)``, (b) the same with ``fused=True``, (c) ``basd_amd.optim.AdamWScheduleFree`` with
``zero_grad_in_step=True`` (one HIP launch).  One process, the three alternating, ``--repeats`` windows of ``--steps``
steps each after ``--warmup`` steps, timed with device events.  GB/s of (c): 32 B per element (4 reads, 3 writes and the
zeroing), 28 B without the zeroing, against the 8 TB/s HBM figure of the project's roofline.
usage: optim_bench.py [--steps 50] [--warmup 10] [--repeats 3] [--only adamw|fused|schedulefree]"""
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
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--only", default=None, choices=["adamw", "fused", "schedulefree"])
args = ap.parse_args()
dev = torch.device("cuda", 0)
HBM_TBS = 8.0
LR, WD = 1e-3, 0.05

with torch.device("meta"):
    shapes = [p.shape for p in SM.StockViT().parameters()]
numel = sum(s.numel() for s in shapes)


def make_params():
    g = torch.Generator().manual_seed(0)
    params = [torch.nn.Parameter((0.02 * torch.randn(s, generator=g)).to(dev)) for s in shapes]
    extra = [torch.nn.Parameter(torch.full((4,), 0.5413, device=dev))]
    for p in params + extra:
        p.grad = (1e-3 * torch.randn(p.shape, generator=g)).to(dev)
    return params, extra


def build(kind):
    params, extra = make_params()
    if kind == "schedulefree":
        opt = AdamWScheduleFree(params, lr=LR, weight_decay=WD, zero_grad_in_step=True)
        opt.add_param_group({"params": extra})
        opt.train()
        return opt.step
    opt = torch.optim.AdamW(params, lr=LR, weight_decay=WD, **({"fused": True} if kind == "fused" else {}))
    opt.add_param_group({"params": extra})

    def step():
        opt.step()
        opt.zero_grad(set_to_none=False)
    return step


kinds = [args.only] if args.only else ["adamw", "fused", "schedulefree"]
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
out = {"elements": numel + 4, "tensors": len(shapes) + 1, "steps": args.steps, "repeats": args.repeats}
for k in kinds:
    best, worst = min(ms[k]), max(ms[k])
    out[k] = {"ms_per_step": [round(v, 4) for v in ms[k]], "median_ms": round(sorted(ms[k])[len(ms[k]) // 2], 4),
              "spread_ms": round(worst - best, 4)}
if "schedulefree" in ms:
    med = out["schedulefree"]["median_ms"]
    gbs = 32.0 * (numel + 4) / (med * 1e-3) / 1e9
    out["schedulefree"].update({"GBps_at_32B": round(gbs, 1), "GBps_at_28B": round(gbs * 28 / 32, 1),
                                "share_of_8TBps_at_32B": round(gbs / (HBM_TBS * 1e3), 3)})
print(json.dumps(out))
