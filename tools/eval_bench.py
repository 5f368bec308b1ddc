"""One validation batch of logits, two ways, on one GPU: (a) ``basd_amd.evaluation.EvalAccumulator.update`` (ONE launch of
``eval_batch_kernel``), (b) what the reference's ``evaluate_model`` queues per batch, restated with torch ops on the
device: the column gather ``outputs[:, valid_indices]`` (when there is one), ``F.cross_entropy * B`` added to a running
total, and two ``topk`` + compare + sum chains (top-1, top-5) -- without the input checks ``torchmetrics`` adds.  Neither
side reads anything back inside the timed window.  Cases (B, C, K) = (256, 1000, 1000) and (256, 1000, 200), fp32 and
bf16 logits, label smoothing 0.1.  One process, the two alternating, ``--repeats`` windows of ``--iters`` batches each
after ``--warmup`` batches, device events around each window, median over the windows.  GB/s of (a): B * K * element
size read + 40 B of atomics per workgroup of four rows.  Writes the report to ``--out`` and prints it.
usage: eval_bench.py [--iters 500] [--warmup 50] [--repeats 5] [--out profiles/eval_batch.txt]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "vit-inductive-bias-distillation_amd"))
import torch
import torch.nn.functional as F
from basd_amd.evaluation import EvalAccumulator

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=500)
ap.add_argument("--warmup", type=int, default=50)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_batch.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("eval_bench.py measures on a GPU: none found")
dev = torch.device("cuda", 0)
EPS, TOP_K = 0.1, 5
CASES = [(256, 1000, 1000), (256, 1000, 200)]


def make_case(B, C, K, dtype):
    g = torch.Generator().manual_seed(1000 * K + (dtype == torch.bfloat16))
    index = None if K == C else torch.randperm(C, generator=g)[:K].tolist()
    logits = 2.0 * torch.randn(B, C, generator=g)
    targets = torch.randint(0, K, (B,), generator=g)
    cols = targets if index is None else torch.tensor(index)[targets]
    logits[torch.arange(B), cols] += (torch.rand(B, generator=g) < 0.5).float() * 4.0
    return logits.to(dtype).to(dev), targets.to(dev), index


def build(B, C, K, dtype):
    logits, targets, index = make_case(B, C, K, dtype)
    acc = EvalAccumulator(C, valid_indices=index, label_smoothing=EPS, top_k=TOP_K, device=dev)
    index_t = None if index is None else torch.tensor(index, device=dev)
    totals = {"loss": torch.zeros((), device=dev), "top1": torch.zeros((), dtype=torch.long, device=dev),
              "top5": torch.zeros((), dtype=torch.long, device=dev), "rows": 0}

    def kernel():
        acc.update(logits, targets)

    def restated():
        z = logits if index_t is None else logits[:, index_t]
        totals["loss"] += F.cross_entropy(z, targets, label_smoothing=EPS) * B
        totals["top1"] += (z.topk(1, dim=1).indices == targets[:, None]).any(1).sum()
        totals["top5"] += (z.topk(TOP_K, dim=1).indices == targets[:, None]).any(1).sum()
        totals["rows"] += B

    def results():
        out = acc.compute()
        n = totals["rows"]
        return out, {"val_acc": 100.0 * totals["top1"].item() / n, "val_acc_top5": 100.0 * totals["top5"].item() / n,
                     "loss": totals["loss"].item() / n}
    return {"kernel": kernel, "restated": restated}, results


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.iters):
        fn()
    e1.record()
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1) / args.iters                # us per batch


lines, report = [], []
for B, C, K in CASES:
    for dtype, name in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
        sides, results = build(B, C, K, dtype)
        for fn in sides.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        us = {k: [] for k in sides}
        for _ in range(args.repeats):
            for k, fn in sides.items():
                us[k].append(window(fn))
        med = {k: sorted(v)[len(v) // 2] for k, v in us.items()}
        ours, theirs = results()
        nbytes = B * K * (4 if dtype == torch.float32 else 2) + 40 * ((B + 3) // 4)
        row = {"B": B, "C": C, "K": K, "dtype": name, "iters": args.iters, "repeats": args.repeats,
               "kernel_us": [round(v, 2) for v in us["kernel"]], "restated_us": [round(v, 2) for v in us["restated"]],
               "kernel_median_us": round(med["kernel"], 2), "restated_median_us": round(med["restated"], 2),
               "ratio": round(med["restated"] / med["kernel"], 2), "bytes": nbytes,
               "kernel_GBps": round(nbytes / (med["kernel"] * 1e-6) / 1e9, 1), "kernel_metrics": ours,
               "restated_metrics": theirs}
        lines.append(json.dumps(row))
        report.append(f"  B={B} C={C} K={K:4d} {name}: kernel {med['kernel']:8.2f} us  (spread "
                      f"{max(us['kernel']) - min(us['kernel']):.2f})   restated {med['restated']:8.2f} us  (spread "
                      f"{max(us['restated']) - min(us['restated']):.2f})   ratio {med['restated'] / med['kernel']:.1f}x   "
                      f"{row['kernel_GBps']} GB/s")
text = "\n".join(
    ["One validation batch, one MI355X: tools/eval_bench.py.  kernel = EvalAccumulator.update (ONE launch of",
     "eval_batch_kernel); restated = gather + F.cross_entropy * B + two topk / compare / sum chains with torch ops on the",
     "device (what the reference's evaluate_model queues per batch, without the torchmetrics input checks).  One process,",
     f"the two alternating, {args.repeats} windows of {args.iters} batches after {args.warmup} warm batches, device events "
     "around each window;",
     "us per batch, median over the windows (spread = max - min).  GB/s = (B * K * element size + 40 B of atomics per",
     "workgroup) over the kernel's time.",
     "", "$ python tools/eval_bench.py"] + lines + [""] + report) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text)
print(text)
