"""Time ``GrassmannianLayerSelector._distances`` forward + backward for multi-layer teachers, through the full-K2
route (``small_student_jacobi``) and through the leading vectors + shifted solves.

    python tools/selector_backward_bench.py [--steps 30] [--warmup 5]

Prints one line per (d_s, rows, teacher layers, route): the median of the per-step times between two events."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(os.path.join(ROOT, "vit-inductive-bias-distillation_amd"))

import torch  # noqa: E402

SHAPES = ((64, 8, 32, 96, 3), (96, 32, 64, 192, 4), (192, 32, 196, 384, 12))      # d_s, batch, tokens, d_t, layers


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    from basd_amd import ops
    from basd_amd.losses import GrassmannianLayerSelector
    dev = "cuda:0"
    for d_s, B, n, d_t, L in SHAPES:
        torch.manual_seed(0)
        sel = GrassmannianLayerSelector(2, d_s, d_t).to(dev)
        g = torch.Generator().manual_seed(d_s)
        teachers = []
        for l in range(L):
            z = torch.randn(B * n, d_s, generator=g)
            z[:, l:l + 8] += 10 * torch.randn(B * n, 8, generator=g)
            teachers.append((z @ sel.proj_t.cpu()).view(B, n, d_t).to(dev))
        teachers = ops._check_common_layout([ops.as_supported(t) for t in teachers], "teacher token tensors")
        students = []
        for e in range(2):
            z = torch.randn(B * n, d_s, generator=g)
            z[:, 2:10] += 10 * torch.randn(B * n, 8, generator=g)
            students.append(z.view(B, n, d_s).to(dev))
        for route, jacobi in (("k2", True), ("solves", False)):
            sel.small_student_jacobi = jacobi
            times = []
            for step in range(args.warmup + args.steps):
                leaves = [x.clone().requires_grad_(True) for x in students]
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                d = sel._distances(leaves, list(range(L)), teachers)
                d.sum().backward()
                t1.record()
                torch.cuda.synchronize()
                if step >= args.warmup:
                    times.append(t0.elapsed_time(t1))
            print(f"selector fwd+bwd d_s={d_s} rows={B * n} L={L} route={route}: median {statistics.median(times):.3f} ms "
                  f"(min {min(times):.3f}) over {args.steps} steps")


if __name__ == "__main__":
    main()
