"""Numbers behind the default thresholds of the residual check (include/basd_hip.h) and the cost of its launches.

    python tools/tridiag_check_measure.py [--cpu-only] [--orders 45,200,...]

1. rho_trace / rho_fro / rho_res of fp32 LAPACK ``ssytrd`` (reflectors applied in fp32 on the CPU) and of this library's
   own factorisations, on a ``randn`` Gram and the families of tests/test_hard_spectra.py, per order; the worst values
   as multiples of sqrt(n).
2. Single-entry corruptions of a good factorisation (d, e, tau, vh of matrix 1 of 3) under the default thresholds.
3. Device-event times of the probe launch and of the two launches behind the factorisation (``basd_tridiag_apply_q`` on
   two rows + the check) at (n, batch) = (384, 3), (768, 28), (1024, 8), against the bytes the probe has to read.
The matrix families and the numpy restatement of the ratios are those of tests/test_tridiag_check.py."""
import argparse
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "vit-inductive-bias-distillation_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import test_tridiag_check as T  # noqa: E402

NAMES = ("rho_trace", "rho_fro", "rho_res")


def ratios_table(orders, gpu):
    from basd_amd import ops
    worst, flagged, plain = {}, [], {"lapack": (0.0, ""), "library": (0.0, "")}     # plain: rho_res as it is
    for n in orders:
        fams = T.MEASURE_FAMILIES
        got = None
        if gpu:
            G = torch.from_numpy(np.stack([T.matrix(f, n) for f in fams])).cuda()
            ts = ops.tridiagonalise(G, check=True)
            torch.cuda.synchronize()
            assert int(ts.err[0].item()) == 0
            got = ts.check.ratios.cpu().tolist()
        laps = [T.ratios(T.matrix(f, n), *T.lapack_factor(T.matrix(f, n)), i) for i, f in enumerate(fams)]
        lap_worst = [max(r[k] for r in laps) for k in range(3)]         # of this order, over the families
        for i, f in enumerate(fams):
            lap = laps[i]
            line = f"n={n:5d} {f:10s} lapack " + " ".join(f"{v:8.3f}" for v in lap)
            for k in range(3):
                worst[("lapack", k)] = max(worst.get(("lapack", k), (0, 0, "")), (lap[k] / math.sqrt(n), lap[k], f"{f} {n}"))
            plain["lapack"] = max(plain["lapack"], (lap[2], f"{f} {n}"))
            if got is not None:
                line += "   library " + " ".join(f"{v:8.3f}" for v in got[i])
                plain["library"] = max(plain["library"], (got[i][2], f"{f} {n}"))
                for k in range(3):
                    worst[("library", k)] = max(worst.get(("library", k), (0, 0, "")),
                                                (got[i][k] / math.sqrt(n), got[i][k], f"{f} {n}"))
                    if got[i][k] > 8 * lap[k]:
                        line += f"   <-- {NAMES[k]} more than 8 x LAPACK's on this family"
                        flagged.append((f, n, NAMES[k], got[i][k], lap[k], lap_worst[k]))
            print(line, flush=True)
    for (who, k), (per, val, where) in sorted(worst.items()):
        print(f"worst {who:8s} {NAMES[k]:10s} {val:8.3f} = {per:.4f} sqrt(n) at {where}")
    for who in ("lapack", "library") if gpu else ("lapack",):
        print(f"worst {who:8s} rho_res as a plain value (it does not grow with n): {plain[who][0]:.3f} at {plain[who][1]}")
    print(f"families where the library exceeds 8 x LAPACK's value on the same family: {len(flagged)}")
    for f, n, name, lib, lap, lap_w in flagged:
        print(f"   {f} {n}: {name} {lib:.3f} against {lap:.3f} (LAPACK's worst {name} over the families of order {n}: "
              f"{lap_w:.3f}; 8 x that {'IS' if lib > 8 * lap_w else 'is not'} exceeded)")
    return worst


def corruptions(worst):
    """Section 2: three randn Grams per order, one entry of d, e, tau or vh of matrix 1 moved; default thresholds."""
    from basd_amd import ops
    for n in (45, 448):
        thr = T.default_thresholds(n)
        G = torch.from_numpy(np.stack([T.matrix("randn", n + k)[:n, :n] for k in range(3)])).cuda()
        probe = ops.tridiag_probe(G)
        ts = ops.tridiagonalise(G.clone())
        torch.cuda.synchronize()
        j, i = n // 3, n // 2
        delta = 1e-3 * float(ts.d[1].abs().max())
        print(f"n={n}: default thresholds {thr[0]:.1f} {thr[1]:.1f} {thr[2]:.1f}")
        for field in ("none", "d", "e", "tau", "vh"):
            parts = {k: getattr(ts, k).clone() for k in ("d", "e", "tau", "vh")}
            if field in ("d", "e"):
                parts[field][1, i] += delta
            elif field == "tau":
                parts["tau"][1, j] += 1e-2
            elif field == "vh":
                parts["vh"][1, j, j + 3] += 1e-2
            v = ops.tridiag_check(ops.TridiagState(parts["d"], parts["e"], parts["tau"], parts["vh"], ts.vals), probe)
            torch.cuda.synchronize()
            got = v.read()
            r = got["ratios"].tolist()
            print(f"   {field:4s} verdict [failed {got['failed']}, first {got['first']}, bits {got['bits']}, checked "
                  f"{got['checked']}]  matrix 1: " + " ".join(f"{x:9.2f}" for x in r[1]))
            if field == "none":
                for m in range(3):
                    for k in range(3):
                        worst[("library", k)] = max(worst[("library", k)], (r[m][k] / math.sqrt(n), r[m][k],
                                                                            f"leading block of randn {n + m}, order {n}"))
    for k in range(3):
        per, val, where = worst[("library", k)]
        print(f"worst library incl. these matrices {NAMES[k]:10s} {val:8.3f} = {per:.4f} sqrt(n) at {where}")


def launch_times(reps=30):
    from basd_amd import ops
    for n, batch in ((384, 3), (768, 28), (1024, 8)):
        g = torch.Generator().manual_seed(n)
        x = torch.randn(batch, n + 8, n, generator=g).cuda()
        G = x.transpose(1, 2) @ x
        ts = ops.tridiagonalise(G.clone())
        probe = ops.tridiag_probe(G)
        ops.tridiag_check(ts, probe)
        torch.cuda.synchronize()
        t_probe, t_check = [], []
        for _ in range(reps):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            e[0].record()
            probe = ops.tridiag_probe(G)
            e[1].record()
            e[2].record()
            ops.tridiag_check(ts, probe)
            e[3].record()
            torch.cuda.synchronize()
            t_probe.append(e[0].elapsed_time(e[1]) * 1e3)
            t_check.append(e[2].elapsed_time(e[3]) * 1e3)
        nbytes = batch * n * n * 4
        tp, tc = statistics.median(t_probe), statistics.median(t_check)
        print(f"(n, batch) = ({n}, {batch}): probe {tp:7.1f} us (min {min(t_probe):.1f}; {nbytes / 1e6:.1f} MB read, "
              f"{nbytes / tp / 1e3:.0f} GB/s), apply_q + check {tc:7.1f} us (min {min(t_check):.1f}); events around "
              f"the calls, caches warm (the same matrices every repetition), median of {reps}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu-only", action="store_true")
    ap.add_argument("--orders", default="45,200,320,384,448,768,1024")
    args = ap.parse_args()
    gpu = not args.cpu_only
    print("== 1. ratios: lapack | library, columns rho_trace rho_fro rho_res")
    worst = ratios_table([int(n) for n in args.orders.split(",")], gpu)
    if gpu:
        print("== 2. corruptions")
        corruptions(worst)
        print("== 3. launches")
        launch_times()
