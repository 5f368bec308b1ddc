"""tridiag_packed_kernel (orders 257..384, the whole factorisation in one CU's registers) after its step loop lost its
scratch accesses, the leading-k Sturm bisection of the selector's tail, and the grid-stride ``scale_unless_one``.

Bounds are those of tests/test_hard_spectra.py for the same quantities on the same route (FACTOR_BOUND for Q Q^T - I and
Q T Q^T - G, TRIDIAG_BOUNDS["val"] for eigenvalues against fp64 LAPACK); the chain's tolerance is the one of
test_principal_angle_distance_single_teacher."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from basd_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR_BOUND = 2e-5          # tests/test_hard_spectra.py: |Q Q^T - I| and |Q T Q^T - G| / |G|_max
VAL_BOUND = 3e-6             # tests/test_hard_spectra.py TRIDIAG_BOUNDS["val"]: |lambda - lambda_fp64| / lambda_max
D_GRASS_RTOL = 2e-4          # tests/test_gpu_parity.py::test_principal_angle_distance_single_teacher
ORDERS = (257, 320, 383, 384)


@functools.lru_cache(maxsize=None)
def grams(n, count, seed=0):
    """``count`` Grams of seeded randn data (4 n x n each), fp32 on the host.  Computed once; never modified."""
    g = torch.Generator().manual_seed(1000 * seed + n)
    x = torch.randn(count, 4 * n, n, generator=g)
    return (x.transpose(1, 2) @ x).contiguous()


@functools.lru_cache(maxsize=None)
def reducible(n):
    """Block diagonal (n // 4, n // 2, the rest): the reflectors across the two block boundaries have xn2 == 0."""
    sizes = [n // 4, n // 2, n - n // 4 - n // 2]
    g = torch.Generator().manual_seed(7 * n)
    blocks = []
    for s in sizes:
        x = torch.randn(4 * s, s, generator=g)
        blocks.append(x.T @ x)
    return torch.block_diag(*blocks).unsqueeze(0).contiguous()


def factor_metrics(G, ts):
    """Worst |Q Q^T - I|, |Q T Q^T - G| / |G|_max and |lambda - lambda_fp64| / lambda_max over a batch."""
    from basd_amd import ops
    batch, n, _ = G.shape
    eye = torch.eye(n, device=DEV).repeat(batch, 1, 1).contiguous()
    Qt = ops.tridiag_apply_q(ts, eye, transpose=False).double()        # row i = Q e_i
    e_off = ts.e[:, :n - 1].double()
    T = torch.diag_embed(ts.d.double()) + torch.diag_embed(e_off, 1) + torch.diag_embed(e_off, -1)
    rec = (Qt.transpose(1, 2) @ T @ Qt).cpu()
    qq = (Qt @ Qt.transpose(1, 2)).cpu()
    ev = torch.linalg.eigvalsh(G.double()).flip(1)
    vals = ts.vals.cpu().double()
    out = dict(qq=0.0, qtq=0.0, val=0.0)
    for i in range(batch):
        out["qq"] = max(out["qq"], float((qq[i] - torch.eye(n, dtype=torch.float64)).abs().max()))
        out["qtq"] = max(out["qtq"], float((rec[i] - G[i].double()).abs().max()) / float(G[i].abs().max()))
        out["val"] = max(out["val"], float((vals[i] - ev[i]).abs().max()) / float(ev[i, 0]))
    return out


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("n", ORDERS)
def test_packed_factorisation_against_fp64(n, batch):
    """Q T Q^T against the matrix, Q Q^T against I and the spectrum against fp64 LAPACK: Grams of random data in a
    launch of ``batch`` matrices, and an exactly reducible matrix (steps with xn2 == 0)."""
    from basd_amd import ops
    for name, G in (("grams", grams(n, batch)), ("reducible", reducible(n))):
        ts = ops.tridiag_eigenvalues(G.to(DEV).clone())
        torch.cuda.synchronize()
        assert int(ts.err[0].item()) == 0
        for t in (ts.d, ts.e, ts.tau, ts.vh, ts.vals):
            assert bool(torch.isfinite(t).all()), (name, n)
        m = factor_metrics(G, ts)
        print(f"packed {name} n={n} batch={G.shape[0]}: " + " ".join(f"{k}={v:.2e}" for k, v in m.items()))
        assert m["qq"] < FACTOR_BOUND and m["qtq"] < FACTOR_BOUND and m["val"] < VAL_BOUND, (name, n, m)
        if name == "reducible":     # the reflector across a block boundary is skipped: e is the exact zero found there
            e = ts.e.cpu()
            assert float(e[0, n // 4 - 1]) == 0.0 and float(e[0, n // 4 + n // 2 - 1]) == 0.0


@pytest.mark.parametrize("n", ORDERS)
def test_packed_mp_rank_on_a_planted_gap(n):
    """The rank from the factorisation launch's own Sturm counts against the fp64 spectrum of the same fp32 matrix, with
    an eigenvalue planted 2e-3 (relative) above / below the threshold (test_mp_rank_dense_with_a_planted_gap's matrix)."""
    from basd_amd import ops
    M = 12544
    g = torch.Generator().manual_seed(5)
    q, _ = torch.linalg.qr(torch.randn(n, n, generator=g, dtype=torch.float64))
    factor = (1 + (n / M) ** 0.5) ** 2
    rng = np.random.default_rng(5)
    for rel in (2e-3, -2e-3):
        lam = np.concatenate([rng.uniform(0.6, 1.0, n - 9), rng.uniform(8.0, 14.0, 8)])
        med = np.sort(np.concatenate([lam, [10.0]]))[(n - 1) // 2]
        lam = np.concatenate([lam, [med * factor * (1 + rel)]])
        G = (q @ torch.diag(torch.from_numpy(lam)) @ q.T)
        G = ((G + G.T) / 2).float()
        ev = torch.linalg.eigvalsh(G.double())
        thr = float(np.float32(float(ev[(n - 1) // 2]) * factor))
        ref = int((ev > thr).sum())
        assert ref == (9 if rel > 0 else 8)
        pin = torch.empty((1 + 8,), dtype=torch.int32, pin_memory=True)
        ts = ops.tridiagonalise(G.to(DEV).unsqueeze(0).contiguous(), mp_rank=(M, n, n - 1, 1, pin))
        torch.cuda.synchronize()
        assert int(ts.ranks[0]) == ref and int(pin[0]) == ref, (n, rel, int(ts.ranks[0]), ref)


@pytest.mark.parametrize("n", [257, 384])
def test_packed_bits_do_not_depend_on_placement_or_cu_history(n):
    """One matrix alone, as member 0, 2 and 5 of a batch of six, and behind an LDS full of NaNs: the same d, e, tau and
    reflectors, bit for bit."""
    from basd_amd import ops, _lib
    one = grams(n, 1)
    others = grams(n, 6, seed=1)

    def run(G):
        ts = ops.tridiagonalise(G.to(DEV).clone())
        torch.cuda.synchronize()
        assert int(ts.err[0].item()) == 0
        return ts

    alone = run(one)
    for member in (0, 2, 5):
        G = others.clone()
        G[member] = one[0]
        got = run(G)
        for name in ("d", "e", "tau", "vh"):
            assert torch.equal(getattr(got, name)[member], getattr(alone, name)[0]), (n, member, name)
    _lib.call("basd_debug_fill_lds", 0x7FC00000, torch.cuda.current_stream().cuda_stream)
    again = run(one)
    for name in ("d", "e", "tau", "vh"):
        assert torch.equal(getattr(again, name), getattr(alone, name)), (n, "stale LDS", name)


def _leading(ts, k, out):
    from basd_amd import _lib
    batch, n = ts.d.shape
    _lib.call("basd_tridiag_eigenvalues_leading", ts.d.data_ptr(), ts.e.data_ptr(), n, k, batch, out.data_ptr(),
              torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("n", [45, 384])
def test_leading_bisection_writes_the_prefix_of_the_full_call(n):
    """k in {1, 63, 64, 65, n} (a k past n is taken as n): elements [0, min(n, 64 ceil(k / 64))) carry the bits of basd_tridiag_eigenvalues, the
    rest of every row of a pre-filled output is untouched."""
    from basd_amd import ops
    ts = ops.tridiag_eigenvalues(grams(n, 3).to(DEV).clone())
    full = ts.vals.clone()
    for k in (1, 63, 64, 65, n):
        out = torch.full((3, n), -777.0, device=DEV)
        _leading(ts, k, out)
        torch.cuda.synchronize()
        written = min(n, 64 * ((k + 63) // 64))
        assert torch.equal(out[:, :written], full[:, :written]), (n, k)
        assert bool((out[:, written:] == -777.0).all()), (n, k)


def test_leading_bisection_on_the_toeplitz_tridiagonal():
    """(2, -1) of order 384: eigenvalues 2 - 2 cos(j pi / (n + 1)), analytic."""
    from basd_amd import ops
    n = 384
    f32 = dict(device=DEV, dtype=torch.float32)
    e = torch.zeros(1, n, **f32)
    e[0, :n - 1] = -1.0
    ts = ops.TridiagState(torch.full((1, n), 2.0, **f32), e, torch.zeros(1, n, **f32), torch.zeros(1, n, n, **f32),
                          torch.empty(1, n, **f32))
    j = torch.arange(n, 0, -1, dtype=torch.float64)
    analytic = 2 - 2 * torch.cos(j * math.pi / (n + 1))
    for k in (65, n):
        out = torch.full((1, n), -777.0, **f32)
        _leading(ts, k, out)
        written = min(n, 64 * ((k + 63) // 64))
        got = out[0, :written].cpu().double()
        err = float((got - analytic[:written]).abs().max()) / float(analytic[0])
        print(f"toeplitz leading k={k}: val={err:.2e}")
        assert err < VAL_BOUND, (k, err)


def test_chain_at_a_packed_order_agrees_with_the_kernel_by_kernel_route():
    """Two consecutive basd_selector_chain steps at the smallest shape it accepts with a packed order (d_s = 264,
    B n_t = 288, E = 2, L = 1) against the kernel-by-kernel layout: ranks equal, d_grass_sq to 2e-4."""
    from basd_amd.losses import BASDLoss
    # the teacher is wider than d_s: a narrower one leaves the projected Gram rank-deficient, its median eigenvalue at
    # round-off and the Marchenko-Pastur rank undecidable (two correct routes then differ by one)
    shape = synth.LossShape("packed chain", 8, 36, 264, 12, 36, 320, 1, 1, False, 10, points=2, r_s=6, r_t=5)
    results = {}
    for use_chain in (True, False):
        torch.manual_seed(42)
        crit = torch.nn.CrossEntropyLoss(label_smoothing=0.01)
        mod = BASDLoss(crit, shape.d_s, shape.d_t, shape.depth, shape.n_s,
                       config=SimpleNamespace(num_extraction_points=shape.points),
                       teacher_has_cls_token=shape.has_cls).to(DEV)
        mod.use_chain = use_chain
        steps = []
        for seed in (11, 12):
            inp = synth.make_inputs(shape, seed, device=DEV, strided=True)
            mod(inp.logits, inp.targets, inp.student, inp.teacher, inp.attn)
            mod.layer_selector.finish_pending()
            torch.cuda.synchronize()
            steps.append((dict(mod.layer_selector.subspace_ranks), mod.last_components["d_grass_sq"].cpu().numpy().copy()))
        if use_chain:
            assert len(mod._chain_plans) == 1, "the chain did not take this shape"
        results[use_chain] = steps
    for step, ((r_c, d_c), (r_k, d_k)) in enumerate(zip(results[True], results[False])):
        print(f"chain step {step}: ranks {r_c} d_grass_sq {d_c.ravel()} vs {d_k.ravel()}")
        assert r_c == r_k, (step, r_c, r_k)
        np.testing.assert_allclose(d_c, d_k, rtol=D_GRASS_RTOL, err_msg=f"step {step}")


def test_scale_unless_one():
    """3 x 1000 + 7 elements (a vector part and a remainder): untouched by an upstream gradient of 1, x * 0.5f by 0.5."""
    from basd_amd import ops
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn(3 * 1000 + 7, generator=g)
    x = x0.to(DEV)
    ops.scale_unless_one(x, torch.ones(1, device=DEV))
    torch.cuda.synchronize()
    assert torch.equal(x.cpu().view(torch.int32), x0.view(torch.int32))
    ops.scale_unless_one(x, torch.full((1,), 0.5, device=DEV))
    torch.cuda.synchronize()
    assert torch.equal(x.cpu().view(torch.int32), (x0 * np.float32(0.5)).view(torch.int32))
    # more float4 groups than the grid has threads: the stride loop's second trip, and a remainder
    y0 = torch.randn(4 * (1024 * 256 + 300) + 3, generator=g)
    y = y0.to(DEV)
    ops.scale_unless_one(y, torch.full((1,), 0.5, device=DEV))
    torch.cuda.synchronize()
    assert torch.equal(y.cpu().view(torch.int32), (y0 * np.float32(0.5)).view(torch.int32))
