"""The eigen-solvers and the principal-angle distance on spectra that Grams of ``randn`` data never show: exact
multiplicities, blocks of eigenvalues at round-off, graded spectra, exactly reducible matrices, zero and multiples of
the identity, scales 2^+-24, tridiagonals given directly, singular values that are all equal or exactly zero, and
principal angles at 0 and pi / 2.

Every matrix is built in fp64 from seeded generators, symmetrised and rounded to fp32; the reference is fp64 LAPACK
(``eigh`` / ``svdvals``) of that same fp32 matrix, or the CPU oracle for the selector.  ``test_fixtures_...`` runs without
a GPU: it holds fp32 LAPACK to the same bounds, so a family that no fp32 solver could pass fails there first."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from basd_amd import synth
from oracle import basd_oracle as O

gpu = pytest.mark.gpu
DEV = "cuda:0"

# bounds the suite already applies to these solvers (test_tridiag_eigensolver,
# test_tridiag_tail_stage_reconstructs_the_matrix, test_sym_eig_block_path): eigenvalues and residuals relative to the
# largest eigenvalue, orthonormality and projectors absolute
TRIDIAG_BOUNDS = dict(val=3e-6, orth=1e-4, res=2e-5, proj=1e-4)
SYM_EIG_BOUNDS = dict(val=3e-6, orth=2e-5, res=2e-5, proj=1e-4)
FACTOR_BOUND = 2e-5          # |Q Q^T - I| and |Q T Q^T - G| / |G|_max
GAP = 0.1                    # a leading subspace counts as isolated when a gap of 0.1 lambda_max lies below it

# the four families whose Marchenko-Pastur rank is decidable come first: ``tridiagonalise(mp_rank=)`` ranks the leading
# matrices of a batch
RANKED = ("mult", "ones", "blocks", "diag")
FAMILIES = RANKED + ("lowrank", "graded", "mult_up", "mult_down", "identity", "zero")
NO_SPIN = ("identity", "zero")          # run only where no workgroup waits for another one (orders <= 384)


# --------------------------------------------------------------------------- #
# 1. the matrix families (CPU)
# --------------------------------------------------------------------------- #
def from_spectrum(lam, seed):
    """Q diag(lam) Q^T in fp64, Q from the QR of a seeded fp64 randn."""
    lam = torch.as_tensor(lam, dtype=torch.float64)
    g = torch.Generator().manual_seed(seed)
    q, _ = torch.linalg.qr(torch.randn(lam.numel(), lam.numel(), generator=g, dtype=torch.float64))
    return (q * lam) @ q.T


def _round(G):
    return ((G + G.T) / 2).float()


def _mult_spectrum(n):
    m = min(20, n // 3)
    return [16.0] + [8.0] * 3 + [4.0] * m + [1.0] * (n - 4 - m), m


@functools.lru_cache(maxsize=None)
def family(name, n):
    """(G fp32 (n, n), k eigenvectors to request, k_iso | None: the leading k_iso eigenvalues are isolated)."""
    seed = 7919 * (FAMILIES.index(name) + 1) + n
    if name in ("mult", "mult_up", "mult_down"):
        lam, m = _mult_spectrum(n)
        G = _round(from_spectrum(lam, 7919 + n))
        if name != "mult":          # an exact power of two: the fp32 matrix is the same mantissas at another exponent
            G = G * (2.0 ** 24 if name == "mult_up" else 2.0 ** -24)
        return G, 4 + m, 4 + m
    if name == "lowrank":           # n - 12 eigenvalues at round-off
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(12, n, generator=g, dtype=torch.float64)
        return _round(x.T @ x), 12, 12
    if name == "graded":
        lam = [max(2.0 ** (-i / 4), 2.0 ** -30) for i in range(n)]
        return _round(from_spectrum(lam, seed)), 8, None
    if name == "ones":              # exact in fp32: n + 2 once, 2 with multiplicity n - 1
        return _round(torch.ones(n, n, dtype=torch.float64) + 2 * torch.eye(n, dtype=torch.float64)), min(40, n - 1), 1
    if name == "blocks":            # exactly reducible: the off-block entries are exact zeros
        sizes = [n // 4, n // 2, n - n // 4 - n // 2]
        G = torch.zeros(n, n, dtype=torch.float64)
        at = 0
        for i, (b, lead) in enumerate(zip(sizes, ((9.0, 7.0), (5.0, 3.0), (11.0, 6.0)))):
            lam = list(lead) + torch.linspace(1.5, 1.0, b - 2, dtype=torch.float64).tolist()
            G[at:at + b, at:at + b] = from_spectrum(lam, seed + 17 * i)
            at += b
        return _round(G), 6, 6
    if name == "diag":
        g = torch.Generator().manual_seed(seed)
        lam = torch.tensor([5.0] * 3 + [2.0] * 7 + [1.0] * (n - 10), dtype=torch.float64)
        return _round(torch.diag(lam[torch.randperm(n, generator=g)])), 10, 10
    if name == "identity":
        return 3 * torch.eye(n), 5, None
    if name == "zero":
        return torch.zeros(n, n), 5, None
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name, n):
    """fp64 eigenvalues (descending) and eigenvectors (columns) of the fp32 matrix.  Computed once; never modified."""
    ev, evec = torch.linalg.eigh(family(name, n)[0].double())
    return ev.flip(0), evec.flip(1)


def eig_metrics(G, ref, vals, vecs, k_iso):
    """Worst errors of eigenvalues ``vals`` (n, descending) and eigenvector rows ``vecs`` (k, n) of the fp32 matrix G
    against its fp64 decomposition ``ref``.  Individual vectors inside a multiplicity are not compared, nor projectors
    onto part of a cluster: neither is defined."""
    ev, evec = ref
    lmax = float(ev[0].abs())
    vals, v = vals.double(), vecs.double()
    k = v.shape[0]
    out = dict(orth=float((v @ v.T - torch.eye(k, dtype=torch.float64)).abs().max()))
    if lmax == 0.0:                                     # the zero matrix: absolute, and every vector is an eigenvector
        out["val_abs"] = float(vals.abs().max())
        return out
    out["val"] = float((vals - ev).abs().max()) / lmax
    out["res"] = float((G.double() @ v.T - v.T * vals[:k]).norm(dim=0).max()) / lmax
    if k_iso is not None and k_iso <= k:
        p = v[:k_iso].T @ v[:k_iso]
        pr = evec[:, :k_iso] @ evec[:, :k_iso].T
        out["proj"] = float((p - pr).abs().max())
    return out


def check_metrics(m, bounds, what):
    for key, got in m.items():
        bound = 1e-30 if key == "val_abs" else bounds[key]
        assert got < bound, (what, key, got, bound)


def fmt(m):
    return " ".join(f"{k}={v:.2e}" for k, v in m.items())


def dense_tridiagonal(d, e):
    d, e = d.double(), e.double()
    return torch.diag(d) + torch.diag(e, 1) + torch.diag(e, -1)


def wilkinson(glued):
    """W21+ (d = |i - 10|, e = 1): its top eigenvalues pair up 7e-14 apart, so in fp32 the two top shifts coincide.
    ``glued``: two copies joined by e = 2^-20 -- the top four eigenvalues then lie within 1e-6 of each other.
    Returns (d, e, k, order of the top cluster)."""
    d = (torch.arange(21) - 10).abs().float()
    e = torch.ones(20)
    if not glued:
        return d, e, 6, 2
    return torch.cat([d, d]), torch.cat([e, torch.tensor([2.0 ** -20]), e]), 8, 4


def test_fixtures_are_well_posed_for_an_fp32_solver():
    """Guards the fixtures and the bounds, not the kernels: fp32 LAPACK meets every bound of the GPU tests below (the
    tighter of the two sets) on every family at n = 45, 200, 384, and the gaps the projector comparisons rely on are
    there in the fp64 spectrum.  A family that is ill-posed for any fp32 solver fails here too: change the family then,
    not the bound."""
    bounds = {k: min(TRIDIAG_BOUNDS[k], SYM_EIG_BOUNDS[k]) for k in TRIDIAG_BOUNDS}
    worst, min_gap = {}, math.inf
    for n in (45, 200, 384):
        for name in FAMILIES:
            G, k, k_iso = family(name, n)
            assert torch.equal(G, G.T) and G.dtype == torch.float32
            ev, _ = reference(name, n)
            if k_iso is not None:
                gap = float(ev[k_iso - 1] - ev[k_iso]) / float(ev[0])
                min_gap = min(min_gap, gap)
                assert gap >= GAP, (name, n, gap)
            vals, vecs = torch.linalg.eigh(G)
            m = eig_metrics(G, reference(name, n), vals.flip(0), vecs.flip(1)[:, :k].T, k_iso)
            print(f"lapack fp32 {name} n={n}: {fmt(m)}")
            check_metrics(m, bounds, (name, n))
            for key, got in m.items():
                worst[key] = max(worst.get(key, 0.0), got)
    for glued in (False, True):
        d, e, k, top = wilkinson(glued)
        T = dense_tridiagonal(d, e)
        ev, evec = torch.linalg.eigh(T)
        ev, evec = ev.flip(0), evec.flip(1)
        gap = float(ev[top - 1] - ev[top]) / float(ev[0])
        min_gap = min(min_gap, gap)
        assert gap >= GAP and float(ev[0] - ev[top - 1]) < 1e-5 * float(ev[0])
        vals, vecs = torch.linalg.eigh(T.float())
        m = eig_metrics(T.float(), (ev, evec), vals.flip(0), vecs.flip(1)[:, :k].T, top)
        print(f"lapack fp32 wilkinson glued={glued}: {fmt(m)}")
        check_metrics(m, bounds, ("wilkinson", glued))
    print("worst over the families:", fmt(worst), f"smallest gap {min_gap:.3f}")


# --------------------------------------------------------------------------- #
# 2. tridiagonal route: values, vectors, factorisation, ranks
# --------------------------------------------------------------------------- #
@pytest.fixture
def tuning():
    """basd_tridiag_tuning(members, pad, lag, threads, tail): test hook of the library; restored afterwards."""
    from basd_amd import _lib

    def set_(members=-1, pad=-1, lag=-1, threads=-1, tail=-1, reset=0):
        _lib.call("basd_tridiag_tuning", members, pad, lag, threads, tail, reset)
    yield set_
    _lib.call("basd_tridiag_tuning", -1, -1, -1, -1, -1, 1)


def oracle_rank(ev, M, n, cap):
    """The oracle's rule (lower median, fp64 factor, threshold rounded to fp32, strict >) on an fp64 spectrum, and the
    relative distance of the nearest eigenvalue from the threshold."""
    asc = ev.sort().values
    thr = float(np.float32(float(asc[(n - 1) // 2]) * O.mp_threshold_factor(M, n)))
    return min(int((asc > thr).sum()), cap), float(((asc - thr).abs() / thr).min())


# 45, 200: tridiag_tail2_kernel runs the whole factorisation; 320, 384: tridiag_packed_kernel; 448: the shared stage
# (whose polling and lock-step depend on step, member and tag only, never on the matrix values) followed by tail2.
# `blocks` and `diag` give each copy of the reflector code steps with xn2 == 0.
@gpu
@pytest.mark.parametrize("n,tail", [(45, None), (200, None), (320, None), (384, None), (448, None)])
def test_tridiag_route_on_hard_spectra(n, tail, tuning):
    """One batch per order: eigenvalues, leading eigenvectors (requested per family), the factorisation itself and the
    Marchenko-Pastur ranks.  Before the pivot rule of tridiag_invit_kernel followed slagts this failed on `zero` at every
    order (all vectors zero) and on `ones` at order 45 (residual 2.9e-5, 3e-5 of the top eigenvector in the cluster)."""
    from basd_amd import ops
    names = [f for f in FAMILIES if n <= 384 or f not in NO_SPIN]
    if tail is not None:
        tuning(tail=tail)
    G0 = torch.stack([family(f, n)[0] for f in names]).to(DEV)
    ts = ops.tridiag_eigenvalues(G0.clone())
    vecs = {f: ops.tridiag_eigenvectors(ts, family(f, n)[1], first=i, count=1)[0].cpu() for i, f in enumerate(names)}
    eye = torch.eye(n, device=DEV).repeat(len(names), 1, 1).contiguous()
    Qt = ops.tridiag_apply_q(ts, eye, transpose=False).double()        # row i = Q e_i
    e_off = ts.e[:, :n - 1].double()
    T = torch.diag_embed(ts.d.double()) + torch.diag_embed(e_off, 1) + torch.diag_embed(e_off, -1)
    rec = (Qt.transpose(1, 2) @ T @ Qt).cpu()
    qq = (Qt @ Qt.transpose(1, 2)).cpu()
    assert int(ts.err[0].item()) == 0
    d, e, vals = ts.d.cpu(), ts.e.cpu(), ts.vals.cpu()
    failures = []
    for i, f in enumerate(names):
        G, k, k_iso = family(f, n)
        assert all(bool(torch.isfinite(t).all()) for t in (d[i], e[i], vals[i], vecs[f])), (f, n)
        m = eig_metrics(G, reference(f, n), vals[i], vecs[f], k_iso)
        m["qq"] = float((qq[i] - torch.eye(n, dtype=torch.float64)).abs().max())
        m["qtq"] = float((rec[i] - G.double()).abs().max()) / max(float(G.abs().max()), 1e-300)
        print(f"tridiag {f} n={n} tail={tail}: {fmt(m)}")
        try:
            check_metrics(m, dict(TRIDIAG_BOUNDS, qq=FACTOR_BOUND, qtq=FACTOR_BOUND), (f, n, tail))
            if f == "blocks":           # the reflector across a block boundary is skipped: e is the exact zero found there
                assert float(e[i, n // 4 - 1]) == 0.0 and float(e[i, n // 4 + n // 2 - 1]) == 0.0
            if f == "diag":             # every reflector is skipped: T is the matrix itself, bit for bit
                assert not e[i, :n - 1].any() and torch.equal(d[i], torch.diagonal(G))
        except AssertionError as err:   # report every family of the order, not only the first one that fails
            failures.append(str(err))
    assert not failures, failures

    # Marchenko-Pastur ranks on the same factorisations, three ways, against the oracle's rule on the fp64 spectrum.
    # Only where the rule is decidable: `lowrank` and `graded` have a median at round-off, `identity` and `zero` tie with
    # everything (and the scaled copies of `mult` repeat it), so they are left out.
    M = 32 * n
    want = []
    for f in RANKED:
        rank, margin = oracle_rank(reference(f, n)[0], M, n, n - 1)
        assert margin > 1e-3, (f, n, margin)            # no eigenvalue within 1e-3 of the threshold
        want.append(rank)
    assert want[1] == 1                                 # `ones`: the median sits inside the (n - 1)-fold eigenvalue
    fast = ops.tridiag_mp_rank(ts, M, n, cap=n - 1).cpu().tolist()[:len(RANKED)]
    full = ops.mp_rank_device(ts.vals, M, n, cap=n - 1).cpu().tolist()[:len(RANKED)]
    pin = torch.empty((len(RANKED) + 8,), dtype=torch.int32, pin_memory=True)
    ts2 = ops.tridiagonalise(G0.clone(), mp_rank=(M, n, n - 1, len(RANKED), pin))
    torch.cuda.synchronize()
    print(f"mp ranks n={n} tail={tail}: oracle {want} tridiag {fast} spectrum {full} fused {ts2.ranks.cpu().tolist()}")
    assert fast == want and full == want and ts2.ranks.cpu().tolist() == want
    assert pin.tolist() == want + [0] * 8


# --------------------------------------------------------------------------- #
# 3. tridiagonals given directly
# --------------------------------------------------------------------------- #
def _solve_tridiagonal(d, e, k):
    """Eigenvalues and leading k eigenvectors of the tridiagonal (d, e) itself: a state with tau = 0 everywhere, so the
    back-transformation applies no reflector."""
    from basd_amd import ops
    n = d.numel()
    f32 = dict(device=DEV, dtype=torch.float32)
    e_pad = torch.zeros(1, n, **f32)
    e_pad[0, :n - 1] = e.to(DEV)
    ts = ops.TridiagState(d.to(DEV).view(1, n).contiguous(), e_pad, torch.zeros(1, n, **f32),
                          torch.zeros(1, n, n, **f32), torch.empty(1, n, **f32))
    ops.tridiag_spectrum(ts)
    vecs = ops.tridiag_eigenvectors(ts, k)
    return ts.vals[0].cpu(), vecs[0].cpu()


@gpu
@pytest.mark.parametrize("n", [21, 201, 384])
def test_toeplitz_tridiagonal(n):
    """(2, -1): eigenvalues 2 - 2 cos(j pi / (n + 1)), analytic; the top of the spectrum is one long cluster."""
    d, e, k = torch.full((n,), 2.0), torch.full((n - 1,), -1.0), 16
    vals, vecs = _solve_tridiagonal(d, e, k)
    T = dense_tridiagonal(d, e)
    j = torch.arange(n, 0, -1, dtype=torch.float64)
    analytic = 2 - 2 * torch.cos(j * math.pi / (n + 1))
    assert bool(torch.isfinite(vals).all()) and bool(torch.isfinite(vecs).all())
    m = eig_metrics(T.float(), (analytic, None), vals, vecs, None)
    print(f"toeplitz n={n}: {fmt(m)}")
    check_metrics(m, TRIDIAG_BOUNDS, ("toeplitz", n))


@gpu
@pytest.mark.parametrize("glued", [False, True])
def test_wilkinson_tridiagonal(glued):
    """W21+ and two copies glued by 2^-20: the projector is compared on the whole top cluster (2, or 4 when glued: the
    glue splits the two pairs by less than fp32 resolves), which a gap of 1.5 separates from the next pair."""
    d, e, k, top = wilkinson(glued)
    vals, vecs = _solve_tridiagonal(d, e, k)
    T = dense_tridiagonal(d, e)
    ev, evec = torch.linalg.eigh(T)
    assert bool(torch.isfinite(vals).all()) and bool(torch.isfinite(vecs).all())
    m = eig_metrics(T.float(), (ev.flip(0), evec.flip(1)), vals, vecs, top)
    print(f"wilkinson glued={glued}: {fmt(m)}")
    check_metrics(m, TRIDIAG_BOUNDS, ("wilkinson", glued))


# --------------------------------------------------------------------------- #
# 4. one-sided Jacobi on degenerate inputs
# --------------------------------------------------------------------------- #
JACOBI_KINDS = ("orthogonal", "paired", "zero", "diag", "scaled")


@functools.lru_cache(maxsize=None)
def jacobi_inputs(n):
    """(5, n, n) fp32: matrix b has columns w[b, c, :]."""
    g = torch.Generator().manual_seed(100 + n)
    q, _ = torch.linalg.qr(torch.randn(n, n, generator=g, dtype=torch.float64))        # every sigma is 1
    paired = torch.randn(n, n, generator=g, dtype=torch.float64)
    paired[1:2 * (n // 2):2] = paired[0:2 * (n // 2):2]        # columns 2j and 2j + 1 equal: exact zeros and sigma pairs
    ties = torch.tensor(([3.0] * 4 + [2.0] * 5 + [0.5] * n)[:n], dtype=torch.float64)
    diag = torch.diag(ties[torch.randperm(n, generator=g)])[torch.randperm(n, generator=g)]
    scaled = torch.randn(n, n, generator=g, dtype=torch.float64)
    scaled[n // 3] *= 2.0 ** 20
    return torch.stack([q, paired, torch.zeros(n, n, dtype=torch.float64), diag, scaled]).float()


def jacobi_metrics(w0, w, sigma, k=None):
    """One matrix: columns w0[c, :k] before, w[c, :k] after (c < k), sigma (k,) the returned column norms."""
    k = w0.shape[0] if k is None else k
    x0, x = w0[:k, :k].double(), w[:k, :k].double()
    sv = torch.linalg.svdvals(x0)
    assert bool(torch.isfinite(sigma[:k]).all())
    got = sigma[:k].double().sort(descending=True).values
    if float(sv[0]) == 0.0:
        assert not got.any(), "the zero matrix must keep sigma == 0 exactly"
        return dict(sig=0.0, cos=0.0, gram=float((x.T @ x).abs().max()))
    gram = x @ x.T
    nrm = torch.diagonal(gram).sqrt()
    live = (nrm > 1e-6 * nrm.max()).double()               # the suite's definition: the rest is round-off
    cos = (gram - torch.diag(nrm ** 2)).abs() / (nrm[:, None] * nrm[None, :]).clamp_min(1e-30) * live[:, None] * live[None, :]
    g0 = x0.T @ x0
    return dict(sig=float((got - sv).abs().max() / sv[0]), cos=float(cos.max()),
                gram=float((x.T @ x - g0).norm() / g0.norm()))


JACOBI_BOUNDS = dict(sig=3e-6, cos=5e-6, gram=1e-5)

# 49: the LDS-resident solver; 96: the order from which small batches of plain matrices take the register-resident
# odd-even solver; 200: the block path.  lanes=4 forces the plain batched route of the transposed Procrustes cores,
# with both of its orderings (0: round-robin through LDS, also at order 96; the 16-lane LDS solver sees order 96 in the
# per-matrix-order test below).
@gpu
@pytest.mark.parametrize("n,lanes,ordering", [(49, 0, 1), (96, 0, 1), (200, 0, 1), (49, 4, 1), (49, 4, 0), (96, 4, 1),
                                              (96, 4, 0)])
def test_jacobi_on_degenerate_inputs(n, lanes, ordering):
    from basd_amd import ops, _lib
    w0 = jacobi_inputs(n)
    _lib.call("basd_jacobi_ordering", ordering)
    _lib.call("basd_jacobi_tuning", lanes)
    try:
        W = w0.clone().to(DEV)
        sigma, sweeps = ops.jacobi_onesided(W, n, want_sweeps=True)
        W, sigma, sweeps = W.cpu(), sigma.cpu(), sweeps.cpu()
    finally:
        _lib.call("basd_jacobi_ordering", 1)
        _lib.call("basd_jacobi_tuning", 0)
    for b, kind in enumerate(JACOBI_KINDS):
        assert int(sweeps[b]) < ops.MAX_SWEEPS, (kind, n, "did not converge")
        m = jacobi_metrics(w0[b], W[b], sigma[b])
        print(f"jacobi {kind} n={n} lanes={lanes} ordering={ordering}: {fmt(m)} sweeps={int(sweeps[b])}")
        check_metrics(m, JACOBI_BOUNDS, (kind, n, lanes, ordering))


@gpu
@pytest.mark.parametrize("n", [49, 96, 200])
def test_jacobi_degenerate_inputs_with_per_matrix_orders(n):
    """The same inputs in one batch with orders (n, n - 1, 1, 0) of their leading blocks (``n_arr``: the LDS-resident
    solver up to order 192, the block path beyond); storage outside a matrix's leading block stays as it was."""
    from basd_amd import ops
    w0 = jacobi_inputs(n)[[0, 1, 4, 3]].contiguous()        # orthogonal, paired, scaled, diag
    orders = [n, n - 1, 1, 0]
    W = w0.clone().to(DEV)
    sigma, sweeps = ops.jacobi_onesided(W, n, n_arr=torch.tensor(orders, dtype=torch.int32, device=DEV),
                                        want_sweeps=True)
    W, sigma, sweeps = W.cpu(), sigma.cpu(), sweeps.cpu()
    for b, k in enumerate(orders):
        assert int(sweeps[b]) < ops.MAX_SWEEPS, (b, k)
        outside = torch.ones(n, n, dtype=torch.bool)
        outside[:k, :k] = False
        assert torch.equal(W[b][outside], w0[b][outside]), (b, k, "storage past the order changed")
        if k == 0:
            continue
        m = jacobi_metrics(w0[b], W[b], sigma[b], k)
        print(f"jacobi n_arr storage {n} order {k}: {fmt(m)} sweeps={int(sweeps[b])}")
        check_metrics(m, JACOBI_BOUNDS, (n, k))


@gpu
def test_sym_eig_on_hard_spectra():
    """The block-Jacobi eigen route at order 200.  One ``kmax`` serves the batch: of each family the leading
    min(k, 24) vectors are checked (past its 12 non-zero eigenvalues `lowrank` has no vectors to ask for)."""
    from basd_amd import ops
    n, kmax = 200, 24
    names = ("mult", "lowrank", "ones", "blocks")
    G0 = torch.stack([family(f, n)[0] for f in names]).to(DEV)
    vals, vecs, _, _ = ops.sym_eig(G0.clone(), kmax=kmax)
    vals, vecs = vals.cpu(), vecs.cpu()
    for i, f in enumerate(names):
        G, k, k_iso = family(f, n)
        assert bool(torch.isfinite(vals[i]).all()) and bool(torch.isfinite(vecs[i]).all())
        m = eig_metrics(G, reference(f, n), vals[i], vecs[i, :min(k, kmax)], k_iso)
        print(f"sym_eig {f} n={n}: {fmt(m)}")
        check_metrics(m, SYM_EIG_BOUNDS, (f, n))
        if k_iso is not None:
            assert "proj" in m


# --------------------------------------------------------------------------- #
# 5. the selector at angles 0 and pi / 2
# --------------------------------------------------------------------------- #
SHAPE = synth.LossShape("hard angles", 8, 32, 64, 12, 32, 96, 1, 1, False, 10, points=2)
ACOS_AT_THE_CLAMP_SQ = math.acos(1.0 - O.F32_EPS) ** 2          # 2.384e-7: the distance when every cosine is 1


class _AngleCase:
    """Features made in the projected coordinates: z = randn(M, d_s) + 10 randn on chosen columns; the teacher tokens
    are z_t proj_t and the student's z_s proj_s, so (orthonormal rows / orthogonal) projecting them gives z back."""

    def __init__(self, kind):
        torch.manual_seed(42)
        self.state = O.SelectorState.create(SHAPE.points, SHAPE.d_s, SHAPE.d_t)
        self.layers = synth.extraction_layers(SHAPE.depth, SHAPE.points)
        g = torch.Generator().manual_seed(2024)
        M, B = SHAPE.batch * SHAPE.n_s, SHAPE.batch
        z_t = torch.randn(M, SHAPE.d_s, generator=g)
        z_t[:, :8] += 10 * torch.randn(M, 8, generator=g)
        self.teacher = {0: (z_t @ self.state.proj_t).view(B, SHAPE.n_t, SHAPE.d_t)}
        self.student = {}
        for l in self.layers:
            z_s = torch.randn(M, SHAPE.d_s, generator=g)
            if kind == "aligned":
                z_s = z_t.clone()
            elif kind == "orthogonal":
                z_s[:, 8:16] += 10 * torch.randn(M, 8, generator=g)
            else:
                z_s[:, 8:12] += 10 * torch.randn(M, 4, generator=g)
                z_s[:, 0:4] = z_t[:, 0:4]
            self.student[l] = (z_s @ self.state.proj_s).view(B, SHAPE.n_s, SHAPE.d_s)
        self.attn = {0: torch.ones(B, 1, SHAPE.n_t, SHAPE.n_t) / SHAPE.n_t}
        self.logits = torch.randn(B, SHAPE.num_classes, generator=g)
        self.targets = torch.randint(0, SHAPE.num_classes, (B,), generator=g)
        self.crit = torch.nn.CrossEntropyLoss(label_smoothing=0.01)
        self.ref_leaves = {l: v.clone().requires_grad_(True) for l, v in self.student.items()}
        self.ref, trace = O.basd_forward(self.state, self.crit, self.layers, SHAPE.n_s, SHAPE.has_cls, self.logits,
                                         self.targets, self.ref_leaves, self.teacher, self.attn)
        if kind == "orthogonal":        # the only case with a gradient: acos has no finite derivative at the clamp
            self.ref.backward()
        self.ranks = dict(trace.selector.ranks)
        self.d_grass_sq = np.stack([trace.selector.d_grass_sq[l].numpy() for l in self.layers])

    def module(self):
        from basd_amd.losses import BASDLoss
        torch.manual_seed(42)
        return BASDLoss(self.crit, SHAPE.d_s, SHAPE.d_t, SHAPE.depth, SHAPE.n_s,
                        config=SimpleNamespace(num_extraction_points=SHAPE.points),
                        teacher_has_cls_token=SHAPE.has_cls).to(DEV)

    def on_device(self):
        move = lambda d: {k: v.to(DEV) for k, v in d.items()}
        return SimpleNamespace(logits=self.logits.to(DEV), targets=self.targets.to(DEV), student=move(self.student),
                               teacher=move(self.teacher), attn=move(self.attn))


@functools.lru_cache(maxsize=None)
def angle_case(kind):
    return _AngleCase(kind)


@gpu
@pytest.mark.parametrize("chain", ["1", "0"])
@pytest.mark.parametrize("kind", ["aligned", "orthogonal", "half"])
def test_selector_at_extreme_angles(kind, chain, monkeypatch):
    """d_grass_sq where every cosine is 1 (the clamp), where all are about 0, and where half of them are each, through
    ``basd_selector_chain`` and through the kernel-by-kernel layout."""
    case = angle_case(kind)
    assert case.ranks == {0: 8}, case.ranks                 # on the CPU, before anything of the library runs
    monkeypatch.setenv("BASD_SELECTOR_CHAIN", chain)
    mod = case.module()
    inp = case.on_device()
    loss = mod(inp.logits, inp.targets, inp.student, inp.teacher, inp.attn)
    mod.layer_selector.finish_pending()
    torch.cuda.synchronize()
    d = mod.last_components["d_grass_sq"].cpu().numpy()
    print(f"selector {kind} chain={chain}: d_grass_sq {d.ravel()} oracle {case.d_grass_sq.ravel()} "
          f"loss {loss.item():.6f} oracle {case.ref.item():.6f}")
    assert dict(mod.layer_selector.subspace_ranks) == case.ranks
    assert np.isfinite(d).all() and math.isfinite(loss.item())
    if kind == "aligned":
        # theta^2 ~ 2 (1 - sigma): twice the suite's 3e-6 bound on a singular value, plus the clamp value itself.
        # The fp32 oracle (5e-7) passes; a sigma off by 1e-3 would not.
        assert np.abs(d - ACOS_AT_THE_CLAMP_SQ).max() <= 8e-6
        assert np.abs(case.d_grass_sq - ACOS_AT_THE_CLAMP_SQ).max() <= 8e-6
    else:
        np.testing.assert_allclose(d, case.d_grass_sq, rtol=2e-4)


@gpu
def test_selector_backward_at_right_angles():
    """One backward on the `orthogonal` case: loss and student gradients finite, the gradients against the oracle's
    autograd at the multi-layer bound of the suite."""
    case = angle_case("orthogonal")
    mod = case.module()
    inp = case.on_device()
    leaves = {k: v.requires_grad_(True) for k, v in inp.student.items()}
    loss = mod(inp.logits, inp.targets, leaves, inp.teacher, inp.attn)
    loss.backward()
    torch.cuda.synchronize()
    assert dict(mod.layer_selector.subspace_ranks) == case.ranks
    assert math.isfinite(loss.item())
    np.testing.assert_allclose(loss.item(), case.ref.item(), rtol=1e-4)
    for l in case.layers:
        got, want = leaves[l].grad.cpu(), case.ref_leaves[l].grad
        assert bool(torch.isfinite(got).all())
        err = float((got - want).norm() / want.norm())
        print(f"selector orthogonal backward layer {l}: student gradient error {err:.2e}")
        assert err < 2e-3, (l, err)
