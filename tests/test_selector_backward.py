"""The backward of the Grassmannian selector for multi-layer teachers, kernel by kernel: the shifted tridiagonal solve
(``basd_tridiag_shifted_solve``) on tridiagonals given directly, among them nearly reducible ones whose coupling entry
is tiny but not zero, then ``basd_eigvec_k2``, ``basd_build_angle_stack``, ``basd_grassmann_distance_bwd`` and
``basd_token_weight_bwd`` each alone, and the two routes of ``_distance_backward`` composed.

Every input is built from seeded generators and rounded to fp32; the reference of every test is the same fp32 input
evaluated in fp64 on the CPU.  The unmarked tests run without a GPU: they hold an fp32 CPU solver to the bounds of the
GPU tests, so a fixture that no fp32 code could pass fails there first, and they measure the fp32 errors that some of
the bounds are multiples of."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
DEV = "cuda:0"
EPS32 = 2.0 ** -23


# --------------------------------------------------------------------------- #
# 1. the shifted solve on tridiagonals given directly
# --------------------------------------------------------------------------- #
# Bound of every case: the relative 2-norm error on the orthogonal complement of the shift's cluster is at most
# 4 eps32 ||T||_2 / gap -- the condition number of the solve on the complement times the unit round-off; gap is the
# distance of the shift from the nearest eigenvalue outside its cluster (eigenvalues within 1e-5 ||T|| of the shift's).
# The fp32 bordered-system solve of the unmarked test stays at or below 0.3 of the same product.
SOLVE_FACTOR = 4.0
CLUSTER = 1e-5
GLUES = (0.0, 2.0 ** -50, 2.0 ** -33, 2.0 ** -27, 2.0 ** -23, 2.0 ** -20, 2.0 ** -17, 2.0 ** -13)      # g / ||T||
S44 = math.sqrt(44.0)


def householder_tridiagonal(G):
    """(d, e) of Q^T G Q for a symmetric fp64 matrix, by Householder reflectors in fp64."""
    A = np.array(G, dtype=np.float64)
    n = A.shape[0]
    for k in range(n - 2):
        x = A[k + 1:, k]
        alpha = -math.copysign(float(np.linalg.norm(x)), float(x[0]) if x[0] != 0 else 1.0)
        v = x.copy()
        v[0] -= alpha
        nv = float(np.linalg.norm(v))
        if nv == 0.0:
            continue
        v /= nv
        A[k + 1:, :] -= 2.0 * np.outer(v, v @ A[k + 1:, :])
        A[:, k + 1:] -= 2.0 * np.outer(A[:, k + 1:] @ v, v)
    return np.diagonal(A).copy(), np.diagonal(A, 1).copy()


@functools.lru_cache(maxsize=None)
def randn_gram_tridiagonal(rows, n, seed, lead=True):
    """The tridiagonal of the Gram of a seeded ``randn`` (rows, n); ``lead``: the first eight columns scaled 6 ... 2 as in
    test_tridiag_apply_q_and_shifted_solve."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, n, generator=g, dtype=torch.float64)
    if lead:
        x[:, :8] *= torch.linspace(6.0, 2.0, 8, dtype=torch.float64)
    return householder_tridiagonal((x.T @ x).numpy())


class SolveCase:
    """One tridiagonal (d, e) in fp32 with the eigenvalue indices (descending order) to shift by.  The fp64
    decomposition of the fp32 tridiagonal and the right-hand sides are computed once and never modified."""

    def __init__(self, name, d, e, js, seed=0):
        self.name, self.js = name, tuple(js)
        self.d = torch.as_tensor(np.asarray(d, dtype=np.float64)).float()
        self.e = torch.as_tensor(np.asarray(e, dtype=np.float64)).float()
        self.n = n = self.d.numel()
        assert self.e.numel() == n - 1
        T = torch.diag(self.d.double()) + torch.diag(self.e.double(), 1) + torch.diag(self.e.double(), -1)
        ev, evec = torch.linalg.eigh(T)
        self.T, self.ev, self.evec = T, ev.flip(0), evec.flip(1)
        self.norm = float(self.ev.abs().max())
        g = torch.Generator().manual_seed(1000 + seed)
        raw = torch.randn(len(self.js), n, generator=g, dtype=torch.float64)
        self.rhs = torch.stack([self.project(j, raw[i]) for i, j in enumerate(self.js)]).float()

    def cluster(self, j):
        return (self.ev - self.ev[j]).abs() <= CLUSTER * self.norm

    def project(self, j, x):
        vc = self.evec[:, self.cluster(j)]
        return x - vc @ (vc.T @ x)

    def judge(self, i, shift, x):
        """(relative error on the complement, bound, largest raw entry over its limit) of the fp32 solution ``x`` for
        right-hand side i and the fp32 ``shift`` that was used."""
        j = self.js[i]
        out = ~self.cluster(j)
        shift = float(shift)
        assert abs(shift - float(self.ev[j])) <= 4 * EPS32 * self.norm, (self.name, j, shift, float(self.ev[j]))
        rhs = self.rhs[i].double()
        v = self.evec[:, out]
        ref = v @ ((v.T @ rhs) / (self.ev[out] - shift))
        gap = float((self.ev[out] - shift).abs().min())
        err = float((self.project(j, x.double()) - ref).norm() / ref.norm())
        raw = float(x.abs().max()) / (float(rhs.norm()) / (EPS32 ** 2 * self.norm))
        return err, SOLVE_FACTOR * EPS32 * self.norm / gap, raw


def _ones(n):
    """ones + 2 I after one reflector: the top eigenvalue n + 2 lives in the leading 2 x 2 block, glued by g; past
    order 45 the diagonal continues with 2."""
    return lambda g: ([3.0, 46.0] + [2.0] * (n - 2), [-S44] + [g] * (n - 2))


def _chain(g):
    return [3.0, 46.0, 103.0, 146.0, 203.0, 246.0, 1.0, 1.0, 1.0], [-S44, g, -S44, g, -S44, g, g, g]


def _glued_randn(g):
    d, e = randn_gram_tridiagonal(200, 40, 11, lead=False)
    return [403.0, 446.0] + list(d), [-S44, g] + list(e)


# The same three with the block [[43, 2], [2, 46]] (eigenvalues 47 and 42) in place of [[3, -sqrt 44], [-sqrt 44, 46]]:
# every entry and the eigenvalue are fp32 numbers and the elimination of the block is exact, so the reduced diagonal
# entry at its end is exactly 0 in any arithmetic, fused or not.  With sqrt 44 it is a rounding residue whose size
# depends on whether the compiler contracts a - m * b.
def _exact(n):
    return lambda g: ([43.0, 46.0] + [2.0] * (n - 2), [2.0] + [g] * (n - 2))


def _chain_exact(g):
    return [43.0, 46.0, 143.0, 146.0, 243.0, 246.0, 1.0, 1.0, 1.0], [2.0, g, 2.0, g, 2.0, g, g, g]


def _glued_randn_exact(g):
    d, e = randn_gram_tridiagonal(200, 40, 11, lead=False)
    return [443.0, 446.0] + list(d), [2.0, g] + list(e)


GLUED_FAMILIES = (("ones45", _ones(45), 47.0, (0,)),
                  ("ones200", _ones(200), 47.0, (0,)),
                  ("chain", _chain, 247.0, (0, 1, 2)),
                  ("glued_randn", _glued_randn, 447.0, (0,)),
                  ("exact45", _exact(45), 47.0, (0,)),
                  ("exact200", _exact(200), 47.0, (0,)),
                  ("chain_exact", _chain_exact, 247.0, (0, 1, 2)),
                  ("glued_randn_exact", _glued_randn_exact, 447.0, (0,)))


@functools.lru_cache(maxsize=None)
def solve_cases():
    cases = []
    for fi, (name, make, norm, js) in enumerate(GLUED_FAMILIES):
        for gi, rel in enumerate(GLUES):
            d, e = make(rel * norm)
            cases.append(SolveCase(f"{name} g/|T|=2^{math.log2(rel):.0f}" if rel else f"{name} g=0", d, e, js,
                                   seed=16 * fi + gi))
    cases.append(SolveCase("wilkinson21", np.abs(np.arange(21) - 10.0), np.ones(20), (0, 2), seed=90))
    cases.append(SolveCase("toeplitz201", np.full(201, 2.0), np.full(200, -1.0), (0, 5), seed=91))
    for n in (100, 384):
        d, e = randn_gram_tridiagonal(4 * n, n, 3 * n)
        cases.append(SolveCase(f"randn_gram{n}", d, e, range(8), seed=92 + n))
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def strided_case():
    """70 right-hand sides at order 45 (64 vectors per workgroup: a second workgroup with a partial tail), the shifts
    cycling through the leading 35 eigenvalues."""
    d, e = randn_gram_tridiagonal(180, 45, 135)
    return SolveCase("randn_gram45 k=70", d, e, [t % 35 for t in range(70)], seed=95)


def bordered_fp32(case, i, shift):
    """The fp32 reference solver: numpy's LU in float32 of [[T - shift I, V_c], [V_c^T, 0]]."""
    n, j = case.n, case.js[i]
    vc = case.evec[:, case.cluster(j)].numpy().astype(np.float32)
    c = vc.shape[1]
    A = np.zeros((n + c, n + c), dtype=np.float32)
    A[:n, :n] = case.T.numpy().astype(np.float32) - np.float32(shift) * np.eye(n, dtype=np.float32)
    A[:n, n:], A[n:, :n] = vc, vc.T
    b = np.concatenate([case.rhs[i].numpy(), np.zeros(c, dtype=np.float32)])
    x = np.linalg.solve(A, b)
    assert x.dtype == np.float32
    return torch.from_numpy(x[:n].copy())


def test_solve_fixtures_are_well_posed_for_an_fp32_solver():
    """Guards the fixtures and the bound, not the kernel: an fp32 LU of the bordered system meets the bound of the GPU
    test on every case, and every right-hand side is orthogonal to its cluster."""
    worst = 0.0
    for case in solve_cases() + (strided_case(),):
        assert case.d.dtype == torch.float32 and case.n <= 384
        for i, j in enumerate(case.js):
            shift = np.float32(float(case.ev[j]))
            vc = case.evec[:, case.cluster(j)]
            assert float((vc.T @ case.rhs[i].double()).abs().max()) <= 4 * EPS32 * float(case.rhs[i].norm())
            err, bound, raw = case.judge(i, shift, bordered_fp32(case, i, shift))
            if i < 8:
                print(f"fp32 bordered {case.name} j={j}: err {err:.2e} bound {bound:.2e} "
                      f"ratio {err / bound * SOLVE_FACTOR:.3f}")
            worst = max(worst, err / bound * SOLVE_FACTOR)
            assert err <= bound and raw <= 1.0, (case.name, j, err, bound, raw)
    print(f"fp32 bordered: worst err / (eps |T| / gap) = {worst:.3f} (the bound allows {SOLVE_FACTOR})")


def _state(cases):
    """A TridiagState of the cases' tridiagonals themselves (one order): tau = 0, so no reflector is applied."""
    from basd_amd import ops
    n, b = cases[0].n, len(cases)
    f32 = dict(device=DEV, dtype=torch.float32)
    d = torch.stack([c.d for c in cases]).to(DEV).contiguous()
    e = torch.zeros(b, n, **f32)
    e[:, :n - 1] = torch.stack([c.e for c in cases]).to(DEV)
    ts = ops.TridiagState(d, e, torch.zeros(b, n, **f32), torch.zeros(b, n, n, **f32), torch.empty(b, n, **f32))
    ops.tridiag_spectrum(ts)
    return ts


def _run_solves(cases, shift_pad=0):
    """Two launches per order and number of shifts: with the shifts the library's own bisection returned (``ts.vals``)
    and with the fp64 eigenvalues rounded to fp32, which may differ by an ulp.  Returns {(case name, shift source):
    [(j, err, bound, raw, finite)]}."""
    from basd_amd import ops
    groups = {}
    for c in cases:
        groups.setdefault((c.n, len(c.js)), []).append(c)
    out = {}
    for (n, k), group in groups.items():
        ts = _state(group)
        idx = torch.tensor([c.js for c in group], device=DEV)
        rhs = torch.stack([c.rhs for c in group]).to(DEV).contiguous()
        nearest = torch.stack([c.ev[list(c.js)] for c in group]).float().to(DEV)
        for source, values in (("bisection", ts.vals.gather(1, idx)), ("nearest", nearest)):
            shifts = torch.full((len(group), k + shift_pad), float("nan"), device=DEV)
            shifts[:, :k] = values
            x = ops.tridiag_shifted_solve(ts, shifts[:, :k], rhs).cpu()
            used = shifts[:, :k].cpu()
            for b, c in enumerate(group):
                rows = []
                for i, j in enumerate(c.js):
                    finite = bool(torch.isfinite(x[b, i]).all())
                    err, bound, raw = c.judge(i, used[b, i], torch.nan_to_num(x[b, i], nan=0.0, posinf=0.0, neginf=0.0))
                    rows.append((j, err, bound, raw, finite))
                out[c.name, source] = rows
    return out


def _check_solves(results, limit=None):
    failures = []
    for (name, source), rows in results.items():
        for j, err, bound, raw, finite in rows[:limit]:
            print(f"shifted solve {name} j={j} shift={source}: err {err:.2e} bound {bound:.2e} raw/limit {raw:.1e}")
        for j, err, bound, raw, finite in rows:
            if not (finite and err <= bound and raw <= 1.0):
                failures.append((name, source, j, err, bound, raw, finite))
    assert not failures, failures


@gpu
@pytest.mark.parametrize("family", [f[0] for f in GLUED_FAMILIES])
def test_shifted_solve_on_nearly_reducible_tridiagonals(family):
    """The glue sweep: a leading 2 x 2 block holds the shift's eigenvalue and is coupled to the rest by g, from exactly
    0 through far below eps ||T|| to 2^-13 ||T||.  The elimination reduces the diagonal entry at the end of the block to
    about 0 and then meets g.  Before the kernel moved that diagonal entry to +-eps ||T|| ahead of the pivot choice, an
    exact 0 there lost the comparison to any g != 0, and the pivot replaced during the back substitution was the
    off-diagonal g: the `exact` families (reduced entry exactly 0 in any arithmetic) came out with relative errors of
    5e-5 ... 4e+5 for g / ||T|| <= 2^-23 and up to 4 times the bound at 2^-20, on an MI355X.  The families with
    sqrt(44) passed there even before: the compiler contracts a - m * b, which leaves a residue of 6e-8 instead of
    the 0 that unfused fp32 arithmetic gives, and with it the comparison goes the other way."""
    _check_solves(_run_solves([c for c in solve_cases() if c.name.startswith(family + " ")]))


@gpu
def test_shifted_solve_on_healthy_tridiagonals():
    """W21+ (a shift inside a pair 7e-14 apart), Toeplitz(2, -1) at 201 and the tridiagonals of ``randn`` Grams at 100
    and 384 (the input of test_tridiag_apply_q_and_shifted_solve, held to the bound of this file)."""
    names = ("wilkinson21", "toeplitz201", "randn_gram100", "randn_gram384")
    _check_solves(_run_solves([c for c in solve_cases() if c.name in names]))


@gpu
def test_shifted_solve_second_workgroup_and_shift_stride():
    """k = 70 at order 45: 64 vectors in the first workgroup, 6 in the second; the shifts are a slice of a wider array
    (``shift_stride`` 96 > k) whose other entries are NaN."""
    _check_solves(_run_solves([strided_case()], shift_pad=26), limit=3)


# --------------------------------------------------------------------------- #
# 2. basd_eigvec_k2
# --------------------------------------------------------------------------- #
K2_SHAPES = ((64, 64), (64, 8), (200, 37), (1, 1))          # (D, kmax); D == kmax is the k x k call with lam_k
K2_BATCH = 3
# pairs of neighbours (i, i + 1) planted where kmax >= 8: exactly equal, 0.5e-6 lam_0 apart (both masked: the kernel
# divides only where |lam_j - lam_i| > 1e-6 lam_0) and 2e-6 lam_0 apart (divided)
K2_EQUAL, K2_NEAR, K2_DIVIDED = 1, 4, 6


@functools.lru_cache(maxsize=None)
def k2_inputs(D, kmax):
    """(M (batch, D, kmax), lam (batch, D)) fp32: lam descending from about 100 in steps of 0.5 ... 1.5, a gap of 20
    below the leading kmax."""
    g = torch.Generator().manual_seed(17 * D + kmax)
    step = 0.5 + torch.rand(K2_BATCH, D, generator=g, dtype=torch.float64)
    if kmax < D:
        step[:, kmax] += 20.0
    lam = 100.0 + 4.0 * torch.arange(K2_BATCH, dtype=torch.float64).view(-1, 1) + 1.6 * D + 20.0 - step.cumsum(1)
    lam = lam.float()
    if kmax >= 8:
        lam0 = lam[:, 0]
        lam[:, K2_EQUAL + 1] = lam[:, K2_EQUAL]
        lam[:, K2_NEAR + 1] = (lam[:, K2_NEAR].double() - 0.5e-6 * lam0.double()).float()
        lam[:, K2_DIVIDED + 1] = (lam[:, K2_DIVIDED].double() - 2e-6 * lam0.double()).float()
    m = torch.randn(K2_BATCH, D, kmax, generator=g, dtype=torch.float64).float()
    return m, lam


def k2_reference(m, lam):
    """(K2 in fp64 with the kernel's mask, the element-wise bound 4 eps (|M_ij| + |M_ji|) / |lam_j - lam_i|, the mask)
    from the fp32 inputs; M is taken as 0 past its kmax columns."""
    batch, D, kmax = m.shape
    full = torch.zeros(batch, D, D, dtype=torch.float64)
    full[:, :, :kmax] = m.double()
    den = lam.double().unsqueeze(1) - lam.double().unsqueeze(2)            # den[i][j] = lam_j - lam_i
    thr = (torch.tensor(1e-6, dtype=torch.float32) * lam[:, 0]).double().view(-1, 1, 1)
    lead = torch.arange(D) < kmax
    mask = (den.abs() > thr) & (lead.view(1, -1, 1) | lead.view(1, 1, -1)) & ~torch.eye(D, dtype=torch.bool)
    safe = torch.where(mask, den, torch.ones_like(den))
    ref = torch.where(mask, (full - full.transpose(1, 2)) / safe, torch.zeros_like(den))
    bound = torch.where(mask, 4 * EPS32 * (full.abs() + full.abs().transpose(1, 2)) / safe.abs(), torch.zeros_like(den))
    return ref, bound, mask


def test_k2_fixtures_plant_the_pairs_away_from_the_threshold():
    """No pair of eigenvalues lies within a factor 1.5 of the kernel's threshold 1e-6 lam_0, so the mask of the
    reference cannot differ from the kernel's by a rounding; the planted pairs are where the docstring says; and the
    formula in fp32 on the CPU stays within the bound."""
    for D, kmax in K2_SHAPES:
        m, lam = k2_inputs(D, kmax)
        assert bool((lam[:, :-1] >= lam[:, 1:]).all()) and bool((lam > 0).all())
        ref, bound, mask = k2_reference(m, lam)
        den = (lam.double().unsqueeze(1) - lam.double().unsqueeze(2)).abs() / lam[:, :1].double().unsqueeze(2)
        off = ~torch.eye(D, dtype=torch.bool).expand_as(den)
        assert not bool(((den > 1e-6 / 1.5) & (den < 1.5e-6) & off).any()), (D, kmax)
        if kmax >= 8:
            assert not bool(mask[:, K2_EQUAL, K2_EQUAL + 1].any()) and bool((den[:, K2_EQUAL, K2_EQUAL + 1] == 0).all())
            assert not bool(mask[:, K2_NEAR, K2_NEAR + 1].any()) and bool((den[:, K2_NEAR, K2_NEAR + 1] > 0).all())
            assert bool(mask[:, K2_DIVIDED, K2_DIVIDED + 1].all())
            assert bool((den[:, K2_DIVIDED, K2_DIVIDED + 1] < 3e-6).all())
        full = torch.zeros_like(ref, dtype=torch.float32)
        full[:, :, :kmax] = m
        d32 = lam.unsqueeze(1) - lam.unsqueeze(2)
        got = torch.where(mask, (full - full.transpose(1, 2)) / torch.where(mask, d32, torch.ones_like(d32)),
                          torch.zeros_like(d32))
        ratio = float(((got.double() - ref).abs()[mask] / bound[mask].clamp_min(1e-300)).max()) if mask.any() else 0.0
        print(f"eigvec_k2 fp32 cpu D={D} kmax={kmax}: worst error / bound {ratio:.3f}")
        assert ratio <= 1.0


@gpu
@pytest.mark.parametrize("D,kmax", K2_SHAPES)
def test_eigvec_k2_elementwise(D, kmax):
    """K2[i][j] = (M[i][j] - M[j][i]) / (lam_j - lam_i) against fp64, element by element; symmetric bit for bit; zero on
    the diagonal, in the trailing x trailing block and at pairs closer than 1e-6 lam_0."""
    from basd_amd import ops
    m, lam = k2_inputs(D, kmax)
    ref, bound, mask = k2_reference(m, lam)
    k2 = ops.eigvec_k2(m.to(DEV).contiguous(), lam.to(DEV).contiguous()).cpu()
    assert k2.shape == (K2_BATCH, D, D) and bool(torch.isfinite(k2).all())
    assert torch.equal(k2, k2.transpose(1, 2)), "K2 must be symmetric bit for bit"
    assert not bool(k2[~mask].any()), "non-zero where the definition has a zero"
    excess = (k2.double() - ref).abs() - bound
    ratio = float(((k2.double() - ref).abs()[mask] / bound[mask].clamp_min(1e-300)).max()) if mask.any() else 0.0
    print(f"eigvec_k2 D={D} kmax={kmax}: worst error / bound {ratio:.3f} divided {int(mask.sum())} of {mask.numel()}")
    assert bool((excess <= 0).all()), (D, kmax, float(excess.max()))
    if kmax >= 8:
        assert bool((k2[:, K2_DIVIDED, K2_DIVIDED + 1] != 0).all())


# --------------------------------------------------------------------------- #
# 3. basd_build_angle_stack
# --------------------------------------------------------------------------- #
@gpu
@pytest.mark.parametrize("kmax", [1, 8, 37, 200])
def test_angle_stack_is_the_definition(kmax):
    """Column c of item m is [cos[m][c][0 .. k) , 0 ... ; e_c] for c < k and [0 ; e_c] beyond, exactly; ``cos`` holds NaN
    outside its k x k block, which the kernel must not read into the result."""
    from basd_amd import ops
    ks = [kmax, kmax - 1, 1, 0]
    g = torch.Generator().manual_seed(kmax)
    cos = torch.full((len(ks), kmax, kmax), float("nan"))
    want = torch.zeros(len(ks), kmax, 2 * kmax)
    for m, k in enumerate(ks):
        block = torch.randn(k, k, generator=g)
        cos[m, :k, :k] = block
        want[m, :k, :k] = block
        want[m, :, kmax:] = torch.eye(kmax)
    got = ops.angle_stack(cos.to(DEV), torch.tensor(ks, dtype=torch.int32, device=DEV)).cpu()
    print(f"angle_stack kmax={kmax} k={ks}: equal {torch.equal(got, want)}")
    assert torch.equal(got, want)


# --------------------------------------------------------------------------- #
# 4. basd_grassmann_distance_bwd
# --------------------------------------------------------------------------- #
GD_KMAX = (8, 37, 64, 200, 300)
GD_KINDS = ("spread", "tied", "small", "clamped_and_zero", "all_clamped")
ONE_BELOW = 1.0 - 2.0 ** -24          # the largest fp32 below 1: at or past the clamp 1 - 2^-23, so it contributes 0


@functools.lru_cache(maxsize=None)
def gd_inputs(kmax):
    """Five items of order k < kmax: W = V diag(s) U^T from seeded fp64 orthogonal factors and prescribed singular
    values; the solver's output is emulated as the columns [s_c U_c ; V_c] (zero-padded to kmax, [0 ; e_c] for c >= k),
    shuffled over all kmax positions by a fixed permutation and rounded to fp32, with ``colnorm`` = s in the same
    order.  sw: three rows of a wider array, positive and decreasing.  Returns a namespace of fp32 CPU tensors."""
    g = torch.Generator().manual_seed(31 * kmax)
    ks = [kmax - 1, max(kmax - 3, 2), kmax // 2 + 1, max(kmax - 2, 3), kmax - 1]
    stack = torch.zeros(len(ks), kmax, 2 * kmax, dtype=torch.float64)
    colnorm = torch.zeros(len(ks), kmax, dtype=torch.float64)
    sw_wide = torch.rand(3, kmax + 5, generator=g, dtype=torch.float64).sort(dim=1, descending=True).values + 0.1
    for m, (kind, k) in enumerate(zip(GD_KINDS, ks)):
        s = 0.05 + (0.999 - 0.05) * torch.rand(k, generator=g, dtype=torch.float64)
        if kind == "tied":                               # the two largest
            s[0], s[1], s[2:] = 0.9, 0.9, s[2:] * 0.85
        elif kind == "small":
            s[k // 2] = 1e-3
        elif kind == "clamped_and_zero":
            s[0], s[1] = ONE_BELOW, 0.0
        elif kind == "all_clamped":
            s[0::2], s[1::2] = ONE_BELOW, 0.0
        u, _ = torch.linalg.qr(torch.randn(k, k, generator=g, dtype=torch.float64))
        v, _ = torch.linalg.qr(torch.randn(k, k, generator=g, dtype=torch.float64))
        cols = torch.zeros(kmax, 2 * kmax, dtype=torch.float64)
        cols[:k, :k] = (u * s).T                         # column c, top part: s_c U[:, c]
        cols[:k, kmax:kmax + k] = v.T                    # bottom part: V[:, c]
        cols[k:, kmax:] = torch.eye(kmax, dtype=torch.float64)[k:]
        norms = torch.cat([s, torch.zeros(kmax - k, dtype=torch.float64)])
        perm = torch.randperm(kmax, generator=g)
        stack[m], colnorm[m] = cols[perm], norms[perm]
    sw_wide[0, 1] = sw_wide[0, 0]     # the tied pair (largest two of item 1, row 0) shares one spectral weight: its
    sw_wide = sw_wide.float()         # contribution then does not depend on the basis chosen inside the pair
    return SimpleNamespace(stack=stack.float(), colnorm=colnorm.float(), ks=ks, sw_wide=sw_wide,
                           sw_index=[2, 0, 1, 2, 0], gd=(0.5 + torch.rand(len(ks), generator=g)).float())


def gd_formula(inp, dtype):
    """dd/dW^T = sum_c f'_c / s_c (top_c)(bottom_c)^T of the kernel's comment, in ``dtype`` on the CPU: columns sorted by
    ``colnorm`` descending (ties: lower index first), the p-th largest paired with sw[p], f' = 0 at the clamp and at 0."""
    kmax = inp.colnorm.shape[1]
    outs = []
    for m, k in enumerate(inp.ks):
        s_all = inp.colnorm[m].to(dtype)
        order = torch.sort(s_all, descending=True, stable=True).indices[:k]
        s = s_all[order]
        w = inp.sw_wide[inp.sw_index[m], :kmax].to(dtype)[:k]
        live = (inp.colnorm[m][order] < np.float32(1.0) - np.float32(2.0 ** -23)) & (inp.colnorm[m][order] > 1e-20)
        s_safe = torch.where(live, s, torch.full_like(s, 0.5))
        f = inp.gd[m].to(dtype) * w * (-2 * torch.acos(s_safe) / torch.sqrt(1 - s_safe * s_safe)) / w.sum() / s_safe
        f = torch.where(live, f, torch.zeros_like(f))
        cols = inp.stack[m].to(dtype)[order]
        out = torch.zeros(kmax, kmax, dtype=dtype)
        out[:k, :k] = ((cols[:, :kmax] * f.unsqueeze(1)).T @ cols[:, kmax:])[:k, :k]
        outs.append(out)
    return torch.stack(outs)


@functools.lru_cache(maxsize=None)
def gd_reference(kmax):
    """(fp64 result, worst error of the fp32 CPU evaluation relative to the item's largest entry).  Never modified."""
    inp = gd_inputs(kmax)
    ref, got = gd_formula(inp, torch.float64), gd_formula(inp, torch.float32)
    worst = 0.0
    for m, kind in enumerate(GD_KINDS):
        if kind != "all_clamped":
            worst = max(worst, float((got[m].double() - ref[m]).abs().max() / ref[m].abs().max()))
    return ref, worst


def test_distance_bwd_fixtures_and_the_fp32_error():
    """The fixtures are what the docstrings say (tied pair with one spectral weight, the clamped and the zero singular
    values present, orders below kmax) and the error of the formula in fp32 on the CPU, four times which is the bound of
    the GPU test, is a few eps."""
    for kmax in GD_KMAX:
        inp = gd_inputs(kmax)
        assert all(0 < k < kmax for k in inp.ks) and inp.sw_wide.stride(0) > kmax
        srt = inp.colnorm.sort(dim=1, descending=True).values
        assert float(srt[1, 0]) == float(srt[1, 1])
        assert float(srt[3, 0]) == np.float32(ONE_BELOW) and int((inp.colnorm[3] == 0).sum()) == kmax - inp.ks[3] + 1
        assert abs(float(inp.colnorm[2][inp.colnorm[2] > 0].min()) - 1e-3) < 1e-9
        ref, worst = gd_reference(kmax)
        assert not bool(ref[4].any()), "every singular value of the last item is clamped or zero"
        assert bool(torch.isfinite(ref).all()) and all(bool(ref[m].any()) for m in range(4))
        print(f"distance_bwd fp32 cpu kmax={kmax}: worst error / largest entry {worst:.2e}")
        assert worst < 64 * EPS32, (kmax, worst)


@gpu
@pytest.mark.parametrize("kmax", GD_KMAX)
def test_grassmann_distance_bwd_alone(kmax):
    """gWt against V diag(f') U^T in fp64 on stacks that no Jacobi sweep produced; bound: four times the error of the
    same formula in fp32 on the CPU.  Clamped and zero singular values contribute exactly 0; entries outside k x k are 0."""
    from basd_amd import ops
    inp = gd_inputs(kmax)
    ref, worst32 = gd_reference(kmax)
    sw = inp.sw_wide.to(DEV)[:, :kmax]
    got = ops.grassmann_distance_bwd(inp.stack.to(DEV).contiguous(), inp.colnorm.to(DEV).contiguous(),
                                     torch.tensor(inp.ks, dtype=torch.int32, device=DEV), sw,
                                     torch.tensor(inp.sw_index, dtype=torch.int32, device=DEV), inp.gd.to(DEV)).cpu()
    assert bool(torch.isfinite(got).all())
    failures = []
    for m, (kind, k) in enumerate(zip(GD_KINDS, inp.ks)):
        outside = torch.ones(kmax, kmax, dtype=torch.bool)
        outside[:k, :k] = False
        assert not bool(got[m][outside].any()), (kind, "non-zero outside k x k")
        if kind == "all_clamped":
            print(f"distance_bwd kmax={kmax} {kind}: non-zero entries {int(got[m].count_nonzero())}")
            assert not bool(got[m].any())
            continue
        err = float((got[m].double() - ref[m]).abs().max() / ref[m].abs().max())
        print(f"distance_bwd kmax={kmax} {kind} k={k}: err {err:.2e} bound {4 * worst32:.2e} (fp32 cpu {worst32:.2e})")
        if err > 4 * worst32:
            failures.append((kind, err, 4 * worst32))
    assert not failures, failures


# --------------------------------------------------------------------------- #
# 5. basd_token_weight_bwd
# --------------------------------------------------------------------------- #
TW_GRIDS = ((49, 49), (49, 196), (196, 49), (300, 64))        # (n_a, n_s): no taps, up, down, n_a past one block
TW_E, TW_B, TW_L = 2, 3, 3


@functools.lru_cache(maxsize=None)
def tw_inputs(n_a, n_s, has_cls, H, bf16, sliced):
    """L attention maps (softmax rows; fp32 or bf16; ``sliced``: H heads cut out of H + 2), mixing weights, the raw
    attention-grid weight of the mix rounded to fp32 (the kernel's input) and gomega."""
    from oracle import basd_oracle as O
    g = torch.Generator().manual_seed(1000 * n_a + 10 * n_s + 4 * H + 2 * has_cls + bf16)
    A = n_a + 1 if has_cls else n_a
    heads = H + 2 if sliced else H
    maps = [torch.softmax(2.0 * torch.randn(TW_B, heads, A, A, generator=g), dim=-1) for _ in range(TW_L)]
    maps = [m.bfloat16() if bf16 else m for m in maps]
    views = [m[:, 1:H + 1] if sliced else m for m in maps]
    mix = torch.softmax(torch.randn(TW_E, TW_L, generator=g, dtype=torch.float64), dim=1)
    rowmean = torch.stack([v.double()[:, :, 0, 1:].mean(dim=1) if has_cls else v.double().mean(dim=(1, 2))
                           for v in views])                                  # (L, B, n_a): relational.py:22-26
    raw = torch.einsum("el,lbj->ebj", mix, rowmean).float()
    gomega = torch.randn(TW_E, TW_B, n_s, generator=g)
    return SimpleNamespace(maps=maps, views=views, mix=mix, rowmean=rowmean, raw=raw, gomega=gomega, A=A, O=O)


def tw_reference(inp, n_a, n_s):
    """fp64 autograd of ``oracle.token_weights`` at the fp32 ``raw`` (fed in as the CLS row of a one-head map), dotted
    with gomega: g_raw (E, B, n_a), partial (E, B, L) and the bound of each, (terms + 4) eps sum |terms|, with the
    absolute values carried through the same chain (normalisation, adjoint of the interpolation, layer mean)."""
    E, B, L = TW_E, TW_B, TW_L
    leaf = inp.raw.double().clone().requires_grad_(True)
    fake = torch.cat([torch.zeros(E * B, 1, 1, 1, dtype=torch.float64), leaf.view(E * B, 1, 1, n_a)], dim=3)
    omega = inp.O.token_weights(fake, True, n_s).view(E, B, n_s)
    (g_raw,) = torch.autograd.grad((omega * inp.gomega.double()).sum(), leaf)
    partial = torch.einsum("ebj,lbj->ebl", g_raw, inp.rowmean)
    # absolute sums: d omega_s / d v_t = (delta_st - omega_s) / total  ->  |go_s| + sum_s |go_s| omega_s, over total
    v = leaf.detach()
    if n_a != n_s:
        i0, i1, lam = inp.O.interp_taps(n_a, n_s)
        lam = lam.double()
        v = (1 - lam) * v[..., i0] + lam * v[..., i1]
    total = v.sum(dim=-1, keepdim=True)
    abs_gv = (inp.gomega.double().abs() + (inp.gomega.double().abs() * v / total).sum(dim=-1, keepdim=True)) / total
    per_row = torch.ones(n_a, dtype=torch.float64)
    if n_a != n_s:
        abs_graw = torch.zeros(E, B, n_a, dtype=torch.float64)
        abs_graw.index_add_(2, i0, (1 - lam) * abs_gv)
        abs_graw.index_add_(2, i1, lam * abs_gv)
        per_row = torch.zeros(n_a, dtype=torch.float64).index_add_(0, i0, torch.ones(n_s, dtype=torch.float64))
        per_row.index_add_(0, i1, torch.ones(n_s, dtype=torch.float64))
    else:
        abs_graw = abs_gv
    H = inp.views[0].shape[1]
    inner = 2 * n_s + (H if inp.A == n_a + 1 else H * inp.A)          # the two sums over n_s, the head / query mean
    b_graw = (per_row + 2 * n_s + 4) * EPS32 * abs_graw
    b_partial = (n_a + float(per_row.max()) + inner + 4) * EPS32 * torch.einsum("ebj,lbj->ebl", abs_graw, inp.rowmean)
    return g_raw, partial, b_graw, b_partial


def _tw_ratio(got, ref, bound):
    """Worst error / bound; an element whose bound is 0 (an attention-grid row that no student token taps) must be
    exactly the reference."""
    err = (got.double() - ref).abs()
    assert bool((err[bound == 0] == 0).all())
    return float((err[bound > 0] / bound[bound > 0]).max())


def test_token_weight_reference_is_the_oracle_chain():
    """The reference of the GPU test (autograd at the rounded ``raw``, then a dot with the layers' row means) agrees
    with fp64 autograd straight through ``oracle.token_weights`` of the mixed maps with respect to the mixing weights,
    up to the rounding of ``raw`` to fp32."""
    for (n_a, n_s), has_cls in zip(TW_GRIDS, (True, False, True, False)):
        inp = tw_inputs(n_a, n_s, has_cls, 3, False, False)
        _, partial, _, b_partial = tw_reference(inp, n_a, n_s)
        mix = inp.mix.clone().requires_grad_(True)
        direct = torch.zeros_like(partial)
        for e in range(TW_E):
            mixed = sum(mix[e, l] * inp.views[l].double() for l in range(TW_L))
            omega = inp.O.token_weights(mixed, has_cls, n_s)
            for b in range(TW_B):
                (gm,) = torch.autograd.grad((omega[b] * inp.gomega[e, b].double()).sum(), mix, retain_graph=True)
                direct[e, b] = gm[e]
        gap = float(((direct - partial).abs() / b_partial).max())
        # the kernel's formulas in fp32 torch on the CPU: the bounds must leave room for an fp32 evaluation
        g_ref, _, b_graw, _ = tw_reference(inp, n_a, n_s)
        v = inp.raw
        if n_a != n_s:
            i0, i1, lam = inp.O.interp_taps(n_a, n_s)
            v = (1 - lam) * v[..., i0] + lam * v[..., i1]
        total = v.sum(dim=-1, keepdim=True)
        gv = (inp.gomega - (inp.gomega * (v / total)).sum(dim=-1, keepdim=True)) / total
        g32 = gv
        if n_a != n_s:
            g32 = torch.zeros(TW_E, TW_B, n_a).index_add_(2, i0, (1 - lam) * gv).index_add_(2, i1, lam * gv)
        p32 = torch.einsum("ebj,lbj->ebl", g32, inp.rowmean.float())
        r_p, r_g = _tw_ratio(p32, partial, b_partial), _tw_ratio(g32, g_ref, b_graw)
        print(f"token_weight reference n_a={n_a} n_s={n_s} cls={has_cls}: |chain - direct| / bound {gap:.2e}; "
              f"fp32 cpu partial err / bound {r_p:.3f} g_raw err / bound {r_g:.3f}")
        assert gap < 1.0 and r_p <= 1.0 and r_g <= 1.0


@gpu
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("has_cls", [False, True], ids=["nocls", "cls"])
@pytest.mark.parametrize("n_a,n_s", TW_GRIDS)
def test_token_weight_bwd_alone(n_a, n_s, has_cls, H, bf16):
    """partial[e][b][l] and g_raw[e][b][j] against fp64, element by element, with ``graw_out`` given and null; for H = 3
    the maps are slices along the heads of wider tensors (batch and head strides that are not the packed ones)."""
    from basd_amd import ops, _lib
    sliced = H == 3
    inp = tw_inputs(n_a, n_s, has_cls, H, bf16, sliced)
    g_ref, p_ref, b_graw, b_partial = tw_reference(inp, n_a, n_s)
    maps = [m.to(DEV) for m in inp.maps]
    views = [m[:, 1:H + 1] if sliced else m for m in maps]
    assert views[0].is_contiguous() == (not sliced)
    tp = ops.taps(n_a, n_s, torch.device(DEV))
    tap_args = [t.data_ptr() for t in (tp.tap0, tp.tap1, tp.lam, tp.range0, tp.range1)] if tp else [None] * 5
    table = ops._ptr_table(views)
    sb, sh, sq, sk = views[0].stride()
    assert all(v.stride() == views[0].stride() for v in views)
    gomega, raw = inp.gomega.to(DEV), inp.raw.to(DEV)
    outs = []
    for want_graw in (True, False):
        partial = torch.full((TW_E, TW_B, TW_L), float("nan"), device=DEV)
        g_raw = torch.full((TW_E, TW_B, n_a), float("nan"), device=DEV) if want_graw else None
        _lib.call("basd_token_weight_bwd", gomega.data_ptr(), raw.data_ptr(), TW_E, TW_B, n_a, n_s, *tap_args,
                  table.data_ptr(), ops._dtype_code(views[0]), TW_L, sb, sh, sq, sk, H, inp.A, int(has_cls),
                  partial.data_ptr(), g_raw.data_ptr() if want_graw else None, ops._stream())
        outs.append((partial.cpu(), g_raw.cpu() if want_graw else None))
    (partial, g_raw), (partial_null, _) = outs
    assert torch.equal(partial, partial_null), "the result must not depend on whether g_raw is written"
    assert bool(torch.isfinite(partial).all()) and bool(torch.isfinite(g_raw).all())
    r_p, r_g = _tw_ratio(partial, p_ref, b_partial), _tw_ratio(g_raw, g_ref, b_graw)
    print(f"token_weight_bwd n_a={n_a} n_s={n_s} cls={has_cls} H={H} {'bf16' if bf16 else 'fp32'} sliced={sliced}: "
          f"partial err / bound {r_p:.3f}  g_raw err / bound {r_g:.3f}")
    assert r_p <= 1.0 and r_g <= 1.0, (r_p, r_g)


# --------------------------------------------------------------------------- #
# 6. the two routes of _distance_backward, composed
# --------------------------------------------------------------------------- #
RT = SimpleNamespace(E=2, L=3, B=8, n=32, d_s=64, d_t=96, k=8)
ROUTE_KINDS = ("rotated", "blocks", "graded")
RT_GD = ((0.7, -0.4, 1.1), (-0.9, 0.6, 0.5))          # d (sum gd * d_grass_sq): both signs, no layer left out


def route_distances(proj_s, proj_t, students, teachers, ranks, dtype, cos_range=None):
    """layer_selector.py:86-105 (and :23-37 for the teacher subspaces) restated with every intermediate in ``dtype``:
    the oracle's ``selector_forward`` pins float32.  Returns d_grass_sq (E, L), differentiable in the students.
    ``cos_range``: a list that receives (smallest, largest) cosine of every (student layer, teacher layer)."""
    from oracle import basd_oracle as O
    ps, pt = proj_s.to(dtype), proj_t.to(dtype)
    bases = []
    with torch.no_grad():
        for t, k in zip(teachers, ranks):
            z = t.reshape(-1, t.shape[2]).to(dtype) @ pt.T
            z = z - z.mean(dim=0, keepdim=True)
            _, S, Vh = torch.linalg.svd(z, full_matrices=False)
            bases.append((Vh[:k].T, S[:k]))
    rows = []
    for x in students:
        z = x.reshape(-1, x.shape[2]).to(dtype) @ ps.T
        z = z - z.mean(dim=0, keepdim=True)
        Vh_s = torch.linalg.svd(z, full_matrices=False)[2]
        dists = []
        for (U, sw), k in zip(bases, ranks):
            cosines = torch.linalg.svdvals(Vh_s[:k] @ U)
            if cos_range is not None:
                cos_range.append((float(cosines.detach().min()), float(cosines.detach().max())))
            theta = torch.acos(cosines.clamp(max=1.0 - O.F32_EPS))
            dists.append((sw * theta.square()).sum() / sw.sum())
        rows.append(torch.stack(dists))
    return torch.stack(rows)


class _RouteCase:
    """Three teacher layers with 8 strong columns each (columns 4 l ... 4 l + 7 of the projected coordinates, scaled by
    10) and two student layers whose leading 8 directions lie at prescribed angles to them.

    ``rotated``: student features in the projected coordinates, strong direction i = cos(phi_i) e_i + sin(phi_i)
    e_(8 + i), phi from 0.25 to 1.25: against teacher layer 0 the principal angles are about phi, against the others a
    mixture -- none at 0 or pi / 2.
    ``graded``: as ``rotated`` with the 8 leading amplitudes falling from 10 to 1 (lam_k / lam_0 about 1e-2) over
    a background whose column scales run from 0.3 to 0.01: a trailing spectrum from 1e-3 lam_0 to 1e-6 lam_0, across
    sqrt(eps) lam_0, where normalised columns of G J stop being eigenvectors.
    ``blocks``: student tokens made in their own coordinates from two independent groups of 32 columns, the first with 8
    strong columns, the second multiplied by 2^-12: its block of the Gram sits at 2^-24 of the first, the cross block at
    2^-12, and the tridiagonal form the library reduces it to is nearly reducible."""

    def __init__(self, kind):
        from oracle import basd_oracle as O
        self.kind = kind
        torch.manual_seed(42)
        self.state = O.SelectorState.create(RT.E, RT.d_s, RT.d_t)
        g = torch.Generator().manual_seed({"rotated": 77, "blocks": 78, "graded": 79}[kind])
        M = RT.B * RT.n
        self.teachers, self.ranks = [], []
        for l in range(RT.L):
            z = torch.randn(M, RT.d_s, generator=g)
            z[:, 4 * l:4 * l + 8] += 10 * torch.randn(M, 8, generator=g)
            tok = z @ self.state.proj_t
            self.teachers.append(tok.view(RT.B, RT.n, RT.d_t))
            self.ranks.append(min(O.mp_rank(tok @ self.state.proj_t.T), RT.d_s - 1))
        self.students = []
        for e in range(RT.E):
            if kind == "rotated":
                z = torch.randn(M, RT.d_s, generator=g)
                phi = torch.linspace(0.25, 1.25, 8) + 0.05 * e
                amp = 10 * torch.randn(M, 8, generator=g)
                z[:, 0:8] += amp * torch.cos(phi)
                z[:, 8:16] += amp * torch.sin(phi)
                x = z @ self.state.proj_s
            elif kind == "graded":
                tail = torch.logspace(math.log10(0.3), -2, RT.d_s)[torch.randperm(RT.d_s, generator=g)]
                z = torch.randn(M, RT.d_s, generator=g) * tail
                phi = torch.linspace(0.25, 1.25, 8) + 0.05 * e
                amp = torch.logspace(1, 0, 8) * torch.randn(M, 8, generator=g)
                z[:, 0:8] += amp * torch.cos(phi)
                z[:, 8:16] += amp * torch.sin(phi)
                x = z @ self.state.proj_s
            else:
                x = torch.randn(M, RT.d_s, generator=g)
                x[:, 0:8] += 10 * torch.randn(M, 8, generator=g)
                x[:, 32:] *= 2.0 ** -12
            self.students.append(x.view(RT.B, RT.n, RT.d_s).contiguous())
        self.gd = torch.tensor(RT_GD, dtype=torch.float64)
        self.d64, self.g64 = self._autograd(torch.float64)
        d32, g32 = self._autograd(torch.float32)
        self.d32_err = float(((d32.double() - self.d64).abs() / self.d64.abs()).max())
        self.g32_err = max(float((a.double() - b).norm() / b.norm()) for a, b in zip(g32, self.g64))

    def _autograd(self, dtype):
        leaves = [x.to(dtype).clone().requires_grad_(True) for x in self.students]
        cos_range = []
        d = route_distances(self.state.proj_s, self.state.proj_t, leaves, self.teachers, self.ranks, dtype, cos_range)
        if dtype == torch.float64:
            self.cos_range = cos_range                   # (smallest, largest) fp64 cosine per (e, l)
        (d * self.gd.to(dtype)).sum().backward()
        return d.detach(), [x.grad for x in leaves]


@functools.lru_cache(maxsize=None)
def route_case(kind):
    return _RouteCase(kind)


def test_route_fixtures_and_the_fp32_oracle_error():
    """On the CPU, before the library runs: every teacher rank is 8; the angles of the `rotated` case stay away from 0
    and pi / 2; the restated formula in fp32 is the oracle's own ``selector_forward``; and the error of fp32 autograd
    against fp64, four times which is the bound of each route on the GPU, is written down."""
    from oracle import basd_oracle as O
    for kind in ROUTE_KINDS:
        case = route_case(kind)
        assert case.ranks == [RT.k] * RT.L, case.ranks
        keys = list(range(RT.L))
        attn = {k: torch.ones(RT.B, 1, RT.n, RT.n) / RT.n for k in keys}
        state = O.SelectorState(case.state.proj_s, case.state.proj_t, case.state.log_temperatures)
        _, _, trace = O.selector_forward(state, dict(enumerate(case.students)), dict(zip(keys, case.teachers)), attn,
                                         list(range(RT.E)))
        d_oracle = torch.stack([trace.d_grass_sq[e] for e in range(RT.E)]).double()
        assert float(((d_oracle - case.d64).abs() / case.d64).max()) <= max(4 * case.d32_err, 1e-5)
        # no principal angle at 0 (the clamp) or at pi / 2: every fp64 cosine of every (student, teacher) pair
        lo, hi = min(c[0] for c in case.cos_range), max(c[1] for c in case.cos_range)
        assert len(case.cos_range) == RT.E * RT.L and lo > 0.005 and hi < 0.99, (kind, lo, hi)
        x = case.students[0].reshape(-1, RT.d_s).double()
        ev = torch.linalg.eigvalsh((x - x.mean(0)).T @ (x - x.mean(0))).flip(0)
        assert float(ev[RT.k - 1] - ev[RT.k]) > (0.3 * float(ev[0]) if kind != "graded" else 0.8 * float(ev[RT.k - 1])), \
            "no planted gap below the leading 8"
        if kind == "blocks":
            assert float(ev[32]) < 4 * EPS32 * float(ev[0])
        if kind == "graded":                    # lam_k / lam_0 about 1e-2, a tail from 1e-3 lam_0 across sqrt(eps) lam_0
            assert 5e-3 < float(ev[RT.k - 1] / ev[0]) < 2e-2 and float(ev[RT.k] / ev[0]) > 5e-4
            assert float(ev[-1] / ev[0]) < 2e-6 and int((ev < math.sqrt(EPS32) * ev[0]).sum()) > 20
            below_k = float(ev[RT.k - 1] / ev[RT.k])
            assert below_k > 5.0, below_k
        print(f"routes fp32 cpu oracle {kind}: d_grass_sq err {case.d32_err:.2e} student gradient err {case.g32_err:.2e} "
              f"cosines {lo:.4f} ... {hi:.4f} d_grass_sq {[round(float(v), 4) for v in case.d64.ravel()]}")


@gpu
@pytest.mark.parametrize("kind", ROUTE_KINDS)
def test_distance_backward_routes_against_fp64(kind):
    """``GrassmannianLayerSelector._distances`` forward and backward through the full-K2 route (all student
    eigenvectors from Jacobi) and through the leading vectors plus shifted solves, each against fp64 autograd at four
    times the fp32 CPU oracle's error, and against each other at the sum of the two bounds.  Before the full-K2 route
    took its eigenvectors from the rotations of Jacobi on [G ; I] (they were normalised columns of G J, round-off below
    about eps lam_0: |V V^T - I| = 0.66) its student gradient on `blocks` was 146 % off; the solves route was at 5e-6
    then as now.  `graded` has little room (1.35e-5 and 1.07e-5 of 1.65e-5 on an MI355X): both routes start from the fp32
    Gram and pay eps lam_0 / lam_k = 1.4e-5, the fp32 oracle takes the SVD of the tokens and pays eps sigma_0 / sigma_k."""
    from basd_amd import ops
    from basd_amd.losses import GrassmannianLayerSelector
    case = route_case(kind)
    assert case.ranks == [RT.k] * RT.L          # on the CPU, before anything of the library runs
    torch.manual_seed(42)
    sel = GrassmannianLayerSelector(RT.E, RT.d_s, RT.d_t).to(DEV)
    assert torch.equal(sel.proj_s.cpu(), case.state.proj_s) and torch.equal(sel.proj_t.cpu(), case.state.proj_t)
    teachers = ops._check_common_layout([ops.as_supported(t.to(DEV)) for t in case.teachers], "teacher token tensors")
    gd = case.gd.float().to(DEV)
    b_d, b_g = 4 * case.d32_err, 4 * case.g32_err
    results, failures = {}, []
    for route, jacobi in (("k2", True), ("solves", False)):
        sel.small_student_jacobi = jacobi
        calls = []
        inner = sel._eigvec_adjoint_leading
        sel._eigvec_adjoint_leading = lambda sv, gvt: calls.append(1) or inner(sv, gvt)
        leaves = [x.to(DEV).requires_grad_(True) for x in case.students]
        try:
            d = sel._distances(leaves, list(range(RT.L)), teachers)
            (d * gd).sum().backward()
            torch.cuda.synchronize()
        finally:
            del sel._eigvec_adjoint_leading
        assert len(calls) == (0 if jacobi else 1), (route, "took the other route")
        assert [sel.subspace_ranks[k] for k in range(RT.L)] == case.ranks
        d, grads = d.detach().cpu().double(), [x.grad.cpu().double() for x in leaves]
        assert bool(torch.isfinite(d).all()) and all(bool(torch.isfinite(g).all()) for g in grads)
        e_d = float(((d - case.d64).abs() / case.d64.abs()).max())
        e_g = max(float((g - r).norm() / r.norm()) for g, r in zip(grads, case.g64))
        print(f"routes {kind} {route}: d_grass_sq err {e_d:.2e} bound {b_d:.2e}; student gradient err {e_g:.2e} "
              f"bound {b_g:.2e} (fp32 cpu oracle {case.d32_err:.2e} / {case.g32_err:.2e})")
        if e_d > b_d or e_g > b_g:
            failures.append((route, e_d, b_d, e_g, b_g))
        results[route] = (d, grads)
    between = max(float((a - b).norm() / r.norm()) for a, b, r in zip(results["k2"][1], results["solves"][1], case.g64))
    print(f"routes {kind}: the two routes differ by {between:.2e} (allowed {2 * b_g:.2e})")
    if between > 2 * b_g:
        failures.append(("between", between, 2 * b_g))
    assert not failures, failures
