"""The opt-in residual check of the tridiagonal factorisations (``ops.tridiag_probe`` / ``ops.tridiag_check`` /
``ops.tridiagonalise(check=True)`` / ``GrassmannianLayerSelector.check_factorisations``).

For a symmetric A of order n, a factorisation (d, e, tau, vh) and the probe vector x (+-1 from the integer hash of
``include/basd_hip.h``), with eps = 2^-24 and everything accumulated in fp64:

    rho_trace = |sum d - tr A| / (eps |A|_F)
    rho_fro   = |sum d^2 + 2 sum e^2 - |A|_F^2| / (eps |A|_F^2)
    rho_res   = |Q^T (A x) - T (Q^T x)|_2 / (eps |A|_F |x|_2)

The yardstick of the thresholds is fp32 LAPACK ``ssytrd`` with the reflectors applied in fp32 on the CPU (code that
shares nothing with the kernels): the unmarked tests hold it to a QUARTER of every default threshold on the families of
``tests/test_hard_spectra.py`` plus a ``randn`` Gram, and show that four single-entry corruptions exceed the thresholds.
The measured values behind the constants are in ``profiles/tridiag_check.txt``."""
import functools
import math
import os
import re
import sys
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_hard_spectra as H  # noqa: E402  (the matrix families; nothing of it is collected from here)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24

MEASURE_FAMILIES = ("randn",) + H.FAMILIES
GPU_FAMILIES = ("randn", "ones", "diag", "graded", "zero")


# --------------------------------------------------------------------------- #
# numpy restatement (CPU)
# --------------------------------------------------------------------------- #
def header_constants():
    """The numbers of the specification, read from include/basd_hip.h."""
    text = open(os.path.join(ROOT, "include", "basd_hip.h")).read()
    out = {}
    for name in ("BASD_TRIDIAG_PROBE_MUL_M", "BASD_TRIDIAG_PROBE_MUL_I", "BASD_TRIDIAG_PROBE_ADD",
                 "BASD_TRIDIAG_PROBE_MIX_1", "BASD_TRIDIAG_PROBE_MIX_2", "BASD_TRIDIAG_PROBE_ROWS",
                 "BASD_TRIDIAG_VERDICT_INTS"):
        out[name] = int(re.search(rf"#define\s+{name}\s+(0x[0-9A-Fa-f]+|\d+)", text).group(1), 0)
    for name in ("BASD_TRIDIAG_CHECK_TRACE_PER_SQRT_N", "BASD_TRIDIAG_CHECK_FRO_PER_SQRT_N", "BASD_TRIDIAG_CHECK_RES"):
        out[name] = float(re.search(rf"#define\s+{name}\s+([0-9.eE+-]+)", text).group(1))
    return out


def default_thresholds(n):
    c = header_constants()
    r = math.sqrt(n)
    return (c["BASD_TRIDIAG_CHECK_TRACE_PER_SQRT_N"] * r, c["BASD_TRIDIAG_CHECK_FRO_PER_SQRT_N"] * r,
            c["BASD_TRIDIAG_CHECK_RES"])


def probe_vector(m, n):
    """x of matrix index m: the hash of include/basd_hip.h restated in numpy's uint32 arithmetic."""
    c = header_constants()
    with np.errstate(over="ignore"):
        i = np.arange(n, dtype=np.uint32)
        h = np.uint32(m) * np.uint32(c["BASD_TRIDIAG_PROBE_MUL_M"]) + i * np.uint32(c["BASD_TRIDIAG_PROBE_MUL_I"]) \
            + np.uint32(c["BASD_TRIDIAG_PROBE_ADD"])
        h ^= h >> np.uint32(15)
        h *= np.uint32(c["BASD_TRIDIAG_PROBE_MIX_1"])
        h ^= h >> np.uint32(12)
        h *= np.uint32(c["BASD_TRIDIAG_PROBE_MIX_2"])
        h ^= h >> np.uint32(15)
    return np.where(h >> np.uint32(31), -1.0, 1.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def matrix(name, n):
    """fp32 (n, n) numpy matrix of a family; never modified."""
    if name == "randn":
        g = torch.Generator().manual_seed(1000 + n)
        x = torch.randn(3 * n + 5, n, generator=g, dtype=torch.float64)
        G = H._round(x.T @ x)
    else:
        G = H.family(name, n)[0]
    a = G.numpy().copy()
    a.setflags(write=False)
    return a


def lapack_factor(a):
    """fp32 LAPACK ssytrd (lower) in this library's layout: d, e, tau (n,) and vh (n, n) whose row j is reflector j
    (1 at j + 1, zeros before), A = Q T Q^T with Q = H_0 H_1 ... H_{n-2}, H_j = I - tau_j v_j v_j^T."""
    from scipy.linalg import lapack
    n = a.shape[0]
    d, e, tau = (np.zeros(n, np.float32) for _ in range(3))
    vh = np.zeros((n, n), np.float32)
    if n == 1:
        d[0] = a[0, 0]
        return d, e, tau, vh
    c, dd, ee, tt, info = lapack.ssytrd(np.asfortranarray(a), lower=1)
    assert info == 0
    d[:], e[:n - 1], tau[:n - 1] = dd, ee, tt
    for j in range(n - 1):
        vh[j, j + 1] = 1.0
        vh[j, j + 2:] = c[j + 2:, j]
    return d, e, tau, vh


def apply_qt(tau, vh, x, dtype=np.float32):
    """Q^T x = H_{n-2} ... H_0 x in fp32 (``dtype`` fp64: the fp32 reflectors applied without further rounding, the
    result rounded to fp32 once -- what tools/tridiag_check_host_check.cpp does)."""
    x, tau, vh = x.astype(dtype), tau.astype(dtype), vh.astype(dtype)
    for j in range(len(tau) - 1):
        if tau[j] != 0:
            v = vh[j]
            x -= dtype(tau[j] * np.dot(v, x)) * v
    return x.astype(np.float32)


def ratio(num, den):
    if num == 0.0 and den == 0.0:
        return 0.0
    with np.errstate(all="ignore"):
        return float(np.float64(num) / np.float64(den))


def ratios(a, d, e, tau, vh, m, q_dtype=np.float32):
    """The three ratios of matrix index m, as the kernels define them."""
    n = a.shape[0]
    a64 = a.astype(np.float64)
    x = probe_vector(m, n)
    y = (a64 @ x.astype(np.float64)).astype(np.float32)            # accumulated in fp64, rounded once
    tr, fro2 = float(np.trace(a64)), float((a64 * a64).sum())
    fro = math.sqrt(fro2) if fro2 >= 0 else float("nan")
    u, v = (apply_qt(tau, vh, t, q_dtype).astype(np.float64) for t in (x, y))
    d64, e64 = d.astype(np.float64), e[:n - 1].astype(np.float64)
    tu = d64 * u
    tu[:-1] += e64 * u[1:]
    tu[1:] += e64 * u[:-1]
    res = math.sqrt(float(((v - tu) ** 2).sum()))
    return (ratio(abs(float(d64.sum()) - tr), EPS * fro),
            ratio(abs(float((d64 * d64).sum() + 2 * (e64 * e64).sum()) - fro2), EPS * fro2),
            ratio(res, EPS * fro * math.sqrt(n)))


def failed_bits(r, thr):
    return sum(1 << k for k in range(3) if not r[k] <= thr[k])


# --------------------------------------------------------------------------- #
# unmarked: the yardstick and the corruptions (CPU)
# --------------------------------------------------------------------------- #
@functools.lru_cache(maxsize=None)
def lapack_case(name, n):
    """(a, d, e, tau, vh) of fp32 LAPACK; computed once, never modified."""
    a = matrix(name, n)
    out = (a,) + lapack_factor(a)
    for t in out[1:]:
        t.setflags(write=False)
    return out


def test_probe_vector_is_the_headers_hash():
    """The numpy restatement against an independent evaluation of the header's formula in Python integers, and the
    vector is not degenerate: both signs, different matrices differ."""
    c = header_constants()
    assert c["BASD_TRIDIAG_PROBE_ROWS"] == 16 and c["BASD_TRIDIAG_VERDICT_INTS"] == 8
    mask = 0xFFFFFFFF
    for m in (0, 1, 2, 27, 65534):
        want = []
        for i in range(1024):
            h = (m * c["BASD_TRIDIAG_PROBE_MUL_M"] + i * c["BASD_TRIDIAG_PROBE_MUL_I"] + c["BASD_TRIDIAG_PROBE_ADD"]) & mask
            h ^= h >> 15
            h = (h * c["BASD_TRIDIAG_PROBE_MIX_1"]) & mask
            h ^= h >> 12
            h = (h * c["BASD_TRIDIAG_PROBE_MIX_2"]) & mask
            h ^= h >> 15
            want.append(-1.0 if h >> 31 else 1.0)
        got = probe_vector(m, 1024)
        assert got.tolist() == want
        assert 400 < int((got > 0).sum()) < 624
    assert (probe_vector(0, 64) != probe_vector(1, 64)).any()


@pytest.mark.parametrize("n", [45, 200])
def test_lapack_stays_under_a_quarter_of_the_thresholds(n):
    thr = default_thresholds(n)
    for name in MEASURE_FAMILIES:
        a, d, e, tau, vh = lapack_case(name, n)
        r = ratios(a, d, e, tau, vh, 0)
        print(f"lapack {name} n={n}: rho_trace {r[0]:.3f} rho_fro {r[1]:.3f} rho_res {r[2]:.3f} (thresholds "
              f"{thr[0]:.1f} {thr[1]:.1f} {thr[2]:.1f})")
        for k in range(3):
            assert r[k] <= thr[k] / 4, (name, n, k, r, thr)


def test_zero_matrix_and_small_orders():
    for n in (1, 2, 45):
        a = np.zeros((n, n), np.float32)
        assert ratios(a, *lapack_factor(a), 3) == (0.0, 0.0, 0.0)
    for n in (1, 2):                                     # no reflector
        a = np.array([[3.0, -1.0], [-1.0, 0.5]], np.float32)[:n, :n]
        r = ratios(a, *lapack_factor(a), 1)
        assert max(r) <= 1.0, r


@pytest.mark.parametrize("n", [45, 200])
def test_single_entry_corruptions_exceed_the_thresholds(n):
    """One d or one e entry moved by 1e-3 max|d| on every family that has a scale; one tau or one vh entry of an
    active reflector moved by 1e-2 on the randn Gram."""
    thr = default_thresholds(n)
    i = n // 2
    for name in MEASURE_FAMILIES:
        a, d, e, tau, vh = lapack_case(name, n)
        delta = np.float32(1e-3) * np.abs(d).max()
        if delta == 0:                                   # `zero`: nothing to move an entry by
            continue
        d2 = d.copy()
        d2[i] += delta
        r = ratios(a, d2, e, tau, vh, 0)
        assert failed_bits(r, thr) & 1, (name, n, "d", r, thr)
        e2 = e.copy()
        e2[i] += delta
        r = ratios(a, d, e2, tau, vh, 0)
        assert failed_bits(r, thr) & 6, (name, n, "e", r, thr)
    a, d, e, tau, vh = lapack_case("randn", n)
    j = n // 3
    assert tau[j] != 0
    tau2 = tau.copy()
    tau2[j] += np.float32(1e-2)
    r = ratios(a, d, e, tau2, vh, 0)
    assert failed_bits(r, thr) & 4, ("tau", n, r, thr)
    vh2 = vh.copy()
    vh2[j, j + 3] += np.float32(1e-2)
    r = ratios(a, d, e, tau, vh2, 0)
    assert failed_bits(r, thr) & 4, ("vh", n, r, thr)
    nan = d.copy()
    nan[0] = np.nan
    assert failed_bits(ratios(a, nan, e, tau, vh, 0), thr) == 7


# --------------------------------------------------------------------------- #
# unmarked: csrc/tridiag_check_core.h on the host, under the sanitizers
# --------------------------------------------------------------------------- #
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    import shutil
    import subprocess
    source = os.path.join(ROOT, "tools", "tridiag_check_host_check.cpp")
    out = str(tmp_path_factory.mktemp("tridiag_check_host") / "tridiag_check_host_check")
    compilers = [c for c in (os.environ.get("CXX"), "g++", "clang++", "c++") if c and shutil.which(c)]
    if not compilers:
        pytest.skip("no host C++ compiler found")
    # first a toolchain that builds AND runs a trivial program under the sanitizers (their runtimes linked statically
    # where the compiler can: the program then stands alone); only its absence skips.  Then the source under test with
    # exactly that toolchain: any error there fails.
    trivial = tmp_path_factory.mktemp("tridiag_check_probe") / "trivial.cpp"
    trivial.write_text("#include <vector>\nint main() { std::vector<int> v(3, 1); return v[0] + v[2] - 2; }\n")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-ffp-contract=off", "-fno-sanitize-recover=all"]
    toolchain = None
    for cxx in compilers:
        for static in (["-static-libasan", "-static-libubsan"], ["-static-libsan"], []):
            exe = str(trivial) + ".bin"
            done = subprocess.run([cxx, *flags, *static, "-o", exe, str(trivial)], capture_output=True, text=True)
            if done.returncode == 0 and subprocess.run([exe], capture_output=True).returncode == 0:
                toolchain = [cxx, *flags, *static]
                break
        if toolchain:
            break
    if toolchain is None:
        pytest.skip("no host compiler with the sanitizer runtimes found")
    done = subprocess.run([*toolchain, "-o", out, source], capture_output=True, text=True)
    assert done.returncode == 0, "the sanitizer build of tools/tridiag_check_host_check.cpp failed:\n" + done.stderr[-3000:]
    return out


def _run_host(program, cases, tmp_path, name, thresholds=None):
    """cases: list of (a, d, e, tau, vh) of one order -> (sums (b, 2), ratios (b, 3), bits (b,), rows (b, 2, n))."""
    import subprocess
    n, b = cases[0][0].shape[0], len(cases)
    src, dst = str(tmp_path / f"{name}.in"), str(tmp_path / f"{name}.out")
    with open(src, "wb") as f:
        f.write(np.array([0x54434B31, n, b, int(thresholds is not None)], dtype="<i8").tobytes())
        f.write(np.array(thresholds if thresholds is not None else (0, 0, 0), dtype="<f4").tobytes())
        for case in cases:
            for t in case:
                f.write(np.ascontiguousarray(t, dtype="<f4").tobytes())
    done = subprocess.run([program, src, dst], capture_output=True, text=True)
    assert done.returncode == 0 and not done.stderr, (name, done.returncode, done.stderr[-2000:])
    raw = np.fromfile(dst, dtype=np.uint8)
    assert raw.size == b * 48 + b * 2 * n * 4
    rec = raw[:b * 48].reshape(b, 48)
    sums = rec[:, :16].copy().view("<f8")
    rho = rec[:, 16:40].copy().view("<f8")
    bits = rec[:, 40:44].copy().view("<i4")[:, 0]
    return sums, rho, bits, raw[b * 48:].copy().view("<f4").reshape(b, 2, n)


@pytest.mark.parametrize("n", [1, 2, 45, 200])
def test_host_build_under_the_sanitizers(host_check, tmp_path, n):
    """The functions the kernels call, compiled for the host: the same ratios as the numpy restatement (fp64 sums in
    another order: 1e-9 relative and 1e-6 absolute of ratios of order 1), the same verdict bits, the same probe rows."""
    if n <= 2:
        mats = [np.array([[3.0, -1.0], [-1.0, 0.5]], np.float32)[:n, :n], np.zeros((n, n), np.float32)]
        cases = [(a,) + lapack_factor(a) for a in mats]
    else:
        cases = [lapack_case(f, n) for f in ("randn", "ones", "graded", "zero")]
        a, d, e, tau, vh = lapack_case("randn", n)
        d2 = d.copy()
        d2[n // 2] += np.float32(1e-3) * np.abs(d).max()
        tau2 = tau.copy()
        tau2[n // 3] += np.float32(1e-2)
        nan = a.copy()
        nan[3, 5] = nan[5, 3] = np.nan
        cases += [(a, d2, e, tau, vh), (a, d, e, tau2, vh), (nan, d, e, tau, vh)]
    sums, rho, bits, rows = _run_host(host_check, cases, tmp_path, f"n{n}")
    thr = default_thresholds(n)
    for m, (a, d, e, tau, vh) in enumerate(cases):
        want = ratios(a, d, e, tau, vh, m, q_dtype=np.float64)
        a64 = a.astype(np.float64)
        assert rows[m, 0].tolist() == probe_vector(m, n).tolist()
        if np.isfinite(a).all():
            np.testing.assert_allclose(sums[m], [np.trace(a64), (a64 * a64).sum()], rtol=1e-12)
            np.testing.assert_allclose(rho[m], want, rtol=1e-9, atol=1e-6)
        else:
            assert np.isnan(rho[m]).all()
        assert int(bits[m]) == failed_bits(want, thr), (m, rho[m], want)
    if n > 2:
        assert bits.tolist()[:4] == [0, 0, 0, 0] and bits[4] & 1 and bits[5] == 4 and bits[6] == 7
        assert rho[3].tolist() == [0.0, 0.0, 0.0]
    loose = _run_host(host_check, cases, tmp_path, f"n{n}_loose", thresholds=(1e30, 1e30, 1e30))[2]
    assert all(int(b) in (0, 7) for b in loose)          # only a NaN still fails


# --------------------------------------------------------------------------- #
# gpu: the two kernels
# --------------------------------------------------------------------------- #
def gpu_matrix(name, n):
    if n < 10 and name in ("diag", "randn"):
        if name == "diag":
            return np.diag(np.array([5.0, 2.0], np.float32)[:n])
        x = np.random.default_rng(n).standard_normal((5, n))
        return (x.T @ x).astype(np.float32)
    return matrix(name, n)


def hand_state(G):
    """Order 1: there is nothing to factor (and basd_tridiag takes no such call): T = A, no reflector."""
    from basd_amd import ops
    b, n = G.shape[0], G.shape[1]
    assert n == 1
    z = torch.zeros((b, n), device=G.device)
    return ops.TridiagState(G.reshape(b, n).clone(), z, z.clone(), torch.zeros_like(G), z.clone())


def read(verdict):
    torch.cuda.synchronize()
    return verdict.read()


@gpu
@pytest.mark.parametrize("n", [1, 2, 45, 200, 320, 384, 448])
def test_orders_and_routes(n):
    """Batches of 3 over randn Gram, ones, diag, graded and zero: orders 1 and 2 (no reflector), 45 and 200 (one CU), 320
    and 384 (packed), 448 (shared stage + tail, default tuning).  No matrix fails, every ratio is under its threshold,
    the zero matrix gives 0 / 0 / 0."""
    from basd_amd import ops
    thr = default_thresholds(n)
    for names in (("randn", "ones", "diag"), ("graded", "zero", "randn")):
        G = torch.from_numpy(np.stack([gpu_matrix(f, n) for f in names])).to(DEV)
        if n == 1:
            verdict = ops.tridiag_check(hand_state(G), ops.tridiag_probe(G))
        else:
            ts = ops.tridiagonalise(G.clone(), check=True)
            verdict = ts.check
            assert int(ts.err[0].item()) == 0
        got = read(verdict)
        for f, r in zip(names, got["ratios"].tolist()):
            print(f"gpu {f} n={n}: rho_trace {r[0]:.3f} rho_fro {r[1]:.3f} rho_res {r[2]:.3f} (thresholds "
                  f"{thr[0]:.1f} {thr[1]:.1f} {thr[2]:.1f})")
        assert (got["failed"], got["first"], got["bits"], got["checked"]) == (0, -1, 0, 3), got
        ratios_ = got["ratios"].numpy()
        assert (ratios_ <= np.array(thr, np.float32)).all(), (names, ratios_, thr)
        assert got["worst"] == ratios_.max(axis=0).tolist()
        assert ratios_[names.index("zero")].tolist() == [0.0, 0.0, 0.0] if "zero" in names else True


@gpu
@pytest.mark.parametrize("n,ranked", [(200, False), (384, True), (448, False), (448, True)])
def test_the_check_changes_nothing(n, ranked):
    """d, e, tau, vh and the ranks of ``tridiagonalise(..., check=True)`` equal ``check=False`` bit for bit."""
    from basd_amd import ops
    G = torch.from_numpy(np.stack([gpu_matrix(f, n) for f in ("randn", "ones", "graded")])).to(DEV)
    out = []
    for check in (False, True, False):
        pin = torch.empty((2 + 8,), dtype=torch.int32, pin_memory=True)
        ts = ops.tridiagonalise(G.clone(), mp_rank=(32 * n, n, n - 1, 2, pin) if ranked else None, check=check)
        torch.cuda.synchronize()
        assert (ts.check is not None) == check
        out.append((ts.d, ts.e[:, :n - 1], ts.tau[:, :n - 1], ts.vh[:, :n - 1], ts.err,
                    ts.ranks if ranked else ts.err, pin if ranked else ts.err))
    for got in out[1:]:
        for a, b in zip(out[0], got):
            assert torch.equal(a.cpu(), b.cpu())


@gpu
@pytest.mark.parametrize("n,pad", [(1, 0), (3, 0), (45, 0), (200, 0), (200, 1), (200, 4), (1024, 0)])
def test_probe_kernel(n, pad):
    """tr A and |A|_F^2 to 1e-12 relative and y to one fp32 rounding of the fp64 numpy values (plus the fp64 summation
    error n 2^-52 sum_j |a_ij|), x = the hash; a second call leaves the same bits; guard bytes around the buffer are
    untouched.  45 and pad 1: single loads; 200 and 1024: 16-byte loads (1024: all four groups per lane)."""
    from basd_amd import _lib, ops
    b = 3
    g = torch.Generator().manual_seed(n)
    x = torch.randn(b, n + 3, n, generator=g)
    A = torch.zeros(b, n * n + pad)
    A[:, :n * n] = (x.transpose(1, 2) @ x).reshape(b, n * n)
    A_dev = A.to(DEV)
    size = _lib.query("basd_tridiag_probe_bytes", n, b)
    bufs = []
    for _ in range(2):
        raw = torch.full((size + 64,), 0xA5, dtype=torch.uint8, device=DEV)
        _lib.call("basd_tridiag_probe", A_dev.data_ptr(), n * n + pad, n, b, raw[32:].data_ptr(), ops._stream())
        torch.cuda.synchronize()
        assert (raw[:32] == 0xA5).all() and (raw[32 + size:] == 0xA5).all()
        bufs.append(raw[32:32 + size].clone())
    assert torch.equal(bufs[0], bufs[1])
    probe = ops.TridiagProbe(bufs[0], n, b)
    rows, parts = probe.rows.cpu().numpy(), probe.parts.cpu().numpy()
    assert parts.shape == (b, -(-n // 16), 2)
    a64 = A[:, :n * n].reshape(b, n, n).numpy().astype(np.float64)
    for m in range(b):
        xm = probe_vector(m, n)
        assert rows[m, 0].tolist() == xm.tolist()
        y64 = a64[m] @ xm.astype(np.float64)
        slack = 0.5 * np.spacing(np.abs(y64).astype(np.float32)).astype(np.float64) \
            + n * 2.0 ** -52 * np.abs(a64[m]).sum(axis=1)
        assert (np.abs(rows[m, 1].astype(np.float64) - y64) <= slack).all()
        np.testing.assert_allclose(parts[m].sum(axis=0), [np.trace(a64[m]), (a64[m] ** 2).sum()], rtol=1e-12)
    if pad == 0:              # the public wrapper leaves the same bits (`sums` is basd_tridiag_check's to fill)
        again = ops.tridiag_probe(A_dev.view(b, n, n))
        torch.cuda.synchronize()
        assert torch.equal(again.rows, probe.rows) and torch.equal(again.parts, probe.parts)


@gpu
@pytest.mark.parametrize("n", [45, 448])
def test_corruptions_are_flagged(n):
    """A clone of a good state with one entry of d, e, tau or vh moved in matrix 1 of 3: only matrix 1 is flagged, with the
    expected bit, the pinned mirror equals the device verdict, and the same probe serves check after check.  A NaN in A
    (probe of the damaged matrix against the good factorisation) is flagged with every bit."""
    from basd_amd import ops
    thr = np.array(default_thresholds(n), np.float32)
    G = torch.from_numpy(np.stack([matrix("randn", n + k) [:n, :n] for k in range(3)])).to(DEV)
    probe = ops.tridiag_probe(G)
    ts = ops.tridiagonalise(G.clone())
    torch.cuda.synchronize()
    assert int(ts.err[0].item()) == 0
    j, i = n // 3, n // 2
    assert float(ts.tau[1, j]) != 0.0
    delta = 1e-3 * float(ts.d[1].abs().max())

    def variant(field):
        parts = {k: getattr(ts, k).clone() for k in ("d", "e", "tau", "vh")}
        if field == "d":
            parts["d"][1, i] += delta
        elif field == "e":
            parts["e"][1, i] += delta
        elif field == "tau":
            parts["tau"][1, j] += 1e-2
        elif field == "vh":
            parts["vh"][1, j, j + 3] += 1e-2
        return ops.TridiagState(parts["d"], parts["e"], parts["tau"], parts["vh"], ts.vals)

    for field, must, may in (("none", 0, 0), ("d", 1, 7), ("e", 0, 6), ("tau", 4, 4), ("vh", 4, 4), ("none", 0, 0)):
        pin = torch.full((8,), -7, dtype=torch.int32).pin_memory()
        verdict = ops.tridiag_check(variant(field), probe, host_mirror=pin)
        got = read(verdict)
        print(f"gpu n={n} corrupt {field}: verdict {verdict.verdict.tolist()[:4]} ratios {got['ratios'].tolist()}")
        assert pin.tolist() == verdict.verdict.cpu().tolist()
        over = (~(got["ratios"].numpy() <= thr)).any(axis=1).tolist()
        if field == "none":
            assert (got["failed"], got["first"], got["bits"], got["checked"]) == (0, -1, 0, 3) and not any(over)
            continue
        assert (got["failed"], got["first"], got["checked"]) == (1, 1, 3), (field, got)
        assert over == [False, True, False]
        assert got["bits"] & must == must and got["bits"] & ~may == 0 and got["bits"], (field, got)
    bad = G.clone()
    bad[1, 3, 5] = bad[1, 5, 3] = float("nan")
    got = read(ops.tridiag_check(ts, ops.tridiag_probe(bad)))
    assert (got["failed"], got["first"], got["bits"], got["checked"]) == (1, 1, 7, 3)
    assert all(math.isnan(w) for w in got["worst"])
    tight = read(ops.tridiag_check(ts, probe, thresholds=(0.0, 0.0, 0.0)))          # caller's limits are used
    assert tight["failed"] == 3 and tight["first"] == 0


@gpu
def test_three_more_launches_per_checked_factorisation():
    """Counted with ``torch.profiler``: exactly three more kernels per checked ``tridiagonalise`` -- the probe, the
    existing ``backtransform_kernel`` (``basd_tridiag_apply_q``) and the check -- and none of the two new ones with the
    check off.  No memset and no copy beyond the factorisation's own."""
    from basd_amd import ops
    from torch.profiler import ProfilerActivity, profile
    n = 200
    G = torch.from_numpy(np.stack([matrix("randn", n)] * 3)).to(DEV)
    counts, copies_and_memsets = {}, {}
    for check in (False, True):
        ops.tridiagonalise(G.clone(), check=check)
        torch.cuda.synchronize()
        copies = [G.clone() for _ in range(5)]
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for c in copies:
                ops.tridiagonalise(c, check=check)
            torch.cuda.synchronize()
        device_events = [e for e in prof.events() if "cuda" in str(e.device_type).lower()]
        host_names = {e.name for e in prof.events() if "cuda" not in str(e.device_type).lower()}
        others = [e.name for e in device_events if "memcpy" in e.name.lower() or "memset" in e.name.lower()]
        kernels = [e.name for e in device_events if e.name not in host_names and e.name not in others]
        counts[check], copies_and_memsets[check] = kernels, others
    # (the factorisation clears its own status words with a memset; the check adds neither a memset nor a copy)
    assert len(copies_and_memsets[True]) == len(copies_and_memsets[False]), copies_and_memsets
    ours = [k for k in counts[True] if "tridiag_probe_kernel" in k or "tridiag_check_kernel" in k]
    assert len(counts[False]) >= 5, ("the profiler saw no factorisation launch", sorted(set(counts[False])))
    print(f"[tridiag_check] profiler, 5 factorisations: {len(counts[False])} kernels off, {len(counts[True])} on")
    assert not any("tridiag_probe_kernel" in k or "tridiag_check_kernel" in k for k in counts[False])
    assert len(counts[True]) == len(counts[False]) + 3 * 5, (sorted(set(counts[True])), sorted(set(counts[False])))
    assert len(ours) == 2 * 5 and sum("backtransform_kernel" in k for k in counts[True]) == 5


# --------------------------------------------------------------------------- #
# the selector and the loss
# --------------------------------------------------------------------------- #
def test_switch_defaults_and_error_type(monkeypatch):
    """Off by default; BASD_TRIDIAG_CHECK is read when a selector is constructed, like its neighbouring switches."""
    from basd_amd.losses import GrassmannianLayerSelector, TridiagCheckFailed, TridiagGiveUp
    monkeypatch.delenv("BASD_TRIDIAG_CHECK", raising=False)
    sel = GrassmannianLayerSelector(2, 16, 24)
    assert sel.check_factorisations is False and sel.last_check is None
    monkeypatch.setenv("BASD_TRIDIAG_CHECK", "1")
    assert GrassmannianLayerSelector(2, 16, 24).check_factorisations is True and sel.check_factorisations is False
    monkeypatch.setenv("BASD_TRIDIAG_CHECK", "0")
    assert GrassmannianLayerSelector(2, 16, 24).check_factorisations is False
    err = TridiagCheckFailed("teacher", 4, (1.0, 2.0, 300.0), 4, 1, 6)
    assert isinstance(err, TridiagGiveUp) and err.matrix == 4 and err.ratios == (1.0, 2.0, 300.0) and err.bits == 4
    assert "rho_res" in str(err) and "matrix 4" in str(err)


# d_s = 64, three teacher layers, two student layers.  d_t = 96 <= 1.5 d_s: with a backward the teacher side is factored
# alone (rank-one route of the ranks; the students go through Jacobi), without one teacher and student Grams share a launch
MULTI = None
SINGLE = None


def _shapes():
    from basd_amd import synth
    global MULTI, SINGLE
    if MULTI is None:
        MULTI = synth.LossShape("check multi", 8, 49, 64, 12, 49, 96, 3, 4, True, 20, points=2, r_s=6, r_t=0)
        SINGLE = synth.LossShape("check single", 8, 49, 64, 12, 49, 160, 1, 1, False, 20, points=2, r_s=6, r_t=8)
    return MULTI, SINGLE


def _module(shape, check, chain=True):
    from basd_amd.losses import BASDLoss
    torch.manual_seed(42)
    mod = BASDLoss(torch.nn.CrossEntropyLoss(label_smoothing=0.01), shape.d_s, shape.d_t, shape.depth, shape.n_s,
                   config=SimpleNamespace(num_extraction_points=shape.points),
                   teacher_has_cls_token=shape.has_cls).to(DEV)
    mod.layer_selector.check_factorisations = check
    mod.use_chain = chain
    return mod


def _step(mod, shape, grad, seed=5):
    from basd_amd import synth
    inp = synth.make_inputs(shape, seed, device=DEV, strided=True)
    sel = mod.layer_selector
    if grad:
        leaves = {k: v.detach().clone().requires_grad_(True) for k, v in inp.student.items()}
        loss = mod(inp.logits, inp.targets, leaves, inp.teacher, inp.attn)
        loss.backward()
    else:
        leaves = None
        with torch.no_grad():
            loss = mod(inp.logits, inp.targets, inp.student, inp.teacher, inp.attn)
    sel.finish_pending()
    torch.cuda.synchronize()
    out = dict(loss=loss.detach().cpu(), d=mod.last_components["d_grass_sq"].cpu(),
               mix=mod.last_components["mix"].cpu(), ranks=dict(sel.subspace_ranks))
    if grad:
        out.update({f"grad{l}": leaves[l].grad.cpu() for l in mod.token_layers})
    return out


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]) if isinstance(a[k], torch.Tensor) else a[k] == b[k], k


@pytest.fixture
def restore_tuning():
    from basd_amd import _lib
    yield
    _lib.call("basd_tridiag_tuning", -1, -1, -1, -1, -1, 1)


@gpu
@pytest.mark.parametrize("grad", [True, False], ids=["grad", "nograd"])
def test_selector_with_the_switch_on_equals_off(grad):
    """Distances, mixing weights, loss, ranks and student gradients bit for bit; ``last_components["tridiag_check"]``
    holds the step's worst ratios (under the thresholds of order 64) and the number of matrices checked."""
    multi, _ = _shapes()
    off = _step(_module(multi, False), multi, grad)
    mod = _module(multi, True)
    on = _step(mod, multi, grad)
    _same(off, on)
    info = mod.last_components["tridiag_check"]
    print(f"selector check, grad={grad}: {info}")
    assert info["checked"] == (3 if grad else 5)
    assert all(0.0 < w <= t for w, t in zip(info["worst"], default_thresholds(64)))
    assert "tridiag_check" not in _module(multi, False).last_components


@gpu
def test_selector_single_teacher_step_takes_the_kernel_by_kernel_layout():
    """One teacher layer with the switch on: the step of ``BASD_SELECTOR_CHAIN=0``, bit for bit, checked."""
    _, single = _shapes()
    legacy = _step(_module(single, False, chain=False), single, True)
    mod = _module(single, True)
    on = _step(mod, single, True)
    _same(legacy, on)
    assert not mod._chain_plans
    info = mod.last_components["tridiag_check"]
    print(f"selector check, single teacher: {info}")
    assert info["checked"] >= 2 and all(w <= t for w, t in zip(info["worst"], default_thresholds(64)))
    chained = _module(single, False)
    _step(chained, single, True)
    assert chained._chain_plans                          # (the shape does take the chain call when the switch is off)


def _perturbing(monkeypatch, every_call, side=None):
    """``ops.tridiagonalise`` wrapped: the first (or every) checked call returns a d with one entry of matrix 0 moved by
    1e-3 max|d|, and the verdict of THAT state.  ``side``: only calls of the "teacher" (``mp_rank=`` given) or the
    "student" side (not given) of the kernel-by-kernel layout of a single-teacher step count."""
    from basd_amd import ops
    real, calls = ops.tridiagonalise, []

    def wrapped(G, mp_rank=None, check=False):
        other_side = side is not None and (side == "teacher") != (mp_rank is not None)
        if check is False or other_side or (calls and not every_call):
            return real(G, mp_rank=mp_rank, check=check)
        calls.append(1)
        probe = ops.tridiag_probe(G)
        ts = real(G, mp_rank=mp_rank)
        ts.d[0, 5] += 1e-3 * ts.d[0].abs().max()
        ts.check = ops.tridiag_check(ts, probe, host_mirror=check if isinstance(check, torch.Tensor) else None)
        return ts
    monkeypatch.setattr(ops, "tridiagonalise", wrapped)
    return calls


@gpu
def test_selector_redoes_a_step_whose_check_failed(monkeypatch, restore_tuning):
    multi, _ = _shapes()
    clean = _step(_module(multi, False), multi, True)
    calls = _perturbing(monkeypatch, every_call=False)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        redone = _step(_module(multi, True), multi, True)
    ours = [w for w in seen if "residual check" in str(w.message)]
    assert len(calls) == 1 and len(ours) == 1 and issubclass(ours[0].category, RuntimeWarning), [str(w.message) for w in seen]
    assert "rho_trace" in str(ours[0].message)
    _same(clean, redone)


@gpu
def test_selector_raises_when_the_redone_step_fails_too(monkeypatch, restore_tuning):
    from basd_amd.losses import TridiagCheckFailed
    multi, _ = _shapes()
    calls = _perturbing(monkeypatch, every_call=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(TridiagCheckFailed) as info:
            _step(_module(multi, True), multi, True)
    assert len(calls) == 2 and info.value.matrix == 0 and info.value.bits & 1
    assert info.value.ratios[0] > default_thresholds(64)[0]
    torch.cuda.synchronize()


@gpu
def test_marchenko_pastur_rank_follows_the_switch(monkeypatch):
    """``marchenko_pastur_rank`` (and with it ``capture.estimate_intrinsic_dim``): the same rank with the check on, and
    ``TridiagCheckFailed`` when the factorisation it is handed is off."""
    from basd_amd import losses
    g = torch.Generator().manual_seed(3)
    feats = torch.randn(512, 96, generator=g)
    feats[:, :7] += 6 * torch.randn(512, 7, generator=g)
    feats = feats.to(DEV)
    off = losses.marchenko_pastur_rank(feats)
    monkeypatch.setenv("BASD_TRIDIAG_CHECK", "1")
    with warnings.catch_warnings():
        warnings.simplefilter("error")                   # order 96 IS checked: nothing to warn about
        assert losses.marchenko_pastur_rank(feats) == off and 1 <= off < 96
    calls = _perturbing(monkeypatch, every_call=True)
    with pytest.raises(losses.TridiagCheckFailed) as info:
        losses.marchenko_pastur_rank(feats)
    assert len(calls) == 1 and info.value.matrix == 0 and info.value.bits & 1


@gpu
def test_marchenko_pastur_rank_says_when_it_is_not_checked(monkeypatch):
    """Switch on, but an eigen-solve the check does not cover (the Jacobi solver): the rank as ever, and one warning per
    process saying that nothing was checked."""
    from basd_amd import losses, ops
    g = torch.Generator().manual_seed(4)
    feats = torch.randn(256, 48, generator=g).to(DEV)
    monkeypatch.setattr(ops, "EIG_SOLVER", "jacobi")
    want = losses.marchenko_pastur_rank(feats)
    monkeypatch.setenv("BASD_TRIDIAG_CHECK", "1")
    monkeypatch.setattr(losses, "_UNCHECKED_WARNED", False)
    with pytest.warns(RuntimeWarning, match="NOT checked"):
        assert losses.marchenko_pastur_rank(feats) == want
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert losses.marchenko_pastur_rank(feats) == want


def _forward(mod, shape, seed=5):
    """One forward WITHOUT ``finish_pending``: what a training loop does between steps."""
    from basd_amd import synth
    inp = synth.make_inputs(shape, seed, device=DEV, strided=True)
    with torch.no_grad():
        return mod(inp.logits, inp.targets, inp.student, inp.teacher, inp.attn).detach().cpu()


@gpu
def test_deferred_student_verdict_is_read_by_finish_pending(monkeypatch, restore_tuning):
    """Single-teacher step: nothing waits for the student side, so its verdict is read late.  A perturbed student
    factorisation warns (nothing to redo) when ``finish_pending`` reads it, and the verdict is read exactly once."""
    _, single = _shapes()
    calls = _perturbing(monkeypatch, every_call=False, side="student")
    mod = _module(single, True)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        _forward(mod, single)
        assert mod.layer_selector._pending_checks and not [w for w in seen if "residual check" in str(w.message)]
        mod.layer_selector.finish_pending()
    ours = [str(w.message) for w in seen if "residual check" in str(w.message)]
    assert len(calls) == 1 and len(ours) == 1 and "previous step" in ours[0], ours
    info = mod.layer_selector.last_check
    assert info["late"] == info["checked"] == 2 and info["worst"][0] > default_thresholds(64)[0]
    assert not mod.layer_selector._pending_checks
    torch.cuda.synchronize()


@gpu
def test_late_failure_does_not_hide_a_failure_of_this_step(monkeypatch, restore_tuning):
    """One read-back with a failing LATE verdict (previous step's student side) and a failing CURRENT one (this step's
    teacher side): the late one warns, the current one is still raised -- here through ``_read_ranks`` directly, with the
    entries a step leaves -- and in a real second step the teacher failure is redone and matches the clean step."""
    from basd_amd.losses import TridiagCheckFailed
    _, single = _shapes()
    clean_mod = _module(single, False, chain=False)
    clean = _forward(clean_mod, single)
    clean_mod.layer_selector.finish_pending()
    mod = _module(single, True)
    sel = mod.layer_selector
    calls = _perturbing(monkeypatch, every_call=True, side="student")
    _forward(mod, single)                                # leaves a failing deferred student verdict
    late = list(sel._pending_checks)
    assert len(calls) == 1 and len(late) == 1
    monkeypatch.undo()
    # (a) both in ONE read: a current entry made from a perturbed teacher-side factorisation
    calls = _perturbing(monkeypatch, every_call=True)
    from basd_amd import ops
    G = torch.from_numpy(np.stack([matrix("randn", 64), matrix("ones", 64)])).to(DEV)
    pin = torch.empty((8,), dtype=torch.int32).pin_memory()
    ts = ops.tridiagonalise(G, check=pin)
    ev = torch.cuda.Event()
    ev.record()
    st = dict(checks=[dict(verdict=ts.check, event=ev, where="teacher", deferred=False)])
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        with pytest.raises(TridiagCheckFailed) as info:
            sel._read_checks(st)
    assert info.value.matrix == 0 and info.value.bits & 1
    assert len([w for w in seen if "previous step" in str(w.message)]) == 1
    assert sel.last_check["late"] == 2 and sel.last_check["checked"] == 4
    monkeypatch.undo()
    # (b) a real second step whose teacher factorisation fails once: redone, equal to the clean step
    sel._pending_checks = late
    calls = _perturbing(monkeypatch, every_call=False, side="teacher")
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        loss = _forward(mod, single)
        sel.finish_pending()
    torch.cuda.synchronize()
    msgs = [str(w.message) for w in seen if "residual check" in str(w.message)]
    assert len(calls) == 1 and len(msgs) == 2 and sum("previous step" in m for m in msgs) == 1, msgs
    assert torch.equal(loss, clean) and dict(sel.subspace_ranks) == dict(clean_mod.layer_selector.subspace_ranks)
