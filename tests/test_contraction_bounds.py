"""Element-by-element bounds on the contraction kernels of csrc/gemm.hip, on both arithmetic paths.

The products behind every Gram matrix, projection and column mean of the loss run either on the bf16 matrix cores with
three-way split operands (``basd_gemm_tuning(1)``, the default) or on the fp32 MFMA (``basd_gemm_tuning(0)``).  Every GPU
test here runs on both (fixture ``path``; the process-wide switch is put back afterwards).

Part A -- bit-exact products of integer data.  The operands are integers times powers of two, small enough that
max(|A|^T |B|) * 1.02 < 2^24 (asserted on the CPU in fp64 before the GPU call).  Every bf16 piece, every piece product
and every partial sum in any order is then exactly representable in fp32, so the kernel must return the int64
reference bit for bit: indexing, tails, layouts, dispatch.  No tolerance.

Part B -- element-wise error on graded random data.  rho = max_ij |C - ref|_ij / (u (|A|^T |B|)_ij), u = 2^-24, against
fp64 of the same operation.  K <= 8: rho <= 6 K + 3, the a-priori bound for any summation order of the six exact piece
products in round-to-nearest fp32 (6 K - 1 additions: gamma_{6K-1} ~ (6K - 1) u) plus the dropped terms (mid lo, lo mid,
lo lo: <= 2^-26 |x y| = u |x y| / 4 together) -- not a measurement.  K in {33, 100}: rho <= 10, which rests on the CPU
emulation below: on these inputs the correct algorithm and a plain fp32 matmul stay <= 6.7 (the Gram diagonals at
K = 100, sums of squares; <= 3.6 elsewhere), the weakest single-term omission gives 22.8.  Measured on an MI355X
(profiles/contraction_bounds.txt): <= 8.2 on the split path and <= 6.4 on the fp32 MFMA, both at the same Gram diagonals.

Part C -- a CPU companion (not marked gpu) that emulates the split algorithm in numpy on the very inputs of Part B and
asserts (a) that it stays within Part B's bounds and (b) that it exceeds them at every K used as soon as one of
hi lo, lo hi, mid mid is left out; and one end-to-end step on the fp32-MFMA path against the golden fixture.

Every rho is printed (``pytest -s``); one GPU run is recorded in profiles/contraction_bounds.txt.
"""
import os
import sys

import numpy as np
import pytest
import torch

U = 2.0 ** -24
FILL = 12345.0          # what padding, CLS rows and the float in front of a misaligned base hold: never to be read


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(params=[1, 0], ids=["split", "fp32mfma"])
def path(request):
    """basd_gemm_tuning(1 = split operands on the bf16 matrix cores, 0 = fp32 MFMA); the previous value of the
    process-wide switch is restored afterwards, also when the test fails."""
    from basd_amd import _lib
    prev = _lib.query("basd_gemm_tuning_get")
    _lib.call("basd_gemm_tuning", request.param)
    try:
        yield request.param
    finally:
        _lib.call("basd_gemm_tuning", prev)


# --------------------------------------------------------------------------- #
# helpers: integer data, power-of-two scales, storage layouts
# --------------------------------------------------------------------------- #
def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _ints(g, shape, amax):
    """int64 uniform in [-amax, amax]"""
    return torch.randint(-int(amax), int(amax) + 1, shape, generator=g)


def _pow2(g, n, lo=-30, hi=30):
    return torch.pow(2.0, torch.randint(lo, hi + 1, (n,), generator=g).double())


def _guard(a_abs, b_abs):
    """max(|A|^T |B|) * 1.02 < 2^24 for (k, m) and (k, n) magnitudes (fp64): what makes exactness a theorem."""
    worst = float((a_abs.double().transpose(-1, -2) @ b_abs.double()).max())
    assert worst * 1.02 < 2.0 ** 24, worst


def _assert_exact32(x):
    assert torch.equal(x.float().double(), x), "the test's own expected value is not an fp32 number"


def _amax(krows, other, cap, shift=0):
    """largest |a| (<= cap) for which krows * (|a| + shift) * other stays under the guard"""
    return max(1, min(cap, int(2.0 ** 24 / 1.03 / (krows * other)) - shift))


def _place(x, layout, dev):
    """The values of the CPU tensor x (rows, cols) on the device in the named storage layout (a view):
    contig   row-major, row stride = cols
    padded   row stride rounded up to a multiple of 4 (+4): the 16-byte loaders with a column count that is no multiple of 4
    offset1  `padded` with the base pointer one element past a 16-byte boundary: only the base breaks the alignment
    chan     channel-major storage (cols, rows), viewed transposed: column stride = rows
    """
    R, C = x.shape
    if layout == "contig":
        return x.to(dev).contiguous()
    if layout == "chan":
        return x.t().contiguous().to(dev).t()
    ld = (C + 3) // 4 * 4 + 4
    off = 1 if layout == "offset1" else 0
    assert layout in ("padded", "offset1"), layout
    buf = torch.full((R * ld + 4,), FILL, dtype=x.dtype, device=dev)
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + R * ld].view(R, ld)[:, :C]
    view.copy_(x.to(dev))
    return view


def _place_tokens(x, n, dev, cls, layout="contig"):
    """(rows, cols) -> a (ceil(rows / n), n, cols) token view; cls: sliced out of (B, n + 1, cols) (the CLS row and the
    rows past the end hold FILL).  layout `padded`: column stride padded as in _place."""
    R, C = x.shape
    nb = (R + n - 1) // n
    ld = C if layout == "contig" else (C + 3) // 4 * 4 + 4
    buf = torch.full((nb, n + (1 if cls else 0), ld), FILL, dtype=x.dtype, device=dev)
    full = torch.full((nb * n, C), FILL, dtype=x.dtype)
    full[:R] = x
    view = buf[:, (1 if cls else 0):, :C]
    view.copy_(full.view(nb, n, C).to(dev))
    return view


def _eq(out, ref, what=""):
    """bit-exact: torch.equal against the fp64 reference cast to fp32 (which the caller has checked to be exact)"""
    _assert_exact32(ref)
    got = out.detach().cpu()
    want = ref.float().reshape(got.shape)
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        i = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{what}: {bad.shape[0]} of {got.numel()} elements differ, first at {i}: "
                             f"got {got[i].item()!r}, want {want[i].item()!r}")


# --------------------------------------------------------------------------- #
# Part A.1: gemm_nt
# --------------------------------------------------------------------------- #
NT_SHAPES = [(1, 1, 1), (127, 129, 31), (129, 127, 33), (130, 260, 64), (257, 128, 101), (2049, 129, 40)]
NT_LAYOUTS = ["contig", "padded", "offset1", "k33", "chan", "cls49", "bf16", "bf16_chan", "batch3", "bias_scale", "beta"]


def _nt_data(M, N, K, batch, amax, key, row_scale=True):
    """A = a * r_m * s_k, B = b * c_n / s_k with integers a (|a| <= amax: hi and mid planes populated at 12 bits),
    |b| <= 7 and powers of two r, c (2^-30..2^30), s (2^-10..2^10): A B^T = (a b^T) r_m c_n exactly."""
    g = _gen(M, N, K, *key)
    a = _ints(g, (batch, M, K), amax)
    b = _ints(g, (batch, N, K), 7)
    _guard(a.abs().transpose(1, 2), b.abs().transpose(1, 2))
    r = _pow2(g, M) if row_scale else torch.ones(M, dtype=torch.float64)
    c = _pow2(g, N)
    s = _pow2(g, K, -10, 10)
    A = a.double() * r[:, None] * s
    B = b.double() * c[:, None] / s
    ref = (a @ b.transpose(1, 2)).double() * r[:, None] * c
    return A, B, ref, r, c, g


@pytest.mark.gpu
@pytest.mark.parametrize("layout", NT_LAYOUTS)
@pytest.mark.parametrize("M,N,K", NT_SHAPES)
def test_gemm_nt_integer_exact(dev, path, M, N, K, layout):
    """C = A B^T bit for bit.  Instance of gemm_nt_kernel<Path, TA, VEC_A> reached (Path = SplitBf16 on path 1, Fp32Mfma
    on path 0; <TA, VEC_A> below):
    contig      <float, VEC> where K % 4 == 0 (64, 40), else <float, !VEC> (row stride no multiple of 4)
    padded      <float, VEC> at every K: ragged last K chunk of the 16-byte loader (K = 1, 31, 33, 101, 40)
    offset1     <float, !VEC>: base pointer off by one float, strides aligned
    k33         <float, !VEC>: K = 33 contiguous, row stride 33
    chan        <float, !VEC> with sd != 1: the strided(-pair) loader, full last chunk at K = 64, ragged elsewhere
    cls49       3-D (B, 50, K)[:, 1:] view, rows_per_batch = 49 (row_off), `rows=M` cuts the last item short
    bf16        <bf16, VEC>;  bf16_chan  <bf16, !VEC>
    batch3      blockIdx.z = 3 with batch strides on A, B and C
    bias_scale  C = 0.25 A B^T - 1 bias^T;  beta  C = 0.5 C0 + A B^T
    (2049, 129, 40): 17 row tiles x 2 column tiles, the 1-D XCD-aware grid with a ragged last row tile (the ids
    decoded past it return at once);
    (130, 260, 64) and (257, 128, 101): more than one tile along N / M on the plain 3-D grid.
    B is always fp32 row-major with a leading dimension that is a multiple of 4 (the entry point requires it)."""
    from basd_amd import ops
    if layout == "k33":
        K = 33
    bf16 = layout.startswith("bf16")
    batch = 3 if layout == "batch3" else 1
    A, B, ref, r, c, g = _nt_data(M, N, K, batch, 255 if bf16 else 4095, (NT_LAYOUTS.index(layout),),
                                  row_scale=layout != "bias_scale")
    dt = torch.bfloat16 if bf16 else torch.float32
    assert torch.equal(A.to(dt).double(), A) and torch.equal(B.float().double(), B)
    ldb = (K + 3) // 4 * 4
    b_dev = torch.full((batch, N, ldb), FILL, device=dev)
    b_dev[:, :, :K] = B.float().to(dev)
    b_arg = b_dev[0, :, :K]
    a_cpu = A[0].to(dt)
    kw = {}
    if layout in ("contig", "k33", "bf16", "bias_scale", "beta"):
        a_arg = _place(a_cpu, "contig", dev)
    elif layout in ("padded", "offset1"):
        a_arg = _place(a_cpu, layout, dev)
    elif layout in ("chan", "bf16_chan"):
        a_arg = _place(a_cpu, "chan", dev)
        assert a_arg.stride(1) != 1 or M == 1
    elif layout == "cls49":
        a_arg = _place_tokens(a_cpu, 49, dev, cls=True)
        kw = dict(rows=M)
    else:
        a_all = A.float().to(dev).contiguous()
        a_arg = a_all[0]
        kw = dict(batch=3, a_batch_stride=M * K, b_batch_stride=N * ldb)
    if layout == "bias_scale":
        bias_i = _ints(g, (N,), 100).double() * c
        kw.update(scale=0.25, bias=bias_i.float().to(dev))
        ref = 0.25 * ref - bias_i
    if layout == "beta":
        c0 = (2 * _ints(g, (M, N), 500)).double() * r[:, None] * c
        kw.update(beta=0.5, out=c0.float().to(dev))
        ref = 0.5 * c0 + ref
    out = ops.gemm_nt(a_arg, b_arg, **kw)
    _eq(out, ref if batch > 1 else ref[0], f"gemm_nt {layout} path {path}")


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", [(1, 1, 1), (256, 129, 31), (130, 260, 64), (2049, 129, 40)])
def test_gemm_nt_column_sums_exact(dev, path, M, N, K):
    """The epilogue's column sums of a row tile are sums of integers (times the column's power of two): exact, so
    ``col_sums=`` must hold the int64 tile sums and ``col_mean=True`` float32(sum) * (float32(1) / float32(M)), the
    kernel's documented formula (itself exact at M = 256).  No row scaling: a column's terms must share one exponent.
    (2049, 129, 40) folds 17 tile sums on the XCD-aware grid; bias and scale go through the same epilogue."""
    from basd_amd import ops
    g = _gen(M, N, K, 77)
    amax = _amax(M * K, 7 * 4, 4095)          # x4: the sums are formed of 0.5 * product - bias
    a = _ints(g, (M, K), amax)
    b = _ints(g, (N, K), 7)
    bias_i = _ints(g, (N,), 3)
    c = _pow2(g, N)
    s = _pow2(g, K, -10, 10)
    assert float((a.abs().double().sum(0) @ b.abs().double().t() * 0.5 + M * 3).max()) * 1.02 < 2.0 ** 23
    ldb = (K + 3) // 4 * 4
    b_dev = torch.full((N, ldb), FILL, device=dev)
    b_dev[:, :K] = (b.double() * c[:, None] / s).float().to(dev)
    a_dev = _place((a.double() * s).float(), "padded", dev)
    prod = (a @ b.t()).double()
    tiles = (M + 127) // 128
    inv = np.float32(1.0) / np.float32(M)

    def mean_of(total):          # float32(sum) * float32(1 / M), in fp32
        _assert_exact32(total)
        return torch.from_numpy(total.float().numpy() * inv)

    # col_mean with scale and bias
    val = 0.5 * prod * c - bias_i.double() * c
    out, mean = ops.gemm_nt(a_dev, b_dev[:, :K], scale=0.5, bias=(bias_i.double() * c).float().to(dev), col_mean=True)
    _eq(out, val, "C")
    assert torch.equal(mean.cpu(), mean_of(val.sum(0))), "column means"
    # col_sums: the row-tile sums themselves
    part = torch.full((tiles * N,), FILL, device=dev)
    out = ops.gemm_nt(a_dev, b_dev[:, :K], col_sums=part)
    _eq(out, prod * c, "C")
    want = torch.stack([(prod[t * 128:(t + 1) * 128].sum(0)) * c for t in range(tiles)])
    _eq(part.view(tiles, N), want, "row-tile column sums")


# --------------------------------------------------------------------------- #
# Part A.2: gemm_tn
# --------------------------------------------------------------------------- #
TN_CASES = [(kr, M, N, v) for (kr, M, N) in [(1, 1, 1), (31, 127, 129), (33, 130, 4), (245, 129, 130), (520, 64, 260),
                                             (2592, 8, 8)]
            for v in ["plain", "means", "padded_means", "offset1", "bf16", "bf16_means"]
            + (["tok49", "tok49_cls", "tok49_cls_padded"] if kr == 245 else [])]
# appended, never inserted: the index of a case seeds its data
TN_CASES += [(kr, M, N, v) for (kr, M, N) in [(31, 127, 129), (245, 129, 130)] for v in ["chan", "bf16_chan"]]


def _tn_data(kr, M, N, bf16, means, key):
    """A = a * ca_m * s_k, B = b * cb_n / s_k (s = 1 when a mean is subtracted: a column's rows must share one
    exponent), means = integer * column scale, so that x - mean is exact."""
    g = _gen(kr, M, N, *key)
    shift_a, shift_b = (64, 3) if means else (0, 0)
    a = _ints(g, (kr, M), _amax(kr, 7 + shift_b, 255 if bf16 else 4095, shift_a))
    b = _ints(g, (kr, N), 7)
    ma = _ints(g, (M,), shift_a) if means else torch.zeros(M, dtype=torch.int64)
    mb = _ints(g, (N,), shift_b) if means else torch.zeros(N, dtype=torch.int64)
    _guard((a - ma).abs(), (b - mb).abs())
    ca, cb = _pow2(g, M), _pow2(g, N)
    s = torch.ones(kr, dtype=torch.float64) if means else _pow2(g, kr, -10, 10)
    A = a.double() * ca * s[:, None]
    B = b.double() * cb / s[:, None]
    ref = ((a - ma).t() @ (b - mb)).double() * ca[:, None] * cb
    return A, B, (ma.double() * ca).float(), (mb.double() * cb).float(), ref


@pytest.mark.gpu
@pytest.mark.parametrize("kr,M,N,variant", TN_CASES)
def test_gemm_tn_integer_exact(dev, path, kr, M, N, variant):
    """C = 0.5 (A - 1 mean_a^T)^T (B - 1 mean_b^T) bit for bit: gemm_tn_kernel<Path, T, VEC> with Path = SplitBf16 on
    path 1, Fp32Mfma on path 0; <T, VEC> below.
    plain / means     contiguous: <float, VEC> at (520, 64, 260) and (2592, 8, 8), else <float, !VEC> (column counts
                      that are no multiple of 4 make the row stride one)
    padded_means      <float, VEC> with column counts 127, 129, 130: ragged last column tile of the 16-byte loader
    offset1           <float, !VEC>: bases off by one float
    bf16, bf16_means  <bf16, VEC>
    chan, bf16_chan   channel-major storage of both operands (column stride != 1) at (31, 127, 129) and (245, 129, 130):
                      <float, !VEC> with sd != 1 and <bf16, !VEC>, the latter reached by no other exact case
    tok49*            (5, 49, .) token views, CLS-sliced from (5, 50, .): rows_per_batch % 4 != 0, the 4-row groups
                      straddle batch items (tn_row), both loaders (`_padded`: VEC)
    (520, 64, 260): two K-splits (basd_gemm_tn_splits = 2), 17 chunks: the second split ends in a ragged chunk;
    (2592, 8, 8): 10 splits over 81 chunks of 9, the tenth split is empty and must contribute exact zeros."""
    from basd_amd import ops, _lib
    if kr == 520:
        assert _lib.query("basd_gemm_tn_splits", kr) == 2
    if kr == 2592:
        assert _lib.query("basd_gemm_tn_splits", kr) == 10
    bf16 = variant.startswith("bf16")
    means = "means" in variant or variant.startswith("tok49")
    A, B, mean_a, mean_b, ref = _tn_data(kr, M, N, bf16, means, (TN_CASES.index((kr, M, N, variant)),))
    dt = torch.bfloat16 if bf16 else torch.float32
    assert torch.equal(A.to(dt).double(), A) and torch.equal(B.to(dt).double(), B)
    if variant.startswith("tok49"):
        lay = "padded" if variant.endswith("padded") else "contig"
        a_arg = _place_tokens(A.to(dt), 49, dev, cls="cls" in variant, layout=lay)
        b_arg = _place_tokens(B.to(dt), 49, dev, cls="cls" in variant, layout=lay)
        assert a_arg.shape == (5, 49, M)
    else:
        lay = {"padded_means": "padded", "offset1": "offset1", "chan": "chan", "bf16_chan": "chan"}.get(variant, "contig")
        a_arg, b_arg = _place(A.to(dt), lay, dev), _place(B.to(dt), lay, dev)
        if lay == "chan":
            assert a_arg.stride(1) != 1 and b_arg.stride(1) != 1
    kw = dict(mean_a=mean_a.to(dev), mean_b=mean_b.to(dev)) if means else {}
    out = ops.gemm_tn(a_arg, b_arg, scale=0.5, **kw)
    _eq(out, 0.5 * ref, f"gemm_tn {variant} path {path}")


@pytest.mark.gpu
def test_gemm_tn_batched_no_split_exact(dev, path):
    """The batched form without K-splits (batch 6 of 49 x 49 by 49 x 130, blockIdx.z = batch item)."""
    from basd_amd import ops
    g = _gen(6, 49, 130)
    a = _ints(g, (6, 49, 49), 4095)
    b = _ints(g, (6, 49, 130), 7)
    _guard(a.abs(), b.abs())
    ca, cb = _pow2(g, 49), _pow2(g, 130)
    a_dev = (a.double() * ca).float().to(dev)
    b_dev = (b.double() * cb).float().to(dev)
    out = ops.gemm_tn(a_dev[0], b_dev[0], batch=6, a_batch_stride=49 * 49, b_batch_stride=49 * 130, krows=49,
                      m_cols=49, n_cols=130, split=False)
    _eq(out, (a.transpose(1, 2) @ b).double() * ca[:, None] * cb, "batched gemm_tn")


# --------------------------------------------------------------------------- #
# Part A.3: centered_grams
# --------------------------------------------------------------------------- #
def _gram_data(kr, cols, n, bf16, key):
    """n integer matrices, mostly |x| <= 15 with 3 % of the entries up to 1023 (255 for bf16), times a per-column power
    of two; integer means times the same scale."""
    g = _gen(kr, cols, n, *key)
    x = _ints(g, (n, kr, cols), 15)
    big = _ints(g, (n, kr, cols), 255 if bf16 else 1023)
    x = torch.where(torch.rand((n, kr, cols), generator=g) < 0.03, big, x)
    mu = _ints(g, (n, cols), 4)
    c = _pow2(g, cols)
    return x, mu, c


def _gram_check(out, x, mu, c, centered, scales, what):
    for i in range(x.shape[0]):
        z = x[i] - (mu[i] if centered[i] else 0)
        _guard(z.abs(), z.abs())
        ref = (z.t() @ z).double() * c[:, None] * c * scales[i]
        _eq(out[i], ref, f"{what}, matrix {i}")
        assert torch.equal(out[i], out[i].T), "mirrored tiles must be bit-identical"


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 8])
@pytest.mark.parametrize("kr", [1, 33, 70, 245])
@pytest.mark.parametrize("cols", [1, 127, 129, 257])
def test_centered_grams_integer_exact(dev, path, cols, kr, n):
    """G_z = (X_z - 1 mu_z^T)^T (X_z - 1 mu_z^T) bit for bit and symmetric (syrk_tn_kernel<SplitBf16, ...> /
    syrk_tn_kernel<Fp32Mfma, ...> with syrk_reduce_kernel).  Row stride padded to a multiple of 4: <float, VEC> at
    column counts 1, 127, 129, 257 (one to three tiles, up to six tile pairs with mirrored off-diagonal ones); kr = 245
    is a (5, 49, .) token view (4-row groups straddle items).  n = 8 runs with splits = 1 and 3: units % 8 == 0, the XCD-aware decode of the grid, with
    off-diagonal pairs at 129 and 257 columns; at kr = 33 / 70 the third split of three gets no chunk / a ragged one."""
    from basd_amd import ops
    x, mu, c = _gram_data(kr, cols, n, False, ())
    vals = (x.double() * c).float()
    if kr == 245:
        xs = [_place_tokens(vals[i], 49, dev, cls=False, layout="padded") for i in range(n)]
    else:
        xs = [_place(vals[i], "padded", dev) for i in range(n)]
    means = (mu.double() * c).float().to(dev)
    for splits in ((1, 3) if n == 8 else (None,)):
        out, _ = ops.centered_grams(xs, means=means, splits=splits)
        _gram_check(out.cpu(), x, mu, c, [True] * n, [1.0] * n, f"centered_grams splits {splits} path {path}")


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["contig", "offset1", "bf16", "bf16_chan", "chan", "cls_tokens", "empty_split",
                                     "mixed_scaled"])
def test_centered_grams_variants_exact(dev, path, variant):
    """The remaining dispatch branches of basd_syrk_multi, 3 matrices of 129 columns (two tiles, three pairs):
    contig        <float, !VEC>: contiguous rows of 129 floats
    offset1       <float, !VEC>: aligned strides, bases off by one float (vec_ok = 0)
    bf16          <bf16, VEC>;  bf16_chan  <bf16, !VEC>;  chan  <float, !VEC> with sd != 1
    cls_tokens    (5, 50, .)[:, 1:] views, contiguous columns: !VEC with straddling 4-row groups
    empty_split   splits forced to 4 at 70 rows (3 chunks): the fourth split is empty and must add exact zeros
    mixed_scaled  centered = [True, False, True] with per-matrix power-of-two scales (syrk_reduce_kernel)"""
    from basd_amd import ops
    kr, cols, n = (245 if variant == "cls_tokens" else 70), 129, 3
    bf16 = variant.startswith("bf16")
    x, mu, c = _gram_data(kr, cols, n, bf16, (7,))
    dt = torch.bfloat16 if bf16 else torch.float32
    vals = (x.double() * c).to(dt)
    assert torch.equal(vals.double(), x.double() * c)
    if variant == "cls_tokens":
        xs = [_place_tokens(vals[i], 49, dev, cls=True) for i in range(n)]
    else:
        lay = {"contig": "contig", "offset1": "offset1", "chan": "chan", "bf16_chan": "chan"}.get(variant, "padded")
        xs = [_place(vals[i], lay, dev) for i in range(n)]
    if variant == "offset1":
        assert all(t.data_ptr() % 16 == 4 for t in xs)
    means = (mu.double() * c).float().to(dev)
    centered, scales, kw = [True] * n, [1.0] * n, {}
    if variant == "empty_split":
        kw = dict(splits=4)
    if variant == "mixed_scaled":
        centered, scales = [True, False, True], [0.5, 2.0 ** -7, 4.0]
        kw = dict(centered=centered, scales=scales)
    out, _ = ops.centered_grams(xs, means=means, **kw)
    _gram_check(out.cpu(), x, mu, c, centered, scales, f"centered_grams {variant} path {path}")


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", [(256, 129, 8), (128, 40, 5)])
def test_centered_grams_fold_route_exact(dev, path, M, N, K):
    """The ``fold=`` route: the column means are folded inside the Gram launch from the row-tile sums that the
    gemm_nt(..., col_sums=) epilogue left behind.  Y = A B^T is integer-valued with column sums that are multiples of
    M (the columns of A are nudged to sum to a multiple of M), M a power of two: the folded mean sum * (1 / M) is an
    integer times the column's scale, and G = (Y - 1 mean^T)^T (Y - 1 mean^T) must be exact.  A first, unfolded and
    uncentred matrix rides along (fold_from = 1)."""
    from basd_amd import ops
    g = _gen(M, N, K, 5)
    a = _ints(g, (M, K), 6)
    rem = a.sum(0) % M                                   # take 1 off the first `rem` rows of each column
    a = a - (torch.arange(M)[:, None] < rem[None, :]).long()
    assert bool((a.sum(0) % M == 0).all())
    b = _ints(g, (N, K), 3)
    c = _pow2(g, N)
    y = a @ b.t()
    mean = y.sum(0) // M
    assert bool((mean * M == y.sum(0)).all())
    ldb = (K + 3) // 4 * 4
    b_dev = torch.zeros((N, ldb), device=dev)
    b_dev[:, :K] = (b.double() * c[:, None]).float().to(dev)
    tiles = ops.gemm_nt_row_tiles(M, N, K)
    part = torch.full((tiles * N,), FILL, device=dev)
    y_dev = ops.gemm_nt(a.float().to(dev), b_dev[:, :K], col_sums=part)
    _eq(y_dev, y.double() * c, "projection")
    z = _ints(g, (M, N), 15)
    cz = _pow2(g, N)
    z_dev = (z.double() * cz).float().to(dev)
    out, _ = ops.centered_grams([z_dev, y_dev], fold=(part.view(1, tiles, N), 1))
    out = out.cpu()
    yc = y - mean
    _guard(yc.abs(), yc.abs())
    _guard(z.abs(), z.abs())
    _eq(out[0], (z.t() @ z).double() * cz[:, None] * cz, "unfolded, uncentred matrix")
    _eq(out[1], (yc.t() @ yc).double() * c[:, None] * c, "folded, centred matrix")
    assert torch.equal(out[0], out[0].T) and torch.equal(out[1], out[1].T)


# --------------------------------------------------------------------------- #
# Part A.4: colmean, column_means
# --------------------------------------------------------------------------- #
MEAN_CASES = [(rows, cols, layout) for rows in [1, 255, 256, 520] for cols in [1, 3, 130, 132]
              for layout in ["contig", "offset1", "bf16", "tokens"] if layout != "tokens" or rows % 5 == 0]


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols,layout", MEAN_CASES)
def test_column_means_integer_exact(dev, path, rows, cols, layout):
    """colmean and column_means against float32(sum) * float32(1 / rows): the sums are sums of integers times the
    column's power of two (exact in any order), the one multiplication is the kernels' documented formula, itself exact
    at 256 rows.  520 rows: two row slices (basd_colmean_parts).  colsum_partial_kernel at column counts 1, 3, 130 and
    behind a misaligned base; colsum_partial_vec_kernel at 132 columns (fp32 contiguous; bf16 rows of 264 bytes are not
    16-byte aligned: scalar kernel).  `tokens`: a (B, 6, .)[:, 1:] view of 5 rows per item.  The kernels do not
    depend on the arithmetic path; the parametrisation only shows that the switch leaves them alone."""
    from basd_amd import ops
    bf16 = layout == "bf16"
    g = _gen(rows, cols, 3)
    x = _ints(g, (3, rows, cols), 255 if bf16 else 4095)
    c = _pow2(g, cols)
    dt = torch.bfloat16 if bf16 else torch.float32
    vals = (x.double() * c).to(dt)
    assert torch.equal(vals.double(), x.double() * c)
    if layout == "tokens":
        xs = [_place_tokens(vals[i], 5, dev, cls=True) for i in range(3)]
    else:
        xs = [_place(vals[i], "offset1" if layout == "offset1" else "contig", dev) for i in range(3)]
    total = x.sum(1).double() * c
    _assert_exact32(total)
    want = torch.from_numpy(total.float().numpy() * (np.float32(1.0) / np.float32(rows)))
    assert torch.equal(ops.colmean(xs[1]).cpu(), want[1]), "colmean"
    assert torch.equal(ops.column_means(xs).cpu(), want), "column_means"


# --------------------------------------------------------------------------- #
# Part B: element-wise error bounds on graded random data (inputs shared with the CPU companion)
# --------------------------------------------------------------------------- #
B_KS = [1, 3, 8, 33, 100]
B_ENTRIES = ["gemm_nt", "gemm_tn", "gemm_tn_means", "centered_grams"]


def rho_bound(K):
    """K <= 8: a priori (6 K - 1 roundings of the sum of 6 K exact piece products, plus the dropped terms and the
    second-order part: 6 K + 3); K = 33, 100: 10, from the CPU emulation (see the module docstring)."""
    return 6 * K + 3 if K <= 8 else 10


def _graded(entry, K, bf16=False):
    """Part B's operands as staged by the kernels, in the A^T B form: a list of (Xa (K, M), Xb (K, N), raw A, raw B,
    mean_a, mean_b) fp32 CPU tensors, one per output matrix.  randn times a per-column scale 2^e, e in [-20, 20] (the
    column of the A^T B form: an output row / column, so the element-wise bound bites at every scale), plus half the
    column's scale on one operand.  Where a mean is subtracted it is 0.4375 of the column's scale, in fp32, and the
    staged value is fl32(x - mean) as in the kernels.  bf16: the raw operands are rounded to bf16 first (gemm_nt: A only)."""
    g = _gen(B_ENTRIES.index(entry), K, 11)
    M, N = (40, 72) if entry == "gemm_nt" else (40, 40)
    n = 3 if entry == "centered_grams" else 1
    cases = []
    for i in range(n):
        ca = torch.pow(2.0, torch.randint(-20, 21, (M,), generator=g).float())
        cb = torch.pow(2.0, torch.randint(-20, 21, (N,), generator=g).float())
        a = torch.randn(K, M, generator=g) * ca + 0.5 * ca
        b = torch.randn(K, N, generator=g) * cb
        if bf16:
            a = a.bfloat16().float()
            if entry != "gemm_nt":
                b = b.bfloat16().float()
        ma = mb = None
        if entry == "gemm_tn_means":
            ma, mb = 0.4375 * ca, 0.4375 * cb
        if entry == "centered_grams":
            b, cb = a, ca
            if i != 1:
                ma = mb = 0.4375 * ca
        xa = a - ma if ma is not None else a
        xb = b - mb if mb is not None else b
        cases.append((xa, xb, a, b, ma, mb))
    return cases


def _rho(C, xa, xb, scale=1.0):
    """max_ij |C - ref| / (u |Xa|^T |Xb|) against fp64; where the denominator is 0, C must be 0."""
    C = np.asarray(C, dtype=np.float64)
    xa, xb = xa.double().numpy(), xb.double().numpy()
    ref = scale * (xa.T @ xb)
    den = U * scale * (np.abs(xa).T @ np.abs(xb))
    assert np.all(np.isfinite(C))
    assert np.all(C[den == 0] == 0), "an element with no non-zero product must be exactly 0"
    ok = den > 0
    return float((np.abs(C - ref)[ok] / den[ok]).max()) if ok.any() else 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("K", B_KS)
@pytest.mark.parametrize("entry", B_ENTRIES)
def test_elementwise_error_bound(dev, path, entry, K, bf16):
    """rho <= 6 K + 3 (K <= 8), <= 10 (K = 33, 100) for gemm_nt at M = 40, N = 72, gemm_tn at M = N = 40 with and
    without means, centered_grams at 40 columns with 3 matrices (the middle one uncentred); scale = 2^-3."""
    from basd_amd import ops
    cases = _graded(entry, K, bf16)
    dt = torch.bfloat16 if bf16 else torch.float32
    scale = 0.125
    if entry == "gemm_nt":
        xa, xb, a, b, _, _ = cases[0]
        ldb = (K + 3) // 4 * 4
        b_dev = torch.zeros((72, ldb), device=dev)
        b_dev[:, :K] = b.t().to(dev)
        outs = [ops.gemm_nt(_place(a.t().contiguous().to(dt), "padded", dev), b_dev[:, :K], scale=scale)]
    elif entry.startswith("gemm_tn"):
        xa, xb, a, b, ma, mb = cases[0]
        kw = dict(mean_a=ma.to(dev), mean_b=mb.to(dev)) if ma is not None else {}
        outs = [ops.gemm_tn(a.to(dt).to(dev), b.to(dt).to(dev), scale=scale, **kw)]
    else:
        xs = [c[2].to(dt).to(dev) for c in cases]
        means = torch.stack([c[4] if c[4] is not None else torch.zeros(40) for c in cases]).to(dev)
        out, _ = ops.centered_grams(xs, means=means, centered=[True, False, True], scales=[scale] * 3)
        outs = list(out)
    rho = max(_rho(o.cpu().numpy(), c[0], c[1], scale) for o, c in zip(outs, cases))
    print(f"rho gpu  {entry:15s} path={'split' if path else 'fp32mfma'} {'bf16' if bf16 else 'fp32'} K={K:3d}: "
          f"{rho:7.3f}  (bound {rho_bound(K)})")
    assert rho <= rho_bound(K), rho


# --------------------------------------------------------------------------- #
# Part C: CPU companion -- the split algorithm in numpy on Part B's inputs, with and without each small term
# --------------------------------------------------------------------------- #
def _pieces(x):
    """hi + mid + lo = x exactly, bf16 round-to-nearest pieces (torch.bfloat16), as split3 in gemm.hip"""
    hi = x.bfloat16().float()
    r = x - hi
    mid = r.bfloat16().float()
    lo = (r - mid).bfloat16().float()
    assert torch.equal(hi.double() + mid.double() + lo.double(), x.double())
    return [p.double().numpy() for p in (hi, mid, lo)]


# the six piece products that the kernels keep, as (piece of A, piece of B); 0 = hi, 1 = mid, 2 = lo
TERMS = [(2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0)]
OMIT = {"hi*lo": (0, 2), "lo*hi": (2, 0), "mid*mid": (1, 1)}


def _emulate(xa, xb, drop=None):
    """The split algorithm: per k-step the six piece products (each exact) are formed and summed in fp64, and the
    step's sum is added to an fp32 accumulator (one rounding per k-step).  drop: a (piece of A, piece of B) pair that is
    left out."""
    pa, pb = _pieces(xa), _pieces(xb)
    acc = np.zeros((xa.shape[1], xb.shape[1]), dtype=np.float32)
    for k in range(xa.shape[0]):
        step = sum(np.outer(pa[i][k], pb[j][k]) for (i, j) in TERMS if (i, j) != drop)
        acc = (acc.astype(np.float64) + step).astype(np.float32)
    return acc


@pytest.mark.parametrize("K", B_KS)
@pytest.mark.parametrize("entry", B_ENTRIES)
def test_split_emulation_keeps_the_bound_and_needs_every_term(entry, K):
    """(a) the emulated split algorithm stays within Part B's bound on Part B's inputs (fp32 and bf16); (b) on the fp32
    inputs (bf16 values have no mid and lo pieces to lose), with hi*lo, lo*hi or
    mid*mid left out it exceeds the bound, at every K that Part B uses -- so a kernel that drops a term cannot pass
    Part B.  No deliberately wrong kernel ever runs on the GPU."""
    cases = _graded(entry, K)
    rho = max(_rho(_emulate(xa, xb), xa, xb) for xa, xb, *_ in cases)
    rho16 = max(_rho(_emulate(xa, xb), xa, xb) for xa, xb, *_ in _graded(entry, K, bf16=True))
    plain = max(_rho((xa.t() @ xb).numpy(), xa, xb) for xa, xb, *_ in cases)
    line = (f"rho emul {entry:15s} K={K:3d}: fp32 {rho:6.3f}  bf16 {rho16:6.3f}  (bound {rho_bound(K)}, plain fp32 matmul "
            f"{plain:.3f})")
    assert rho <= rho_bound(K), rho
    assert rho16 <= rho_bound(K), rho16
    assert plain <= rho_bound(K), plain
    for name, pair in OMIT.items():
        worst = max(_rho(_emulate(xa, xb, drop=pair), xa, xb) for xa, xb, *_ in cases)
        line += f"  without {name}: {worst:.1f}"
        assert worst > rho_bound(K), (name, worst)
    print(line)


# --------------------------------------------------------------------------- #
# Part C: one whole step on the fp32-MFMA path
# --------------------------------------------------------------------------- #
@pytest.mark.gpu
def test_full_small_golden_on_the_fp32_mfma_path(golden):
    """The `cnn` case of full_small.npz with basd_gemm_tuning(0): token layers, ranks and the loss (rtol 1e-4) as in
    test_full_small_golden -- the fallback path carries a whole step."""
    from types import SimpleNamespace
    from basd_amd import _lib, synth
    from basd_amd.losses import BASDLoss
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_goldens_shapes as S
    g = golden("full_small.npz")
    tag = "cnn"
    shape, seed = S.SMALL[tag]
    prev = _lib.query("basd_gemm_tuning_get")
    _lib.call("basd_gemm_tuning", 0)
    try:
        torch.manual_seed(42)
        crit = torch.nn.CrossEntropyLoss(label_smoothing=0.01)
        mod = BASDLoss(crit, shape.d_s, shape.d_t, shape.depth, shape.n_s,
                       config=SimpleNamespace(num_extraction_points=shape.points),
                       teacher_has_cls_token=shape.has_cls).to("cuda:0")
        inp = synth.make_inputs(shape, seed, device="cuda:0")
        leaves = {k: v.requires_grad_(True) for k, v in inp.student.items()}
        loss = mod(inp.logits.requires_grad_(True), inp.targets, leaves, inp.teacher, inp.attn)
        assert mod.token_layers == list(g[f"{tag}_token_layers"])
        assert [mod.layer_selector.subspace_ranks[k] for k in sorted(inp.teacher)] == list(g[f"{tag}_ranks"])
        np.testing.assert_allclose(loss.item(), g[f"{tag}_loss"], rtol=1e-4)
    finally:
        _lib.call("basd_gemm_tuning", prev)
