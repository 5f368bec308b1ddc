"""The front end of the Procrustes call (csrc/procrustes.hip in front of the SVD cores), kernel by kernel against
fp64 of the same operation: token weights, student projection, teacher centring, the split fp64 Gram and the stack
products.  Only well-conditioned inputs: this file stops where the Jacobi starts.

References are torch fp64 on the CPU from the same fp32 / bf16 input values, written from relational.py:22-50,
combined.py:9-14 and layer_selector.py:110-112.  The interpolation matrices I (n_out x n_in) are built densely from
ops._taps_cpu and, once per grid pair, compared for equality with torch.nn.functional.interpolate(mode="linear",
align_corners=False) in fp64 (``_interp``): every pair used here has a dyadic ratio (4, 2, 1/2, 1/4, 3/2), so lam and
1 - lam are exact fp32 numbers and the comparison needs no tolerance.

Every input buffer's padding (CLS rows, stride gaps, the float in front of a misaligned base) holds FILL; every output
buffer sits between guard elements holding FILL; the guards must stay, every owned element must change.

Part A -- exact data, bit for bit.  Token weights c_n / P with integers c_n in {floor(P / n), floor(P / n) + 1}
summing to P (P = 256; 512 at more than 256 tokens; at 196 tokens that is c_n in {1, 2}), token values integers in
[-8, 8], mixing weights and lam dyadic.  Every term of every sum is then a multiple of a power of two q, and the sum of
the absolute values of the terms stays below 2^24 q (asserted on the CPU in fp64 before the GPU call, ``_guard_exact``):
each partial sum of any order is an fp32 number, and indexing, tails, layouts and dispatch must reproduce the
reference exactly (``torch.equal``).  The stack products get lower-triangular integer factors.

Part B -- element-wise error on graded random data (magnitudes 2^e_token 2^f_feature, e and f in [-3, 3], a common
offset of 0.5; token weights softmax(2 N(0, 1))).  rho = max |got - ref| / (u S), u = 2^-24, S the fp64 sum of the
absolute values of the terms of that very element.  Every bound counts the roundings of the kernel as written and
holds for ANY summation order (each term passes through at most the counted number of round-to-nearest operations:
gamma_k = k u / (1 - k u), the factor 1.001 below covers the second order); no bound rests on a measurement and none
had to be replaced by a cap from the emulation, because the weakest mutation of Part C lands orders of magnitude
above them (printed by the companion test).  With F the adds of the fold (3 in student_project_kernel, 32 in
student_project_v4_kernel):

  token weights  K_raw = L + H A_q + 2 (A_q = 1 with a CLS row, else A): one product, L adds of the layer mix,
                 H A_q adds of the mean, one division; all terms are positive, so S is the value itself;
                 K_v = K_raw + 2 (interpolation: a product and an add); omega: K_om = n_s + 2 K_v + 1 (the sum of n_s
                 values in any order, the division); |sum omega - 1| <= (n_s + 2) u (the common factor 1 / total
                 cancels up to the n_s roundings of the total and one of the division);
                 omega_t against I^T omega (the kernel's own omega, in fp64): K_fold = 2 r + 1, r the longest tap
                 range; omega_t against the reference: K_om + K_fold; |sum omega_t - 1| <= (n_s + 2 + K_fold) u.
  projection     mu: K_mu = n_s + F, S_mu = sum_n w_n |x_n|.
                 a_prime: S = S_a + C_j S_mu with S_a = sum_n I[n, j] w_n |x_n - mu|, C_j = sum_n I[n, j] w_n; the own
                 chain has r + 3 <= K_mu roundings (coefficient times weight, the subtraction, r fmas) and the error of
                 mu enters times C_j: rho <= K_mu.
                 trace partial of a slab of W features: |err| <= u (n_s W + 8) T + sum_d (2 e_d A_d + e_d^2) with
                 T = sum_d sum_n w_n (x_n - mu)^2, e_d = K_mu u S_mu, A_d = sum_n w_n |x_n - mu| (n_s W terms in any
                 order, at most 8 local roundings per term, and the perturbation of the mean).
  centring       K_t = n + ceil(n / 16) + L + 2 (the layer mix: L fmas; the gather: a product and an add; the mean: n
                 fmas, folded over ceil(n / 16) chunk sums in the stream form); mu: S_mu = sum_j omega_t[j] S_v[j],
                 S_v = sum_l |mix_l| (I |x_l|); tc: S = S_v + S_mu, rho <= K_t + 1.
                 |sum_j omega_t[j] tc[j, :]| <= |mu| |1 - sum omega_t| + sum_j omega_t[j] (K_t + 1) u S[j].
  Gram           u = 2^-53: products of fp32 numbers are exact in fp64, D of them summed in any order and `splits`
                 partial Grams folded: rho <= D + splits; normwise 1e-14 as test_gram_chol_f64.

Part C -- a CPU companion (not marked gpu): a numpy fp32 emulation of the two student projections and of the LDS
centring kernel on the very inputs of Parts A and B, in the kernels' summation order (row groups, then the fold; fma
as one rounding of the fp64 value).  It must be bit-exact on Part A's data and within Part B's bounds, and each
mutation of MUTATIONS must break Part A's equality and exceed Part B's bounds on at least one case, per emulated
kernel it applies to.  And one gpu test on ops.procrustes_forward that compares the context's own intermediates on
every centre x projection route with the same references under the same bounds.

Every rho is printed (``pytest -s``); one GPU run is recorded in profiles/procrustes_front.txt.
"""
import math
from functools import lru_cache

import numpy as np
import pytest
import torch

U = 2.0 ** -24
U64 = 2.0 ** -53
SECOND_ORDER = 1.001    # (1 + gamma) factors of the bounds: k u <= 2e-3 at every k used here (k <= 324 * 64 + 8)
FILL = 12345.0          # what padding and guard elements hold: never to be read, never to be written
GUARD = 64              # guard elements on either side of an output (256 bytes: the output stays 16-byte aligned)
EUNSUPPORTED = -2       # BASD_EUNSUPPORTED of include/basd_hip.h
F32, BF16 = torch.float32, torch.bfloat16


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


# --------------------------------------------------------------------------- #
# helpers: generators, interpolation matrices, guarded outputs, storage layouts
# --------------------------------------------------------------------------- #
def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


_INTERP = {}


def _interp(n_in, n_out):
    """I (n_out, n_in) in fp64 from ops._taps_cpu, cross-checked once per pair against F.interpolate in fp64 (equality:
    the ratio is dyadic), with the ranges checked to cover the taps."""
    key = (n_in, n_out)
    if key not in _INTERP:
        from basd_amd import ops
        t0, t1, lam, r0, r1 = ops._taps_cpu(n_in, n_out)
        assert torch.equal((1.0 - lam).double(), 1.0 - lam.double()), "1 - lam is not exact in fp32"
        assert torch.equal((lam.double() * 64).round(), lam.double() * 64), "lam is not dyadic"
        rows = torch.arange(n_out)
        I = torch.zeros(n_out, n_in, dtype=torch.float64)
        I.index_put_((rows, t0.long()), 1.0 - lam.double(), accumulate=True)
        I.index_put_((rows, t1.long()), lam.double(), accumulate=True)
        ref = torch.nn.functional.interpolate(torch.eye(n_in, dtype=torch.float64)[None], size=n_out, mode="linear",
                                              align_corners=False)[0].t()
        assert torch.equal(I, ref), f"taps {n_in} -> {n_out} differ from F.interpolate"
        for j in range(n_in):
            touched = (I[:, j] != 0).nonzero().flatten()
            assert touched.numel() == 0 or (int(r0[j]) <= int(touched[0]) and int(touched[-1]) < int(r1[j]))
        _INTERP[key] = I
    return _INTERP[key]


def _taps_np(n_in, n_out):
    from basd_amd import ops
    return tuple(t.numpy() for t in ops._taps_cpu(n_in, n_out))


def _max_range(n_in, n_out):
    _, _, _, r0, r1 = _taps_np(n_in, n_out)
    return int((r1 - r0).max())


def _out(dev, *shape, dtype=F32, off=0):
    """(buffer, view): the output `shape` between GUARD sentinel elements, all pre-filled with FILL.  off = 1 puts the
    output one element past 16-byte alignment."""
    n = math.prod(shape)
    buf = torch.full((n + 2 * GUARD + off,), FILL, dtype=dtype, device=dev)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[GUARD + off:GUARD + off + n].view(*shape)


def _check_out(buf, view, what, written=True):
    """guards untouched; every owned element changed (written=False: the call was refused, nothing may change)"""
    flat = buf.cpu()
    lo, n = view.storage_offset(), view.numel()
    assert bool((flat[:lo] == FILL).all()) and bool((flat[lo + n:] == FILL).all()), f"{what}: guard elements overwritten"
    if written:
        left = int((flat[lo:lo + n] == FILL).sum())
        assert left == 0, f"{what}: {left} of {n} owned elements were not written"
    else:
        assert bool((flat == FILL).all()), f"{what}: a refused call wrote to its output"


def _place3(x, layout, dev):
    """The values of the CPU tensor x (B, n, D) on the device as a view in the named storage layout:
    contig    row-major
    cls       sliced out of (B, n + 1, D): the CLS rows hold FILL
    padded    row stride D + 4: the gaps hold FILL
    offset1   row-major with the base pointer one element past a 16-byte boundary (FILL in front and behind)
    chan      channel-major storage (B, D, n + 3) viewed transposed: token stride 1, feature stride n + 3, gaps FILL
    """
    B, n, D = x.shape
    if layout == "contig":
        return x.to(dev).contiguous()
    if layout == "cls":
        full = torch.full((B, n + 1, D), FILL, dtype=x.dtype, device=dev)
        view = full[:, 1:, :]
    elif layout == "padded":
        full = torch.full((B, n, D + 4), FILL, dtype=x.dtype, device=dev)
        view = full[:, :, :D]
    elif layout == "offset1":
        full = torch.full((B * n * D + 8,), FILL, dtype=x.dtype, device=dev)
        view = full[1:1 + B * n * D].view(B, n, D)
        assert view.data_ptr() % 16 == x.element_size()
    else:
        assert layout == "chan", layout
        full = torch.full((B, D, n + 3), FILL, dtype=x.dtype, device=dev)
        view = full[:, :, :n].transpose(1, 2)
        assert view.stride(1) == 1
    view.copy_(x.to(dev))
    return view


def _quantum(t):
    """the largest power of two (<= 1) of which every entry of the fp64 tensor t is a multiple"""
    for k in range(0, 48):
        s = t * 2.0 ** k
        if torch.equal(s.round(), s):
            return 2.0 ** -k
    raise AssertionError("not dyadic")


def _guard_exact(abs_sum, q, what):
    """all terms are multiples of q and sum |terms| < 2^24 q: every partial sum of any order is an fp32 number"""
    worst = float(abs_sum.max()) / q
    assert worst * 1.02 < 2.0 ** 24, (what, worst)


def _assert_exact32(x, what):
    assert torch.equal(x.float().double(), x), f"{what}: the test's own expected value is not an fp32 number"


def _eq(got, ref, what):
    """bit-exact against the fp64 reference cast to fp32 (checked to be exact); int32 views, so that a signed zero
    would show"""
    _assert_exact32(ref, what)
    got = got.detach().cpu().contiguous()
    want = (ref.float() + 0.0).reshape(got.shape).contiguous()      # + 0.0: the reference's own -0 becomes +0
    if not torch.equal(got.view(torch.int32), want.view(torch.int32)):
        bad = (got.view(torch.int32) != want.view(torch.int32)).nonzero()
        i = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{what}: {bad.shape[0]} of {got.numel()} elements differ, first at {i}: "
                             f"got {got[i].item()!r}, want {want[i].item()!r}")


def _ratio(got, ref, denom):
    """max |got - ref| / denom over the elements with denom > 0; where denom == 0 the value must be exact"""
    got = torch.as_tensor(np.asarray(got.cpu() if torch.is_tensor(got) else got)).double().reshape(ref.shape)
    assert bool(torch.isfinite(got).all())
    err = (got - ref).abs()
    assert bool((err[denom == 0] == 0).all()), "an element with no non-zero term must be exact"
    ok = denom > 0
    return float((err[ok] / denom[ok]).max()) if bool(ok.any()) else 0.0


def _token_weights_exact(g, shape, n):
    """c / P with integers c in {floor(P / n), floor(P / n) + 1} summing to P along the last axis"""
    P = 256 if n <= 256 else 512
    base, extra = P // n, P - (P // n) * n
    c = torch.full((*shape, n), base, dtype=torch.int64)
    order = torch.rand((*shape, n), generator=g).argsort(dim=-1)
    c += (order < extra).long()
    assert bool((c.sum(-1) == P).all()) and int(c.min()) >= 1
    return (c.double() / P).float()


def _graded(g, B, n, D):
    """randn 2^e_n 2^f_d + 0.5 with integers e, f in [-3, 3]: magnitudes over 2^+-6, a common offset"""
    e = torch.randint(-3, 4, (B, n, 1), generator=g).float()
    f = torch.randint(-3, 4, (1, 1, D), generator=g).float()
    return torch.randn(B, n, D, generator=g) * torch.pow(2.0, e) * torch.pow(2.0, f) + 0.5


def _softmax_weights(g, shape):
    return torch.softmax(2.0 * torch.randn(shape, generator=g), dim=-1)


def _dyadic_mix(G, L):
    """(G, L) rows of dyadic weights summing to 1 (1/2, 1/4, ..., the last two equal), rolled by the group index"""
    if L == 1:
        return torch.ones(G, 1)
    base = [2.0 ** -(i + 1) for i in range(L - 1)]
    base.append(base[-1])
    assert sum(base) == 1.0
    return torch.stack([torch.tensor(base).roll(g) for g in range(G)]).float()


def _tap_ptrs(tp, ranges):
    if tp is None:
        return (None,) * (5 if ranges else 3)
    ptrs = (tp.tap0.data_ptr(), tp.tap1.data_ptr(), tp.lam.data_ptr())
    return ptrs + (tp.range0.data_ptr(), tp.range1.data_ptr()) if ranges else ptrs


# --------------------------------------------------------------------------- #
# student projection: cases, data, reference, bounds, GPU runner
# --------------------------------------------------------------------------- #
SP_W1, SP_W = 64, 32          # slab widths: student_project_kernel, student_project_v4_kernel (procrustes_plan.h)
FOLD1, FOLD4 = 3, 32          # adds of the row-group fold in the two kernels


def _pc(n_s, n_t, D, E=1, B=2, dtype=F32, layout="contig", shared=True, flag=None):
    return dict(n_s=n_s, n_t=n_t, D=D, E=E, B=B, dtype=dtype, layout=layout, shared=shared, flag=flag)


PROJ_CASES = {
    "n49_d96": _pc(49, 49, 96),
    "d100_tail": _pc(49, 49, 100),                            # tail slab partly outside 64 and 32
    "up196_taps": _pc(196, 49, 96),                           # taps and ranges, ratio 4
    "rows260": _pc(260, 65, 40, B=3),                         # more rows than one pass of 256 threads loads
    "e3_shared_omega": _pc(49, 49, 64, E=3),                  # omega_e_stride = 0
    "e3_own_omega": _pc(196, 49, 36, E=3, shared=False),      # omega_e_stride = B * n_s
    "bf16_up128": _pc(128, 64, 104, dtype=BF16),              # bf16 tokens, ratio 2
    "cls_rows": _pc(49, 49, 100, layout="cls", B=3),
    "padded_rows": _pc(196, 49, 52, layout="padded"),
    "d102_refused": _pc(49, 49, 102),                         # D % 4 != 0: the all-layers kernel does not apply
    "offset1_refused": _pc(196, 49, 96, layout="offset1"),    # base one element past 16-byte alignment
    "flag0_refused": _pc(49, 49, 96, flag=0),                 # ptrs_16B_aligned = 0 although the bases are aligned
}
REFUSED = {"d102_refused", "offset1_refused", "flag0_refused"}


def _project_multi_applies(flag, dtype, sb, sn, D, n_s):
    """plan::project_multi_applies of procrustes_plan.h"""
    esz = 4 if dtype == F32 else 2
    quads = D % 4 == 0 and (sb * esz) % 16 == 0 and (sn * esz) % 16 == 0 and (esz == 4 or D % 8 == 0)
    return bool(flag) and quads and 4 * (n_s * SP_W + 5 * n_s) <= 96 * 1024


@lru_cache(maxsize=None)
def _proj_data(name, kind):
    """(xs: E CPU tensors (B, n_s, D) in the case's dtype, omega (Ge, B, n_s) fp32) -- shared by the GPU tests and
    the CPU companion"""
    c = PROJ_CASES[name]
    g = _gen(list(PROJ_CASES).index(name), kind == "exact", 17)
    E, B, n_s, D = c["E"], c["B"], c["n_s"], c["D"]
    Ge = 1 if c["shared"] else E
    if kind == "exact":
        xs = [torch.randint(-8, 9, (B, n_s, D), generator=g).to(c["dtype"]) for _ in range(E)]
        omega = _token_weights_exact(g, (Ge, B), n_s)
    else:
        xs = [_graded(g, B, n_s, D).to(c["dtype"]) for _ in range(E)]
        omega = _softmax_weights(g, (Ge, B, n_s))
    return xs, omega


def _proj_ref(xs, omega, n_t):
    """fp64: mu (E, B, D), a_prime (E, B, n_t, D), per-feature trace (E, B, D), and the absolute sums of the bounds.
    relational.py:36-45 (student half) with the transpose of combined.py:9-14: A' = I^T diag(w) (X - 1 mu^T)."""
    X = torch.stack([x.double() for x in xs])
    E, B, n_s, D = X.shape
    w = omega.double().expand(E, B, n_s)
    I = _interp(n_t, n_s) if n_t != n_s else torch.eye(n_s, dtype=torch.float64)
    mu = torch.einsum("ebn,ebnd->ebd", w, X)
    Xc = X - mu[:, :, None]
    r = dict(mu=mu, ap=torch.einsum("nj,ebn,ebnd->ebjd", I, w, Xc), trd=torch.einsum("ebn,ebnd->ebd", w, Xc * Xc),
             S_mu=torch.einsum("ebn,ebnd->ebd", w, X.abs()), S_a=torch.einsum("nj,ebn,ebnd->ebjd", I, w, Xc.abs()),
             C=torch.einsum("nj,ebn->ebj", I, w), A1=torch.einsum("ebn,ebnd->ebd", w, Xc.abs()), I=I, w=w, Xc=Xc)
    return r


def _proj_guard_exact(xs, omega, n_t, r):
    """Part A's theorem for this case, asserted in fp64"""
    q_w, q_I = _quantum(omega.double()), _quantum(r["I"])
    _guard_exact(r["S_mu"], q_w, "mu")                              # terms w x: integers times q_w
    q_c = _quantum(r["Xc"])                                         # x - mu
    _guard_exact(r["S_a"], q_I * q_w * q_c, "a_prime")              # terms I w (x - mu)
    _guard_exact(r["Xc"].abs(), q_c, "x - mu")
    _assert_exact32(r["mu"], "mu")
    _assert_exact32(r["ap"], "a_prime")


def _slab_sums(t, W):
    """(E, B, D) -> (E, B, ceil(D / W)): sums over slabs of W features"""
    E, B, D = t.shape
    slabs = (D + W - 1) // W
    pad = torch.zeros(E, B, slabs * W, dtype=t.dtype)
    pad[:, :, :D] = t
    return pad.view(E, B, slabs, W).sum(-1)


def _proj_rhos(r, n_s, W, fold, mu, ap, tr):
    """{quantity: (rho, bound)} of one projection's outputs mu (E, B, D), ap (E, B, n_t, D), tr (E, B, slabs) against
    the reference r; the trace entry is |err| / bound with bound 1"""
    K_mu = n_s + fold
    e_d = K_mu * U * r["S_mu"] * SECOND_ORDER
    tr_ref = _slab_sums(r["trd"], W)
    tr_bound = U * (n_s * W + 8) * SECOND_ORDER * tr_ref + _slab_sums(2 * e_d * r["A1"] + e_d * e_d, W)
    tr = torch.as_tensor(np.asarray(tr.cpu() if torch.is_tensor(tr) else tr)).double()
    assert tr.shape == tr_ref.shape, "number of trace partials"
    fold_err = float(((tr.sum(-1) - r["trd"].sum(-1)).abs() / tr_bound.sum(-1)).max())
    return {"mu": (_ratio(mu, r["mu"], U * r["S_mu"]), K_mu * SECOND_ORDER),
            "a_prime": (_ratio(ap, r["ap"], U * (r["S_a"] + r["C"][..., None] * r["S_mu"][:, :, None])),
                        K_mu * SECOND_ORDER),
            "trace partials": (_ratio(tr, tr_ref, tr_bound), 1.0),
            "folded trace": (fold_err, 1.0)}


def _report(tag, rhos, check=True):
    line = f"rho {tag:44s}" + "".join(f"  {k} {v:.3g} (<= {b:.4g})" for k, (v, b) in rhos.items())
    print(line)
    if check:
        for k, (v, b) in rhos.items():
            assert v <= b, (tag, k, v, b)
    return line


def _run_projections(dev, name, kind):
    """Both entry points on one case: returns (per-layer outputs, all-layers outputs or None, reference)."""
    from basd_amd import _lib, ops
    c = PROJ_CASES[name]
    E, B, n_s, n_t, D = c["E"], c["B"], c["n_s"], c["n_t"], c["D"]
    xs, omega = _proj_data(name, kind)
    r = _proj_ref(xs, omega, n_t)
    if kind == "exact":
        _proj_guard_exact(xs, omega, n_t, r)
    xd = [_place3(x, c["layout"], dev) for x in xs]
    om = omega.to(dev)
    om_stride = 0 if c["shared"] else B * n_s
    tp = ops.taps(n_t, n_s, dev)
    sb, sn, sd = xd[0].stride()
    assert sd == 1
    code = ops._dtype_code(xd[0])
    s1, s4 = (D + SP_W1 - 1) // SP_W1, (D + SP_W - 1) // SP_W
    # per layer
    bufs1 = [_out(dev, E, B, D), _out(dev, E, B, s1), _out(dev, E, B, n_t, D)]
    (_, mu1), (_, tr1), (_, ap1) = bufs1
    for e in range(E):
        _lib.call("basd_student_project", xd[e].data_ptr(), code, sb, sn, B, n_s, n_t, D,
                  om.data_ptr() + 4 * e * om_stride, *_tap_ptrs(tp, True), mu1[e].data_ptr(), tr1[e].data_ptr(),
                  ap1[e].data_ptr(), ops._stream())
    torch.cuda.synchronize()
    for (buf, view), what in zip(bufs1, ("mu", "trace partials", "a_prime")):
        _check_out(buf, view, f"basd_student_project {name} {what}")
    # all layers in one launch
    flag = int(all(x.data_ptr() % 16 == 0 for x in xd)) if c["flag"] is None else c["flag"]
    applies = _project_multi_applies(flag, c["dtype"], sb, sn, D, n_s)
    assert applies == (name not in REFUSED)
    bufs4 = [_out(dev, E, B, D), _out(dev, E, B, s4), _out(dev, E, B, n_t, D)]
    (_, mu4), (_, tr4), (_, ap4) = bufs4
    status = _lib.load().basd_student_project_multi(
        ops._ptr_table(xd).data_ptr(), code, sb, sn, E, B, n_s, n_t, D, flag, om.data_ptr(), om_stride,
        *_tap_ptrs(tp, True), mu4.data_ptr(), tr4.data_ptr(), ap4.data_ptr(), ops._stream())
    torch.cuda.synchronize()
    assert status == (0 if applies else EUNSUPPORTED), status
    for (buf, view), what in zip(bufs4, ("mu", "trace partials", "a_prime")):
        _check_out(buf, view, f"basd_student_project_multi {name} {what}", written=applies)
    return (mu1, tr1, ap1), ((mu4, tr4, ap4) if applies else None), r


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PROJ_CASES))
def test_student_project_exact(dev, name):
    """Part A: basd_student_project and basd_student_project_multi on the same exact inputs: mu and a_prime bit for
    bit against fp64 and against each other; basd_student_project_multi answers BASD_EUNSUPPORTED exactly where
    plan::project_multi_applies says so and then leaves its outputs untouched, the per-layer kernel stays exact."""
    one, four, r = _run_projections(dev, name, "exact")
    _eq(one[0], r["mu"], f"basd_student_project {name} mu")
    _eq(one[2], r["ap"], f"basd_student_project {name} a_prime")
    if four is not None:
        _eq(four[0], r["mu"], f"basd_student_project_multi {name} mu")
        _eq(four[2], r["ap"], f"basd_student_project_multi {name} a_prime")
        assert torch.equal(one[0], four[0]) and torch.equal(one[2], four[2])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PROJ_CASES))
def test_student_project_bounds(dev, name):
    """Part B: mu, a_prime, the per-slab trace partials (64 features per layer, 32 in the all-layers kernel:
    plan::trace_slabs) and their fold, under the bounds of the module docstring."""
    n_s = PROJ_CASES[name]["n_s"]
    one, four, r = _run_projections(dev, name, "graded")
    _report(f"gpu  basd_student_project {name}", _proj_rhos(r, n_s, SP_W1, FOLD1, *[one[i] for i in (0, 2, 1)]))
    if four is not None:
        _report(f"gpu  basd_student_project_multi {name}",
                _proj_rhos(r, n_s, SP_W, FOLD4, *[four[i] for i in (0, 2, 1)]))


# --------------------------------------------------------------------------- #
# teacher centring: cases, data, reference, bounds, GPU runner
# --------------------------------------------------------------------------- #
TCS_ROWS, TCM_G = 16, 4       # procrustes_plan.h


def _cc(n_t, n, D, L=3, G=2, B=2, dtype=F32, layout="contig", tc_off=0):
    return dict(n_t=n_t, n=n, D=D, L=L, G=G, B=B, dtype=dtype, layout=layout, tc_off=tc_off)


CEN_CASES = {
    "l1": _cc(49, 49, 64, L=1, G=1),
    "l3_g2": _cc(49, 49, 64),
    "g4_limit": _cc(49, 49, 32, G=4),
    "l5_g2": _cc(49, 49, 64, L=5, B=3),                        # the four-layers-at-a-time loop and its remainder
    "cls_d100": _cc(49, 49, 100, layout="cls"),                # row layout with a CLS row, tail of the 64- and 16-wide slabs
    "chan_d50": _cc(49, 49, 50, layout="chan", B=3),           # channel-major (sn == 1), D % 4 != 0
    "gather256": _cc(256, 64, 64),                             # gathered 256 -> 64 (lam = 1/2)
    "gather96_d50": _cc(96, 64, 50, layout="cls"),             # gathered 96 -> 64 (lam = 1/4, 3/4)
    "n33_d68": _cc(33, 33, 68, L=2),                           # three 16-row chunks, the last one partial
    "bf16_cls": _cc(49, 49, 100, dtype=BF16, layout="cls"),
    "offset1_base": _cc(49, 49, 64, layout="offset1"),         # v4 planned, misaligned bases: scalar loop inside it
    "tc_misaligned": _cc(49, 49, 64, tc_off=1),                # output off 16-byte alignment: the scalar stream form
}


def _stream_v4_applies(dtype, gathered, sb, sn, D, tc_ptr, scratch_ptr):
    """plan::stream_v4_applies of procrustes_plan.h"""
    return (dtype == F32 and not gathered and D % 4 == 0 and sb % 4 == 0 and sn % 4 == 0 and tc_ptr % 16 == 0
            and scratch_ptr % 16 == 0)


@lru_cache(maxsize=None)
def _cen_data(name, kind):
    """(xs: L CPU tensors (B, n_t, D), mix (G, L) fp32, omega_t (G, B, n) fp32)"""
    c = CEN_CASES[name]
    g = _gen(list(CEN_CASES).index(name), kind == "exact", 29)
    L, G, B, n_t, n, D = c["L"], c["G"], c["B"], c["n_t"], c["n"], c["D"]
    if kind == "exact":
        xs = [torch.randint(-8, 9, (B, n_t, D), generator=g).to(c["dtype"]) for _ in range(L)]
        return xs, _dyadic_mix(G, L), _token_weights_exact(g, (G, B), n)
    xs = [_graded(g, B, n_t, D).to(c["dtype"]) for _ in range(L)]
    mix = torch.softmax(torch.randn(G, L, generator=g), dim=-1) if L > 1 else torch.ones(G, 1)
    return xs, mix, _softmax_weights(g, (G, B, n))


def _cen_ref(xs, mix, omega_t, n):
    """fp64: layer_selector.py:110-111 (mix), combined.py:9-14 (gather to n tokens where the teacher grid is finer),
    relational.py:37,39 (weighted centring); omega_t may be given in fp64."""
    X = torch.stack([x.double() for x in xs])                   # (L, B, n_t, D)
    n_t = X.shape[2]
    I = _interp(n_t, n) if n_t != n else torch.eye(n, dtype=torch.float64)
    m, w = mix.double(), omega_t.double()
    v = torch.einsum("gl,jr,lbrd->gbjd", m, I, X)
    S_v = torch.einsum("gl,jr,lbrd->gbjd", m.abs(), I, X.abs())
    mu = torch.einsum("gbj,gbjd->gbd", w, v)
    return dict(v=v, mu=mu, tc=v - mu[:, :, None], S_v=S_v, S_mu=torch.einsum("gbj,gbjd->gbd", w, S_v), w=w, I=I, m=m)


def _cen_guard_exact(r):
    q_v = _quantum(r["m"]) * _quantum(r["I"])                     # tokens are integers
    _guard_exact(r["S_v"], q_v, "mixed tokens")
    q_w = _quantum(r["w"])
    _guard_exact(r["S_mu"], q_v * q_w, "weighted mean")
    _guard_exact(r["S_v"] + r["S_mu"][:, :, None], q_v * q_w, "centred tokens")
    _assert_exact32(r["mu"], "mu")
    _assert_exact32(r["tc"], "tc")


def _cen_K(n, L):
    return n + (n + TCS_ROWS - 1) // TCS_ROWS + L + 2


def _cen_rhos(r, n, L, mu, tc, extra=0):
    """{quantity: (rho, bound)} for mu (G, B, D) and tc (G, B, n, D); extra: roundings of omega_t itself where the
    reference was given a more exact omega_t than the kernel (the composed call)"""
    K = _cen_K(n, L) + extra
    S_tc = r["S_v"] + r["S_mu"][:, :, None]
    tcd = torch.as_tensor(np.asarray(tc.cpu() if torch.is_tensor(tc) else tc)).double().reshape(r["tc"].shape)
    adj = torch.einsum("gbj,gbjd->gbd", r["w"], tcd).abs()
    adj_bound = (r["mu"].abs() * (1.0 - r["w"].sum(-1)).abs()[..., None]
                 + torch.einsum("gbj,gbjd->gbd", r["w"], (K + 1) * U * SECOND_ORDER * S_tc))
    out = {"tc": (_ratio(tc, r["tc"], U * S_tc), (K + 1) * SECOND_ORDER),
           "|sum omega_t tc|": (float((adj / adj_bound).max()), 1.0)}
    if mu is not None:
        out = {"mu": (_ratio(mu, r["mu"], U * r["S_mu"]), K * SECOND_ORDER), **out}
    return out


def _run_centrings(dev, name, kind):
    """Every form that applies to the case: {form: (mu, tc)} and the reference."""
    from basd_amd import _lib, ops
    c = CEN_CASES[name]
    L, G, B, n_t, n, D = c["L"], c["G"], c["B"], c["n_t"], c["n"], c["D"]
    xs, mix, omega_t = _cen_data(name, kind)
    r = _cen_ref(xs, mix, omega_t, n)
    if kind == "exact":
        _cen_guard_exact(r)
    xd = [_place3(x, c["layout"], dev) for x in xs]
    tab = ops._ptr_table(xd).data_ptr()
    code = ops._dtype_code(xd[0])
    sb, sn, sd = xd[0].stride()
    gt = ops.taps(n_t, n, dev)
    mixd, wt = mix.to(dev), omega_t.to(dev)
    got = {}

    def outputs():
        return _out(dev, G, B, D), _out(dev, G, B, n, D, off=c["tc_off"])

    def checked(form, bufs):
        torch.cuda.synchronize()
        for (buf, view), what in zip(bufs, ("mu", "tc")):
            _check_out(buf, view, f"{form} {name} {what}")
        got[form] = (bufs[0][1], bufs[1][1])

    bufs = outputs()
    for k in range(G):
        _lib.call("basd_teacher_center", tab, code, mixd[k].data_ptr(), L, sb, sn, sd, B, n, D, *_tap_ptrs(gt, False),
                  wt[k].data_ptr(), bufs[0][1][k].data_ptr(), bufs[1][1][k].data_ptr(), ops._stream())
    checked("basd_teacher_center", bufs)
    bufs = outputs()
    _lib.call("basd_teacher_center_multi", tab, code, mixd.data_ptr(), L, G, sb, sn, sd, B, n, D, *_tap_ptrs(gt, False),
              wt.data_ptr(), bufs[0][1].data_ptr(), bufs[1][1].data_ptr(), ops._stream())
    checked("basd_teacher_center_multi", bufs)
    bufs = outputs()
    floats = _lib.query("basd_teacher_center_stream_scratch_floats", G, B, n, D)
    assert floats == (n + TCS_ROWS - 1) // TCS_ROWS * G * B * D
    sbuf, scratch = _out(dev, floats)
    status = _lib.load().basd_teacher_center_stream(tab, code, mixd.data_ptr(), L, G, sb, sn, sd, B, n, D,
                                                    *_tap_ptrs(gt, False), wt.data_ptr(), bufs[0][1].data_ptr(),
                                                    bufs[1][1].data_ptr(), scratch.data_ptr(), ops._stream())
    if sd != 1:
        torch.cuda.synchronize()
        assert status == EUNSUPPORTED, status
        for (buf, view) in (*bufs, (sbuf, scratch)):
            _check_out(buf, view, f"basd_teacher_center_stream {name}", written=False)
    else:
        assert status == 0, status
        v4 = _stream_v4_applies(c["dtype"], gt is not None, sb, sn, D, bufs[1][1].data_ptr(), scratch.data_ptr())
        assert v4 == (name in STREAM_V4_CASES), "which stream form the case reaches"
        checked("basd_teacher_center_stream" + (" (v4)" if v4 else " (scalar)"), bufs)
        _check_out(sbuf, scratch, f"basd_teacher_center_stream {name} scratch")
    return got, r


# the cases on which plan::stream_v4_applies holds (fp32, own grid, quads, aligned outputs); on offset1_base the v4
# kernel then finds misaligned layer bases and takes its scalar loop
STREAM_V4_CASES = {"l1", "l3_g2", "g4_limit", "l5_g2", "cls_d100", "n33_d68", "offset1_base"}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CEN_CASES))
def test_teacher_center_exact(dev, name):
    """Part A: basd_teacher_center (once per group), basd_teacher_center_multi and basd_teacher_center_stream (the
    four-features-per-thread form and the scalar form, as plan::stream_v4_applies separates them) bit for bit against
    fp64: mu and tc.  The stream form refuses channel-major tokens (sd != 1) and leaves its outputs alone."""
    got, r = _run_centrings(dev, name, "exact")
    assert len(got) == (2 if CEN_CASES[name]["layout"] == "chan" else 3)
    for form, (mu, tc) in got.items():
        _eq(mu, r["mu"], f"{form} {name} mu")
        _eq(tc, r["tc"], f"{form} {name} tc")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CEN_CASES))
def test_teacher_center_bounds(dev, name):
    """Part B: mu, tc and the vanishing adjoint |sum_j omega_t[j] tc[j, :]| of every centring form."""
    c = CEN_CASES[name]
    got, r = _run_centrings(dev, name, "graded")
    for form, (mu, tc) in got.items():
        _report(f"gpu  {form} {name}", _cen_rhos(r, c["n"], c["L"], mu, tc))


@pytest.mark.gpu
def test_teacher_center_refuses_five_groups(dev):
    """G = 5 is past TCM_G = 4: the multi and the stream form answer BASD_EUNSUPPORTED and write nothing."""
    from basd_amd import _lib, ops
    G, L, B, n, D = 5, 2, 2, 33, 32
    g = _gen(5, 5)
    xd = [torch.randn(B, n, D, generator=g).to(dev) for _ in range(L)]
    tab, code = ops._ptr_table(xd).data_ptr(), ops._dtype_code(xd[0])
    sb, sn, sd = xd[0].stride()
    mix = torch.softmax(torch.randn(G, L, generator=g), -1).to(dev)
    wt = _softmax_weights(g, (G, B, n)).to(dev)
    bufs = [_out(dev, G, B, D), _out(dev, G, B, n, D), _out(dev, 3 * G * B * D)]
    (_, mu), (_, tc), (_, scratch) = bufs
    lib = _lib.load()
    assert lib.basd_teacher_center_multi(tab, code, mix.data_ptr(), L, G, sb, sn, sd, B, n, D, None, None, None,
                                         wt.data_ptr(), mu.data_ptr(), tc.data_ptr(), ops._stream()) == EUNSUPPORTED
    assert lib.basd_teacher_center_stream(tab, code, mix.data_ptr(), L, G, sb, sn, sd, B, n, D, None, None, None,
                                          wt.data_ptr(), mu.data_ptr(), tc.data_ptr(), scratch.data_ptr(),
                                          ops._stream()) == EUNSUPPORTED
    torch.cuda.synchronize()
    for buf, view in bufs:
        _check_out(buf, view, "G = 5", written=False)


# --------------------------------------------------------------------------- #
# Part A: stack products of integer factors
# --------------------------------------------------------------------------- #
STACK_LDS_LIMIT = 78 * 1024                                     # basd_stack_product: `lds <= 78 * 1024` bytes
STACK_LDS_MAX_N = math.isqrt(STACK_LDS_LIMIT // 16)             # two n x n fp64 factors: n <= 70 in LDS, 71 is tiled


def _int_factors(g, batch, n):
    """lower-triangular factors of integers in [-3, 3] with a positive diagonal, zeros above (as basd_chol_f64
    leaves them)"""
    L = torch.randint(-3, 4, (batch, n, n), generator=g).double().tril(-1)
    return L + torch.diag_embed(torch.randint(1, 4, (batch, n), generator=g).double())


@pytest.mark.gpu
@pytest.mark.parametrize("n,batch,period,pad", [(49, 3, 3, 0), (STACK_LDS_MAX_N, 2, 2, 0), (STACK_LDS_MAX_N + 1, 2, 2, 0),
                                                (98, 2, 2, 0), (99, 2, 2, 0), (130, 2, 2, 0), (49, 6, 2, 8),
                                                (99, 6, 2, 8)])
def test_stack_product_exact(dev, n, batch, period, pad):
    """basd_stack_product: W[b] = [L_a^T L_b ; L_b] column-major (2n x n), bit for bit.  The launcher takes the LDS
    kernel while both fp64 factors fit STACK_LDS_LIMIT = 78 KB, i.e. up to n = 70, and the tiled kernel from n = 71
    (49, 70 | 71, 98, 99, 130: three and five tiles a side, ragged last tiles); batch 6 with lb_period 2 (one teacher
    factor for three layers) and a padded w_batch_stride, on both kernels."""
    from basd_amd import _lib, ops
    assert STACK_LDS_MAX_N == 70
    g = _gen(n, batch, period)
    la, lb = _int_factors(g, batch, n), _int_factors(g, period, n)
    m = la.transpose(1, 2) @ lb[torch.arange(batch) % period]
    stride = 2 * n * n + pad
    buf, w = _out(dev, batch, stride)
    la_d, lb_d = la.to(dev), lb.to(dev)
    _lib.call("basd_stack_product", la_d.data_ptr(), lb_d.data_ptr(), n * n, n, batch, period, w.data_ptr(), stride,
              ops._stream())
    torch.cuda.synchronize()
    flat = buf.cpu()
    assert bool((flat[:GUARD] == FILL).all()) and bool((flat[GUARD + batch * stride:] == FILL).all())
    w = w.cpu()
    assert bool((w[:, 2 * n * n:] == FILL).all()), "the padding between two cores was written"
    cores = w[:, :2 * n * n].reshape(batch, n, 2 * n)               # column j of the core = row j of this view
    assert bool((cores != FILL).all())
    _eq(cores[:, :, :n], m.transpose(1, 2), f"top half L_a^T L_b, n = {n}")
    _eq(cores[:, :, n:], lb[torch.arange(batch) % period].transpose(1, 2), f"bottom half L_b, n = {n}")


@pytest.mark.gpu
@pytest.mark.parametrize("n,batch,period", [(31, 2, 2), (32, 2, 2), (33, 2, 2), (70, 6, 2)])
def test_stack_product_t_and_stash_exact(dev, n, batch, period):
    """basd_stack_product_t: M = L_a^T L_b compact and row-major, bit for bit (one tile, exactly one, two, three with
    a ragged last one); basd_ustack_stash behind it: the bottom half of w_stack holds M row-major, the top half is
    untouched."""
    from basd_amd import _lib, ops
    g = _gen(n, batch, period, 1)
    la, lb = _int_factors(g, batch, n), _int_factors(g, period, n)
    m = la.transpose(1, 2) @ lb[torch.arange(batch) % period]
    stride = 2 * n * n
    buf, w = _out(dev, batch, stride)
    la_d, lb_d = la.to(dev), lb.to(dev)
    _lib.call("basd_stack_product_t", la_d.data_ptr(), lb_d.data_ptr(), n * n, n, batch, period, w.data_ptr(), stride,
              ops._stream())
    sbuf, ws = _out(dev, batch, stride + 4)
    _lib.call("basd_ustack_stash", w.data_ptr(), stride, n, batch, ws.data_ptr(), stride + 4, ops._stream())
    torch.cuda.synchronize()
    flat = buf.cpu()
    assert bool((flat[:GUARD] == FILL).all()) and bool((flat[GUARD + batch * stride:] == FILL).all())
    w = w.cpu()
    assert bool((w[:, n * n:] == FILL).all()), "basd_stack_product_t wrote past its compact n x n"
    _eq(w[:, :n * n].reshape(batch, n, n), m, f"M row-major, n = {n}")
    flat = sbuf.cpu()
    assert bool((flat[:GUARD] == FILL).all()) and bool((flat[GUARD + batch * (stride + 4):] == FILL).all())
    ws = ws.cpu()
    assert bool((ws[:, stride:] == FILL).all())
    halves = ws[:, :stride].reshape(batch, n, 2 * n)
    assert bool((halves[:, :, :n] == FILL).all()), "basd_ustack_stash touched the top half"
    _eq(halves[:, :, n:], m, f"stashed M, n = {n}")


# --------------------------------------------------------------------------- #
# Part B: token weights
# --------------------------------------------------------------------------- #
def _tw(has_cls, H, L, dtype, n_a, n_t, n_s, strided=False, raw=True, B=2):
    return dict(has_cls=has_cls, H=H, L=L, dtype=dtype, n_a=n_a, n_t=n_t, n_s=n_s, strided=strided, raw=raw, B=B)


# n_t is the core grid the call is given (min of the token grids, as basd_procrustes_forward_fused passes it)
TW_CASES = {
    "cls_h3_l3_49": _tw(True, 3, 3, F32, 49, 49, 49),
    "nocls_h1_l1_49": _tw(False, 1, 1, F32, 49, 49, 49),
    "nocls_h3_l3_bf16_up196": _tw(False, 3, 3, BF16, 49, 49, 196, strided=True),     # weights up, omega_t folded back
    "cls_h3_l1_bf16_down64": _tw(True, 3, 1, BF16, 256, 64, 64),                     # n_a = n_t = 256 -> n_s = 64
    "nocls_a196_h1_aligned49": _tw(False, 1, 3, F32, 196, 49, 49),                   # aligned tokens, raw attention
    "cls_up324_strided": _tw(True, 1, 3, F32, 81, 81, 324, strided=True),            # more than one pass of 256 threads
    "cls_h3_l3_49_no_raw": _tw(True, 3, 3, F32, 49, 49, 49, raw=False),
    "nocls_h3_l1_a64_up128": _tw(False, 3, 1, F32, 64, 64, 128, B=3),
}


@lru_cache(maxsize=None)
def _tw_data(name):
    c = TW_CASES[name]
    g = _gen(list(TW_CASES).index(name), 41)
    A = c["n_a"] + int(c["has_cls"])
    attns = [torch.softmax(2.0 * torch.randn(c["B"], c["H"], A, A, generator=g), dim=-1).to(c["dtype"])
             for _ in range(c["L"])]
    mix = torch.softmax(torch.randn(c["L"], generator=g), dim=-1) if c["L"] > 1 else torch.ones(1)
    return attns, mix


def _tw_ref(attns, mix, has_cls, n_a, n_t, n_s):
    """fp64: layer_selector.py:112 (mixed attention), relational.py:22-34 (weights, interpolation, normalisation);
    omega_t = I_tok^T omega is the fold that lets the teacher side use the weights on its own grid."""
    mixed = sum(m * a.double() for m, a in zip(mix.double(), attns))
    raw = mixed[:, :, 0, 1:].mean(dim=1) if has_cls else mixed.mean(dim=(1, 2))
    v = raw @ _interp(n_a, n_s).t() if n_a != n_s else raw
    omega = v / v.sum(dim=-1, keepdim=True)
    I_tok = _interp(n_t, n_s) if n_t != n_s else None
    return raw, omega, (omega @ I_tok if I_tok is not None else omega), I_tok


def _tw_K(c):
    A_q = 1 if c["has_cls"] else c["n_a"]
    K_raw = c["L"] + c["H"] * A_q + 2
    K_v = K_raw + (2 if c["n_a"] != c["n_s"] else 0)
    K_om = c["n_s"] + 2 * K_v + 1
    K_fold = 2 * _max_range(c["n_t"], c["n_s"]) + 1 if c["n_t"] != c["n_s"] else 0
    return K_raw, K_om, K_fold


def _tw_rhos(c, ref, raw, omega, omega_t):
    raw_ref, om_ref, omt_ref, I_tok = ref
    K_raw, K_om, K_fold = _tw_K(c)
    om64 = omega.double().cpu()
    omt64 = omega_t.double().cpu()
    own = om64 @ I_tok if I_tok is not None else om64
    out = {"omega": (_ratio(omega, om_ref, U * om_ref), K_om * SECOND_ORDER),
           "omega_t": (_ratio(omega_t, omt_ref, U * omt_ref), (K_om + K_fold) * SECOND_ORDER),
           "omega_t vs I^T omega": (_ratio(omega_t, own, U * own), K_fold * SECOND_ORDER),
           "|sum omega - 1|/u": (float((om64.sum(-1) - 1).abs().max()) / U, (c["n_s"] + 2) * SECOND_ORDER),
           "|sum omega_t - 1|/u": (float((omt64.sum(-1) - 1).abs().max()) / U,
                                   (c["n_s"] + 2 + K_fold) * SECOND_ORDER)}
    if raw is not None:
        out = {"raw": (_ratio(raw, raw_ref, U * raw_ref), K_raw * SECOND_ORDER), **out}
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TW_CASES))
def test_token_weights_bounds(dev, name):
    """Part B: basd_token_weights -- raw_out, omega, omega_t element by element, the two normalisations, and omega_t
    against I^T omega, under the bounds of the module docstring (all terms are positive: S is the value itself)."""
    from basd_amd import _lib, ops
    c = TW_CASES[name]
    B, H, L, n_a, n_t, n_s = c["B"], c["H"], c["L"], c["n_a"], c["n_t"], c["n_s"]
    A = n_a + int(c["has_cls"])
    attns, mix = _tw_data(name)
    ref = _tw_ref(attns, mix, c["has_cls"], n_a, n_t, n_s)
    if c["strided"]:        # a view of a larger buffer: the rows and matrices around it hold FILL
        ad = []
        for a in attns:
            full = torch.full((B, H + 1, A + 2, A + 3), FILL, dtype=a.dtype, device=dev)
            view = full[:, 1:, 1:A + 1, 2:A + 2]
            view.copy_(a.to(dev))
            ad.append(view)
    else:
        ad = [a.to(dev) for a in attns]
    atp, tp = ops.taps(n_a, n_s, dev), ops.taps(n_t, n_s, dev)
    bufs = [_out(dev, B, n_s), _out(dev, B, n_t), _out(dev, B, n_a)]
    (_, omega), (_, omega_t), (_, raw) = bufs
    mix_d = mix.to(dev)
    _lib.call("basd_token_weights", ops._ptr_table(ad).data_ptr(), ops._dtype_code(ad[0]), mix_d.data_ptr(), L,
              *ad[0].stride(), B, H, A, int(c["has_cls"]), n_a, n_t, n_s, *_tap_ptrs(atp, False), *_tap_ptrs(tp, False),
              omega.data_ptr(), omega_t.data_ptr(), raw.data_ptr() if c["raw"] else None, ops._stream())
    torch.cuda.synchronize()
    for (buf, view), what in zip(bufs, ("omega", "omega_t", "raw_out")):
        _check_out(buf, view, f"basd_token_weights {name} {what}", written=c["raw"] or what != "raw_out")
    _report(f"gpu  basd_token_weights {name}", _tw_rhos(c, ref, raw if c["raw"] else None, omega, omega_t))


# --------------------------------------------------------------------------- #
# Part B: the split fp64 Gram
# --------------------------------------------------------------------------- #
@pytest.mark.gpu
@pytest.mark.parametrize("n,D,splits", [(49, 100, 2), (49, 272, 3), (196, 100, 3), (196, 272, 2)])
def test_gram_f64_split_bounds(dev, n, D, splits):
    """basd_gram_f64_split against basd_gram_f64 and against fp64 at feature counts that are no multiple of
    splits x 32: relative 1e-14 (the figure of test_gram_chol_f64), element by element rho <= D + splits with
    u = 2^-53, and identical bits from two calls (the partial Grams are folded in a fixed order)."""
    from basd_amd import _lib, ops
    batch = 2
    p = _graded(_gen(n, D, splits), batch, n, D)
    ref = p.double() @ p.double().transpose(1, 2)
    S = p.double().abs() @ p.double().abs().transpose(1, 2)
    pd = p.to(dev)
    outs = []
    for _ in range(2):
        gbuf, G = _out(dev, batch, n, n, dtype=torch.float64)
        sbuf, slabs = _out(dev, splits, batch, n, n, dtype=torch.float64)
        _lib.call("basd_gram_f64_split", pd.data_ptr(), n * D, n, D, batch, splits, slabs.data_ptr(), G.data_ptr(),
                  ops._stream())
        torch.cuda.synchronize()
        _check_out(gbuf, G, "basd_gram_f64_split G")
        _check_out(sbuf, slabs, "basd_gram_f64_split slabs")
        outs.append(G.cpu())
    assert torch.equal(outs[0].view(torch.int64), outs[1].view(torch.int64)), "two calls differ: the fold order is not fixed"
    assert torch.equal(outs[0], outs[0].transpose(1, 2))
    gbuf, G1 = _out(dev, batch, n, n, dtype=torch.float64)
    _lib.call("basd_gram_f64", pd.data_ptr(), n * D, n, D, batch, G1.data_ptr(), n * n, ops._stream())
    torch.cuda.synchronize()
    _check_out(gbuf, G1, "basd_gram_f64 G")
    rel = float((outs[0] - ref).norm() / ref.norm())
    rel1 = float((G1.cpu() - ref).norm() / ref.norm())
    rel_each = float((outs[0] - G1.cpu()).norm() / ref.norm())
    print(f"rel  basd_gram_f64_split n={n} D={D} splits={splits}: {rel:.2e}  unsplit {rel1:.2e}  split vs unsplit {rel_each:.2e}")
    assert rel < 1e-14 and rel1 < 1e-14 and rel_each < 1e-14
    _report(f"gpu  basd_gram_f64 n={n} D={D} splits={splits}",
            {"split (u = 2^-53)": (_ratio(outs[0], ref, U64 * S), (D + splits) * SECOND_ORDER),
             "unsplit (u = 2^-53)": (_ratio(G1, ref, U64 * S), D * SECOND_ORDER)})


# --------------------------------------------------------------------------- #
# Part C: CPU companion -- the kernels' arithmetic in numpy fp32, with and without each mutation
# --------------------------------------------------------------------------- #
MUTATIONS = ["tap1_last", "lam_swap", "drop_group", "skip_last_feature", "mean_1_over_n", "range1_short"]
CENTER_MUTATIONS = ["tap1_last", "lam_swap", "skip_last_feature", "mean_1_over_n"]    # no row groups, no ranges there


def _f32(x):
    return np.asarray(x, dtype=np.float32)


def _fma(a, b, c):
    """a b + c with one rounding of the fp64 value (the product of two fp32 numbers is exact in fp64)"""
    return (_f32(a).astype(np.float64) * _f32(b).astype(np.float64) + _f32(c).astype(np.float64)).astype(np.float32)


def _emulate_project(x, w, tp, n_t, v4, mut=None):
    """student_project_kernel (v4 = False: 4 row groups, fold (r0 + r1) + (r2 + r3), slabs of 64) or
    student_project_v4_kernel (32 row groups folded one after the other, slabs of 32, the coefficients (1 - lam) w
    and lam w rounded on their own) for one layer: x (B, n_s, D), w (B, n_s) fp32 numpy.  Outputs start as FILL, as
    on the GPU.  The block sum of the trace is taken in fp64 and rounded once."""
    B, n_s, D = x.shape
    RG, W = (32, SP_W) if v4 else (4, SP_W1)
    live = np.ones(D, dtype=bool)
    if mut == "skip_last_feature":
        live[D - 1] = False
    groups = RG - 1 if mut == "drop_group" else RG
    wm = np.full_like(w, np.float32(1.0) / np.float32(n_s)) if mut == "mean_1_over_n" else w
    zero = np.zeros((B, D), dtype=np.float32)
    red = []
    for rg in range(RG):
        acc = zero
        if rg < groups:
            for n in range(rg, n_s, RG):
                acc = _fma(wm[:, n, None], x[:, n], acc)
        red.append(acc)
    if v4:
        m = zero
        for q in range(RG):
            m = m + red[q]
    else:
        m = (red[0] + red[1]) + (red[2] + red[3])
    mu = np.full((B, D), FILL, dtype=np.float32)
    mu[:, live] = m[:, live]
    part = np.zeros((B, D), dtype=np.float64)
    for rg in range(groups):
        acc = zero
        for n in range(rg, n_s, RG):
            cc = x[:, n] - m
            acc = _fma(w[:, n, None] * cc, cc, acc)
        part += acc
    part[:, ~live] = 0
    slabs = (D + W - 1) // W
    tr = np.stack([part[:, s * W:(s + 1) * W].sum(-1) for s in range(slabs)], axis=-1).astype(np.float32)
    ap = np.full((B, n_t, D), FILL, dtype=np.float32)
    if tp is not None:
        t0, t1, lam, r0, r1 = tp
        t1 = t1.copy()
        if mut == "tap1_last":
            t1[n_s - 1] -= 1
        l1, l0 = lam, np.float32(1.0) - lam
        if mut == "lam_swap":
            l0, l1 = l1, l0
    for j in range(n_t):
        if j % RG >= groups:
            continue
        n0, n1 = (int(r0[j]), int(r1[j])) if tp is not None else (j, j + 1)
        if tp is not None and mut == "range1_short":
            n1 -= 1
        a = zero
        for n in range(n0, n1):
            if tp is None:
                cw = w[:, n]
            elif v4:
                cw = (l0[n] * w[:, n] if t0[n] == j else 0 * w[:, n]) + (l1[n] * w[:, n] if t1[n] == j else 0 * w[:, n])
            else:
                coef = (l0[n] if t0[n] == j else np.float32(0)) + (l1[n] if t1[n] == j else np.float32(0))
                cw = coef * w[:, n]
            a = _fma(_f32(cw)[:, None], x[:, n] - m, a)
        ap[:, j][:, live] = a[:, live]
    return mu, ap, tr


def _emulate_center(xs, mix, wt, gt, n, mut=None):
    """teacher_center_kernel for one group: xs (L, B, n_t, D), mix (L,), wt (B, n) fp32 numpy"""
    L, B, n_t, D = xs.shape
    live = np.ones(D, dtype=bool)
    if mut == "skip_last_feature":
        live[D - 1] = False
    zero = np.zeros((B, D), dtype=np.float32)
    tile = np.zeros((B, n, D), dtype=np.float32)
    if gt is not None:
        g0, g1, lam = gt[0], gt[1].copy(), gt[2]
        if mut == "tap1_last":
            g1[n - 1] -= 1
        l1, l0 = lam, np.float32(1.0) - lam
        if mut == "lam_swap":
            l0, l1 = l1, l0
    for j in range(n):
        if gt is None:
            v = zero
            for l in range(L):
                v = _fma(mix[l], xs[l][:, j], v)
        else:
            a0 = a1 = zero
            for l in range(L):
                a0 = _fma(mix[l], xs[l][:, g0[j]], a0)
                a1 = _fma(mix[l], xs[l][:, g1[j]], a1)
            v = l0[j] * a0 + l1[j] * a1
        tile[:, j] = v
    wm = np.full_like(wt, np.float32(1.0) / np.float32(n)) if mut == "mean_1_over_n" else wt
    acc = zero
    for j in range(n):
        acc = _fma(wm[:, j, None], tile[:, j], acc)
    mu = np.full((B, D), FILL, dtype=np.float32)
    tc = np.full((B, n, D), FILL, dtype=np.float32)
    mu[:, live] = acc[:, live]
    tc[:, :, live] = (tile - acc[:, None])[:, :, live]
    return mu, tc


def _emulated_projection(name, kind, v4, mut=None):
    c = PROJ_CASES[name]
    xs, omega = _proj_data(name, kind)
    tp = _taps_np(c["n_t"], c["n_s"]) if c["n_t"] != c["n_s"] else None
    outs = [_emulate_project(x.float().numpy(), omega[0 if c["shared"] else e].numpy(), tp, c["n_t"], v4, mut)
            for e, x in enumerate(xs)]
    return [np.stack([o[i] for o in outs]) for i in range(3)]


def _emulated_centring(name, kind, mut=None):
    c = CEN_CASES[name]
    xs, mix, omega_t = _cen_data(name, kind)
    gt = _taps_np(c["n_t"], c["n"]) if c["n_t"] != c["n"] else None
    X = np.stack([x.float().numpy() for x in xs])
    outs = [_emulate_center(X, mix[k].numpy(), omega_t[k].numpy(), gt, c["n"], mut) for k in range(c["G"])]
    return [np.stack([o[i] for o in outs]) for i in range(2)]


def _same_bits(got, ref):
    want = ref.float().numpy()
    return got.shape == want.shape and bool(np.array_equal(got, want))


@lru_cache(maxsize=None)
def _proj_ref_of(name, kind):
    xs, omega = _proj_data(name, kind)
    return _proj_ref(xs, omega, PROJ_CASES[name]["n_t"])


@lru_cache(maxsize=None)
def _cen_ref_of(name, kind):
    xs, mix, omega_t = _cen_data(name, kind)
    return _cen_ref(xs, mix, omega_t, CEN_CASES[name]["n"])


@pytest.mark.parametrize("v4", [False, True], ids=["per_layer", "all_layers"])
@pytest.mark.parametrize("name", list(PROJ_CASES))
def test_emulated_projection_exact_and_bounded(name, v4):
    """(a) the emulation of both student projections is bit-exact on Part A's data and within Part B's bounds on
    Part B's data (every case, also those the all-layers kernel refuses on the GPU: the arithmetic is the same)."""
    n_s = PROJ_CASES[name]["n_s"]
    r = _proj_ref_of(name, "exact")
    _proj_guard_exact(*_proj_data(name, "exact"), PROJ_CASES[name]["n_t"], r)
    mu, ap, _ = _emulated_projection(name, "exact", v4)
    assert _same_bits(mu, r["mu"]) and _same_bits(ap, r["ap"])
    mu, ap, tr = _emulated_projection(name, "graded", v4)
    W, fold = (SP_W, FOLD4) if v4 else (SP_W1, FOLD1)
    _report(f"emul student_project{'_v4' if v4 else ''} {name}", _proj_rhos(_proj_ref_of(name, "graded"), n_s, W, fold, mu, ap, tr))


@pytest.mark.parametrize("name", list(CEN_CASES))
def test_emulated_centring_exact_and_bounded(name):
    """(a) the emulation of teacher_center_kernel is bit-exact on Part A's data and within Part B's bounds."""
    c = CEN_CASES[name]
    r = _cen_ref_of(name, "exact")
    _cen_guard_exact(r)
    mu, tc = _emulated_centring(name, "exact")
    assert _same_bits(mu, r["mu"]) and _same_bits(tc, r["tc"])
    mu, tc = _emulated_centring(name, "graded")
    _report(f"emul teacher_center {name}", _cen_rhos(_cen_ref_of(name, "graded"), c["n"], c["L"], mu, tc))


def _worst(rhos, keys):
    return max(rhos[k][0] / rhos[k][1] for k in keys)


MUTATION_PAIRS = ([(k, m) for k in ("per_layer", "all_layers") for m in MUTATIONS]
                  + [("centring", m) for m in CENTER_MUTATIONS])


@pytest.mark.parametrize("kernel,mut", MUTATION_PAIRS)
def test_every_mutation_is_caught(kernel, mut):
    """(b) a kernel with this mistake breaks Part A's equality and exceeds Part B's bounds (on mu or a_prime / tc
    alone: the trace is not even needed) on at least one case -- so the GPU tests above would fail on it.  No
    deliberately wrong kernel ever runs on the GPU."""
    if kernel == "centring":
        broke, worst = [], {}
        for name, c in CEN_CASES.items():
            r = _cen_ref_of(name, "exact")
            mu, tc = _emulated_centring(name, "exact", mut)
            if not (_same_bits(mu, r["mu"]) and _same_bits(tc, r["tc"])):
                broke.append(name)
            mu, tc = _emulated_centring(name, "graded", mut)
            worst[name] = _worst(_cen_rhos(_cen_ref_of(name, "graded"), c["n"], c["L"], mu, tc), ("mu", "tc"))
    else:
        v4 = kernel == "all_layers"
        W, fold = (SP_W, FOLD4) if v4 else (SP_W1, FOLD1)
        broke, worst = [], {}
        for name, c in PROJ_CASES.items():
            r = _proj_ref_of(name, "exact")
            mu, ap, _ = _emulated_projection(name, "exact", v4, mut)
            if not (_same_bits(mu, r["mu"]) and _same_bits(ap, r["ap"])):
                broke.append(name)
            mu, ap, tr = _emulated_projection(name, "graded", v4, mut)
            worst[name] = _worst(_proj_rhos(_proj_ref_of(name, "graded"), c["n_s"], W, fold, mu, ap, tr), ("mu", "a_prime"))
    over = {k: v for k, v in worst.items() if v > 1.0}
    print(f"mutation {mut:18s} {kernel:10s}: Part A broken on {len(broke)} cases, Part B exceeded on {len(over)} cases, "
          f"by a factor of {min(over.values(), default=0):.3g} .. {max(over.values(), default=0):.3g}")
    assert broke, f"{mut}: Part A's data do not catch it"
    assert over, f"{mut}: Part B's data do not catch it"


# --------------------------------------------------------------------------- #
# Part C: the composed call -- every centre x projection route of basd_procrustes_forward_fused
# --------------------------------------------------------------------------- #
CENTER_STREAM_V4, CENTER_STREAM, CENTER_MULTI, CENTER_PER_GROUP = 1, 2, 3, 4      # plan::Center
PROJECT_MULTI, PROJECT_PER_LAYER = 1, 2                                            # plan::Project

def _co(E, L, n_s, d_s, n_t, d_t, H, has_cls, centre, project, split, s_dtype=F32, t_dtype=F32, B=2):
    return dict(E=E, L=L, B=B, n_s=n_s, d_s=d_s, n_t=n_t, d_t=d_t, H=H, has_cls=has_cls, centre=centre, project=project,
                split=split, s_dtype=s_dtype, t_dtype=t_dtype)


COMPOSED = {
    "per_group_multi_split": _co(2, 1, 49, 64, 49, 512, 2, True, CENTER_PER_GROUP, PROJECT_MULTI, 1),
    # bf16 students with d_s % 8 != 0: their rows are no 16-byte quads, the projection goes layer by layer
    "multi_per_layer_up196": _co(2, 2, 196, 52, 49, 64, 2, False, CENTER_MULTI, PROJECT_PER_LAYER, 0, s_dtype=BF16),
    "stream_v4_multi": _co(3, 4, 49, 64, 49, 64, 2, True, CENTER_STREAM_V4, PROJECT_MULTI, 0),
    "stream_gather_bf16": _co(2, 4, 64, 48, 256, 64, 1, True, CENTER_STREAM, PROJECT_MULTI, 0, t_dtype=BF16),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(COMPOSED))
def test_composed_call_intermediates(dev, name):
    """ops.procrustes_forward on small shapes, one per centre x projection route that basd_procrustes_plan_query
    reports (the route is asserted from the plan's fields): the context's own omega, mu_s, a_prime, tr_s and the tc of
    `mixgrad` against fp64 under Part B's bounds -- each stage's reference starts from the fp32 values that the call
    itself handed to that stage (omega as the call left it).  This is the check that fused.hip gives each kernel the
    right strides, group (mix + g L, omega + e stride) and scratch (the stream centring borrows W).  tr_s is the fp32
    fold of the partials: `slabs` further roundings.  tc: omega_t is not kept, the reference folds the call's omega
    in fp64, which adds the fold's 2 r + 1 roundings to K_t."""
    from basd_amd import ops
    c = COMPOSED[name]
    E, L, B, n_s, d_s, n_t, d_t, H, has_cls = (c[k] for k in ("E", "L", "B", "n_s", "d_s", "n_t", "d_t", "H", "has_cls"))
    centre, project, split = c["centre"], c["project"], c["split"]
    g = _gen(list(COMPOSED).index(name), 53)
    n = min(n_s, n_t)
    A = n_t + int(has_cls)
    students = [_graded(g, B, n_s, d_s).to(c["s_dtype"]) for _ in range(E)]
    teachers = [_graded(g, B, n_t, d_t).to(c["t_dtype"]) for _ in range(L)]
    attns = [torch.softmax(2.0 * torch.randn(B, H, A, A, generator=g), dim=-1) for _ in range(L)]
    mix = torch.softmax(torch.randn(E, L, generator=g), dim=-1)
    ctx = ops.procrustes_forward([s.to(dev) for s in students], [t.to(dev) for t in teachers],
                                 [a.to(dev) for a in attns], mix.to(dev), has_cls, need_backward=True, need_mix_grad=True)
    torch.cuda.synchronize()
    route = ctx.mixgrad["route"]
    assert (route["center"], route["project"], route["gram_split"]) == (centre, project, split), route
    W = route["slab_width"]
    assert W == (SP_W if project == PROJECT_MULTI else SP_W1) and route["slabs"] == (d_s + W - 1) // W
    G = 1 if L == 1 else E
    assert ctx.omega.shape == (G, B, n_s)
    # token weights, per group
    tw = dict(has_cls=has_cls, H=H, L=L, n_a=n_t, n_t=n, n_s=n_s)
    for k in range(G):
        ref = _tw_ref(attns, mix[k], has_cls, n_t, n, n_s)
        rhos = _tw_rhos(tw, ref, ctx.mixgrad["raw"][k], ctx.omega[k], ref[2].float())
        _report(f"gpu  composed {name} group {k}", {q: rhos[q] for q in ("raw", "omega", "|sum omega - 1|/u")})
    # student side, from the call's own omega
    omega = ctx.omega.cpu()
    r = _proj_ref(students, omega, n)
    fold = FOLD4 if project == PROJECT_MULTI else FOLD1
    K_mu = n_s + fold
    e_d = K_mu * U * r["S_mu"] * SECOND_ORDER
    tr_ref = r["trd"].sum(-1)
    tr_bound = (U * (n_s * W + 8 + route["slabs"]) * SECOND_ORDER * tr_ref + (2 * e_d * r["A1"] + e_d * e_d).sum(-1))
    _report(f"gpu  composed {name} student side",
            {"mu_s": (_ratio(ctx.mu_s, r["mu"], U * r["S_mu"]), K_mu * SECOND_ORDER),
             "a_prime": (_ratio(ctx.a_prime, r["ap"], U * (r["S_a"] + r["C"][..., None] * r["S_mu"][:, :, None])),
                         K_mu * SECOND_ORDER),
             "tr_s": (_ratio(ctx.tr_s, tr_ref, tr_bound), 1.0)})
    # teacher side: omega_t = I^T omega of the call's omega, in fp64
    I_tok = _interp(n, n_s) if n != n_s else None
    omega_t = omega.double() @ I_tok if I_tok is not None else omega.double()
    extra = 2 * _max_range(n, n_s) + 1 if I_tok is not None else 0
    rt = _cen_ref(teachers, mix if L > 1 else torch.ones(1, 1), omega_t, n)
    _report(f"gpu  composed {name} teacher side", _cen_rhos(rt, n, L, None, ctx.mixgrad["tc"], extra=extra))


def test_cases_reach_every_form():
    """The case tables themselves (no GPU): both stream forms and both sides of every dispatch are present."""
    assert STREAM_V4_CASES < set(CEN_CASES)
    rows = {k for k, c in CEN_CASES.items() if c["layout"] != "chan"}
    assert rows - STREAM_V4_CASES >= {"gather256", "bf16_cls", "tc_misaligned"}       # the scalar stream form
    assert any(c["G"] == TCM_G for c in CEN_CASES.values())
    assert any(c["n"] > 2 * TCS_ROWS and c["n"] % TCS_ROWS for c in CEN_CASES.values())
    assert {c["dtype"] for c in PROJ_CASES.values()} == {F32, BF16}
    assert any(c["n_s"] > 256 for c in PROJ_CASES.values()) and any(c["n_s"] > 256 for c in TW_CASES.values())
    assert any(c["D"] % SP_W1 and c["D"] % SP_W for c in PROJ_CASES.values())
    assert {c["centre"] for c in COMPOSED.values()} == {CENTER_STREAM_V4, CENTER_STREAM, CENTER_MULTI, CENTER_PER_GROUP}
    assert {c["project"] for c in COMPOSED.values()} == {PROJECT_MULTI, PROJECT_PER_LAYER}
    assert {c["split"] for c in COMPOSED.values()} == {0, 1}
