"""``basd_procrustes_finish_transposed`` (``procrustes_finish_t_kernel``): the per-sample terms and K' behind the Jacobi
of the transposed route in one launch.  Its arithmetic is that of ``basd_procrustes_finalize`` (null ``k_prime``) +
``basd_kprime_from_transposed`` operation for operation, so every comparison here is on the bits (int32 views)."""
import numpy as np
import pytest
import torch

from basd_amd import _lib

OLD_KERNELS = ("procrustes_finalize_kernel", "kprime_z_kernel", "kprime_from_z_kernel")
NEW_KERNEL = "procrustes_finish_t_kernel"
BATCH, PERIOD = 8, 2


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32)


def _inputs(n: int, n_s: int, dev, batch: int = BATCH):
    """Seeded CPU inputs in the layout of the fused call: W (batch, 2 n n) with X compact in the first half, sigma
    positive and descending, L_b the fp64 Cholesky factor of a random SPD G, per-slab partial traces."""
    from basd_amd import ops
    rng = np.random.default_rng(1000 * n + n_s)
    nn = n * n
    W = rng.standard_normal((batch, 2 * nn)).astype(np.float32)
    sigma = np.sort(rng.uniform(0.05, 3.0, (batch, n)).astype(np.float32), axis=1)[:, ::-1].copy()
    thr = sigma[:, 0] * np.float32(n) * np.float32(1.1920929e-7)            # the kernels' fp32 expression
    if n >= 4:
        sigma[2, -3:] = 0.0                                                  # truncated: exactly zero
        sigma[5, -3:] = thr[5] * np.array([0.999, 0.99, 0.5], np.float32)    # truncated: just under thr
        sigma[6, -3:] = [np.nextafter(thr[6], np.float32(1)), thr[6], np.nextafter(thr[6], np.float32(0))]   # above, at, below
    A = rng.standard_normal((PERIOD, n, n + 3))
    G = A @ A.transpose(0, 2, 1) + 0.1 * np.eye(n)
    Lb = np.linalg.cholesky(G)
    omega = rng.uniform(0.1, 1.0, (PERIOD, n_s)).astype(np.float32)
    omega /= omega.sum(1, keepdims=True)
    slabs = 3
    tr_part = rng.uniform(0.0, 5.0, (batch, slabs)).astype(np.float32)
    tp = ops.taps(n, n_s, dev)                                               # the loss's own resampling tables
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return dict(W=t(W), sigma=t(sigma), G=t(G), Lb=t(Lb), omega=t(omega), tr_part=t(tr_part), slabs=slabs, tp=tp)


def _outputs(n: int, dev, batch: int = BATCH, fill: float = float("nan")):
    return dict(k=torch.full((batch, n, n), fill, device=dev), tr_s=torch.full((batch,), fill, device=dev),
                tr_t=torch.full((batch,), fill, device=dev), nuc=torch.full((batch,), fill, device=dev),
                loss=torch.full((batch,), fill, device=dev))


def _taps_ptrs(tp):
    return (tp.tap0.data_ptr(), tp.tap1.data_ptr(), tp.lam.data_ptr()) if tp is not None else (None, None, None)


def _old_pair(i, o, n, n_s, stream):
    nn = n * n
    batch = i["sigma"].shape[0]
    z = torch.empty((batch, nn), device=i["W"].device)
    _lib.call("basd_procrustes_finalize", i["W"].data_ptr(), 2 * nn, i["sigma"].data_ptr(), n, n_s, batch, PERIOD,
              i["G"].data_ptr(), nn, i["omega"].data_ptr(), *_taps_ptrs(i["tp"]), i["tr_part"].data_ptr(), i["slabs"],
              o["tr_s"].data_ptr(), o["tr_t"].data_ptr(), o["nuc"].data_ptr(), o["loss"].data_ptr(), None, stream)
    _lib.call("basd_kprime_from_transposed", i["W"].data_ptr(), 2 * nn, i["sigma"].data_ptr(), n, batch,
              i["Lb"].data_ptr(), nn, PERIOD, z.data_ptr(), nn, o["k"].data_ptr(), stream)


def _new_status(i, o, n, n_s, stream, batch=None):
    nn = n * n
    batch = batch or i["sigma"].shape[0]
    return _lib.load().basd_procrustes_finish_transposed(
        i["W"].data_ptr(), 2 * nn, i["sigma"].data_ptr(), n, n_s, batch, PERIOD, i["G"].data_ptr(), nn,
        i["omega"].data_ptr(), *_taps_ptrs(i["tp"]), i["tr_part"].data_ptr(), i["slabs"], o["tr_s"].data_ptr(),
        o["tr_t"].data_ptr(), o["nuc"].data_ptr(), o["loss"].data_ptr(), i["Lb"].data_ptr(), nn, PERIOD,
        o["k"].data_ptr(), stream)


# one tile, the exact tile edge, one element past it, the workload's odd order, the limit
@pytest.mark.gpu
@pytest.mark.parametrize("interp", [False, True], ids=["same_grid", "taps"])
@pytest.mark.parametrize("n", [7, 32, 33, 49, 64])
def test_bit_identical_to_the_kept_entry_points(dev, n, interp):
    """Test A: K', tr_s, tr_t, nuc and loss_b of the one-launch kernel equal, bit for bit, those of
    basd_procrustes_finalize (null k_prime) + basd_kprime_from_transposed on the same buffers; batch members 2, 5 and 6
    have singular values that are zero, just under and around the truncation threshold."""
    from basd_amd import ops
    n_s = 2 * n - 1 if interp else n
    i = _inputs(n, n_s, dev)
    assert (i["tp"] is not None) == interp
    old, new = _outputs(n, dev), _outputs(n, dev)
    _old_pair(i, old, n, n_s, ops._stream())
    assert _new_status(i, new, n, n_s, ops._stream()) == 0
    torch.cuda.synchronize()
    for name in ("k", "tr_s", "tr_t", "nuc", "loss"):
        assert torch.isfinite(old[name]).all() and torch.isfinite(new[name]).all(), name      # every element written
        diff = (_bits(old[name]) != _bits(new[name])).sum().item()
        print(f"[finish] n={n} n_s={n_s} {name}: {diff} of {old[name].numel()} words differ")
        assert diff == 0, (name, diff)
    # the truncation branch was taken: the truncated columns contribute nothing, the others do
    assert (new["k"][2] != 0).any() and (new["k"][5] != 0).any()


@pytest.mark.gpu
def test_unsupported_shapes_launch_nothing(dev):
    """n = 65 and batch > 65535 return BASD_EUNSUPPORTED and leave the (sentinel-filled) outputs untouched."""
    from basd_amd import ops
    n = 65
    i = _inputs(n, n, dev)
    out = _outputs(n, dev, fill=-7.0)
    assert _new_status(i, out, n, n, ops._stream()) == _lib.EUNSUPPORTED
    i = _inputs(49, 49, dev)
    out49 = _outputs(49, dev, fill=-7.0)
    assert _new_status(i, out49, 49, 49, ops._stream(), batch=65536) == _lib.EUNSUPPORTED
    torch.cuda.synchronize()
    for o in (out, out49):
        for name, t in o.items():
            assert (t == -7.0).all(), name


E, B, N_TOK, D_S, D_T = 2, 64, 49, 64, 96        # E B = 128: the transposed route without forcing it


def _fused_call(dev):
    from basd_amd import ops, synth
    g = torch.Generator().manual_seed(49)
    students = [synth.structured(g, B, N_TOK, D_S, 16).to(dev) for _ in range(E)]
    t = synth.structured(g, B, N_TOK, D_T, 12).to(dev)
    attn = torch.softmax(torch.randn(B, 2, N_TOK, N_TOK, generator=g), dim=-1).to(dev)
    mix = torch.ones(E, 1, device=dev)
    ce = torch.tensor([1.25], device=dev)
    return lambda: ops.procrustes_forward(students, [t], [attn], mix, False, uwso_ce=ce)


@pytest.mark.gpu
def test_fused_call_is_bit_identical_either_way(dev):
    """Test B: basd_procrustes_forward_fused with basd_procrustes_finish_tuning(1) and (0): loss_b, k_prime, uw_out and
    dx are bit-equal."""
    run = _fused_call(dev)
    prev = _lib.query("basd_procrustes_finish_tuning", -1)
    assert prev == 1                                                    # the default is on
    out = {}
    try:
        for mode in (1, 0):
            _lib.query("basd_procrustes_finish_tuning", mode)
            assert _lib.query("basd_procrustes_finish_tuning", -1) == mode
            out[mode] = run()
            torch.cuda.synchronize()
    finally:
        _lib.query("basd_procrustes_finish_tuning", prev)
    a, b = out[1], out[0]
    for name in ("loss_b", "k_prime", "uw", "dx", "tr_s", "tr_t", "nuc"):
        x, y = getattr(a, name), getattr(b, name)
        assert x.data_ptr() != y.data_ptr() and torch.isfinite(x).all(), name
        diff = (_bits(x) != _bits(y)).sum().item()
        print(f"[finish] fused call {name}: {diff} of {x.numel()} words differ")
        assert diff == 0, (name, diff)


@pytest.mark.gpu
def test_launch_names(dev):
    """Test C: under torch.profiler the call shows procrustes_finish_t_kernel exactly once and none of the three kernels
    it stands in for; with the setting at 0, those three once each and not the new one."""
    from torch.profiler import ProfilerActivity, profile
    run = _fused_call(dev)
    prev = _lib.query("basd_procrustes_finish_tuning", -1)
    counts = {}
    try:
        for mode in (1, 0):
            _lib.query("basd_procrustes_finish_tuning", mode)
            run()                                                       # warm-up: plan, code objects
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                run()
                torch.cuda.synchronize()
            names = [e.name for e in prof.events() if "cuda" in str(e.device_type).lower()]
            counts[mode] = {k: sum(k in nm for nm in names) for k in OLD_KERNELS + (NEW_KERNEL,)}
            print(f"[finish] setting {mode}: {counts[mode]} among {len(names)} device events")
    finally:
        _lib.query("basd_procrustes_finish_tuning", prev)
    assert counts[1] == {**{k: 0 for k in OLD_KERNELS}, NEW_KERNEL: 1}, counts[1]
    assert counts[0] == {**{k: 1 for k in OLD_KERNELS}, NEW_KERNEL: 0}, counts[0]
