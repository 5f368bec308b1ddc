"""Global-norm clipping and the non-finite guard of ``basd_amd.optim.AdamWScheduleFree`` (``basd_grad_sqnorm`` and
``basd_sfadamw_step_clipped`` in ``csrc/optim.hip``), up to ``Trainer``.

What the figures are held against:

* the norm: the squares of fp32 values are exact in fp64 and non-negative, so ANY order of ``n`` fp64 additions is within
  ``n 2^-53`` relative of the exact sum.  The small cases compare with ``math.fsum`` (exactly rounded), the large one with
  numpy's pairwise fp64 sum (itself within that bound, hence ``2 n 2^-53``);
* the coefficient: ``min(1, m / (norm + 1e-6))`` restated here in fp64 (and held against ``clip_grad_norm_`` on the CPU),
  one fp32 ulp for the kernel's single rounding plus the last bits of its fp64 ``sqrt`` and division;
* the update: bit-identical to the existing one-launch step given ``fl32(grad_scale * coef)`` -- no tolerance at all."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn

from basd_amd import _lib
from basd_amd.optim import AdamWScheduleFree, schedule

GROUP_KEYS = {"lr", "betas", "eps", "r", "k", "warmup_steps", "train_mode", "weight_sum", "lr_max", "scheduled_lr",
              "weight_lr_power", "weight_decay", "foreach"}
CHUNK = 4096


# ---------------------------------------------------------------------------------------------------------------------
# the restatement (fp64, plain Python / numpy)
# ---------------------------------------------------------------------------------------------------------------------
def _exact_sqsum(grads) -> float:
    """The exactly rounded sum of the exact squares of every element of every gradient that is not ``None``."""
    terms = []
    for g in grads:
        if g is not None:
            x = g.detach().cpu().double().flatten().numpy()
            terms.append(x * x)                                   # 24-bit x 24-bit significands: exact in fp64
    return math.fsum(np.concatenate(terms).tolist())


def _restated(norm_sq: float, max_norm, grad_scale: float = 1.0):
    """``(norm, coef)`` of the header's formula in fp64."""
    norm = abs(grad_scale) * math.sqrt(norm_sq)
    coef = 1.0 if max_norm is None else min(1.0, max_norm / (norm + 1e-6))
    return norm, coef


def _ulp32(x: float) -> float:
    return float(np.spacing(np.float32(x)))


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [0, 0.0, -1.0, float("inf"), float("-inf"), float("nan")])
def test_max_grad_norm_is_validated(bad):
    p = nn.Parameter(torch.zeros(3))
    with pytest.raises(ValueError, match="max_grad_norm"):
        AdamWScheduleFree([p], max_grad_norm=bad)
    opt = AdamWScheduleFree([p], max_grad_norm=2.5, skip_nonfinite=True)
    assert opt.max_grad_norm == 2.5 and opt.skip_nonfinite is True
    p.grad = torch.zeros(3)
    opt.train()
    with pytest.raises(ValueError, match="max_grad_norm"):          # the per-call override is checked the same way
        opt.step(max_grad_norm=bad)
    assert opt.param_groups[0]["k"] == 0
    with pytest.raises(TypeError):                                   # keyword-only
        AdamWScheduleFree([p], 0.0025, (0.9, 0.999), 1e-8, 0, 0, 0.0, 2.0, True, False, 1.0, 1.0)


def test_groups_and_state_dict_are_unchanged_by_the_switches():
    params = [nn.Parameter(torch.randn(5)), nn.Parameter(torch.randn(2, 3))]
    opt = AdamWScheduleFree(params[:1], lr=2e-3, max_grad_norm=1.0, skip_nonfinite=True)
    opt.add_param_group({"params": params[1:], "weight_decay": 0.0})
    plain = AdamWScheduleFree([nn.Parameter(p.detach().clone()) for p in params[:1]], lr=2e-3)
    plain.add_param_group({"params": [nn.Parameter(p.detach().clone()) for p in params[1:]], "weight_decay": 0.0})
    for g in opt.param_groups:
        assert set(g) == GROUP_KEYS | {"params"}
    sd, sd_plain = opt.state_dict(), plain.state_dict()
    assert sd["param_groups"] == sd_plain["param_groups"]
    assert sorted(sd["state"]) == [0, 1] and all(set(sd["state"][i]) == {"z", "exp_avg_sq"} for i in (0, 1))
    fresh = AdamWScheduleFree([nn.Parameter(torch.zeros(5))])
    fresh.add_param_group({"params": [nn.Parameter(torch.zeros(2, 3))]})
    fresh.load_state_dict(sd)                       # a checkpoint of a guarded optimizer loads into a plain one
    assert fresh.max_grad_norm is None and fresh.skip_nonfinite is False and fresh.skipped_steps() == 0


def test_trainer_refuses_the_switches_without_the_schedulefree_optimizer():
    from basd_amd.trainer import Trainer
    for kw in (dict(max_grad_norm=1.0), dict(skip_nonfinite=True)):
        with pytest.raises(ValueError, match="optimizer='schedulefree'"):
            Trainer(nn.Linear(2, 2), None, None, student_info={}, optimizer="adamw", **kw)


def test_restatement_against_clip_grad_norm():
    g = torch.Generator().manual_seed(7)
    shapes = [(1,), (3,), (17, 5), (4097,), (64, 33)]
    for scale, max_norm in ((1.0, 1.0), (1e-3, 1.0), (30.0, 0.01), (1.0, 1e6)):
        grads32 = [(scale * torch.randn(s, generator=g)).float() for s in shapes]
        params = [nn.Parameter(torch.zeros(s, dtype=torch.float64)) for s in shapes]
        for p, x in zip(params, grads32):
            p.grad = x.double().clone()
        total = float(torch.nn.utils.clip_grad_norm_(params, max_norm))
        norm, coef = _restated(_exact_sqsum(grads32), max_norm)
        assert abs(norm - total) <= 1e-12 * total, (norm, total)
        for p, x in zip(params, grads32):
            want = x.double() * coef
            assert float((p.grad - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert _restated(4.0, None) == (2.0, 1.0) and _restated(4.0, 1.0, grad_scale=0.5)[0] == 1.0


def test_parts_query_is_a_pure_function_of_the_chunk_count():
    parts = [_lib.query("basd_grad_sqnorm_parts", n) for n in (0, 1, 2, 1023, 1024, 1025, 5384, 2 ** 30)]
    assert parts == [1, 1, 2, 1023, 1024, 1024, 1024, 1024]


# ---------------------------------------------------------------------------------------------------------------------
# GPU: helpers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _norm_sq(opt) -> float:
    return float(opt._verdict[0].item())                # BasdGradVerdict.norm_sq


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b) -> bool:
    return all(torch.equal(_bits(s), _bits(t)) for s, t in zip(a, b))


def _state(opt, params):
    return ([p.detach().clone() for p in params], [opt.state[p]["z"].clone() for p in params],
            [opt.state[p]["exp_avg_sq"].clone() for p in params])


def _views(dev, numels, first_offset=1):
    """Gradients as views of one flat buffer, back to back from ``first_offset``: with the sizes used here the views
    start at element offsets of every residue mod 4."""
    flat = torch.zeros(first_offset + sum(numels) + 3, device=dev)
    out, off = [], first_offset
    for n in numels:
        out.append(flat[off:off + n])
        off += n
    return flat, out


def _norm_step(dev, grads, max_norm=1.0, **kw):
    """One guarded step over zero parameters with the given gradients (``None`` = no gradient); returns the optimizer."""
    params = [nn.Parameter(torch.zeros(1 if g is None else g.numel(), device=dev)) for g in grads]
    for p, g in zip(params, grads):
        p.grad = g
    opt = AdamWScheduleFree(params, lr=1e-3)
    opt.train()
    opt.step(max_grad_norm=max_norm, **kw)
    return opt


def _check_norm(name, opt, grads, n, factor=1.0):
    want = _exact_sqsum(grads)
    got = _norm_sq(opt)
    bound = factor * n * 2.0 ** -53
    rel = abs(got - want) / want
    print(f"[grad_clip] {name}: norm_sq {got!r} exact {want!r} rel {rel:.3e} bound {bound:.3e}")
    assert rel <= bound, (name, got, want, rel, bound)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the norm
# ---------------------------------------------------------------------------------------------------------------------
SIZES = [1, 3, 4, 5, 4095, 4096, 4097, 2 * CHUNK + 7]


@pytest.mark.gpu
def test_norm_of_odd_sized_tensors_and_a_missing_gradient(dev):
    assert _lib.query("basd_sfadamw_chunk") == CHUNK
    g = torch.Generator().manual_seed(1)
    grads = [(torch.randn(n, generator=g) * torch.exp(2.0 * torch.randn(n, generator=g))).to(dev) for n in SIZES]
    grads.insert(3, None)
    n = sum(SIZES)
    opt = _norm_step(dev, grads, skip_nonfinite=True)
    _check_norm("odd sizes", opt, grads, n)
    first = (_norm_sq(opt), float(opt.last_grad_norm()), float(opt.last_clip_coef()))
    opt.step(max_grad_norm=1.0, skip_nonfinite=True)                 # the same buffers again: the same bits
    assert (_norm_sq(opt), float(opt.last_grad_norm()), float(opt.last_clip_coef())) == first
    norm, coef = _restated(_exact_sqsum(grads), 1.0)
    assert abs(first[1] - norm) <= _ulp32(norm) and opt.skipped_steps() == 0
    assert opt.last_grad_norm().dtype == torch.float32 and opt.last_grad_norm().dim() == 0
    assert opt.last_grad_norm().device.type == "cuda" and opt.last_clip_coef().dtype == torch.float32


@pytest.mark.gpu
def test_norm_of_300_single_elements(dev):
    g = torch.Generator().manual_seed(2)
    grads = [torch.randn(1, generator=g).to(dev) for _ in range(300)]
    _check_norm("300 x 1", _norm_step(dev, grads), grads, 300)


@pytest.mark.gpu
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_norm_of_views_at_every_element_offset(dev, offset):
    sizes = [5, 4097, 3, 2 * CHUNK + 7, 4, 4096]
    flat, views = _views(dev, sizes, first_offset=offset)
    flat.copy_(torch.randn(flat.numel(), generator=torch.Generator().manual_seed(3 + offset)))
    assert views[0].data_ptr() % 16 == 4 * offset
    assert len({v.data_ptr() % 16 for v in views}) == 3              # this offset and the next two
    _check_norm(f"views from offset {offset}", _norm_step(dev, views), views, sum(sizes))


@pytest.mark.gpu
def test_norm_past_the_cap_on_the_partials(dev):
    n = 2049 * CHUNK + 1                                # 2050 chunks: more than 1024 partials and more than the step's grid
    assert _lib.query("basd_grad_sqnorm_parts", 2050) == 1024
    x = torch.randn(n, generator=torch.Generator().manual_seed(4))
    grad = x.to(dev)
    opt = _norm_step(dev, [grad])
    x64 = x.numpy().astype(np.float64)
    want = float(np.sum(x64 * x64))                     # pairwise fp64: itself within n 2^-53 of the exact sum
    got = _norm_sq(opt)
    rel, bound = abs(got - want) / want, 2.0 * n * 2.0 ** -53
    print(f"[grad_clip] 2049 x 4096 + 1: norm_sq {got!r} numpy {want!r} rel {rel:.3e} bound {bound:.3e}")
    assert rel <= bound
    opt.step(max_grad_norm=1.0)
    assert _norm_sq(opt) == got                         # same buffer, same bits


@pytest.mark.gpu
def test_norm_needs_fp64_at_both_ends_of_the_fp32_range(dev):
    # 3e38 squared overflows fp32: an fp32 accumulator would say inf and the guard would skip a finite gradient
    # (max_norm = 1e3 keeps the coefficient a normal fp32 number: 1e3 / 3e38 and 1e3 / (64 x 3e38))
    one = [torch.full((1,), 3e38, device=dev)]
    opt = _norm_step(dev, one, max_norm=1e3, skip_nonfinite=True)
    assert float(opt.last_grad_norm()) == float(np.float32(3e38)) and opt.skipped_steps() == 0
    many = [torch.full((n,), 3e38, device=dev) for n in (5, 4097)]
    opt = _norm_step(dev, many, max_norm=1e3, skip_nonfinite=True)
    _check_norm("3e38", opt, many, 5 + 4097)
    assert math.isfinite(_norm_sq(opt)) and opt.skipped_steps() == 0 and int(opt.last_step_skipped()) == 0
    # the update ran and stayed finite (``norm`` = 3e38 sqrt(4102) is past fp32 and reads inf; ``norm_sq`` decides)
    assert float(opt.last_clip_coef()) > 0.0
    assert all(bool(torch.isfinite(p).all()) and bool((p != 0).all()) for g in opt.param_groups for p in g["params"])
    # 1e-30 squared underflows fp32: an fp32 accumulator would say 0
    tiny = [torch.full((n,), 1e-30, device=dev) for n in (5, 4097)]
    opt = _norm_step(dev, tiny)
    _check_norm("1e-30", opt, tiny, 5 + 4097)
    assert float(opt.last_grad_norm()) > 0.0 and float(opt.last_clip_coef()) == 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("grad_scale", [1.0, 0.125])
def test_coefficient_against_the_restatement(dev, grad_scale):
    g = torch.Generator().manual_seed(5)
    grads = [torch.randn(n, generator=g).to(dev) for n in SIZES]
    norm = _restated(_exact_sqsum(grads), None, grad_scale)[0]
    for max_norm in (10.0 * norm, norm, 1e-4 * norm):               # above, at and far below the norm
        opt = _norm_step(dev, [t.clone() for t in grads], max_norm=max_norm, grad_scale=grad_scale)
        want_norm, want = _restated(_exact_sqsum(grads), max_norm, grad_scale)
        got, got_norm = float(opt.last_clip_coef()), float(opt.last_grad_norm())
        print(f"[grad_clip] max_norm {max_norm:.6g} grad_scale {grad_scale}: coef {got!r} restated {want!r}; "
              f"norm {got_norm!r} restated {want_norm!r}")
        assert abs(got - want) <= _ulp32(want) and abs(got_norm - want_norm) <= _ulp32(want_norm)
        assert got == 1.0 if max_norm > norm else got <= 1.0
        assert max_norm > 1e-3 * norm or got < 1e-3


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the update
# ---------------------------------------------------------------------------------------------------------------------
NUMELS = [5, 4097, 3, 2 * CHUNK + 7, 4, 4096, 1]
GROUPS = [(dict(lr=1e-3, weight_decay=0.05, warmup_steps=3), [0, 2, 3, 5]),
          (dict(lr=3e-3, weight_decay=0.0, warmup_steps=3), [1, 4, 6])]


def _gradients(step, seed=200):
    g = torch.Generator().manual_seed(seed + step)
    return [torch.randn(n, generator=g) * torch.exp(torch.randn(n, generator=g)) for n in NUMELS]


def _twin(dev, layout, **kw):
    """``(optimizer, params, grads)``: seeded parameters in two groups; ``layout`` "own": every gradient its own
    (aligned) tensor, "views": views of one flat buffer from element offset 1."""
    g = torch.Generator().manual_seed(0)
    params = [nn.Parameter((2.0 * torch.randn(n, generator=g)).to(dev)) for n in NUMELS]
    opt = AdamWScheduleFree([params[i] for i in GROUPS[0][1]], **GROUPS[0][0], **kw)
    opt.add_param_group({"params": [params[i] for i in GROUPS[1][1]], **GROUPS[1][0]})
    if layout == "views":
        _, grads = _views(dev, NUMELS)
        assert any(v.data_ptr() % 16 for v in grads)
    else:
        grads = [torch.zeros(n, device=dev) for n in NUMELS]
        assert not any(v.data_ptr() % 16 for v in grads)
    for p, v in zip(params, grads):
        p.grad = v
    opt.train()
    return opt, params, grads


def _load(grads, step):
    for v, x in zip(grads, _gradients(step)):
        v.copy_(x)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["own", "views"])
@pytest.mark.parametrize("grad_scale", [1.0, 0.125])
def test_clipped_update_is_the_plain_update_with_the_scaled_grad_scale(dev, layout, grad_scale):
    zero = layout == "views"
    a, pa, ga = _twin(dev, layout, zero_grad_in_step=zero, grad_scale=grad_scale, max_grad_norm=1.0)
    b, pb, gb = _twin(dev, layout, zero_grad_in_step=zero)
    coefs = []
    for s in range(5):
        _load(ga, s)
        _load(gb, s)
        a.step()
        coef = np.float32(float(a.last_clip_coef()))
        coefs.append(float(coef))
        b.step(grad_scale=float(np.float32(grad_scale) * coef))          # fl32(grad_scale * coef)
        for name, x, y in zip(("y", "z", "exp_avg_sq"), _state(a, pa), _state(b, pb)):
            assert _same_bits(x, y), f"step {s}: {name} differs"
        assert _same_bits(ga, gb)
        assert all(bool((v == 0).all()) for v in ga) == zero
    assert all(0.0 < c < 1.0 for c in coefs), coefs                        # every step was clipped
    assert a.table_uploads == 1 and a.skipped_steps() == 0
    assert [g["k"] for g in a.param_groups] == [5, 5]


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["own", "views"])
def test_a_far_bound_changes_no_byte(dev, layout):
    a, pa, ga = _twin(dev, layout, zero_grad_in_step=True, grad_scale=0.125)
    b, pb, gb = _twin(dev, layout, zero_grad_in_step=True, grad_scale=0.125)
    for s in range(4):
        _load(ga, s)
        _load(gb, s)
        a.step(max_grad_norm=1e30, skip_nonfinite=True)
        b.step()
        assert float(a.last_clip_coef()) == 1.0
    for x, y in zip(_state(a, pa), _state(b, pb)):
        assert _same_bits(x, y)
    assert _same_bits(ga, gb) and not any(bool(v.any()) for v in ga)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the guard
# ---------------------------------------------------------------------------------------------------------------------
POISON = {"inf at the end of an odd-sized tensor": ("own", 1, NUMELS[1] - 1, float("inf")),      # 4097 elements, group 1
          "nan in a misaligned view": ("views", 3, 4100, float("nan")),                          # second chunk, group 0
          "-inf in the second group": ("own", 4, 2, float("-inf"))}


@pytest.mark.gpu
@pytest.mark.parametrize("zero", [True, False])
@pytest.mark.parametrize("case", list(POISON))
def test_a_nonfinite_step_is_skipped_on_the_device(dev, case, zero):
    layout, tensor, index, value = POISON[case]
    assert NUMELS[1] % 4 != 0 and 4 in GROUPS[1][1]
    a, pa, ga = _twin(dev, layout, zero_grad_in_step=zero, skip_nonfinite=True)
    b, pb, gb = _twin(dev, layout, zero_grad_in_step=zero)
    if layout == "views":
        assert ga[tensor].data_ptr() % 16 != 0
    _load(ga, 0)
    _load(gb, 0)
    a.step()
    b.step()
    before = _state(a, pa)
    _load(ga, 1)
    ga[tensor][index] = value
    poisoned = [v.clone() for v in ga]
    a.step()
    assert int(a.last_step_skipped()) == 1 and a.skipped_steps() == 1
    assert not math.isfinite(float(a.last_grad_norm()))
    for name, x, y in zip(("y", "z", "exp_avg_sq"), _state(a, pa), before):
        assert _same_bits(x, y), f"{name} moved in a skipped step"
    if zero:
        assert not any(bool(v.any()) for v in ga), "a skipped step must still clear the gradients"
    else:
        assert _same_bits(ga, poisoned)
    # the host could not know: k advanced; the twin's schedule is advanced by hand, without a launch
    for group in b.param_groups:
        group.update(schedule(group)[1])
    assert [g["k"] for g in a.param_groups] == [g["k"] for g in b.param_groups] == [2, 2]
    _load(ga, 2)
    _load(gb, 2)
    a.step()
    b.step()
    for name, x, y in zip(("y", "z", "exp_avg_sq"), _state(a, pa), _state(b, pb)):
        assert _same_bits(x, y), f"{name} after the next good step"
    assert int(a.last_step_skipped()) == 0 and a.skipped_steps() == 1
    assert all(bool(torch.isfinite(t).all()) for part in _state(a, pa) for t in part)


@pytest.mark.gpu
def test_without_the_guard_a_nan_goes_through(dev):
    a, pa, ga = _twin(dev, "own", max_grad_norm=1.0)
    _load(ga, 0)
    ga[1][7] = float("nan")
    a.step()
    assert a.skipped_steps() == 0 and math.isnan(float(a.last_grad_norm()))
    assert float(a.last_clip_coef()) == 1.0                              # a NaN norm clips nothing
    y, z, v = _state(a, pa)
    assert all(bool(torch.isnan(t[1][7])) for t in (y, z, v))            # the state holds the NaN, as without the feature
    assert bool(torch.isfinite(y[0]).all())


# ---------------------------------------------------------------------------------------------------------------------
# GPU: launches
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("on", [True, False])
def test_launches_and_copies_of_a_steady_state_step(dev, on):
    from torch.profiler import ProfilerActivity, profile
    kw = dict(max_grad_norm=1.0, skip_nonfinite=True) if on else {}
    opt, params, grads = _twin(dev, "views", zero_grad_in_step=True, **kw)
    for _ in range(3):
        opt.step()
    torch.cuda.synchronize()
    launches = _lib.query("basd_sfadamw_launches")
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(20):
            opt.step()
        torch.cuda.synchronize()
    assert _lib.query("basd_sfadamw_launches") - launches == (40 if on else 20)
    assert opt.table_uploads == 1
    device_events = [e for e in prof.events() if "cuda" in str(e.device_type).lower()]
    host_names = {e.name for e in prof.events() if "cuda" not in str(e.device_type).lower()}
    kernels = [e for e in device_events if e.name not in host_names and "memcpy" not in e.name.lower()
               and "memset" not in e.name.lower()]
    copies = [e for e in prof.events() if "memcpy" in e.name.lower()]
    norm = [e for e in kernels if "grad_sqnorm_kernel" in e.name]
    clipped = [e for e in kernels if "sfadamw_step_clipped_kernel" in e.name]
    plain = [e for e in kernels if "sfadamw_step_kernel" in e.name]
    if norm or clipped or plain:
        print(f"[grad_clip] profiler: {len(kernels)} kernels ({len(norm)} norm, {len(clipped)} clipped, {len(plain)} "
              f"plain), {len(copies)} memcpy in 20 steps")
        want = (20, 20, 0) if on else (0, 0, 20)
        assert (len(norm), len(clipped), len(plain)) == want, sorted({e.name for e in kernels})
        assert len(kernels) == sum(want) and not copies, sorted({e.name for e in kernels + copies})
    else:
        print("[grad_clip] the profiler does not see the ctypes launches here: counted in the library "
              f"({len(kernels)} device kernels, {len(copies)} memcpy events seen by the profiler)")
        assert not kernels and not copies


# ---------------------------------------------------------------------------------------------------------------------
# GPU: inside the trainer
# ---------------------------------------------------------------------------------------------------------------------
def _trainer(dev, **kw):
    from basd_amd import trainer as T
    from tools import stock_models as SM
    torch.manual_seed(3)
    student = SM.StockViT(img_size=32, patch_size=8, embed_dim=48, depth=6, num_heads=4, num_classes=10).to(dev)
    teacher = SM.make_teacher(SM.StockViT(img_size=32, patch_size=8, embed_dim=64, depth=3, num_heads=4,
                                          num_classes=0).to(dev), 32)
    torch.manual_seed(42)
    cfg = SimpleNamespace(training=SimpleNamespace(label_smoothing=0.1, learning_rate=1e-3, weight_decay=0.05,
                                                   num_epochs=1),
                          basd=SimpleNamespace(num_extraction_points=4), model=SimpleNamespace(num_classes=10))
    tr = T.Trainer(student, cfg, teacher, student_info=SM.probe_model(student, 32), mixup=False,
                   optimizer="schedulefree", **kw)
    return tr, student


def _batches(n, B=16):
    out = []
    for i in range(n):
        g = torch.Generator().manual_seed(10 + i)
        clean = 2.0 * torch.randn(B, 3, 1, 1, generator=g) + torch.randn(B, 3, 32, 32, generator=g)
        augmented = 2.0 * torch.randn(B, 3, 1, 1, generator=g) + torch.randn(B, 3, 32, 32, generator=g)
        out.append({"clean": clean, "augmented": augmented, "label": (torch.arange(B) + i) % 10})
    return out


class _PoisonSecond:
    """A loader of three batches that multiplies one parameter's gradient by NaN while the second is in flight."""

    def __init__(self, batches, param):
        self.batches, self.param = batches, param

    def __iter__(self):
        for i, batch in enumerate(self.batches):
            handle = self.param.register_hook(lambda g: g * float("nan")) if i == 1 else None
            yield batch
            if handle is not None:
                handle.remove()


@pytest.mark.gpu
def test_trainer_clips_and_skips(dev):
    tr, student = _trainer(dev, max_grad_norm=1.0, skip_nonfinite=True)
    assert tr.optimizer.max_grad_norm == 1.0 and tr.optimizer.skip_nonfinite
    params = list(student.parameters()) + list(tr.basd_loss.parameters())
    target = list(student.parameters())[5]
    batches = _batches(3)
    snaps, norms = [], []
    for i, batch in enumerate(batches):
        handle = target.register_hook(lambda g: g * float("nan")) if i == 1 else None
        out = tr.train_step(batch)
        if handle is not None:
            handle.remove()
        assert set(out) == {"loss", "correct", "n", "grad_norm"}
        norms.append(float(out["grad_norm"]))
        snaps.append([p.detach().clone() for p in params])
    print("[grad_clip] trainer grad norms:", norms)
    assert _same_bits(snaps[1], snaps[0]), "the poisoned step moved the parameters"
    assert not _same_bits(snaps[2], snaps[1]), "the step after it did not"
    assert all(bool(torch.isfinite(t).all()) for t in snaps[2])
    assert math.isfinite(norms[0]) and norms[0] > 0 and math.isnan(norms[1]) and math.isfinite(norms[2])
    assert tr.optimizer.skipped_steps() == 1 and tr.optimizer.param_groups[0]["k"] == 3

    # the same through _train_epoch: the epoch's own count and the mean over the steps that were kept
    tr, student = _trainer(dev, max_grad_norm=1.0, skip_nonfinite=True)
    metrics = tr._train_epoch(_PoisonSecond(batches, list(student.parameters())[5]))
    assert set(metrics) == {"train_loss", "train_acc", "grad_norm", "skipped_steps"}
    assert metrics["skipped_steps"] == 1 and math.isfinite(metrics["grad_norm"]) and metrics["grad_norm"] > 0
    # the same seeds and steps as above; two runs of the loss path agree to 1e-5 in the loss (test_schedulefree.py),
    # the gradients' norm is given 1e-3
    assert metrics["grad_norm"] == pytest.approx((norms[0] + norms[2]) / 2, rel=1e-3)
    assert tr._train_epoch(batches[:1])["skipped_steps"] == 0                              # per epoch, not a running total


@pytest.mark.gpu
def test_trainer_switched_off_returns_the_old_keys(dev):
    tr, _ = _trainer(dev)
    assert tr.optimizer.max_grad_norm is None and not tr.optimizer.skip_nonfinite
    launches = _lib.query("basd_sfadamw_launches")
    assert set(tr.train_step(_batches(1)[0])) == {"loss", "correct", "n"}
    assert _lib.query("basd_sfadamw_launches") - launches == 1
    assert set(tr._train_epoch(_batches(2))) == {"train_loss", "train_acc"}
