"""Schedule-free AdamW (``basd_amd.optim.AdamWScheduleFree``, kernels in ``csrc/optim.hip``) against restatements of the
recurrence written here with torch ops: fp64 on the CPU is the reference, the SAME recurrence in fp32 on the CPU gives
the error an fp32 evaluation has a right to (``e32``), and the kernel must stay within ``4 * e32 + 1e-7 * max|q|`` per
quantity (the factor 4 covers a different operation order and FMA contraction, nothing more).

The ``schedulefree`` package is not installed where this was written: the recurrence below (from the paper and the
package's published source) is the specification, and nothing here compares against the package itself."""
import copy
import math
import os
from types import SimpleNamespace

import pytest
import torch
import torch.nn as nn

from basd_amd import _lib
from basd_amd.optim import MAX_GROUPS, AdamWScheduleFree, schedule

GROUP_KEYS = {"lr", "betas", "eps", "r", "k", "warmup_steps", "train_mode", "weight_sum", "lr_max", "scheduled_lr",
              "weight_lr_power", "weight_decay", "foreach"}


# ---------------------------------------------------------------------------------------------------------------------
# the restatement: host recurrence and per-tensor update, any dtype, plain torch ops
# ---------------------------------------------------------------------------------------------------------------------
def _new_group(lr=0.0025, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, warmup_steps=0, r=0.0, weight_lr_power=2.0):
    return dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, warmup_steps=warmup_steps, r=r,
                weight_lr_power=weight_lr_power, k=0, weight_sum=0.0, lr_max=-1.0, scheduled_lr=0.0)


def _host(group):
    """One step of the host recurrence, in place; returns (lr, ckp1, bias_correction2)."""
    k = group["k"]
    sched = (k + 1) / group["warmup_steps"] if k < group["warmup_steps"] else 1.0
    bc2 = 1.0 - group["betas"][1] ** (k + 1)
    lr = group["lr"] * sched
    group["scheduled_lr"] = lr
    group["lr_max"] = max(lr, group["lr_max"])
    weight = ((k + 1) ** group["r"]) * (group["lr_max"] ** group["weight_lr_power"])
    group["weight_sum"] += weight
    ckp1 = weight / group["weight_sum"] if group["weight_sum"] != 0.0 else 0.0
    group["k"] = k + 1
    return lr, ckp1, bc2


def _update(y, z, v, grad, group, lr, ckp1, bc2, grad_scale=1.0):
    """The per-element update on tensors of one dtype, in place (y: the parameter in train mode)."""
    beta1, beta2 = group["betas"]
    g = grad * grad_scale
    v.copy_(beta2 * v + ((1.0 - beta2) * g) * g)
    gn = g / ((v / bc2).sqrt() + group["eps"]) + group["weight_decay"] * y
    y.copy_(y + ckp1 * (z - y))
    y.copy_(y + (lr * (beta1 * (1.0 - ckp1) - 1.0)) * gn)
    z.copy_(z - lr * gn)


def _lerp(p, z, w):
    return p + w * (z - p)


class Restated:
    """The whole optimizer on lists of tensors of dtype ``dt`` (CPU): ``groups`` = list of (group dict, [indices])."""

    def __init__(self, params, groups, dt):
        self.y = [p.detach().cpu().to(dt).clone() for p in params]
        self.z = [y.clone() for y in self.y]
        self.v = [torch.zeros_like(y) for y in self.y]
        self.groups = [(_new_group(**kw), idx) for kw, idx in groups]
        self.dt = dt

    def step(self, grads):
        for group, idx in self.groups:
            lr, ckp1, bc2 = _host(group)
            for i in idx:
                if grads[i] is not None:
                    _update(self.y[i], self.z[i], self.v[i], grads[i].cpu().to(self.dt), group, lr, ckp1, bc2)

    def x(self):
        out = []
        for group, idx in self.groups:
            for i in idx:
                out.append((i, _lerp(self.y[i], self.z[i], 1.0 - 1.0 / group["betas"][0])))
        return [t for _, t in sorted(out, key=lambda it: it[0])]


def _maxdist(a_list, b_list):
    return max(float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())
               for a, b in zip(a_list, b_list))


def _maxabs(a_list):
    return max(float(a.detach().cpu().double().abs().max()) for a in a_list)


def _check(name, got, ref64, ref32):
    """``|got - fp64| <= 4 * e32 + 1e-7 * max|fp64|`` with ``e32 = |fp32 restatement - fp64|``; prints the ratio."""
    e32 = _maxdist(ref32, ref64)
    err = _maxdist(got, ref64)
    bound = 4.0 * e32 + 1e-7 * _maxabs(ref64)
    print(f"[schedulefree] {name}: kernel-fp64 {err:.3e}  e32 {e32:.3e}  ratio {err / max(e32, 1e-300):.3f}  "
          f"bound {bound:.3e}  max|q| {_maxabs(ref64):.3e}")
    assert err <= bound, (name, err, e32, bound)


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the host recurrence, the state_dict layout, the boundary
# ---------------------------------------------------------------------------------------------------------------------
def test_host_recurrence_against_the_closed_form():
    lr0, beta2 = 1e-3, 0.999
    opt = AdamWScheduleFree([nn.Parameter(torch.zeros(3))], lr=lr0, betas=(0.9, beta2), warmup_steps=5)
    group = opt.param_groups[0]
    lrs = []
    for k in range(12):
        before = copy.deepcopy({key: val for key, val in group.items() if key != "params"})
        now, new_state = schedule(group)
        assert {key: val for key, val in group.items() if key != "params"} == before        # pure
        group.update(new_state)
        lrs.append(lr0 * min((k + 1) / 5.0, 1.0))
        assert now["lr"] == pytest.approx(lrs[-1], rel=1e-15) and group["scheduled_lr"] == now["lr"]
        assert now["ckp1"] == pytest.approx(lrs[-1] ** 2 / sum(l * l for l in lrs), rel=1e-12)
        assert now["bias_correction2"] == pytest.approx(1.0 - beta2 ** (k + 1), rel=1e-15)
        assert group["k"] == k + 1 and group["lr_max"] == pytest.approx(max(lrs), rel=1e-15)
    # the same numbers from the restatement's own host code
    mine = _new_group(lr=lr0, betas=(0.9, beta2), warmup_steps=5)
    theirs = AdamWScheduleFree([nn.Parameter(torch.zeros(3))], lr=lr0, betas=(0.9, beta2), warmup_steps=5).param_groups[0]
    for _ in range(12):
        lr, ckp1, bc2 = _host(mine)
        now, new_state = schedule(theirs)
        theirs.update(new_state)
        assert (lr, ckp1, bc2) == (now["lr"], now["ckp1"], now["bias_correction2"])
    # lr = 0: weight_sum stays 0, ckp1 is 0 and nothing divides by zero
    zero = AdamWScheduleFree([nn.Parameter(torch.zeros(3))], lr=0.0).param_groups[0]
    for _ in range(3):
        now, new_state = schedule(zero)
        zero.update(new_state)
        assert now["ckp1"] == 0.0 and now["lr"] == 0.0


def test_a_group_added_later_has_its_own_counters():
    opt = AdamWScheduleFree([nn.Parameter(torch.zeros(3))], lr=1e-3, warmup_steps=5)
    for _ in range(3):
        opt.param_groups[0].update(schedule(opt.param_groups[0])[1])
    opt.add_param_group({"params": [nn.Parameter(torch.zeros(2))]})
    first, second = opt.param_groups
    assert first["k"] == 3 and first["weight_sum"] > 0 and first["lr_max"] > 0
    assert second["k"] == 0 and second["weight_sum"] == 0.0 and second["lr_max"] == -1.0
    assert second["lr"] == 1e-3 and second["warmup_steps"] == 5          # constructor defaults
    with pytest.raises(ValueError):
        many = AdamWScheduleFree([nn.Parameter(torch.zeros(1))])
        for _ in range(MAX_GROUPS):
            many.add_param_group({"params": [nn.Parameter(torch.zeros(1))]})


def test_state_dict_layout_and_round_trip():
    params = [nn.Parameter(torch.randn(5)), nn.Parameter(torch.randn(2, 3))]
    opt = AdamWScheduleFree(params[:1], lr=2e-3, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.05, warmup_steps=7, r=1.0,
                            weight_lr_power=1.5)
    opt.add_param_group({"params": params[1:], "weight_decay": 0.0})
    for g in opt.param_groups:
        for _ in range(4):
            g.update(schedule(g)[1])
    sd = opt.state_dict()
    assert len(sd["param_groups"]) == 2
    for g in sd["param_groups"]:
        assert set(g) == GROUP_KEYS | {"params"}
    assert sorted(sd["state"]) == [0, 1]
    for i, p in enumerate(params):
        assert set(sd["state"][i]) == {"z", "exp_avg_sq"}
        assert torch.equal(sd["state"][i]["z"], p.detach()) and not sd["state"][i]["exp_avg_sq"].any()
        assert sd["state"][i]["z"].shape == p.shape and sd["state"][i]["z"].data_ptr() % 16 == 0
    sd["state"][1]["z"].add_(1.0)
    sd["state"][1]["exp_avg_sq"].fill_(0.25)
    sd = copy.deepcopy(sd)
    fresh = AdamWScheduleFree([nn.Parameter(p.detach().clone()) for p in params[:1]])
    fresh.add_param_group({"params": [nn.Parameter(p.detach().clone()) for p in params[1:]]})
    fresh.load_state_dict(sd)
    for got, want in zip(fresh.param_groups, sd["param_groups"]):
        for key in GROUP_KEYS:
            assert got[key] == want[key], key
    p1 = fresh.param_groups[1]["params"][0]
    assert torch.equal(fresh.state[p1]["z"], sd["state"][1]["z"])
    assert torch.equal(fresh.state[p1]["exp_avg_sq"], torch.full((2, 3), 0.25))
    assert fresh.state[p1]["z"].data_ptr() != sd["state"][1]["z"].data_ptr()      # moved into the flat buffers


def test_bucket_wait_can_leave_the_division_to_the_optimizer():
    """``FlatGradBucket.wait(divide=False)`` joins a summed all-reduce without the ``div_`` pass and says so (the
    trainer then hands ``1 / world`` to the step); with nothing pending it owes nothing."""
    from basd_amd.ddp import FlatGradBucket

    class Work:
        waited = 0

        def wait(self):
            Work.waited += 1

    bucket = FlatGradBucket(6, [], "cpu")
    bucket.buffer.fill_(3.0)
    assert bucket.wait(divide=False) is False and bucket.wait() is False
    bucket._pending[0] = (Work(), True)                 # a SUM was queued (a backend without AVG)
    assert bucket.wait(divide=False) is True and Work.waited == 1
    assert bool((bucket.buffer == 3.0).all()) and bucket._pending[0] is None
    bucket._pending[0] = (Work(), False)                # the backend averaged: nothing is owed
    assert bucket.wait(divide=False) is False and Work.waited == 2


def test_boundary_errors():
    p = nn.Parameter(torch.randn(4))
    p.grad = torch.randn(4)
    opt = AdamWScheduleFree([p])
    with pytest.raises(Exception, match="train mode"):          # a fresh optimizer is in eval mode, as in the package
        opt.step()
    opt.train()
    assert opt.param_groups[0]["train_mode"] and opt.param_groups[0]["k"] == 0
    before = p.detach().clone()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step()
    assert torch.equal(p.detach(), before) and opt.param_groups[0]["k"] == 0
    with pytest.raises(TypeError):
        AdamWScheduleFree([nn.Parameter(torch.randn(4).to(torch.bfloat16))])
    with pytest.raises(TypeError):
        opt.add_param_group({"params": [nn.Parameter(torch.randn(4).to(torch.float16))]})
    assert len(opt.param_groups) == 1


# ---------------------------------------------------------------------------------------------------------------------
# GPU: through the C ABI
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


CHUNK = 4096            # asserted against the library in the trajectory test
NUMELS = [1, 3, 4, 5, 4099, 65536 + 1, 2 * CHUNK + 7]
GROUPS = [(dict(lr=1e-3, weight_decay=0.05, warmup_steps=5), [0, 2, 4, 6]),
          (dict(lr=3e-3, weight_decay=0.0, warmup_steps=5), [1, 3, 5])]
SKIPPED, SKIP_STEPS = 4, {3, 10, 11, 40}            # tensor 4 has no gradient on these steps


def _initial(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [2.0 * torch.randn(n, generator=g) for n in NUMELS]


def _gradients(step, seed=100):
    """Seeded gradients with a heavy-tailed scale (exp of a wide normal, per element) and exact zeros."""
    g = torch.Generator().manual_seed(seed + step)
    out = []
    for i, n in enumerate(NUMELS):
        if i == SKIPPED and step in SKIP_STEPS:
            torch.randn(n, generator=g)
            out.append(None)
            continue
        x = torch.randn(n, generator=g) * torch.exp(3.0 * torch.randn(n, generator=g))
        x[torch.rand(n, generator=g) < 0.1] = 0.0
        if step == 0 and n > 4:
            x[:3] = 0.0                 # v = 0 and g = 0: 0 / eps
        out.append(x)
    return out


def _make_optimizer(params, **kw):
    opt = AdamWScheduleFree([params[i] for i in GROUPS[0][1]], **GROUPS[0][0], **kw)
    opt.add_param_group({"params": [params[i] for i in GROUPS[1][1]], **GROUPS[1][0]})
    return opt


def _state(opt, params):
    return ([p.detach().clone() for p in params], [opt.state[p]["z"].clone() for p in params],
            [opt.state[p]["exp_avg_sq"].clone() for p in params])


def _run_plain(dev, steps):
    params = [nn.Parameter(t.to(dev)) for t in _initial()]
    opt = _make_optimizer(params)
    opt.train()
    for s in range(steps):
        for p, g in zip(params, _gradients(s)):
            p.grad = None if g is None else g.to(dev)
        opt.step()
    return opt, params


@pytest.mark.gpu
def test_trajectory_against_fp64(dev):
    assert _lib.query("basd_sfadamw_chunk") == CHUNK and max(NUMELS) > 2 * CHUNK
    steps = 60
    ref64 = Restated(_initial(), GROUPS, torch.float64)
    ref32 = Restated(_initial(), GROUPS, torch.float32)
    for s in range(steps):
        grads = _gradients(s)
        ref64.step(grads)
        ref32.step(grads)
    opt, params = _run_plain(dev, steps)
    y, z, v = _state(opt, params)
    assert all(torch.isfinite(t).all() for t in y + z + v)
    _check("y", y, ref64.y, ref32.y)
    _check("z", z, ref64.z, ref32.z)
    _check("exp_avg_sq", v, ref64.v, ref32.v)
    opt.eval()
    _check("x", [p.detach() for p in params], ref64.x(), ref32.x())
    for (want, _), got in zip(ref64.groups, opt.param_groups):
        assert got["k"] == steps == want["k"] and got["weight_sum"] == want["weight_sum"]
        assert got["scheduled_lr"] == want["scheduled_lr"] and got["lr_max"] == want["lr_max"]


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["bucket", "guarded"])
def test_gradient_views_scaling_and_zeroing_are_exact(dev, layout):
    """Every gradient a view into one flat buffer at odd element offsets, ``grad_scale = 0.5`` on doubled gradients and
    zeroing inside the step: bit-identical to the plain run; the buffer ends all zero and nothing outside the views is
    written."""
    from basd_amd.ddp import FlatGradBucket
    steps = 24
    opt0, params0 = _run_plain(dev, steps)
    y0, z0, v0 = _state(opt0, params0)

    params = [nn.Parameter(t.to(dev)) for t in _initial()]
    opt = _make_optimizer(params, zero_grad_in_step=True, grad_scale=0.5)
    order = GROUPS[0][1] + GROUPS[1][1]
    GUARD = 12345.0
    if layout == "bucket":                  # [group 0 | group 1], back to back: offsets 1, 5, 4104, ...
        bucket = FlatGradBucket(sum(NUMELS[i] for i in GROUPS[0][1]), [params[i] for i in GROUPS[1][1]], dev)
        bucket.attach_grads([params[i] for i in GROUPS[0][1]])
        flat = bucket.buffer
        views = {i: params[i].grad for i in order}
        guards = torch.zeros(0, dtype=torch.long, device=dev)
    else:                                   # guard words before, between and after; every view starts at an odd offset
        off, where = 0, {}
        for i in order:
            pad = 1 if (off + 1) % 2 == 1 else 2
            off += pad
            where[i] = off
            off += NUMELS[i]
        flat = torch.full((off + 3,), GUARD, device=dev)
        views = {i: flat[where[i]:where[i] + NUMELS[i]] for i in order}
        mask = torch.ones(off + 3, dtype=torch.bool, device=dev)
        for i in order:
            assert where[i] % 2 == 1
            mask[where[i]:where[i] + NUMELS[i]] = False
            views[i].zero_()
        guards = mask.nonzero().flatten()
        assert guards.numel() >= len(order) + 3
    assert any(v.data_ptr() % 16 != 0 for v in views.values())
    opt.train()
    for s in range(steps):
        for i, g in enumerate(_gradients(s)):
            if g is None:
                params[i].grad = None
            else:
                views[i].copy_(2.0 * g.to(dev))
                params[i].grad = views[i]
        opt.step()
        inside = torch.cat([views[i] for i in order])
        assert not inside.any(), f"step {s}: gradients not zeroed"
    y, z, v = _state(opt, params)
    for name, a, b in (("y", y, y0), ("z", z, z0), ("exp_avg_sq", v, v0)):
        for i, (s, t) in enumerate(zip(a, b)):
            assert torch.equal(s, t), f"{name}[{i}] (numel {NUMELS[i]}) differs from the plain run"
    if layout == "bucket":
        assert not flat.any()
    else:
        assert bool((flat[guards] == GUARD).all()), "a guard word was written"
    # the per-call override: zeroing switched off for one step leaves the gradient alone
    views[0].fill_(0.5)
    params[0].grad = views[0]
    opt.step(zero_grad_in_step=False, grad_scale=1.0)
    assert float(views[0][0]) == 0.5


@pytest.mark.gpu
def test_mode_switch(dev):
    opt, params = _run_plain(dev, 12)
    y0, z0, v0 = _state(opt, params)
    opt.eval()
    assert not opt.param_groups[0]["train_mode"] and not opt.param_groups[1]["train_mode"]
    x = [p.detach().clone() for p in params]
    opt.eval()                                           # twice is the same as once
    assert all(torch.equal(a, p.detach()) for a, p in zip(x, params))
    with pytest.raises(Exception, match="train mode"):
        opt.step()
    opt.train()
    assert opt.param_groups[0]["train_mode"]
    beta1 = 0.9

    def there_and_back(dt):
        out_x, out_y = [], []
        for y, z in zip(y0, z0):
            y, z = y.cpu().to(dt), z.cpu().to(dt)
            xx = _lerp(y, z, 1.0 - 1.0 / beta1)
            out_x.append(xx)
            out_y.append(_lerp(xx, z, 1.0 - beta1))
        return out_x, out_y

    x64, y64 = there_and_back(torch.float64)
    x32, y32 = there_and_back(torch.float32)
    _check("x after eval()", x, x64, x32)
    _check("y after eval(); train()", [p.detach() for p in params], y64, y32)
    assert _maxdist(x, y0) > 1e-4                      # eval() moved the weights
    _, z1, v1 = _state(opt, params)
    assert all(torch.equal(a, b) for a, b in zip(z0 + v0, z1 + v1))       # state untouched, bit for bit


@pytest.mark.gpu
def test_checkpoint_round_trip_is_bit_identical(dev):
    opt, params = _run_plain(dev, 10)
    sd = copy.deepcopy(opt.state_dict())
    clones = [nn.Parameter(p.detach().clone()) for p in params]
    other = AdamWScheduleFree([clones[i] for i in GROUPS[0][1]])          # defaults: everything comes from the checkpoint
    other.add_param_group({"params": [clones[i] for i in GROUPS[1][1]]})
    other.load_state_dict(sd)
    assert other.param_groups[0]["train_mode"] and other.param_groups[1]["k"] == 10
    for s in range(10, 20):
        for p, q, g in zip(params, clones, _gradients(s)):
            p.grad = None if g is None else g.to(dev)
            q.grad = None if g is None else g.to(dev)
        opt.step()
        other.step()
    for a, b in zip(_state(opt, params), _state(other, clones)):
        assert all(torch.equal(s, t) for s, t in zip(a, b))
    assert [g["weight_sum"] for g in opt.param_groups] == [g["weight_sum"] for g in other.param_groups]


@pytest.mark.gpu
def test_no_hidden_host_work(dev):
    """A steady-state ``step()`` is one kernel launch, no memcpy.  Counted with ``torch.profiler`` (CPU + device
    activities) when it sees launches made through ctypes, and always with the library's own launch counter
    (``basd_sfadamw_launches``) plus the optimizer's table-upload counter; the output says which."""
    from torch.profiler import ProfilerActivity, profile
    params = [nn.Parameter(t.to(dev)) for t in _initial()]
    opt = _make_optimizer(params, zero_grad_in_step=True)
    for p in params:
        p.grad = torch.randn_like(p)
    opt.train()
    for _ in range(3):
        opt.step()
    torch.cuda.synchronize()
    launches, uploads = _lib.query("basd_sfadamw_launches"), opt.table_uploads
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(20):
            opt.step()
        torch.cuda.synchronize()
    assert _lib.query("basd_sfadamw_launches") - launches == 20
    assert opt.table_uploads == uploads == 1
    device_events = [e for e in prof.events() if "cuda" in str(e.device_type).lower()]
    # ranges opened on the host (``Optimizer.step#...``) are mirrored on the device track under the same name: not kernels
    host_names = {e.name for e in prof.events() if "cuda" not in str(e.device_type).lower()}
    kernels = [e for e in device_events if e.name not in host_names and "memcpy" not in e.name.lower()
               and "memset" not in e.name.lower()]
    copies = [e for e in prof.events() if "memcpy" in e.name.lower()]
    ours = [e for e in kernels if "sfadamw_step_kernel" in e.name]
    if ours:
        print(f"[schedulefree] profiler: {len(kernels)} kernels ({len(ours)} sfadamw_step_kernel), {len(copies)} memcpy "
              "in 20 steps")
        assert len(ours) == 20 and len(kernels) == 20, sorted({e.name for e in kernels})
        assert not copies, sorted({e.name for e in copies})
    else:
        print("[schedulefree] the profiler does not see the ctypes launches here: counted in the library "
              f"({len(kernels)} device kernels, {len(copies)} memcpy events seen by the profiler)")
        assert not kernels and not copies


# ---------------------------------------------------------------------------------------------------------------------
# GPU: inside the trainer
# ---------------------------------------------------------------------------------------------------------------------
def _config(points=4, classes=10, epochs=1):
    return SimpleNamespace(training=SimpleNamespace(label_smoothing=0.1, learning_rate=1e-3, weight_decay=0.05,
                                                    num_epochs=epochs),
                           basd=SimpleNamespace(num_extraction_points=points), model=SimpleNamespace(num_classes=classes))


def _structured_images(B, size, seed):
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(B, 3, 1, 1, generator=g) * 2.0
    return base + torch.randn(B, 3, size, size, generator=g)


def _toy_models(dev):
    from tools import stock_models as SM
    torch.manual_seed(3)
    student = SM.StockViT(img_size=32, patch_size=8, embed_dim=48, depth=6, num_heads=4, num_classes=10).to(dev)
    teacher = SM.StockViT(img_size=32, patch_size=8, embed_dim=64, depth=3, num_heads=4, num_classes=0).to(dev)
    return student, SM.make_teacher(teacher, 32)


class TorchScheduleFree(torch.optim.Optimizer):
    """The restatement as an optimizer the trainer can hold: torch ops on the parameters' device, state in ``dt``
    (fp64: the parameters are a rounded copy of an fp64 master ``y``)."""

    def __init__(self, params, lr, weight_decay, dt):
        super().__init__(params, dict(_new_group(lr=lr, weight_decay=weight_decay), train_mode=False))
        self.dt = dt

    def _st(self, p):
        st = self.state[p]
        if not st:
            st["y"] = p.detach().to(self.dt).clone()
            st["z"] = st["y"].clone()
            st["v"] = torch.zeros_like(st["y"])
        return st

    @torch.no_grad()
    def step(self):
        assert self.param_groups[0]["train_mode"]
        for group in self.param_groups:
            lr, ckp1, bc2 = _host(group)
            for p in group["params"]:
                if p.grad is not None:
                    st = self._st(p)
                    _update(st["y"], st["z"], st["v"], p.grad.to(self.dt), group, lr, ckp1, bc2)
                    p.copy_(st["y"])

    @torch.no_grad()
    def _mode(self, train):
        for group in self.param_groups:
            if group["train_mode"] != train:
                for p in group["params"]:
                    if self.state[p]:
                        st = self.state[p]
                        p.copy_(st["y"] if train else _lerp(st["y"], st["z"], 1.0 - 1.0 / group["betas"][0]))
                group["train_mode"] = train

    def train(self):
        self._mode(True)

    def eval(self):
        self._mode(False)


def _trainer(dev, which):
    from basd_amd import trainer as T
    from tools import stock_models as SM
    student, teacher = _toy_models(dev)
    torch.manual_seed(42)
    cfg = _config()
    if which == "kernel":
        tr = T.Trainer(student, cfg, teacher, student_info=SM.probe_model(student, 32), mixup=False,
                       optimizer="schedulefree")
        assert isinstance(tr.optimizer, AdamWScheduleFree) and tr.optimizer.param_groups[0]["train_mode"]
        assert tr.optimizer.param_groups[0]["lr"] == 1e-3 and tr.optimizer.param_groups[0]["weight_decay"] == 0.05
    else:
        tr = T.Trainer(student, cfg, teacher, student_info=SM.probe_model(student, 32), mixup=False)
        tr.optimizer = TorchScheduleFree(student.parameters(), cfg.training.learning_rate, cfg.training.weight_decay,
                                         which)
        tr.optimizer.add_param_group({"params": list(tr.basd_loss.parameters())})
        tr.optimizer.train()
    assert len(tr.optimizer.param_groups) == 2
    assert tr.optimizer.param_groups[1]["params"][0] is tr.basd_loss.layer_selector.log_temperatures
    return tr, student


def _batches(n, B=16):
    return [{"clean": _structured_images(B, 32, 10 + i), "augmented": _structured_images(B, 32, 50 + i),
             "label": (torch.arange(B) + i) % 10} for i in range(n)]


@pytest.mark.gpu
def test_trainer_with_the_schedulefree_optimizer(dev):
    batches = _batches(4)
    runs = {}
    for which in ("kernel", torch.float32, torch.float64):
        tr, student = _trainer(dev, which)
        losses = [float(tr.train_step(b)["loss"]) for b in batches]
        weights = [p.detach().cpu().clone() for p in list(student.parameters()) + list(tr.basd_loss.parameters())]
        runs[which] = (losses, weights)
    (l_k, w_k), (l_32, w_32), (_, w_64) = runs["kernel"], runs[torch.float32], runs[torch.float64]
    print("[schedulefree] trainer losses:", l_k, l_32)
    for a, b in zip(l_k, l_32):
        assert math.isfinite(a) and abs(a - b) <= 1e-5 * abs(b), (l_k, l_32)
    assert l_k[0] != l_k[-1]
    _check("trainer parameters after 4 steps", w_k, w_64, w_32)


@pytest.mark.gpu
def test_trainer_validates_on_the_averaged_weights(dev):
    tr, student = _trainer(dev, "kernel")
    opt = tr.optimizer
    seen = {}

    def evaluate(model, loader):
        seen["mode"] = [g["train_mode"] for g in opt.param_groups]
        seen["weights"] = [p.detach().clone() for p in model.parameters()]
        return {"val_acc": 12.5}

    history = tr.train(_batches(3), val_loader=[0], evaluate=evaluate)
    assert history["val_acc"] == [12.5] and seen["mode"] == [False, False]
    assert all(g["train_mode"] for g in opt.param_groups)                   # back in train mode afterwards
    params = list(student.parameters())
    y = [p.detach().clone() for p in params]
    z = [opt.state[p]["z"] for p in params]

    def expected(dt):
        return [_lerp(a.cpu().to(dt), b.cpu().to(dt), 1.0 - 1.0 / 0.9) for a, b in zip(y, z)]

    # x was made from y by one fp32 interpolation and y came back by a second one: at most 3 roundings each, of values
    # below 2 max|y| -- 6 x 2^-23 max|y|, taken as 8 x 2^-23
    tol = 8.0 * 2.0 ** -23 * _maxabs(y)
    e = _maxdist(seen["weights"], expected(torch.float64))
    print(f"[schedulefree] validation weights vs lerp(y, z, 1 - 1 / beta1): {e:.3e} (tolerance {tol:.3e})")
    assert e <= tol, e
    assert _maxdist(seen["weights"], y) > 1e-5                                  # x is not y
    # a checkpoint holds the averaged weights and an optimizer in eval mode; the live ones stay on the y sequence
    state = tr.state_dict(epoch=0)
    assert not state["optimizer"]["param_groups"][0]["train_mode"]
    name0 = next(iter(dict(student.named_parameters())))
    assert _maxdist([state["model"][name0]], [seen["weights"][0]]) <= tol
    assert all(g["train_mode"] for g in opt.param_groups)
    assert _maxdist(params, y) <= tol
    path = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"basd_sf_trainer_{os.getpid()}.pth")
    tr.save_checkpoint(path, epoch=0)
    assert tr.load_checkpoint(path) == 1
    os.remove(path)
    assert all(g["train_mode"] for g in opt.param_groups) and opt.param_groups[0]["k"] == 3
    tr.train_step(_batches(1)[0])
    assert opt.param_groups[0]["k"] == 4


@pytest.mark.gpu
def test_trainer_step_over_the_flat_bucket(dev):
    """The multi-rank layout on one GPU: every gradient a ``FlatGradBucket`` view, the update zeroes the bucket itself
    (no separate ``zero_grad``) and takes its ``grad_scale`` from the reduction; same losses as the trainer without a
    bucket (1e-5 relative, as above)."""
    from basd_amd.ddp import FlatGradBucket
    batches = _batches(4)
    plain, _ = _trainer(dev, "kernel")
    want = [float(plain.train_step(b)["loss"]) for b in batches]
    tr, student = _trainer(dev, "kernel")
    tr._bucket = FlatGradBucket(sum(p.numel() for p in tr._params), list(tr.basd_loss.parameters()), dev)
    tr._bucket.attach_grads(tr._params)
    tr.optimizer.zero_grad_in_step = True
    zero_grad_calls = []
    tr.optimizer.zero_grad = lambda *a, **k: zero_grad_calls.append(1)
    got = []
    for b in batches:
        got.append(float(tr.train_step(b)["loss"]))
        assert not tr._bucket.buffer.any()                                # zeroed by the step
    print("[schedulefree] trainer losses over the bucket:", got, want)
    for a, b in zip(got, want):
        assert abs(a - b) <= 1e-5 * abs(b), (got, want)
    assert not zero_grad_calls and tr.reattached == 0
    lo, hi = tr._bucket.buffer.data_ptr(), tr._bucket.buffer.data_ptr() + 4 * tr._bucket.buffer.numel()
    assert all(p.grad is not None and lo <= p.grad.data_ptr() < hi
               for p in list(student.parameters()) + list(tr.basd_loss.parameters()))
    assert tr.optimizer.table_uploads == 1 and tr.optimizer.param_groups[0]["k"] == 4
