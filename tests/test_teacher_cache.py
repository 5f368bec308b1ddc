"""The cached teacher side of single-layer teachers: basd_procrustes_plan_query_cached against the uncached planner,
the host logic of ``TeacherCache`` and of ``Trainer(teacher_cache=...)`` (no GPU), and on the GPU: bit identity of
``forward`` -> ``last_teacher_side`` -> ``store`` -> ``load`` -> ``forward_cached`` with ``forward`` per route, the
gather / scatter kernels (shuffled, repeated and equal indices, offsets past 2^32), two trainer epochs with and without
the cache, and the errors of the device path."""
import ctypes as C
import os
import sys
from types import SimpleNamespace

import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_procrustes_plan import FIELDS, _args          # noqa: E402  (the argument block the uncached plan tests use)

GIVEN = 5                                # field 0 of basd_procrustes_plan_query_cached
TEACHER_FIELDS = {"center": GIVEN, "gram_split": 0, "w_borrow_floats": 0, "lds_center": 0}      # fields 0, 4, 13, 14

# (name, E, B, n_s, n_t, d_s, d_t): the GPU cases of this file ...
SMALL = [("a", 2, 3, 16, 16, 64, 64), ("b", 4, 32, 16, 16, 64, 64), ("c", 2, 3, 16, 20, 64, 64),
         ("d", 2, 3, 16, 4, 64, 64), ("e", 2, 3, 16, 16, 64, 512), ("f", 2, 3, 16, 16, 64, 64),
         ("g", 2, 3, 49, 49, 64, 64)]
# ... and the production shapes (cfg-1, cfg-2, cfg-5)
PLANNED = [("plain", 2, 4, 49, 49, 64, 64), ("cfg1", 4, 32, 64, 1, 192, 512), ("cfg2", 4, 256, 196, 49, 384, 2048),
           ("cfg5", 4, 64, 576, 144, 768, 1536)] + SMALL


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _query(a, cached):
    from basd_amd import _lib
    out = (C.c_long * len(FIELDS))()
    name = "basd_procrustes_plan_query_cached" if cached else "basd_procrustes_plan_query"
    rc = _lib.query(name, C.addressof(a) if a is not None else None, C.cast(out, C.c_void_p))
    return rc, dict(zip(FIELDS, out))


# ---------------------------------------------------------------------------------------------------------------------
# not marked gpu
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PLANNED, ids=[c[0] for c in PLANNED])
@pytest.mark.parametrize("offered", [(), ("k_prime", "dx", "uw_ce"), ("k_prime", "dx", "uw_ce", "jac_ws", "g_split")],
                         ids=["forward", "step", "step+workspaces"])
def test_cached_plan_is_the_uncached_plan_without_the_teacher(case, offered):
    _, E, B, n_s, n_t, d_s, d_t = case
    a = _args(E, 1, B, n_s, n_t, d_s, d_t, offered=offered)
    rc_u, plain = _query(a, cached=False)
    rc_c, given = _query(a, cached=True)
    assert rc_u == 0 and rc_c == 0, (case, rc_u, rc_c)          # every shape used on the GPU below has a plan at all
    for name in FIELDS:
        want = TEACHER_FIELDS.get(name, plain[name])
        assert given[name] == want, (case, offered, name, given[name], want)
    assert plain["center"] != GIVEN and plain["center"] != 0
    assert plain["gram_split"] == int("g_split" in offered)     # the uncached plan does split where it is offered


def test_cached_plan_rejects_what_it_cannot_take():
    from basd_amd import _lib
    out = (C.c_long * len(FIELDS))()
    ptr = C.cast(out, C.c_void_p)
    good = _args(2, 1, 3, 16, 16, 64, 64)
    assert _lib.query("basd_procrustes_plan_query_cached", C.addressof(good), ptr) == 0
    assert _lib.query("basd_procrustes_plan_query_cached", None, ptr) == _lib.EINVAL
    assert _lib.query("basd_procrustes_plan_query_cached", C.addressof(good), None) == _lib.EINVAL
    multi = _args(2, 3, 3, 16, 16, 64, 64)                     # three teacher layers: G == E
    assert multi.G == 2
    assert _lib.query("basd_procrustes_plan_query", C.addressof(multi), ptr) == 0
    assert _lib.query("basd_procrustes_plan_query_cached", C.addressof(multi), ptr) == _lib.EINVAL
    for field, value in (("E", 0), ("L", 0), ("B", 0), ("n", 15), ("d_s", 0), ("d_t", 0), ("G", 3)):
        bad = _args(2, 1, 3, 16, 16, 64, 64)
        setattr(bad, field, value)
        assert _lib.query("basd_procrustes_plan_query", C.addressof(bad), ptr) == _lib.EINVAL, field
        assert _lib.query("basd_procrustes_plan_query_cached", C.addressof(bad), ptr) == _lib.EINVAL, field


def test_teacher_cache_host_logic():
    from basd_amd.ops import TeacherSide
    from basd_amd.teacher_cache import TeacherCache
    assert TeacherCache.record_bytes(49, 49) == 19600
    assert TeacherCache.record_bytes(16, 16) == 8 * 256 + 64 + 64
    for bad in ((0, 4, 4), (8, 0, 4), (8, 4, 0), (8, 5, 4), (True, 4, 4), (8.0, 4, 4)):
        with pytest.raises(ValueError):
            TeacherCache(*bad, "cpu")
    cache = TeacherCache(8, 4, 6, "cpu")                       # the bookkeeping is the host's; the launches are not
    assert cache.nbytes == 8 * TeacherCache.record_bytes(4, 6)
    assert (cache.g.shape, cache.omega.shape, cache.omega_t.shape) == ((8, 4, 4), (8, 6), (8, 4))
    assert (cache.g.dtype, cache.omega.dtype, cache.omega_t.dtype) == (torch.float64, torch.float32, torch.float32)
    index = torch.tensor([5, 0, 7])
    assert cache.has(index) is False
    side = TeacherSide(torch.zeros(3, 4, 4, dtype=torch.float64), torch.zeros(3, 6), torch.zeros(3, 4))
    for bad in (torch.tensor([5, 0, 8]), torch.tensor([-1, 0, 2]), torch.tensor([[5, 0, 7]]),
                torch.tensor([5, 0, 7], dtype=torch.int32), torch.tensor([5.0, 0.0, 7.0]), [5, 0, 7],
                torch.tensor([], dtype=torch.int64)):
        with pytest.raises(ValueError):
            cache.has(bad)
        with pytest.raises(ValueError):
            cache.load(bad)
        with pytest.raises(ValueError):
            cache.store(bad, side)
    with pytest.raises(ValueError, match="4 entries for a batch of 3"):
        cache.store(torch.tensor([5, 0, 7, 1]), side)
    for wrong in (side._replace(g=torch.zeros(3, 4, 5, dtype=torch.float64)), side._replace(g=torch.zeros(3, 4, 4)),
                  side._replace(omega=torch.zeros(3, 4)), side._replace(omega_t=torch.zeros(2, 4))):
        with pytest.raises(ValueError, match="teacher side"):
            cache.store(index, wrong)
    with pytest.raises(KeyError, match="5"):                   # decided on the host: the first row never stored
        cache.load(index)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cache.store(index, side)
    assert cache.has(index) is False                           # a store that was not queued fills nothing
    cache._filled[[5, 0, 7]] = True
    assert cache.has(index) is True and cache.has(torch.tensor([5, 1])) is False
    with pytest.raises(KeyError, match="1"):
        cache.load(torch.tensor([5, 1, 2]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cache.load(index)
    cache.clear()
    assert cache.has(index) is False


def _config(points=4, classes=10):
    return SimpleNamespace(training=SimpleNamespace(label_smoothing=0.1, learning_rate=1e-3, weight_decay=0.05),
                           basd=SimpleNamespace(num_extraction_points=points), model=SimpleNamespace(num_classes=classes))


def _toy_models(kind, dev="cpu"):
    """The toy sizes of tests/test_trainer_step.py."""
    from tools import stock_models as SM
    torch.manual_seed(3)
    student = SM.StockViT(img_size=32, patch_size=8, embed_dim=48, depth=6, num_heads=4, num_classes=10).to(dev)
    if kind == "cnn":
        teacher = SM.StockResNet(layers=(1, 1, 1, 1), bottleneck=False, width=16).to(dev)
    else:
        teacher = SM.StockViT(img_size=32, patch_size=8, embed_dim=64, depth=3, num_heads=4, num_classes=0).to(dev)
    return student, SM.make_teacher(teacher, 32)


def test_trainer_option_host_logic():
    from basd_amd import trainer as T
    from tools import stock_models as SM
    from test_trainer_step import OracleBASD
    student, vit_teacher = _toy_models("vit")
    info = SM.probe_model(student, 32)
    assert vit_teacher.feature_format == "token"
    with pytest.raises(ValueError, match="mixing weights depend on the student"):
        T.Trainer(student, _config(), vit_teacher, student_info=info, loss_cls=OracleBASD, teacher_cache=64)
    student, cnn_teacher = _toy_models("cnn")
    for bad in (0, -3, True, 2.5, "all"):
        with pytest.raises(ValueError, match="teacher_cache must be"):
            T.Trainer(student, _config(), cnn_teacher, student_info=info, loss_cls=OracleBASD, teacher_cache=bad)
    tr = T.Trainer(student, _config(), cnn_teacher, student_info=info, loss_cls=OracleBASD, teacher_cache=64, mixup=False)
    batch = {"clean": torch.randn(4, 3, 32, 32), "augmented": torch.randn(4, 3, 32, 32), "label": torch.arange(4)}
    with pytest.raises(KeyError, match="index"):
        tr.prepare_batch(batch)
    with pytest.raises(ValueError, match="3 entries for a batch of 4"):
        tr.prepare_batch(dict(batch, index=torch.tensor([2, 0, 1])))
    prepared = tr.prepare_batch(dict(batch, index=torch.tensor([9, 2, 0, 1])))
    assert prepared["teacher_cached"] is False and "clean" in prepared and prepared["index"].tolist() == [9, 2, 0, 1]
    # without the option nothing asks for the key and nothing is added
    plain = T.Trainer(student, _config(), cnn_teacher, student_info=info, loss_cls=OracleBASD, mixup=False)
    assert sorted(plain.prepare_batch(batch)) == ["augmented", "clean", "mixed_targets", "targets"]


# ---------------------------------------------------------------------------------------------------------------------
# marked gpu
# ---------------------------------------------------------------------------------------------------------------------
def _loss_case(dev, name, E, B, n_s, n_t, d_s, d_t):
    """(module, logits, targets, student tokens, teacher tokens, teacher attention): randn with fixed seeds (the teacher's
    tokens with a per-sample offset, so that its spectrum has something above the noise floor for the selector)."""
    from basd_amd.losses import BASDLoss
    gen = torch.Generator().manual_seed(1234 + ord(name))
    token_format = name == "f"                   # one token-format layer passed alone: CLS, per-head softmax attention
    torch.manual_seed(7)
    mod = BASDLoss(nn.CrossEntropyLoss(label_smoothing=0.1), d_s, d_t, E, n_s,
                   config=SimpleNamespace(num_extraction_points=E), teacher_has_cls_token=token_format).to(dev)
    assert mod.token_layers == list(range(E))
    s_dtype = torch.bfloat16 if token_format else torch.float32
    students = [torch.randn(B, n_s, d_s, generator=gen).to(dev, s_dtype) for _ in range(E)]
    teacher = (torch.randn(B, n_t, d_t, generator=gen) + 2.0 * torch.randn(B, 1, d_t, generator=gen)).to(dev)
    if token_format:
        attn = torch.softmax(torch.randn(B, 2, n_t + 1, n_t + 1, generator=gen), dim=-1).to(dev)
    else:                                        # what capture.extract_intermediates makes for a CNN teacher
        attn = torch.full((B, 1, 1, 1), 1.0 / n_t, device=dev).expand(B, 1, n_t, n_t)
    logits = torch.randn(B, 10, generator=gen).to(dev)
    targets = (torch.arange(B) % 10).to(dev)
    return mod, logits, targets, students, teacher, attn


def _run(mod, logits, targets, students, call):
    """One loss step on fresh leaves: (total, geo_layers, student gradients), detached."""
    leaves = {l: s.detach().clone().requires_grad_(True) for l, s in zip(mod.token_layers, students)}
    total = call(logits, targets, leaves)
    total.backward()
    return total.detach().clone(), mod.last_components["geo_layers"].clone(), [leaves[l].grad.clone() for l in leaves]


def _same(a, b):
    flat_a, flat_b = [a[0], a[1], *a[2]], [b[0], b[1], *b[2]]
    return all(x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y) for x, y in zip(flat_a, flat_b))


@pytest.mark.gpu
@pytest.mark.parametrize("case", SMALL, ids=[c[0] for c in SMALL])
def test_forward_cached_has_the_bits_of_forward(dev, case):
    """``forward`` twice (the determinism the suite relies on), then ``forward`` -> ``last_teacher_side`` -> ``store`` ->
    ``load`` -> ``forward_cached``: total, geo_layers and the student gradients bit for bit.  A derived condition, not a
    tolerance: the cached call runs the same kernels on the same inputs."""
    from basd_amd.teacher_cache import TeacherCache
    name, E, B, n_s, n_t, d_s, d_t = case
    mod, logits, targets, students, teacher, attn = _loss_case(dev, *case)
    n = min(n_s, n_t)

    def uncached(lg, tg, leaves):
        return mod(lg, tg, leaves, {0: teacher}, {0: attn})

    first = _run(mod, logits, targets, students, uncached)
    second = _run(mod, logits, targets, students, uncached)
    assert torch.isfinite(first[0]) and all(torch.isfinite(g).all() for g in first[2])
    assert _same(first, second), "forward is not deterministic on this shape"
    side = mod.last_teacher_side()
    assert (tuple(side.g.shape), tuple(side.omega.shape), tuple(side.omega_t.shape)) == ((B, n, n), (B, n_s), (B, n))
    if name == "f":
        assert not torch.equal(side.omega, torch.full_like(side.omega, 1.0 / n_s))          # attention-weighted tokens
    cache = TeacherCache(B + 8, n, n_s, dev)
    index = torch.randperm(B + 8, generator=torch.Generator().manual_seed(1))[:B].contiguous()
    cache.store(index, side)
    wanted = tuple(t.clone() for t in side)
    mod.layer_selector.finish_pending()
    ranks_before = dict(mod.layer_selector.subspace_ranks)

    def cached(lg, tg, leaves):
        return mod.forward_cached(lg, tg, leaves, cache.load(index))

    third = _run(mod, logits, targets, students, cached)
    print(f"[teacher_cache] case {name}: total {first[0].item():.9g} / {third[0].item():.9g}, "
          f"max |d grad| = {max(float((x.double() - y.double()).abs().max()) for x, y in zip(first[2], third[2])):.3e}")
    assert _same(first, third)
    # what the cached call read is what the uncached one produced
    got = mod.last_teacher_side()
    assert all(torch.equal(x, y) for x, y in zip(got, wanted))
    comp = mod.last_components
    assert sorted(comp) == ["ce", "geo_layers", "mix"] and torch.equal(comp["mix"], torch.ones(E, 1, device=dev))
    assert dict(mod.layer_selector.subspace_ranks) == ranks_before          # the selector did not run
    # a TeacherSide of plain tensors is taken as well (copied into the call's slots)
    fourth = _run(mod, logits, targets, students, lambda lg, tg, leaves: mod.forward_cached(lg, tg, leaves, wanted))
    assert _same(first, fourth)


def _random_side(B, n, n_s, dev, seed):
    from basd_amd.ops import TeacherSide
    gen = torch.Generator().manual_seed(seed)
    return TeacherSide(torch.randn(B, n, n, generator=gen, dtype=torch.float64).to(dev),
                       torch.randn(B, n_s, generator=gen).to(dev), torch.randn(B, n, generator=gen).to(dev))


@pytest.mark.gpu
@pytest.mark.parametrize("n,n_s", [(4, 16), (7, 9)], ids=["pairs", "doubles"])
def test_store_scatters_and_load_gathers(dev, n, n_s):
    from basd_amd.teacher_cache import TeacherCache
    cache = TeacherCache(40, n, n_s, dev)
    sentinel = (-7.5, 3.25, -1.125)
    for t, v in zip((cache.g, cache.omega, cache.omega_t), sentinel):
        t.fill_(v)
    rows = _random_side(12, n, n_s, dev, 5)
    index = torch.tensor([31, 4, 17, 0, 39, 22, 9, 36, 2, 28, 13, 6])
    assert cache.has(index) is False
    cache.store(index, rows)
    # no device wait: asked with work queued and nothing synchronised, plain Python comes back
    with torch.cuda.stream(torch.cuda.Stream(dev)):
        answers = [cache.has(torch.tensor([i])) for i in range(40)]
    assert all(type(a) is bool for a in answers) and not isinstance(cache._filled, torch.Tensor)
    assert [i for i, a in enumerate(answers) if a] == sorted(index.tolist())
    assert cache.has(index) is True and cache.has(torch.tensor([31, 5])) is False
    for stored, given in zip((cache.g, cache.omega, cache.omega_t), rows):
        assert torch.equal(stored[index.to(dev)], given)
    untouched = torch.ones(40, dtype=torch.bool)
    untouched[index] = False
    for stored, v in zip((cache.g, cache.omega, cache.omega_t), sentinel):
        assert (stored[untouched.to(dev)] == v).all()
    # a permutation that repeats one index
    order = torch.tensor([5, 0, 11, 3, 3, 8, 1, 10, 2, 7, 6, 9, 4])
    back = cache.load(index[order])
    for got, given in zip(back.tensors(), rows):
        assert torch.equal(got, given[order.to(dev)])
    assert torch.equal(back.g, rows.g[order.to(dev)])
    # the same index twice in one call, with equal rows
    twice = _random_side(3, n, n_s, dev, 6)
    twice = type(twice)(*(torch.cat([t, t[1:2]]) for t in twice))
    cache.store(torch.tensor([20, 21, 23, 21]), twice)
    for got, given in zip(cache.load(torch.tensor([21, 20, 23])).tensors(), twice):
        assert torch.equal(got, given[torch.tensor([1, 0, 2], device=dev)])
    # an index on the device is taken too
    for got, given in zip(cache.load(torch.tensor([23], device=dev)).tensors(), twice):
        assert torch.equal(got, given[2:3])
    with pytest.raises(KeyError, match="24"):
        cache.load(torch.tensor([20, 24, 25]))
    cache.clear()
    with pytest.raises(KeyError, match="20"):
        cache.load(torch.tensor([20]))


@pytest.mark.gpu
def test_rows_past_4_gib_round_trip(dev):
    """capacity * n * n * 8 = 4.5 GB: the last row's offset does not fit 32 bits."""
    from basd_amd.teacher_cache import TeacherCache
    capacity, n = 2_200_000, 16
    if torch.cuda.mem_get_info(dev)[0] < 6 << 30:
        pytest.fail("this test needs 6 GB of free device memory")
    cache = TeacherCache(capacity, n, n, dev)              # allocated, not filled
    assert cache.g.numel() * 8 > 1 << 32 and cache.nbytes == capacity * (2048 + 128)
    rows = _random_side(2, n, n, dev, 8)
    index = torch.tensor([0, capacity - 1])
    cache.store(index, rows)
    assert torch.equal(cache.g[capacity - 1], rows.g[1]) and torch.equal(cache.g[0], rows.g[0])
    # the row a 32-bit byte offset would have reached instead
    wrapped = ((capacity - 1) * n * n * 8 % (1 << 32)) // (n * n * 8)
    assert not torch.equal(cache.g[wrapped], rows.g[1])
    back = cache.load(torch.tensor([capacity - 1, 0])).tensors()
    for got, given in zip(back, rows):
        assert torch.equal(got, given.flip(0))
    assert not torch.equal(back.g[1], rows.g[1])           # row 0 is not what was written to the last row
    del cache, back
    torch.cuda.empty_cache()


STATS = {"clean": ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5)), "augmented": ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))}


def _uint8_batches():
    """Three uint8 batches with non-monotonic dataset indices."""
    out = []
    for k, index in enumerate(([40, 3, 17, 8, 29, 11, 0, 35, 21, 6, 44, 13, 27, 2, 38, 19],
                               [5, 47, 10, 33, 1, 24, 42, 15, 30, 7, 45, 18, 36, 9, 26, 4],
                               [23, 12, 46, 31, 14, 41, 20, 37, 16, 43, 22, 39, 25, 32, 28, 34])):
        g = torch.Generator().manual_seed(100 + k)
        views = []
        for _ in range(2):
            x = torch.randn(16, 3, 1, 1, generator=g) * 2.0 + torch.randn(16, 3, 32, 32, generator=g)
            views.append((x * 40.0 + 128.0).clamp(0, 255).to(torch.uint8))
        out.append({"clean": views[0], "augmented": views[1], "label": torch.arange(16) % 10,
                    "index": torch.tensor(index)})
    return out


def _two_epochs(dev, batches, teacher_cache, prefetch):
    """The stock student's own backward is not reproducible run to run as torch dispatches it by default: two runs
    WITHOUT the cache then differ in the last bits of most gradients, which Adam turns into up to 2e-4 of the attention
    biases.  Bit identity of two trainings needs a reproducible model, so the models of this test run with the math
    scaled_dot_product_attention and deterministic convolutions -- with both, two runs without the cache agree bit for
    bit (which of the two the difference came from was not separated).  Nothing of the package under test is switched."""
    from torch.nn.attention import SDPBackend, sdpa_kernel
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        with sdpa_kernel(SDPBackend.MATH):
            return _two_epochs_reproducible(dev, batches, teacher_cache, prefetch)
    finally:
        torch.backends.cudnn.deterministic = was


def _two_epochs_reproducible(dev, batches, teacher_cache, prefetch):
    from basd_amd import trainer as T
    from tools import stock_models as SM
    student, teacher = _toy_models("cnn", dev)
    calls = []
    teacher.model.stem.register_forward_hook(lambda m, i, o: calls.append(1))       # once per teacher forward
    torch.manual_seed(42)
    tr = T.Trainer(student, _config(), teacher, student_info=SM.probe_model(student, 32), mixup="fused",
                   image_stats=STATS, teacher_cache=teacher_cache, prefetch=prefetch)
    del calls[:]
    torch.manual_seed(11)
    losses, clean_seen = [], []
    tr.model.train()
    for epoch in range(2):
        for prepared in tr._prefetcher.iterate(batches):
            clean_seen.append("clean" in prepared)
            losses.append(tr.step_prepared(prepared)["loss"])
    tr._finish_loss()
    torch.cuda.synchronize()
    params = [p.detach().clone() for p in list(tr.model.parameters()) + list(tr.basd_loss.parameters())]
    return torch.stack(losses).cpu(), params, len(calls), clean_seen, tr


@pytest.mark.gpu
@pytest.mark.parametrize("prefetch", [0, 1])
def test_two_epochs_with_the_cache_equal_two_without(dev, prefetch):
    from basd_amd.teacher_cache import TeacherCache
    batches = _uint8_batches()
    plain = _two_epochs(dev, batches, None, prefetch)
    cached = _two_epochs(dev, batches, 48, prefetch)
    print(f"[teacher_cache] prefetch={prefetch}: losses {plain[0].tolist()} / {cached[0].tolist()}, "
          f"max |d param| = {max(float((x.double() - y.double()).abs().max()) for x, y in zip(plain[1], cached[1])):.3e}")
    assert torch.isfinite(plain[0]).all()
    assert torch.equal(plain[0], cached[0])                                 # every step's loss
    assert all(torch.equal(x, y) for x, y in zip(plain[1], cached[1]))      # the final parameters
    assert (plain[2], cached[2]) == (6, 3)                                  # teacher forwards
    assert plain[3] == [True] * 6 and cached[3] == [True] * 3 + [False] * 3
    tr = cached[4]
    assert isinstance(tr.teacher_cache, TeacherCache) and tr.teacher_cache.capacity == 48
    assert tr.teacher_cache.has(torch.arange(48)) and "teacher_cache" not in str(sorted(tr.state_dict(0)))


@pytest.mark.gpu
def test_errors_on_the_device_path(dev):
    from basd_amd.losses import BASDLoss
    from basd_amd.teacher_cache import TeacherCache
    E, B, n, d = 2, 3, 16, 64
    mod, logits, targets, students, teacher, attn = _loss_case(dev, "a", E, B, n, n, d, d)
    leaves = {l: s.clone().requires_grad_(True) for l, s in zip(mod.token_layers, students)}
    with pytest.raises(RuntimeError, match="no forward"):
        mod.last_teacher_side()
    mod(logits, targets, leaves, {0: teacher}, {0: attn})
    side = mod.last_teacher_side()
    sides = tuple(t.clone() for t in side)
    why = "mixing weights depend on the student"
    # two teacher layers' worth of arguments, in every form they can take
    with pytest.raises(ValueError, match=why):
        mod.forward_cached(logits, targets, leaves, [sides, sides])
    with pytest.raises(ValueError, match=why):
        mod.forward_cached(logits, targets, leaves, {0: sides, 1: sides})
    with pytest.raises(ValueError, match=why):
        mod.forward_cached(logits, targets, leaves, tuple(torch.stack([t, t]) for t in sides))
    with pytest.raises(ValueError, match="requires grad"):
        mod.forward_cached(logits, targets, leaves, (sides[0], sides[1].clone().requires_grad_(True), sides[2]))
    with pytest.raises(ValueError, match="does not fit"):
        mod.forward_cached(logits, targets, leaves, tuple(t[:2] for t in sides))
    # a multi-layer forward has no teacher side
    multi = BASDLoss(nn.CrossEntropyLoss(), d, d, E, n, config=SimpleNamespace(num_extraction_points=E),
                     teacher_has_cls_token=False).to(dev)
    gen = torch.Generator().manual_seed(3)
    two = {k: (torch.randn(B, n, d, generator=gen) + 2.0 * torch.randn(B, 1, d, generator=gen)).to(dev) for k in (0, 1)}
    multi(logits, targets, leaves, two, {0: attn, 1: attn})
    with pytest.raises(ValueError, match=why):
        multi.last_teacher_side()
    # a teacher that is not frozen
    mod(logits, targets, leaves, {0: teacher.clone().requires_grad_(True)}, {0: attn})
    with pytest.raises(ValueError, match="requires grad"):
        mod.last_teacher_side()
    mod.layer_selector.finish_pending()
    cache = TeacherCache(6, n, n, dev)
    cache.store(torch.tensor([4, 1, 2]), sides)
    with pytest.raises(KeyError, match="3"):
        cache.load(torch.tensor([4, 3, 2]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cache.store(torch.tensor([0, 1, 2]), tuple(t.cpu() for t in sides))
    torch.cuda.synchronize()
