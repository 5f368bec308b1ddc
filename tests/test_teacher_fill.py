"""The teacher side of a set of images computed by itself (basd_procrustes_teacher_side, ``ops.procrustes_teacher_side``,
``BASDLoss.teacher_side``) and what the trainer builds on it: ``Trainer.fill_teacher_cache`` and partly cached steps
(``Trainer(teacher_partial=k)``).  Host only: the split rule, the plan query against the uncached planner, the padding
rule and the option logic.  On the GPU: rows bit for bit those of ``forward`` whatever else is in the call, ``as_batch``,
freshness, strided teacher maps, a partly cached loss call, a filled cache in front of an epoch and a partly cached
trainer step."""
import ctypes as C
import dataclasses
import os
import sys

import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_procrustes_plan import FIELDS, PTR, _args                                      # noqa: E402
from test_teacher_cache import (PLANNED, SMALL, STATS, _config, _loss_case, _run, _same, _toy_models,   # noqa: E402
                                _uint8_batches)

# fields of basd_procrustes_plan_query_teacher_side that are the uncached query's; every other field is 0 ("none")
TEACHER_FIELDS = ("center", "gram_split", "w_borrow_floats", "lds_center", "lds_gram")
CASES = {c[0]: c for c in SMALL}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _query(a, name):
    from basd_amd import _lib
    out = (C.c_long * len(FIELDS))()
    rc = _lib.query(name, C.addressof(a) if a is not None else None, C.cast(out, C.c_void_p))
    return rc, dict(zip(FIELDS, out))


# ---------------------------------------------------------------------------------------------------------------------
# not marked gpu
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("GB,d_t,want", [(3, 64, 1), (3, 512, 2), (3, 1024, 4), (300, 1024, 3), (256, 2048, 4),
                                         (64, 1536, 6), (1024, 2048, 1), (1023, 512, 1)])
def test_teacher_gram_splits(GB, d_t, want):
    from basd_amd import ops
    assert ops.teacher_gram_splits(GB, d_t) == want


@pytest.mark.parametrize("case", PLANNED, ids=[c[0] for c in PLANNED])
@pytest.mark.parametrize("offered", [(), ("k_prime", "dx", "uw_ce"), ("k_prime", "dx", "uw_ce", "jac_ws", "g_split")],
                         ids=["forward", "step", "step+workspaces"])
def test_teacher_side_plan_is_the_teacher_half_of_the_uncached_plan(case, offered):
    _, E, B, n_s, n_t, d_s, d_t = case
    a = _args(E, 1, B, n_s, n_t, d_s, d_t, offered=offered)
    rc_u, plain = _query(a, "basd_procrustes_plan_query")
    rc_t, side = _query(a, "basd_procrustes_plan_query_teacher_side")
    assert rc_u == 0 and rc_t == 0, (case, rc_u, rc_t)
    for name in FIELDS:
        want = plain[name] if name in TEACHER_FIELDS else 0
        assert side[name] == want, (case, offered, name, side[name], want)
    assert side["center"] == 4 and side["lds_center"] > 0 and side["lds_gram"] > 0       # per group: L == 1, G == 1
    assert side["gram_split"] == int("g_split" in offered)
    # nothing of the student is read: the same answer with its fields blank
    blank = _args(E, 1, B, n_s, n_t, d_s, d_t, offered=offered)
    blank.E = blank.d_s = blank.s_sb = blank.s_sn = 0
    blank.student_ptrs = blank.student_host_ptrs = None
    assert _query(blank, "basd_procrustes_plan_query_teacher_side") == (rc_t, side)


def test_teacher_side_plan_status_is_the_teacher_side_predicates():
    from basd_amd import _lib
    name = "basd_procrustes_plan_query_teacher_side"
    out = (C.c_long * len(FIELDS))()
    ptr = C.cast(out, C.c_void_p)
    good = _args(2, 1, 3, 16, 16, 64, 64)
    assert _lib.query(name, C.addressof(good), ptr) == 0
    assert _lib.query(name, None, ptr) == _lib.EINVAL
    assert _lib.query(name, C.addressof(good), None) == _lib.EINVAL
    # the centring kernel's tile past LDS (plan::center_fits: 4 * (66 n + 64) <= 150 KiB, n <= 580): no route in either
    for n, status in ((580, 0), (581, _lib.EUNSUPPORTED)):
        a = _args(2, 1, 3, n, n, 64, 64)
        rc_u, plain = _query(a, "basd_procrustes_plan_query")
        rc_t, side = _query(a, name)
        assert (rc_u, rc_t) == (status, status), (n, rc_u, rc_t)
        assert side["center"] == plain["center"] == (4 if status == 0 else 0)
    # more than one teacher layer (G == E): the uncached call takes it, the teacher half alone does not
    multi = _args(2, 3, 3, 16, 16, 64, 64)
    assert multi.G == 2 and _lib.query("basd_procrustes_plan_query", C.addressof(multi), ptr) == 0
    rc, side = _query(multi, name)
    assert rc == _lib.EUNSUPPORTED and all(v == 0 for v in side.values())
    layers = _args(2, 1, 3, 16, 16, 64, 64)
    layers.L = 2
    assert _lib.query(name, C.addressof(layers), ptr) == _lib.EUNSUPPORTED
    for field, value in (("L", 0), ("G", 0), ("B", 0), ("n", 15), ("d_t", 0), ("B", 65536)):
        bad = _args(2, 1, 3, 16, 16, 64, 64)
        setattr(bad, field, value)
        assert _lib.query(name, C.addressof(bad), ptr) == _lib.EINVAL, field


def test_teacher_rows_padding_rule():
    from basd_amd.trainer import _teacher_rows
    T_, F_ = True, False

    def rows(filled, k):
        got = _teacher_rows(filled, k)
        if got is not None:
            assert got.dtype == torch.int64 and got.dim() == 1
        return None if got is None else got.tolist()

    assert rows([T_] * 8, 4) == []                                         # no misses: a cached step
    assert rows([T_] * 8, 1) == []
    # the misses in batch order, then the first filled positions in batch order
    assert rows([T_, T_, T_, T_, T_, F_, T_, T_], 4) == [5, 0, 1, 2]
    assert rows([F_, T_, T_, T_, T_, T_, T_, T_], 4) == [0, 1, 2, 3]
    assert rows([T_, F_, T_, F_, T_, T_, T_, T_], 4) == [1, 3, 0, 2]
    assert rows([T_, F_, T_, F_, T_, T_, T_, T_], 2) == [1, 3]             # a multiple already: no padding
    assert rows([T_, F_, T_, F_, T_, F_, T_, T_], 2) == [1, 3, 5, 0]
    assert rows([F_, F_, T_, F_, F_, T_, F_, T_], 4) is None               # 5 of 8 pad to 8: the uncached step
    assert rows([F_, F_, F_, F_, T_, T_, T_, T_], 4) == [0, 1, 2, 3]       # 4 of 8 need no padding
    assert rows([F_] * 8, 4) is None and rows([F_] * 8, 1) is None         # all missing
    assert rows([T_, F_, F_, T_, F_, T_, F_, F_], 1) == [1, 2, 4, 6, 7]    # k = 1: exactly the misses
    assert rows([F_] * 7 + [T_], 1) == list(range(7))
    assert rows([F_] * 7 + [T_], 2) is None
    assert rows(torch.tensor([T_, F_, T_]), 2) == [1, 0]                   # a bool tensor is taken as well
    assert rows([F_], 1) is None and rows([T_], 1) == []


def test_trainer_option_host_logic():
    from basd_amd import trainer as T
    from tools import stock_models as SM
    from test_trainer_step import OracleBASD
    student, cnn_teacher = _toy_models("cnn")
    info = SM.probe_model(student, 32)
    common = dict(student_info=info, loss_cls=OracleBASD, mixup=False)
    with pytest.raises(ValueError, match="needs teacher_cache"):
        T.Trainer(student, _config(), cnn_teacher, teacher_partial=4, **common)
    for bad in (-1, True, False, 2.0, "4", None):
        with pytest.raises(ValueError, match="teacher_partial must be"):
            T.Trainer(student, _config(), cnn_teacher, teacher_cache=64, teacher_partial=bad, **common)
    assert T.Trainer(student, _config(), cnn_teacher, **common).teacher_partial == 0
    assert T.Trainer(student, _config(), cnn_teacher, teacher_cache=64, teacher_partial=4, **common).teacher_partial == 4

    batch = {"clean": torch.randn(4, 3, 32, 32), "augmented": torch.randn(4, 3, 32, 32), "label": torch.arange(4)}
    indexed = dict(batch, index=torch.tensor([9, 2, 0, 1]))
    student, vit_teacher = _toy_models("vit")
    assert vit_teacher.feature_format == "token"
    tokens = T.Trainer(student, _config(), vit_teacher, **common)
    with pytest.raises(ValueError, match="mixing weights depend on the student"):
        tokens.fill_teacher_cache([indexed], as_batch=4)
    student, cnn_teacher = _toy_models("cnn")
    with pytest.raises(ValueError, match="teacher_cache=None"):
        T.Trainer(student, _config(), cnn_teacher, **common).fill_teacher_cache([indexed], as_batch=4)
    tr = T.Trainer(student, _config(), cnn_teacher, teacher_cache=64, **common)
    for bad in (0, -4, True, 4.0, None):
        with pytest.raises(ValueError, match="as_batch must be"):
            tr.fill_teacher_cache([indexed], as_batch=bad)
    with pytest.raises(KeyError, match="index"):
        tr.fill_teacher_cache([batch], as_batch=4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tr.fill_teacher_cache([indexed], as_batch=4)
    assert tr.teacher_cache == 64                                          # nothing was built, nothing stored
    assert tr.fill_teacher_cache([], as_batch=4) == 0
    # an int cache decides nothing yet: the step is the uncached one, and teacher_rows says so
    partial = T.Trainer(student, _config(), cnn_teacher, teacher_cache=64, teacher_partial=2, **common)
    prepared = partial.prepare_batch(indexed)
    assert prepared["teacher_rows"] is None and prepared["teacher_cached"] is False and prepared["clean"].shape[0] == 4


def test_teacher_side_argument_checks():
    from basd_amd import ops
    from basd_amd.losses import BASDLoss
    from types import SimpleNamespace
    tokens, attn = torch.randn(3, 16, 64), torch.full((3, 1, 16, 16), 1.0 / 16)
    for bad_tokens, bad_attn in ((tokens[0], attn), (tokens, attn[0]), (tokens, attn[:2]), (tokens, attn[:, :, :, :8])):
        with pytest.raises(ValueError, match="ONE teacher layer"):
            ops.procrustes_teacher_side(bad_tokens, bad_attn, False, 16)
    for bad in (0, -1, True, 16.0):
        with pytest.raises(ValueError, match="n_s must be"):
            ops.procrustes_teacher_side(tokens, attn, False, bad)
    for bad in (0, -3, True, 3.0):
        with pytest.raises(ValueError, match="as_batch must be"):
            ops.procrustes_teacher_side(tokens, attn, False, 16, as_batch=bad)
    with pytest.raises(ValueError, match="requires grad"):
        ops.procrustes_teacher_side(tokens.clone().requires_grad_(True), attn, False, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.procrustes_teacher_side(tokens, attn, False, 16)
    mod = BASDLoss(nn.CrossEntropyLoss(), 64, 64, 2, 16, config=SimpleNamespace(num_extraction_points=2),
                   teacher_has_cls_token=False)
    with pytest.raises(ValueError, match="ONE teacher layer"):
        mod.teacher_side({0: tokens, 1: tokens}, {0: attn, 1: attn})
    with pytest.raises(ValueError, match="requires grad"):
        mod.teacher_side({0: tokens.clone().requires_grad_(True)}, {0: attn})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mod.teacher_side({0: tokens}, {0: attn})


# ---------------------------------------------------------------------------------------------------------------------
# marked gpu
# ---------------------------------------------------------------------------------------------------------------------
def _forward(mod, logits, targets, students, teacher, attn):
    return _run(mod, logits, targets, students, lambda lg, tg, leaves: mod(lg, tg, leaves, {0: teacher}, {0: attn}))


def _equal_sides(got, want):
    return all(x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y) for x, y in zip(got, want))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["a", "c", "d", "e", "f", "g"])
def test_teacher_side_rows_are_the_rows_of_forward(dev, name):
    """``forward`` at B = 3, then ``teacher_side`` on subsets, single rows and the reversed batch with ``as_batch=3``:
    every row bit for bit the row of ``last_teacher_side()``.  A derived condition, not a tolerance: the same kernels
    on the same inputs with the same fold order, each working per sample."""
    from basd_amd import ops
    case = CASES[name]
    _, E, B, n_s, n_t, d_s, d_t = case
    mod, logits, targets, students, teacher, attn = _loss_case(dev, *case)
    _forward(mod, logits, targets, students, teacher, attn)
    want = tuple(t.clone() for t in mod.last_teacher_side())
    mod.layer_selector.finish_pending()
    components, ranks = mod.last_components, dict(mod.layer_selector.subspace_ranks)
    n = min(n_s, n_t)
    for rows in ([2, 0], [0], [1], [2], [2, 1, 0]):
        idx = torch.tensor(rows, device=dev)
        side = mod.teacher_side({0: teacher[idx]}, {0: attn[idx]}, as_batch=B)
        assert isinstance(side, ops.TeacherSide)
        assert (side.g.shape, side.omega.shape, side.omega_t.shape) == ((len(rows), n, n), (len(rows), n_s), (len(rows), n))
        diff = max(float((x.double() - y[idx].double()).abs().max()) for x, y in zip(side, want))
        print(f"[teacher_fill] case {name} rows {rows}: max |d| = {diff:.3e}")
        assert _equal_sides(side, tuple(w[idx] for w in want)), (name, rows)
    # at B = 3 the split count of one row alone is the batch's wherever 1024 // B does not bind: as_batch=None too
    if ops.teacher_gram_splits(1, d_t) == ops.teacher_gram_splits(B, d_t):
        assert _equal_sides(mod.teacher_side({0: teacher[1:2]}, {0: attn[1:2]}), tuple(w[1:2] for w in want))
    # neither the selector nor last_components was touched
    assert mod.last_components is components and dict(mod.layer_selector.subspace_ranks) == ranks
    assert _equal_sides(mod.last_teacher_side(), want)


@pytest.mark.gpu
def test_as_batch_is_what_makes_the_rows_equal(dev):
    """d_t = 1024: a step at B = 300 folds 3 slabs per Gram, a call on 5 images by itself 4.  With ``as_batch=300`` the
    5 rows are the step's bit for bit; without it only the split counts are compared -- nothing is claimed about bits."""
    from basd_amd import ops
    E, B, n, d_s, d_t = 2, 300, 16, 64, 1024
    mod, logits, targets, students, teacher, attn = _loss_case(dev, "s", E, B, n, n, d_s, d_t)
    _forward(mod, logits, targets, students, teacher, attn)
    want = tuple(t[:5].clone() for t in mod.last_teacher_side())
    side = mod.teacher_side({0: teacher[:5]}, {0: attn[:5]}, as_batch=B)
    assert _equal_sides(side, want)
    tail = mod.teacher_side({0: teacher[290:]}, {0: attn[290:]}, as_batch=B)          # position 290 of 300 -> 0 of 10
    assert torch.equal(tail.g, mod.last_teacher_side().g[290:])
    assert (ops.teacher_gram_splits(B, d_t), ops.teacher_gram_splits(5, d_t)) == (3, 4)
    for batch, splits in ((B, 3), (5, 4)):
        a = _args(E, 1, batch, n, n, d_s, d_t)
        a.g_slabs, a.g_splits = PTR, ops.teacher_gram_splits(batch, d_t)
        assert a.g_splits == splits
        for query in ("basd_procrustes_plan_query", "basd_procrustes_plan_query_teacher_side"):
            rc, plan = _query(a, query)
            assert rc == 0 and plan["gram_split"] == 1, (batch, query)
    alone = mod.teacher_side({0: teacher[:5]}, {0: attn[:5]})
    print(f"[teacher_fill] 4 slabs against 3: max |d g| = {float((alone.g - want[0]).abs().max()):.3e} "
          f"(|g| up to {float(want[0].abs().max()):.3e})")
    assert torch.equal(alone.omega, want[1]) and torch.equal(alone.omega_t, want[2])      # no Gram in these two


@pytest.mark.gpu
def test_teacher_side_tensors_are_fresh(dev):
    mod, logits, targets, students, teacher, attn = _loss_case(dev, *CASES["e"])
    side = mod.teacher_side({0: teacher}, {0: attn})
    kept = tuple(t.clone() for t in side)
    other = _loss_case(dev, "b", *CASES["e"][1:])               # other values, the same shapes: the same plan and scratch
    assert not torch.equal(other[4], teacher)
    _forward(mod, logits, targets, other[3], other[4], other[5])
    again = mod.teacher_side({0: other[4]}, {0: other[5]})
    torch.cuda.synchronize()
    assert _equal_sides(side, kept)
    assert not torch.equal(again.g, side.g) and again.g.data_ptr() != side.g.data_ptr()
    assert _equal_sides(again, mod.last_teacher_side())


@pytest.mark.gpu
@pytest.mark.parametrize("hw,d_t,n_s,dtype", [(7, 64, 49, torch.float32), (4, 512, 16, torch.float32),
                                              (5, 64, 16, torch.float32), (4, 512, 16, torch.bfloat16)],
                         ids=["49x64", "16x512-split", "25-to-16-gather", "bf16"])
def test_transposed_view_of_a_cnn_map(dev, hw, d_t, n_s, dtype):
    """A CNN teacher's (B, d_t, h, w) map arrives as the transposed view ``flatten(2).transpose(1, 2)``: feature stride
    h * w, token stride 1.  Its rows are those of the same tokens made contiguous."""
    from basd_amd import ops
    B = 3
    gen = torch.Generator().manual_seed(77)
    fmap = (torch.randn(B, d_t, hw, hw, generator=gen) + 2.0 * torch.randn(B, d_t, 1, 1, generator=gen)).to(dev, dtype)
    tokens = fmap.flatten(2).transpose(1, 2)
    assert tokens.stride() == (d_t * hw * hw, 1, hw * hw) and tokens.data_ptr() == fmap.data_ptr()
    N = hw * hw
    attn = torch.full((B, 1, 1, 1), 1.0 / N, device=dev).expand(B, 1, N, N)
    strided = ops.procrustes_teacher_side(tokens, attn, False, n_s, as_batch=B)
    dense = ops.procrustes_teacher_side(tokens.contiguous(), attn.contiguous(), False, n_s, as_batch=B)
    assert torch.isfinite(strided.g).all() and float(strided.g.abs().max()) > 0
    assert _equal_sides(strided, dense)
    one = ops.procrustes_teacher_side(tokens[1:2], attn[1:2], False, n_s, as_batch=B)
    assert _equal_sides(one, tuple(t[1:2] for t in dense))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["a", "e", "f"])
def test_partly_cached_loss_call(dev, name):
    """Row 1 from the forward's own side, rows 0 and 2 by ``teacher_side(as_batch=B)``: ``forward_cached`` on the three
    gives the forward's total, geo_layers and student gradients bit for bit."""
    from basd_amd.teacher_cache import TeacherCache
    case = CASES[name]
    _, E, B, n_s, n_t, d_s, d_t = case
    mod, logits, targets, students, teacher, attn = _loss_case(dev, *case)
    reference = _forward(mod, logits, targets, students, teacher, attn)
    side = mod.last_teacher_side()
    cache = TeacherCache(B + 8, min(n_s, n_t), n_s, dev)
    index = torch.tensor([7, 2, 10])
    cache.store(index[1:2], tuple(t[1:2] for t in side))
    assert cache.filled(index).tolist() == [False, True, False]
    missing = torch.tensor([0, 2], device=dev)
    cache.store(index[[0, 2]], mod.teacher_side({0: teacher[missing]}, {0: attn[missing]}, as_batch=B))
    assert cache.has(index)
    got = _run(mod, logits, targets, students, lambda lg, tg, leaves: mod.forward_cached(lg, tg, leaves, cache.load(index)))
    print(f"[teacher_fill] case {name}: total {reference[0].item():.9g} / {got[0].item():.9g}")
    assert _same(reference, got)


def _reproducible(fn):
    """The models of these tests run as those of test_two_epochs_with_the_cache_equal_two_without: math attention and
    deterministic convolutions, without which two runs of the stock student differ by themselves."""
    from torch.nn.attention import SDPBackend, sdpa_kernel
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        with sdpa_kernel(SDPBackend.MATH):
            return fn()
    finally:
        torch.backends.cudnn.deterministic = was


class _OneByOne(nn.Module):
    """A teacher that evaluates every image alone: independent of the batch it is called with by construction."""

    def __init__(self, inner):
        super().__init__()
        self.inner, self.seen = inner, []

    def forward_features(self, x):
        self.seen.append(x.shape[0])
        return torch.cat([self.inner.forward_features(x[i:i + 1]) for i in range(x.shape[0])])


def _toy_trainer(dev, one_by_one=False, **options):
    """(trainer, the batch sizes the teacher saw so far): the toy ResNet -> ViT pair, seeded as in test_teacher_cache."""
    from basd_amd import trainer as T
    from tools import stock_models as SM
    student, teacher = _toy_models("cnn", dev)
    if one_by_one:
        teacher = dataclasses.replace(teacher, model=_OneByOne(teacher.model))
        seen = teacher.model.seen
    else:
        seen = []
        teacher.model.stem.register_forward_hook(lambda m, i, o: seen.append(i[0].shape[0]))
    torch.manual_seed(42)
    tr = T.Trainer(student, _config(), teacher, student_info=SM.probe_model(student, 32), mixup="fused",
                   image_stats=STATS, **options)
    del seen[:]
    return tr, seen


def _params(tr):
    torch.cuda.synchronize()
    return [p.detach().clone() for p in list(tr.model.parameters()) + list(tr.basd_loss.parameters())]


def _epoch(tr, batches):
    """``_train_epoch`` with every step's loss kept."""
    losses, step = [], tr.step_prepared

    def recording(prepared):
        out = step(prepared)
        losses.append(out["loss"])
        return out

    tr.step_prepared = recording
    torch.manual_seed(11)
    tr._train_epoch(batches)
    del tr.step_prepared
    return torch.stack(losses).cpu()


@pytest.mark.gpu
def test_fill_then_train(dev):
    """The fill's batches are the training batches themselves in another order, at the same batch size: the teacher sees
    equal shapes (and every image at its training position), so the equality below rests on the determinism of the
    convolutions pinned here, not on the teacher being independent of the batch size, which no library promises."""
    from basd_amd.teacher_cache import TeacherCache
    batches = _uint8_batches()

    def plain():
        tr, seen = _toy_trainer(dev)
        return _epoch(tr, batches), _params(tr), list(seen)

    def filled():
        tr, seen = _toy_trainer(dev, teacher_cache=48)
        cpu_state, gpu_state = torch.get_rng_state(), torch.cuda.get_rng_state(dev)
        before, components = _params(tr), tr.basd_loss.last_components
        fill = [{k: v for k, v in b.items() if k in ("clean", "index")} for b in reversed(batches)]
        assert tr.fill_teacher_cache(fill, as_batch=16) == 48
        assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(dev), gpu_state)
        assert all(torch.equal(x, y) for x, y in zip(before, _params(tr)))
        assert isinstance(tr.teacher_cache, TeacherCache) and tr.teacher_cache.has(torch.arange(48))
        assert seen == [16, 16, 16]
        assert tr.basd_loss.last_components is components                    # the loss module ran no step
        del seen[:]
        prepared = tr.prepare_batch(batches[0])
        assert prepared["teacher_cached"] is True and "clean" not in prepared
        losses = _epoch(tr, batches)
        return losses, _params(tr), list(seen)

    want, got = _reproducible(plain), _reproducible(filled)
    print(f"[teacher_fill] losses {want[0].tolist()} / {got[0].tolist()}")
    assert torch.isfinite(want[0]).all() and want[2] == [16, 16, 16]
    assert got[2] == []                                                      # no teacher forward in the epoch
    assert torch.equal(want[0], got[0])
    assert all(torch.equal(x, y) for x, y in zip(want[1], got[1]))


@pytest.mark.gpu
def test_partly_cached_trainer_step(dev):
    """Both runs evaluate the teacher image by image (``_OneByOne``), which makes it independent of the batch size by
    construction -- what this test needs and a vendor convolution does not promise."""
    full = _uint8_batches()[0]
    batch = {k: v[:8] for k, v in full.items()}
    index = batch["index"]
    missing = [2, 5]
    seen_before = [i for i in range(8) if i not in missing]

    def rows_of(b, positions):
        return {k: v[positions] for k, v in b.items() if k in ("clean", "index")}

    def uncached():
        tr, seen = _toy_trainer(dev, one_by_one=True)
        tr.model.train()
        torch.manual_seed(11)
        out = tr.train_step(batch)
        tr._finish_loss()
        return out["loss"].cpu(), _params(tr), list(seen)

    def partial():
        tr, seen = _toy_trainer(dev, one_by_one=True, teacher_cache=48, teacher_partial=4)
        assert tr.fill_teacher_cache([rows_of(batch, seen_before)], as_batch=8) == 6
        cache = tr.teacher_cache
        assert cache.filled(index).tolist() == [i not in missing for i in range(8)] and seen == [6]
        del seen[:]
        padding = index[[0, 1]].to(dev)                                    # the first filled positions in batch order
        stored = [t[padding].clone() for t in (cache.g, cache.omega, cache.omega_t)]
        tr.model.train()
        torch.manual_seed(11)
        prepared = tr.prepare_batch(batch)
        assert prepared["teacher_rows"].tolist() == [2, 5, 0, 1] and prepared["teacher_cached"] is False
        assert prepared["clean"].shape[0] == 4 and prepared["augmented"].shape[0] == 8
        out = tr.step_prepared(prepared)
        result = out["loss"].cpu(), _params(tr), list(seen)
        assert cache.has(index)
        assert all(torch.equal(t[padding], s) for t, s in zip((cache.g, cache.omega, cache.omega_t), stored))
        assert "d_grass_sq" not in tr.basd_loss.last_components          # like a cached step: no selector
        # a fully cached batch: no clean view, no teacher
        del seen[:]
        prepared = tr.prepare_batch(batch)
        assert prepared["teacher_cached"] is True and prepared["teacher_rows"].numel() == 0 and "clean" not in prepared
        tr.step_prepared(prepared)
        assert seen == []
        # 5 missing of 8 pad to 8: the uncached step
        cache.clear()
        assert tr.fill_teacher_cache([rows_of(batch, [1, 4, 6])], as_batch=8) == 3
        del seen[:]
        prepared = tr.prepare_batch(batch)
        assert prepared["teacher_rows"] is None and prepared["clean"].shape[0] == 8
        tr.step_prepared(prepared)
        assert seen == [8] and cache.has(index)
        tr._finish_loss()
        return result

    want, got = _reproducible(uncached), _reproducible(partial)
    print(f"[teacher_fill] partly cached step: loss {want[0].item():.9g} / {got[0].item():.9g}")
    assert want[2] == [8] and got[2] == [4]
    assert torch.isfinite(want[0]) and torch.equal(want[0], got[0])
    assert all(torch.equal(x, y) for x, y in zip(want[1], got[1]))


@pytest.mark.gpu
def test_nothing_moved_without_the_options(dev):
    batch = _uint8_batches()[0]
    keys = ["augmented", "clean", "mixed_targets", "targets"]
    cache_keys = sorted(keys + ["index", "index_host", "teacher_cached"])
    tr, _ = _toy_trainer(dev)
    assert sorted(tr.prepare_batch(batch)) == keys
    tr, _ = _toy_trainer(dev, teacher_cache=48)
    assert tr.teacher_partial == 0 and sorted(tr.prepare_batch(batch)) == cache_keys
    tr, _ = _toy_trainer(dev, teacher_cache=48, teacher_partial=4)
    prepared = tr.prepare_batch(batch)
    assert sorted(prepared) == sorted(cache_keys + ["teacher_rows"]) and prepared["teacher_rows"] is None
