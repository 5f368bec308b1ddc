"""The host frame of the Procrustes call (``ops.procrustes_forward`` / ``ops.procrustes_forward_cached``), on the GPU:
a plan rebuilt after the plan cache was cleared gives the bits of the plan it replaces, and a warm call on the same
tensors uploads no constant table and returns the same bits every time.  Behaviour only: nothing here reads how the
frame is written."""
import pytest
import torch

# (E, B, n_s, n_t, d_s, d_t): cases "a" and "e" (split teacher Gram) of tests/test_teacher_cache.py
CASES = {"a": (2, 3, 16, 16, 64, 64), "e": (2, 3, 16, 16, 64, 512)}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _inputs(dev, E, B, n_s, n_t, d_s, d_t):
    """(students, [teacher], [attention], mix) for ONE teacher layer: randn with a fixed seed, softmax attention."""
    gen = torch.Generator().manual_seed(100 * B + d_t)
    students = [torch.randn(B, n_s, d_s, generator=gen).to(dev) for _ in range(E)]
    teacher = (torch.randn(B, n_t, d_t, generator=gen) + 2.0 * torch.randn(B, 1, d_t, generator=gen)).to(dev)
    attn = torch.softmax(torch.randn(B, 2, n_t, n_t, generator=gen), dim=-1).to(dev)
    return students, [teacher], [attn], torch.ones(E, 1, device=dev)


def _both(ops, students, teachers, attns, mix, **kw):
    """One uncached call, then one cached call fed from its teacher side copied to fresh tensors."""
    plain = ops.procrustes_forward(students, teachers, attns, mix, False, **kw)
    side = ops.TeacherSide(*(t.clone() for t in plain.teacher_side))
    return plain, ops.procrustes_forward_cached(students, side, **kw)


@pytest.mark.gpu
def test_a_plan_rebuilt_after_eviction_gives_the_same_bits(dev):
    """Nine batch sizes of case "a", both entry points in turn: 18 plans pass through a cache that holds 8, so the plans
    of B = 1 are dropped with the ninth and again with the seventeenth.  The cache never holds more than 8, and B = 1
    called again -- on plans built anew -- returns the ``loss_b`` and ``a_prime`` of its first call, bit for bit."""
    from basd_amd import ops
    E, _, n_s, n_t, d_s, d_t = CASES["a"]
    torch.cuda.synchronize()
    ops._PROCRUSTES_PLANS.clear()
    try:
        first = None
        for B in range(1, 10):
            plain, cached = _both(ops, *_inputs(dev, E, B, n_s, n_t, d_s, d_t))
            assert len(ops._PROCRUSTES_PLANS) <= 8
            assert torch.equal(plain.loss_b, cached.loss_b) and torch.equal(plain.a_prime, cached.a_prime)
            if B == 1:
                first = [t.clone() for ctx in (plain, cached) for t in (ctx.loss_b, ctx.a_prime)]
        # inserts 9 and 17 cleared the cache: B = 1 has to build its two plans again
        held = len(ops._PROCRUSTES_PLANS)
        plain, cached = _both(ops, *_inputs(dev, E, 1, n_s, n_t, d_s, d_t))
        assert len(ops._PROCRUSTES_PLANS) == held + 2 <= 8
        again = [t for ctx in (plain, cached) for t in (ctx.loss_b, ctx.a_prime)]
        assert all(torch.isfinite(t).all() for t in again)
        assert all(torch.equal(x, y) for x, y in zip(first, again))
    finally:
        torch.cuda.synchronize()
        ops._PROCRUSTES_PLANS.clear()


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_a_warm_call_uploads_nothing_and_repeats_its_bits(dev, case):
    """With ``uwso_ce`` set, after 3 warm calls on the same tensors 5 more calls of each entry point leave the table of
    device constants (``ops._CONSTS``: the pointer tables, cached by value) as long as it was, and return the same
    ``uw`` and ``dx`` each time."""
    from basd_amd import ops
    students, teachers, attns, mix = _inputs(dev, *CASES[case])
    ce = torch.tensor([2.3], device=dev)
    side = ops.TeacherSide(*(t.clone() for t in ops.procrustes_forward(students, teachers, attns, mix, False).teacher_side))
    calls = {"forward": lambda: ops.procrustes_forward(students, teachers, attns, mix, False, uwso_ce=ce),
             "forward_cached": lambda: ops.procrustes_forward_cached(students, side, uwso_ce=ce)}
    for name, call in calls.items():
        for _ in range(3):
            warm = call()
        uw, dx = warm.uw.clone(), warm.dx.clone()
        assert uw.shape == (4 + 2 * len(students),) and torch.isfinite(uw).all() and torch.isfinite(dx).all(), name
        consts = len(ops._CONSTS)
        for _ in range(5):
            ctx = call()
            assert len(ops._CONSTS) == consts, name
            assert torch.equal(ctx.uw, uw) and torch.equal(ctx.dx, dx), name
