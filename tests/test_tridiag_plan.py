"""The plan of a tridiagonal factorisation (basd_tridiag_plan_query): the route by order and tail hook, the shape of the
shared stage, where the ranks come from, the workspace layout, and the plans of two production shapes.  Host only, except
the last test, which holds the gated entry point to what the query says about it."""
import ctypes as C

import pytest

NONE, SHARED = 0, 1                      # front stage
TAIL2, PACKED = 1, 2                     # back stage (0: none)
SCALAR, VEC, VEC_FULL = 0, 1, 2          # shared-stage kernel
IN_BACK, SEPARATE = 1, 2                 # ranks (0: none)
QUADS, RANKED, GATED = 1, 2, 4           # flags
BUDGET_CAP = 128

ORDERS = list(range(2, 1101)) + [2048, 4096]
BATCHES = (1, 2, 6, 8, 9, 28, 64, 129)
TAILS, MEMBERS, PADS = (0, 1, 3), (0, 1, 5, 16), (-1, 3)


def _query(n, batch, flags, budget=0):
    from basd_amd import _lib
    out = (C.c_int * 12)()
    rc = _lib.query("basd_tridiag_plan_query", n, batch, flags, budget, C.cast(out, C.c_void_p))
    return rc, tuple(out)     # front, back, j_stop, variant, members, grid, threads, lds, ranks, gated, status_off, bytes


class _hooks:
    """Tuning hooks for the duration of a block (the reset first: no call can set pad = -1); the defaults afterwards."""

    def __init__(self, members=0, pad=-1, tail=1, threads=-1):
        self.values = (members, pad, -1, threads, tail, 1)

    def __enter__(self):
        from basd_amd import _lib
        assert _lib.query("basd_tridiag_tuning", *self.values) == 0

    def __exit__(self, *exc):
        from basd_amd import _lib
        _lib.query("basd_tridiag_tuning", -1, -1, -1, -1, -1, 1)


def _check(n, batch, flags, budget, tail, members, pad, plan, workspace_bytes):
    front, back, j_stop, variant, P, grid, threads, lds, ranks, gated, status_off, nbytes = plan
    where = (n, batch, flags, budget, tail, members, pad, plan)
    # route by order
    if tail == 0:
        want = (SHARED, NONE, n - 1)
    elif n <= 256:
        want = (NONE, TAIL2, 0)
    elif tail == 1 and n <= 384:
        want = (NONE, PACKED, 0)
    else:
        want = (SHARED, TAIL2, n - 256)
    assert (front, back, j_stop) == want, where
    # the shared stage
    if front == SHARED:
        assert 1 <= P <= min(16, -(-n // 32)) and (P * batch <= (budget or BUDGET_CAP) or P == 1), where
        if members:
            assert P <= members, where
        batch_pad = batch + pad if pad >= 0 else (batch + 7) // 8 * 8 if P > 1 else batch
        assert grid == P * batch_pad and threads == 1024 and lds == 36 * n, where
        quads = bool(flags & QUADS)
        assert variant == (VEC_FULL if quads and n % 8 == 0 else VEC if quads and n % 4 == 0 else SCALAR), where
    else:
        assert (variant, P, grid, threads, lds) == (0, 0, 0, 0, 0), where
    # ranks, the gate, the workspace
    assert ranks == (0 if not flags & RANKED else IN_BACK if back != NONE and n <= 1024 else SEPARATE), where
    assert gated == (back == PACKED), where
    assert nbytes == workspace_bytes and status_off == nbytes - 32, where


@pytest.mark.parametrize("tail", TAILS)
def test_every_plan_follows_the_route_rules(tail):
    """Over the grid of the dispatch tracer (tools/tridiag_dispatch_trace.cpp): every order, batch and hook setting, with
    and without quads and ranks, at the default budget and at budgets of 16 and 1 workgroups."""
    from basd_amd import _lib
    for members in MEMBERS:
        for pad in PADS:
            with _hooks(members, pad, tail):
                for batch in BATCHES:
                    for n in ORDERS:
                        ws = _lib.query("basd_tridiag_workspace_bytes", n, batch)
                        for flags, budget in ((0, 16), (QUADS | RANKED, 0), (RANKED, 1)):
                            rc, plan = _query(n, batch, flags, budget)
                            assert rc == 0, (n, batch, flags, budget, tail, members, pad)
                            _check(n, batch, flags, budget, tail, members, pad, plan, ws)
                        # the gated call: refused exactly where the gate does not take the shape
                        rc, gplan = _query(n, batch, QUADS | RANKED | GATED)
                        assert rc == (0 if plan[9] else _lib.EUNSUPPORTED), (n, batch, tail)
                        assert rc != 0 or gplan[:2] == (NONE, PACKED), (n, batch, tail)


def test_default_members_fill_the_budget():
    """Without the hook: one member per 32-row block, at most 16, as many as the budget lets be resident together."""
    for budget in (0, 16, 1):
        for batch in BATCHES:
            for n in range(385, 1101, 7):
                fit = [p for p in range(1, min(16, -(-n // 32)) + 1) if p * batch <= (budget or BUDGET_CAP)]
                assert _query(n, batch, QUADS, budget)[1][4] == (fit[-1] if fit else 1), (budget, batch, n)


def test_threads_hook_reaches_the_plan():
    with _hooks(threads=512):
        assert _query(768, 4, QUADS)[1][6] == 512
    assert _query(768, 4, QUADS)[1][6] == 1024


# read off the launches the dispatcher made for these shapes before it had a planner (tools/tridiag_dispatch_trace.cpp)
def test_production_shapes_keep_their_plan():
    from basd_amd import _lib
    # cfg-4, order 768, 28 matrices: 4 members each, 128 workgroups of tridiag_kernel<true, true>, then tail2 over 28
    rc, plan = _query(768, 28, QUADS | RANKED)
    assert rc == 0 and plan[:10] == (SHARED, TAIL2, 512, VEC_FULL, 4, 128, 1024, 27648, IN_BACK, 0)
    # order 384, 6 matrices: the packed kernel alone behind the 32-byte fill of the status words (no shared stage)
    rc, plan = _query(384, 6, QUADS | RANKED)
    assert rc == 0 and plan[:10] == (NONE, PACKED, 0, 0, 0, 0, 0, 0, IN_BACK, 1)
    assert plan[11] == _lib.query("basd_tridiag_workspace_bytes", 384, 6) == 6 * 2 * 384 * 20 + 32


def test_plan_query_rejects_what_the_factorisation_rejects():
    from basd_amd import _lib
    out = (C.c_int * 12)()
    ptr = C.cast(out, C.c_void_p)
    for flags in (0, QUADS | RANKED):
        assert _lib.query("basd_tridiag_plan_query", 4097, 1, flags, 0, ptr) == _lib.EUNSUPPORTED
        assert _lib.query("basd_tridiag_plan_query", 4096, 1, flags, 0, ptr) == 0
        assert _lib.query("basd_tridiag_plan_query", 1, 1, flags, 0, ptr) == _lib.EINVAL
        assert _lib.query("basd_tridiag_plan_query", 0, 1, flags, 0, ptr) == _lib.EINVAL
        assert _lib.query("basd_tridiag_plan_query", 64, 0, flags, 0, ptr) == _lib.EINVAL
        assert _lib.query("basd_tridiag_plan_query", 64, 1, flags, 0, None) == _lib.EINVAL
    assert _lib.query("basd_tridiag_plan_query", 64, 1, 8, 0, ptr) == _lib.EINVAL          # no such flag


def test_tail_hook_takes_only_its_routes():
    """tail = 2 was the four-barrier tail kernel: the number is not reused, the call is refused and nothing changes."""
    from basd_amd import _lib
    with _hooks(tail=3):
        before = _query(320, 2, QUADS)
        for tail in (2, 4, 7):
            assert _lib.query("basd_tridiag_tuning", 9, 9, -1, -1, tail, 0) == _lib.EINVAL
        assert _query(320, 2, QUADS) == before and before[1][:2] == (SHARED, TAIL2)
    assert _query(320, 2, QUADS)[1][:2] == (NONE, PACKED)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [256, 384, 385])
def test_gated_entry_point_takes_what_the_query_says(n):
    """basd_tridiag_ranked_gated answers BASD_EUNSUPPORTED exactly where the plan says the gate does not take the shape;
    where it does, with the word set beforehand (basd_flag_set on the same stream), ranks and factorisation are those of
    basd_tridiag_ranked bit for bit."""
    import torch
    from basd_amd import _lib, ops
    dev, batch, M = "cuda:0", 2, 4 * n
    accepted = bool(_query(n, batch, QUADS | RANKED)[1][9])
    assert accepted == (n == 384)
    g = torch.Generator().manual_seed(n)
    x = torch.randn(batch, M, n, generator=g)
    G0 = (x.transpose(1, 2) @ x / M).to(dev)
    ref = ops.tridiagonalise(G0.clone(), mp_rank=(M, n, n - 1, batch, None))

    G = G0.clone()
    f32 = dict(device=dev, dtype=torch.float32)
    d, e, tau = (torch.zeros((batch, n), **f32) for _ in range(3))
    vh = torch.zeros((batch, n, n), **f32)
    work = torch.zeros((_lib.query("basd_tridiag_workspace_bytes", n, batch),), device=dev, dtype=torch.uint8)
    ranks = torch.full((batch,), -1, device=dev, dtype=torch.int32)
    go = torch.zeros((1,), device=dev, dtype=torch.int32)
    st = torch.cuda.current_stream().cuda_stream
    _lib.call("basd_flag_set", go.data_ptr(), 5, st)
    rc = _lib.query("basd_tridiag_ranked_gated", G.data_ptr(), n * n, n, batch, d.data_ptr(), e.data_ptr(), tau.data_ptr(),
                    vh.data_ptr(), work.data_ptr(), batch, (1 + (n / M) ** 0.5) ** 2, n - 1, ranks.data_ptr(), None,
                    go.data_ptr(), 5, 1500, st)
    torch.cuda.synchronize()
    assert rc == (0 if accepted else _lib.EUNSUPPORTED)
    if not accepted:
        assert torch.equal(G, G0) and ranks.tolist() == [-1] * batch          # nothing was queued
        return
    assert work[-32:].view(torch.int32).tolist() == [0] * 8 and ref.err.tolist() == [0] * 8
    assert torch.equal(ranks, ref.ranks)
    for name, got in (("d", d), ("e", e), ("tau", tau), ("vh", vh)):
        assert torch.equal(got, getattr(ref, name)), name
