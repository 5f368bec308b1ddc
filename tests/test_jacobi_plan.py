"""The Jacobi dispatch plan (basd_jacobi_plan_query): invariants of every plan, the fits queries as views of the
planner, and the plans of the production shapes.  Host only: no GPU is touched."""
import ctypes as C

import pytest

LDS_LIMIT = 156 * 1024
STACKED8, STACKED4, PLAIN8, ODD_EVEN, PLAIN4, LDS16, BLOCK = 1, 2, 3, 4, 5, 6, 7


def _plan(rows_dot, rows_tot, n, batch, per_matrix_orders=False):
    from basd_amd import _lib
    out = (C.c_int * 8)()
    rc = _lib.query("basd_jacobi_plan_query", rows_dot, rows_tot, n, batch, int(per_matrix_orders),
                    C.cast(out, C.c_void_p))
    assert rc == 0, (rows_dot, rows_tot, n, batch, per_matrix_orders, rc)
    return tuple(out)     # route, lpp, epl, dot, threads, lds, bw, nblk


class _hooks:
    """Tuning hooks for the duration of a block; the defaults (automatic lanes, odd-even ordering) afterwards."""

    def __init__(self, lanes, ordering):
        self.values = (lanes, ordering)

    def __enter__(self):
        from basd_amd import _lib
        assert _lib.query("basd_jacobi_tuning", self.values[0]) == 0
        assert _lib.query("basd_jacobi_ordering", self.values[1]) == 0

    def __exit__(self, *exc):
        from basd_amd import _lib
        _lib.query("basd_jacobi_tuning", 0)
        _lib.query("basd_jacobi_ordering", 1)


def _check_plan(rows_dot, rows_tot, n, batch, plan):
    route, lpp, epl, dot, threads, lds, bw, nblk = plan
    where = (rows_dot, rows_tot, n, batch, plan)
    assert STACKED8 <= route <= BLOCK, where           # every order up to basd_jacobi_max_rows() has a kernel shape
    assert 0 < lds <= LDS_LIMIT, where
    assert 0 < threads <= 1024, where
    # zero-padded columns hold every row: the dot rows in the first `dot` elements per lane, riding rows in the rest
    if rows_tot > rows_dot:
        assert lpp * dot >= rows_dot and lpp * (epl - dot) >= rows_tot - rows_dot, where
    else:
        assert dot == epl and lpp * epl >= rows_tot, where
    if route == BLOCK:
        assert bw >= 2 and bw % 2 == 0 and nblk % 2 == 0 and bw * nblk >= n, where
        assert threads == lpp * bw, where
    else:
        assert threads % 64 == 0 and (bw, nblk) == (0, 0), where


def test_every_plan_fits_the_cu():
    for batch in (1, 128, 256, 1024):
        for n in range(1, 1025):
            _check_plan(n, n, n, batch, _plan(n, n, n, batch))
        for n in range(1, 513):
            _check_plan(n, 2 * n, n, batch, _plan(n, 2 * n, n, batch))


def test_fits_queries_are_views_of_the_planner():
    """plain4_fits(n): the plain 4-lane LDS shape fits order n.  With 4 lanes forced and the round-robin ordering the
    planner takes that shape for every order from 7 on that fits, also below the order 40 from which the automatic
    choice (batches >= 128) uses it; the query has always answered 0 below 40 and its callers rely on that, so the
    equivalence holds from n_even >= 40 and both sides are pinned below."""
    from basd_amd import _lib
    with _hooks(4, 0):
        forced4 = {n: _plan(n, n, n, 128)[0] for n in range(1, 1025)}
    for n in range(1, 1025):
        fits = _lib.query("basd_jacobi_plain4_fits", n)
        if n >= 39:
            assert (fits == 1) == (forced4[n] == PLAIN4), n
        else:
            assert fits == 0 and (forced4[n] == PLAIN4) == (n >= 7), n
        lds16 = _plan(n, n, n, 1, per_matrix_orders=True)[0] == LDS16
        assert (_lib.query("basd_jacobi_lds_square_fits", n) == 1) == lds16, n
    assert [n for n in range(1, 1025) if _lib.query("basd_jacobi_plain4_fits", n)] == list(range(39, 197))
    assert [n for n in range(1, 1025) if _lib.query("basd_jacobi_lds_square_fits", n)] == list(range(1, 193))
    for n in (-1, 0):
        assert _lib.query("basd_jacobi_plain4_fits", n) == 0 and _lib.query("basd_jacobi_lds_square_fits", n) == 0


# (rows_dot, rows_tot, n, batch, per-matrix orders) -> plan, read off the launches that the dispatcher made for these
# shapes before it had a planner (tools/jacobi_dispatch_trace.cpp: kernel template arguments, block, LDS bytes, grid)
PRODUCTION = [
    # cfg-2: 1024 transposed cores of 49 x 49; the stacked form 98 x 49
    ((49, 49, 49, 1024, False), (ODD_EVEN, 4, 16, 16, 128, 7696, 0, 0)),
    ((49, 98, 49, 1024, False), (STACKED4, 4, 28, 14, 128, 24400, 0, 0)),
    # cfg-5: 256 cores of 144 x 144; stacked 288 x 144 when the two-pass solver is not used
    ((144, 144, 144, 256, False), (ODD_EVEN, 4, 36, 36, 320, 44968, 0, 0)),
    ((144, 288, 144, 256, False), (BLOCK, 16, 20, 10, 960, 155520, 60, 4)),
    # cfg-4: cores of 196 x 196 in batches >= 128; stacked 392 x 196
    ((196, 196, 196, 128, False), (ODD_EVEN, 4, 50, 50, 448, 79992, 0, 0)),
    ((196, 196, 196, 1024, False), (ODD_EVEN, 4, 50, 50, 448, 79992, 0, 0)),
    ((196, 392, 196, 128, False), (BLOCK, 16, 28, 14, 704, 159104, 44, 6)),
    ((196, 392, 196, 1024, False), (BLOCK, 16, 28, 14, 704, 159104, 44, 6)),
    # speculative principal-angle solves: per-matrix orders in LDS, orders >= 96 also as a plain batch
    ((57, 57, 57, 1, True), (LDS16, 16, 4, 4, 512, 15776, 0, 0)),
    ((168, 168, 168, 1, True), (LDS16, 16, 12, 12, 1024, 131712, 0, 0)),
    ((192, 192, 192, 1, True), (LDS16, 16, 12, 12, 1024, 150528, 0, 0)),
    ((168, 168, 168, 4, False), (ODD_EVEN, 4, 50, 50, 384, 68680, 0, 0)),
    ((192, 192, 192, 4, False), (ODD_EVEN, 4, 50, 50, 384, 78376, 0, 0)),
]


@pytest.mark.parametrize("shape,plan", PRODUCTION, ids=lambda v: "x".join(map(str, v)) if len(v) == 5 else "")
def test_production_shapes_keep_their_plan(shape, plan):
    assert _plan(*shape) == plan


def test_plan_query_rejects_what_the_solver_rejects():
    from basd_amd import _lib
    out = (C.c_int * 8)()
    ptr = C.cast(out, C.c_void_p)
    assert _lib.query("basd_jacobi_plan_query", 49, 98, 49, 4, 1, ptr) == _lib.EINVAL     # orders with riding rows
    assert _lib.query("basd_jacobi_plan_query", 0, 0, 4, 4, 0, ptr) == _lib.EINVAL
    assert _lib.query("basd_jacobi_plan_query", 4, 4, 4, 4, 0, None) == _lib.EINVAL
    too_long = _lib.query("basd_jacobi_max_rows") + 1
    assert _lib.query("basd_jacobi_plan_query", too_long, too_long, too_long, 1, 0, ptr) == 0 and out[0] == 0
