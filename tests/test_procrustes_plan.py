"""The plan of the Procrustes call (basd_procrustes_plan_query, csrc/procrustes_plan.h).  Host only: invariants of
every plan over a sweep of shapes, layouts, options and hooks, the plans of the production shapes, what the query
rejects, and the two hook / workspace mismatches that used to hand unwritten buffers to the backward.  On the GPU: the
kernels one call launches are those its plan names, and loss_b stays on the fp64 evaluation."""
import ctypes as C
import itertools

import pytest

KB = 1024
FIELDS = ("center", "project", "slab_width", "slabs", "gram_split", "chol", "cores", "svd", "finish", "rebuild_usigma",
          "grad", "usigma_in", "tr_part_floats", "w_borrow_floats", "lds_center", "lds_project", "lds_gram", "lds_chol",
          "lds_finish", "lds_grad")
STREAM_V4, STREAM, CENTER_MULTI, PER_GROUP = 1, 2, 3, 4
PROJECT_MULTI, PER_LAYER = 1, 2
TRANSPOSED, STACKED = 1, 2
SVD_TRANSPOSED, SVD_TWO_PASS, SVD_STACKED = 1, 2, 3
FINISH_T, FINALIZE_KPRIME_T, FINALIZE, FINALIZE_TILED = 1, 2, 3, 4
GRAD_NONE, GRAD_FUSED, GRAD_GEMM_MULTI = 0, 1, 2
IN_W, IN_W_STACK = 1, 2
OPTIONAL = ("k_prime", "dx", "raw", "w_stack", "jac_ws", "g_split", "uw_ce")
PTR = 0x1000          # stands for "offered": the planner tests presence and 16-byte alignment only


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _args(E, L, B, n_s, n_t, d_s, d_t, offered=(), s_bf16=False, s_aligned=True, s_pad=0, t_bf16=False, t_sd=1, t_pad=0):
    from basd_amd import _lib
    a = _lib.ProcrustesArgs()
    a.E, a.L, a.G, a.B, a.n_s, a.n_t, a.d_s, a.d_t, a.n = E, L, 1 if L == 1 else E, B, n_s, n_t, d_s, d_t, min(n_s, n_t)
    a.H, a.A, a.n_a, a.max_sweeps = 2, n_t, n_t, 20
    a.s_dtype, a.s_sn, a.s_sb, a.s_aligned = int(s_bf16), d_s + s_pad, (d_s + s_pad) * n_s, int(s_aligned)
    a.t_dtype, a.t_sd = int(t_bf16), t_sd
    a.t_sn, a.t_sb = (d_t + t_pad, (d_t + t_pad) * n_t) if t_sd == 1 else (1, n_t * d_t)
    for name in ("student_ptrs", "student_host_ptrs", "tok_ptrs", "attn_ptrs", "mix", "omega", "omega_t", "mu_t", "tc",
                 "mu_s", "tr_part", "tr_s", "a_prime", "g_all", "l_all", "W", "sigma", "jflags", "tr_t", "nuc", "loss_b"):
        setattr(a, name, PTR)
    if n_t > n_s:
        a.g0 = a.g1 = a.glam = PTR
    for name in offered:
        assert name in OPTIONAL, name
        setattr(a, "g_slabs" if name == "g_split" else name, PTR)
    a.g_splits = 4 if "g_split" in offered else 1
    if "dx" in offered:
        a.h = a.grad_layers = PTR
    if "w_stack" in offered:
        a.sigma_u = PTR
    if "uw_ce" in offered:
        a.uw_out = PTR
    return a


def _query(a):
    from basd_amd import _lib
    out = (C.c_long * len(FIELDS))()
    rc = _lib.query("basd_procrustes_plan_query", C.addressof(a), C.cast(out, C.c_void_p))
    return rc, dict(zip(FIELDS, out))


class _hooks:
    """basd_procrustes_tuning / basd_procrustes_finish_tuning for a block; the defaults afterwards."""

    def __init__(self, transposed, finish=1):
        self.values = (transposed, finish)

    def __enter__(self):
        from basd_amd import _lib
        _lib.query("basd_procrustes_tuning", self.values[0])
        _lib.query("basd_procrustes_finish_tuning", self.values[1])

    def __exit__(self, *exc):
        from basd_amd import _lib
        _lib.query("basd_procrustes_tuning", 1)
        _lib.query("basd_procrustes_finish_tuning", 1)


ORDERS = (4, 16, 20, 49, 64, 65, 100, 144, 196, 197, 252, 253, 576, 664, 665)


def _check(a, offered, rc, p):
    from basd_amd import _lib
    E, B, G, n, n_s, d_s, d_t = a.E, a.B, a.G, a.n, a.n_s, a.d_s, a.d_t
    where = (E, a.L, B, n_s, a.n_t, d_s, d_t, offered, p)
    if rc != 0:       # a stage without a route: the only ones in this sweep are tiles past LDS
        assert rc == _lib.EUNSUPPORTED and (p["center"] == 0 or p["chol"] == 0 or p["lds_gram"] < 0), where
        return
    # exactly one route per stage
    assert p["center"] in (STREAM_V4, STREAM, CENTER_MULTI, PER_GROUP) and p["project"] in (PROJECT_MULTI, PER_LAYER), where
    assert p["chol"] in (1, 2) and p["cores"] in (TRANSPOSED, STACKED) and p["gram_split"] == int("g_split" in offered), where
    if p["cores"] == TRANSPOSED:
        assert p["svd"] == SVD_TRANSPOSED and p["finish"] in (FINISH_T, FINALIZE_KPRIME_T, FINALIZE), where
        assert (p["finish"] == FINALIZE) == ("k_prime" not in offered), where
        assert "raw" not in offered or "w_stack" in offered, where
    else:
        assert p["svd"] == (SVD_TWO_PASS if "jac_ws" in offered else SVD_STACKED), where
        assert p["finish"] in (FINALIZE, FINALIZE_TILED), where
    assert p["rebuild_usigma"] == int(p["cores"] == TRANSPOSED and "raw" in offered), where
    assert p["usigma_in"] == (IN_W_STACK if p["rebuild_usigma"] else IN_W), where
    assert (p["grad"] != GRAD_NONE) == ("dx" in offered) and p["grad"] in (GRAD_NONE, GRAD_FUSED, GRAD_GEMM_MULTI), where
    # LDS of every named launch within what its entry point enforces
    assert 0 <= p["lds_center"] <= 150 * KB and 0 < p["lds_gram"] <= 156 * KB and 0 < p["lds_finish"] <= 156 * KB, where
    assert 0 < p["lds_chol"] <= (158 if p["chol"] == 1 else 156) * KB, where
    assert 0 < p["lds_project"] <= (96 * KB if p["project"] == PROJECT_MULTI else 4 * n_s), where
    assert p["lds_grad"] <= 4 * 64 * (64 + 68) and (p["lds_grad"] > 0) == (p["grad"] == GRAD_FUSED), where
    if p["finish"] == FINISH_T or p["grad"] == GRAD_FUSED:
        assert n <= 64, where
    # scratch
    assert p["slab_width"] == (32 if p["project"] == PROJECT_MULTI else 64), where
    assert p["slabs"] == -(-d_s // p["slab_width"]) and p["tr_part_floats"] == E * B * p["slabs"], where
    if p["center"] in (STREAM_V4, STREAM):
        assert p["w_borrow_floats"] == -(-n // 16) * G * B * d_t <= E * B * 2 * n * n and G > 1 and a.L >= 4, where
    else:
        assert p["w_borrow_floats"] == 0, where


def test_every_plan_names_one_route_per_stage_and_fits():
    option_sets = [(), ("k_prime",), ("k_prime", "dx", "uw_ce", "g_split"), ("k_prime", "dx", "jac_ws"),
                   ("k_prime", "raw"), ("k_prime", "dx", "raw", "w_stack", "jac_ws")]
    layouts = [dict(), dict(s_bf16=True, t_bf16=True), dict(s_aligned=False), dict(s_pad=1, t_pad=1), dict(t_sd=7)]
    seen = set()
    try:
        for hook, finish in itertools.product((0, 1, 2), (0, 1)):
            with _hooks(hook, finish):
                for n_s, n_t, (E, L, B), offered, d_s in itertools.product(
                        ORDERS, ORDERS, ((1, 1, 2), (2, 4, 64), (5, 3, 2), (4, 24, 32), (12, 4, 5462)), option_sets, (64, 68)):
                    if n_t != n_s and n_t not in (49, 196, 665):
                        continue
                    lay = layouts[(n_s + n_t + E + len(offered) + d_s // 4) % len(layouts)]
                    a = _args(E, L, B, n_s, n_t, d_s, 2048 if (n_s + E) % 3 == 0 else 68, offered, **lay)
                    rc, p = _query(a)
                    _check(a, offered, rc, p)
                    seen.add((p["center"], p["project"], p["chol"], p["cores"], p["svd"], p["finish"], p["grad"]))
    finally:
        _hooks(1, 1).__exit__()
    for stage, values in enumerate(((1, 2, 3, 4), (1, 2), (1, 2), (1, 2), (1, 2, 3), (1, 2, 3, 4), (0, 1, 2))):
        assert {s[stage] for s in seen if s[0]} >= set(values), (stage, values)      # the sweep reaches every route


STEP = ("k_prime", "dx", "uw_ce", "g_split")
# (E, L, B, n_s, n_t, d_s, d_t), offered -> the routes read off the launches the call made for these shapes before it had
# a planner (tools/procrustes_dispatch_trace.cpp, fp32 aligned inputs): centre, project, slabs, cores, svd, finish,
# rebuild, grad, U Sigma in, tr_part floats, floats borrowed from W
PRODUCTION = [
    ("cfg1", (4, 1, 32, 64, 1, 192, 512), STEP, (PER_GROUP, PROJECT_MULTI, 6, STACKED, SVD_STACKED, FINALIZE, 0, GRAD_GEMM_MULTI, IN_W, 768, 0)),
    ("cfg2", (4, 1, 256, 196, 49, 384, 2048), STEP, (PER_GROUP, PROJECT_MULTI, 12, TRANSPOSED, SVD_TRANSPOSED, FINISH_T, 0, GRAD_FUSED, IN_W, 12288, 0)),
    ("cfg4", (4, 24, 128, 196, 196, 768, 1024), STEP + ("jac_ws",), (STREAM_V4, PROJECT_MULTI, 24, TRANSPOSED, SVD_TRANSPOSED, FINALIZE_KPRIME_T, 0, GRAD_GEMM_MULTI, IN_W, 12288, 6815744)),
    ("cfg4-mixgrad", (4, 24, 128, 196, 196, 768, 1024), STEP + ("jac_ws", "raw", "w_stack"), (STREAM_V4, PROJECT_MULTI, 24, TRANSPOSED, SVD_TRANSPOSED, FINALIZE_KPRIME_T, 1, GRAD_GEMM_MULTI, IN_W_STACK, 12288, 6815744)),
    ("cfg5", (4, 1, 64, 576, 144, 768, 1536), STEP + ("jac_ws",), (PER_GROUP, PROJECT_MULTI, 24, TRANSPOSED, SVD_TRANSPOSED, FINALIZE_KPRIME_T, 0, GRAD_GEMM_MULTI, IN_W, 6144, 0)),
]


@pytest.mark.parametrize("name,shape,offered,want", PRODUCTION, ids=[p[0] for p in PRODUCTION])
def test_production_shapes_keep_their_plan(name, shape, offered, want):
    rc, p = _query(_args(*shape, offered))
    assert rc == 0
    got = tuple(p[k] for k in ("center", "project", "slabs", "cores", "svd", "finish", "rebuild_usigma", "grad",
                               "usigma_in", "tr_part_floats", "w_borrow_floats"))
    assert got == want and p["gram_split"] == 1 and p["chol"] == 1


def test_query_rejects_what_the_call_rejects():
    from basd_amd import _lib
    out = (C.c_long * len(FIELDS))()
    ptr = C.cast(out, C.c_void_p)
    good = _args(2, 1, 4, 49, 49, 64, 64)
    assert _lib.query("basd_procrustes_plan_query", C.addressof(good), ptr) == 0
    assert _lib.query("basd_procrustes_plan_query", None, ptr) == _lib.EINVAL
    assert _lib.query("basd_procrustes_plan_query", C.addressof(good), None) == _lib.EINVAL
    for field, value in (("E", 0), ("L", 0), ("B", 0), ("G", 3), ("n", 48), ("d_s", 0), ("B", 65536), ("E", 65536)):
        bad = _args(2, 1, 4, 49, 49, 64, 64)
        setattr(bad, field, value)
        if field == "E":
            bad.G = 1
        assert _lib.query("basd_procrustes_plan_query", C.addressof(bad), ptr) == _lib.EINVAL, field
    # tiles past LDS: no centring kernel for 665 core tokens
    assert _query(_args(1, 1, 2, 665, 665, 64, 64))[0] == _lib.EUNSUPPORTED


def test_hook_and_workspace_mismatches_plan_written_buffers():
    """Gradients through the mixing weights read U Sigma.  With the hook at 0 although w_stack is offered, and with the
    default hook below 128 cores, the cores are stacked and U Sigma is in W; hook 2 plans the transposed cores and rebuilds
    it in w_stack."""
    mix = ("k_prime", "raw", "w_stack")
    try:
        with _hooks(0):
            p = _query(_args(4, 24, 128, 196, 196, 768, 1024, mix))[1]          # E B = 512 >= 128
            assert (p["cores"], p["rebuild_usigma"], p["usigma_in"]) == (STACKED, 0, IN_W)
        with _hooks(1):
            p = _query(_args(2, 4, 3, 49, 49, 64, 64, mix))[1]                   # E B = 6 < 128
            assert (p["cores"], p["rebuild_usigma"], p["usigma_in"]) == (STACKED, 0, IN_W)
            p = _query(_args(4, 24, 128, 196, 196, 768, 1024, ("k_prime", "raw")))[1]      # nothing offered
            assert (p["cores"], p["rebuild_usigma"], p["usigma_in"]) == (STACKED, 0, IN_W)
        with _hooks(2):
            p = _query(_args(2, 4, 3, 49, 49, 64, 64, mix))[1]
            assert (p["cores"], p["rebuild_usigma"], p["usigma_in"]) == (TRANSPOSED, 1, IN_W_STACK)
    finally:
        _hooks(1, 1).__exit__()


# ---- on the GPU: one call launches what its plan names ---------------------------------------------------------------
KERNELS = {     # plan field -> value -> kernels of that route (substrings of the profiler's names), once each
    "center": {STREAM_V4: ("teacher_mix_stream_v4_kernel", "teacher_center_apply_kernel"),
               STREAM: ("teacher_mix_stream_kernel", "teacher_center_apply_kernel"),
               CENTER_MULTI: ("teacher_center_multi_kernel",), PER_GROUP: ("teacher_center_kernel",)},
    "project": {PROJECT_MULTI: ("student_project_v4_kernel",), PER_LAYER: ("student_project_kernel",)},
    # (the stacked product picks its LDS or its tiled kernel inside the one entry point: either name counts)
    "cores": {TRANSPOSED: ("stack_product_t_kernel",), STACKED: ("stack_product_kernel|stack_product_global_kernel",)},
    "finish": {FINISH_T: ("procrustes_finish_t_kernel",), FINALIZE_KPRIME_T: ("procrustes_finalize_kernel", "kprime_z_kernel", "kprime_from_z_kernel"),
               FINALIZE: ("procrustes_finalize_kernel",), FINALIZE_TILED: ("procrustes_finalize_kernel", "kprime_tiled_kernel")},
    "grad": {GRAD_NONE: (), GRAD_FUSED: ("student_grad_fused_kernel",), GRAD_GEMM_MULTI: ("gemm_tn_kernel", "student_grad_kernel")},
    "gram_split": {0: (), 1: ("gram_f64_reduce_kernel",)},
    "chol": {1: ("chol_f64_kernel",), 2: ("chol_f64_blocked_kernel",)},
    "rebuild_usigma": {0: (), 1: ("m_stash_kernel", "ustack_from_x_kernel", "ustack_place_kernel")},
    # the SVD's kernels are the Jacobi's business (tests/test_jacobi_plan.py); of its routes only the two-pass solver has
    # kernels of its own
    "svd": {SVD_TRANSPOSED: (), SVD_TWO_PASS: ("jacobi_top_logged_kernel", "jacobi_apply_log_kernel"), SVD_STACKED: ()},
}
ALL_ROUTE_KERNELS = sorted({k for routes in KERNELS.values() for ks in routes.values() for k in ks})


def _fp64_loss_b(students, teachers, attn, mix):
    """relational.py:22-50 in fp64 on the same (for bf16: the same rounded) inputs; one attention map for all layers."""
    import torch
    from oracle import basd_oracle as O
    n_s = students[0].shape[1]
    w3 = O.token_weights(attn.float().cpu(), False, n_s).double().unsqueeze(-1)
    rows = []
    for e, s in enumerate(students):
        t = sum(mix[e, l].double().cpu() * teachers[l].double().cpu() for l in range(len(teachers)))
        t = O.resample_tokens(t, n_s).double()
        s64 = s.double().cpu()
        s_w = w3.sqrt() * (s64 - (w3 * s64).sum(1, keepdim=True))
        t_w = w3.sqrt() * (t - (w3 * t).sum(1, keepdim=True))
        rows.append(s_w.square().sum((1, 2)) + t_w.square().sum((1, 2))
                    - 2 * torch.linalg.svdvals(torch.bmm(s_w.transpose(1, 2), t_w)).sum(-1))
    return torch.stack(rows)


CASES = {   # E, B, n_s, n_t, d_s, d_t, L, bf16 students, grad_layers, mixing-weight gradient, hook,
            # expected (centre, project, cores, svd, finish, U Sigma rebuilt, grad)
    "a-transposed-fused-finish": (2, 64, 49, 49, 64, 96, 1, False, False, False, 1,
                                  (PER_GROUP, PROJECT_MULTI, TRANSPOSED, SVD_TRANSPOSED, FINISH_T, 0, GRAD_NONE)),
    "b-stacked-finalize-fused-grad": (2, 3, 196, 49, 64, 96, 1, False, True, False, 1,
                                      (PER_GROUP, PROJECT_MULTI, STACKED, SVD_STACKED, FINALIZE, 0, GRAD_FUSED)),
    "c-per-layer-bf16-gemm-multi": (2, 2, 20, 20, 68, 96, 1, True, True, False, 1,
                                    (PER_GROUP, PER_LAYER, STACKED, SVD_STACKED, FINALIZE, 0, GRAD_GEMM_MULTI)),
    "d-stream-v4": (2, 2, 16, 16, 64, 96, 4, False, False, False, 1,
                    (STREAM_V4, PROJECT_MULTI, STACKED, SVD_STACKED, FINALIZE, 0, GRAD_NONE)),
    "d-center-multi": (2, 2, 16, 16, 64, 96, 3, False, False, False, 1,
                       (CENTER_MULTI, PROJECT_MULTI, STACKED, SVD_STACKED, FINALIZE, 0, GRAD_NONE)),
    "e-finalize-kprime-t": (1, 2, 100, 100, 64, 96, 1, False, False, False, 2,
                            (PER_GROUP, PROJECT_MULTI, TRANSPOSED, SVD_TRANSPOSED, FINALIZE_KPRIME_T, 0, GRAD_NONE)),
    # beyond the issue's table: the two-pass SVD with a split teacher Gram, and U Sigma rebuilt in w_stack
    "f-two-pass-split-gram": (1, 2, 144, 144, 64, 512, 1, False, False, False, 1,
                              (PER_GROUP, PROJECT_MULTI, STACKED, SVD_TWO_PASS, FINALIZE, 0, GRAD_NONE)),
    "g-mix-grad-usigma-in-w-stack": (2, 2, 49, 49, 64, 96, 3, False, False, True, 2,
                                     (CENTER_MULTI, PROJECT_MULTI, TRANSPOSED, SVD_TRANSPOSED, FINISH_T, 1, GRAD_NONE)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_the_call_launches_what_its_plan_names(dev, case):
    """The plan compared is the one ``ops`` asked for when it sized the workspaces -- queried with stand-ins for the
    per-call tensors, which torch allocates 256-byte aligned like the stand-ins --, not one queried again with the
    call's own argument block; the launcher plans from that block itself, and the kernels seen are its answer."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    from basd_amd import ops, synth
    E, B, n_s, n_t, d_s, d_t, L, bf16, with_grad, mix_grad, hook, want = CASES[case]
    g = torch.Generator().manual_seed(n_s * 7 + n_t + L)
    students = [synth.structured(g, B, n_s, d_s, 16) for _ in range(E)]
    if bf16:
        students = [s.to(torch.bfloat16) for s in students]
    teachers = [synth.structured(g, B, n_t, d_t, 12) for _ in range(L)]
    attn = torch.softmax(torch.randn(B, 2, n_t, n_t, generator=g), dim=-1)
    mix = torch.softmax(torch.randn(E, L, generator=g), dim=-1)
    ref = _fp64_loss_b(students, teachers, attn, mix)
    sd, td = [s.to(dev) for s in students], [t.to(dev) for t in teachers]
    ad = [attn.to(dev)] * L
    gl = torch.full((E,), 0.5, device=dev) if with_grad else None
    run = lambda: ops.procrustes_forward(sd, td, ad, mix.to(dev), False, grad_layers=gl, need_mix_grad=mix_grad)
    ops._PROCRUSTES_PLANS.clear()
    try:
        with _hooks(hook):
            run()                                                           # warm-up: plan, code objects
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                pc = run()
                torch.cuda.synchronize()
            # calls with a mixing-weight gradient are planned per call and hand their plan to the backward
            plan = pc.mixgrad["route"] if mix_grad else next(iter(ops._PROCRUSTES_PLANS.values())).route
    finally:
        _hooks(1, 1).__exit__()
        ops._PROCRUSTES_PLANS.clear()
    got = tuple(plan[k] for k in ("center", "project", "cores", "svd", "finish", "rebuild_usigma", "grad"))
    assert got == want, (got, want)
    assert plan["slab_width"] == (64 if want[1] == PER_LAYER else 32)
    assert plan["gram_split"] == int(d_t >= 512) and plan["chol"] == 1
    if mix_grad:
        in_w_stack = plan["usigma_in"] == IN_W_STACK
        assert in_w_stack == bool(want[5]) and (pc.mixgrad["W"].data_ptr() != pc.a_prime.data_ptr())
        assert pc.mixgrad["sigma"].shape == (E * B, min(n_s, n_t)) and torch.isfinite(pc.mixgrad["W"]).all()
    names = [e.name for e in prof.events() if "cuda" in str(e.device_type).lower()]
    # a name that is a prefix of another ("student_project_kernel" / "..._v4_kernel") is matched up to its "<" or end
    count = lambda k: sum(nm.split("(")[0].split("<")[0].split("::")[-1].strip() in k.split("|") for nm in names)
    expected = {k: 0 for k in ALL_ROUTE_KERNELS}
    for field in KERNELS:
        for k in KERNELS[field][plan[field]]:
            expected[k] += E if (field, plan[field]) == ("project", PER_LAYER) else 1
    seen = {k: count(k) for k in ALL_ROUTE_KERNELS}
    print(f"[plan] {case}: {plan}\n[plan] {seen} among {len(names)} device events")
    assert seen == expected, (seen, expected)
    rel = ((pc.loss_b.double().cpu() - ref).norm() / ref.norm()).item()
    print(f"[plan] {case}: loss_b rel err vs fp64 {rel:.3e}")
    assert rel < 1e-5, rel       # the bound the stand-alone Procrustes tests of test_gpu_kernels.py put on loss_b


@pytest.mark.gpu
def test_a_cached_plan_serves_a_later_hook_setting(dev):
    """Plans without a mixing-weight gradient are cached and outlive a change of the hooks: one built while the cores of
    144 tokens are transposed (hook 2) keeps the two-pass log, and the same plan under hook 0 solves the stacked cores
    with the two-pass SVD, as a plan built under hook 0 would."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    from basd_amd import ops, synth
    g = torch.Generator().manual_seed(144)
    B, n, d_s, d_t = 2, 144, 64, 96
    s = [synth.structured(g, B, n, d_s, 16).to(dev)]
    t = [synth.structured(g, B, n, d_t, 12).to(dev)]
    a = [torch.softmax(torch.randn(B, 2, n, n, generator=g), dim=-1).to(dev)]
    mix = torch.ones(1, 1, device=dev)
    run = lambda: ops.procrustes_forward(s, t, a, mix, False)
    ops._PROCRUSTES_PLANS.clear()
    try:
        with _hooks(2):
            first = run()
            torch.cuda.synchronize()
            (plan,) = ops._PROCRUSTES_PLANS.values()
            assert plan.route["cores"] == TRANSPOSED and plan.jac_ws is not None
        with _hooks(0):
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                second = run()
                torch.cuda.synchronize()
            assert list(ops._PROCRUSTES_PLANS.values()) == [plan]           # the same cached plan
    finally:
        _hooks(1, 1).__exit__()
        ops._PROCRUSTES_PLANS.clear()
    names = [e.name for e in prof.events() if "cuda" in str(e.device_type).lower()]
    assert sum("jacobi_top_logged_kernel" in nm for nm in names) == 1, names
    assert sum("stack_product_t_kernel" in nm for nm in names) == 0, names
    rel = ((first.loss_b.double() - second.loss_b.double()).norm() / second.loss_b.double().norm()).item()
    print(f"[plan] cached plan, hook 2 then 0: loss_b of the two routes differ by {rel:.3e}")
    assert rel < 1e-5, rel       # the bound test_transposed_cores_match_the_stacked_route puts on the two routes
