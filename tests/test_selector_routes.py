"""Every selector route behind a switch or a shape threshold, against an fp64 evaluation of the same formulas.

``GrassmannianLayerSelector._spectra_async`` / ``_angles_from_spectra`` choose between several kernel sequences for the
same mathematics: by the shapes (teacher-space Grams, projected tokens, token-side Gram) and by switches
(``ops.EIG_SOLVER``, ``rank1_mp``, ``merge_factorisations``, ``teacher_space_gram``, ``small_student_jacobi``).  Each
case below sets one of them, proves with counting wrappers that the route it names was the one taken, and compares
ranks, distances, mixing weights, the loss and its gradients with ``oracle.basd_oracle`` run in float64 on the same
inputs -- never with another GPU route.  The unmarked test shows on the CPU that the fixtures are well-posed: the fp32 oracle
itself sits within a tenth of every tolerance, so a route that misses one is wrong, not unlucky.

The second part covers the scheduling switches of the single-teacher step (``basd_selector_chain`` and the
kernel-by-kernel layout): they may move kernels in time, never change a value."""
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
import make_goldens_shapes as S
from basd_amd import synth, ops, losses
from oracle import basd_oracle as O

gpu = pytest.mark.gpu
DEV = "cuda:0"

# name -> (shape, seed of synth.make_inputs); the module state is drawn under torch.manual_seed(42)
FIXTURES = {
    # B n_t = 512 >= d_s and d_t <= 1.5 d_s: Grams in the teacher's own space
    "V": S.SMALL["vit"],
    # d_t = 256 > 1.5 d_s: projected tokens, uncentred and centred Grams in one stacked launch (n_u == d_s)
    "W": (synth.LossShape("wide teacher", 8, 49, 96, 12, 64, 256, 4, 4, True, 50, points=2, r_s=6, r_t=0), 11),
    # B n_t = 50 < d_s: the uncentred Gram is formed on the token side (order 50)
    "F": (synth.LossShape("few tokens", 2, 25, 96, 12, 25, 128, 3, 2, True, 10, points=2, r_s=6, r_t=0), 13),
}
WANT_RANKS = {"V": [16, 18, 20, 22, 24, 26], "W": [16, 18, 20, 22], "F": [16, 18, 19]}
MIN_THRESHOLD_MARGIN = 0.05        # |eigenvalue - MP threshold| / threshold, closest eigenvalue of any teacher layer

# The tolerances the default route is already held to, by quantity:
#   d_grass_sq, mix   rtol 2e-4   test_high_rank_angles.py::test_selector_and_loss_without_gradients
#   loss              rtol 1e-4   the same (and every golden test of test_gpu_parity.py)
#   student gradient  2e-3 relative Frobenius norm per extraction layer
#                                 test_high_rank_angles.py::test_loss_and_gradients
#   log_temperatures.grad   rtol 5e-3, atol 1e-7   the same
TOL = dict(d_grass_sq=2e-4, mix=2e-4, loss=1e-4, student_grad=2e-3, temp_rtol=5e-3, temp_atol=1e-7)


class _Fixture:
    """Inputs and module state of one fixture, and the CPU oracle's results on them per compute dtype."""

    def __init__(self, name: str):
        self.name = name
        self.shape, self.seed = FIXTURES[name]
        self.cpu = synth.make_inputs(self.shape, self.seed)
        sel = self.module("cpu").layer_selector
        self.layers = synth.extraction_layers(self.shape.depth, self.shape.points)
        self.proj_s, self.proj_t = sel.proj_s.detach().clone(), sel.proj_t.detach().clone()
        self.log_temperatures = sel.log_temperatures.detach().clone()

    def module(self, device=DEV):
        from basd_amd.losses import BASDLoss
        s = self.shape
        torch.manual_seed(42)
        return BASDLoss(torch.nn.CrossEntropyLoss(), s.d_s, s.d_t, s.depth, s.n_s,
                        config=SimpleNamespace(num_extraction_points=s.points),
                        teacher_has_cls_token=s.has_cls).to(device)

    def on_device(self):
        move = lambda d: {k: v.to(DEV) for k, v in d.items()}
        c = self.cpu
        return SimpleNamespace(logits=c.logits.to(DEV), targets=c.targets.to(DEV), student=move(c.student),
                               teacher=move(c.teacher), attn=move(c.attn))

    @functools.lru_cache(maxsize=None)
    def oracle(self, dtype: torch.dtype):
        """Ranks, distances, mixing weights, loss and gradients of ``O.basd_forward`` at compute dtype ``dtype``."""
        c, s = self.cpu, self.shape
        state = O.SelectorState(self.proj_s.clone(), self.proj_t.clone(),
                                self.log_temperatures.clone().requires_grad_(True))
        leaves = {k: v.clone().requires_grad_(True) for k, v in c.student.items()}
        loss, trace = O.basd_forward(state, torch.nn.CrossEntropyLoss(), self.layers, s.n_s, s.has_cls, c.logits,
                                     c.targets, leaves, c.teacher, c.attn, dtype=dtype)
        loss.backward()
        sel = trace.selector
        return SimpleNamespace(
            ranks=[sel.ranks[k] for k in sorted(c.teacher)],
            d_grass_sq=np.stack([sel.d_grass_sq[l].double().numpy() for l in self.layers]),
            mix=np.stack([sel.mix_weights[l].double().numpy() for l in self.layers]),
            loss=float(loss.detach().double()),
            student_grads={l: leaves[l].grad.double() for l in self.layers},
            temp_grad=state.log_temperatures.grad.double().numpy())

    def threshold_margin(self) -> float:
        """Smallest |eigenvalue - MP threshold| / threshold over the teacher layers, in fp64
        (layer_selector.py:8-20)."""
        margin = np.inf
        for key in sorted(self.cpu.teacher):
            t = self.cpu.teacher[key].double()
            z = t.reshape(-1, t.shape[2]) @ self.proj_t.double().T
            M, D = z.shape
            ev = torch.linalg.eigvalsh((z.T @ z) / M if M >= D else (z @ z.T) / M)
            lam = float(ev[(ev.numel() - 1) // 2]) * O.mp_threshold_factor(M, D)
            margin = min(margin, float(((ev - lam).abs() / lam).min()))
        return margin


@functools.lru_cache(maxsize=None)
def fixture(name: str) -> _Fixture:
    return _Fixture(name)


def errors(got, ref) -> dict:
    """Measured error per quantity that ``TOL`` bounds; ``got`` / ``ref`` as ``_Fixture.oracle`` returns them
    (``got`` without gradients: the gradient entries are left out)."""
    rel = lambda a, b: float(np.max(np.abs(a - b) / np.abs(b)))
    e = dict(d_grass_sq=rel(got.d_grass_sq, ref.d_grass_sq), mix=rel(got.mix, ref.mix),
             loss=abs(got.loss - ref.loss) / abs(ref.loss))
    if got.student_grads is not None:
        e["student_grad"] = max(float((got.student_grads[l] - want).norm() / want.norm())
                                for l, want in ref.student_grads.items())
        # the quantity np.testing.assert_allclose bounds by 1: |got - ref| / (atol + rtol |ref|)
        e["temp"] = float(np.max(np.abs(got.temp_grad - ref.temp_grad)
                                 / (TOL["temp_atol"] + TOL["temp_rtol"] * np.abs(ref.temp_grad))))
        e["temp_rel"] = rel(got.temp_grad, ref.temp_grad)
    return e


def fmt(e: dict) -> str:
    return " ".join(f"{k}={v:.2e}" for k, v in e.items())


def check(e: dict, what, fraction: float = 1.0) -> None:
    """Every measured error within ``fraction`` of its tolerance."""
    for key in ("d_grass_sq", "mix", "loss"):
        assert e[key] <= fraction * TOL[key], (what, key, e[key])
    if "student_grad" in e:
        assert e["student_grad"] < fraction * TOL["student_grad"], (what, "student_grad", e["student_grad"])
        assert e["temp"] <= fraction, (what, "log_temperatures.grad", e["temp"], e["temp_rel"])


# --------------------------------------------------------------------------- #
# 1. the fixtures, on the CPU
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("name", list(FIXTURES))
def test_fixtures_are_well_posed_for_an_fp32_evaluation(name):
    """Guards the fixtures and the tolerances, not the kernels: the ranks are the expected ones in fp32 and in fp64, no
    eigenvalue of a teacher layer lies within 5 % of its Marchenko-Pastur threshold (a rank cannot flip on round-off),
    and the fp32 oracle agrees with the fp64 one to a tenth of every tolerance the GPU cases below are held to.  A
    fixture that fails here is ill-posed for any fp32 evaluation: change the fixture then, not a tolerance."""
    fix = fixture(name)
    ref, f32 = fix.oracle(torch.float64), fix.oracle(torch.float32)
    margin = fix.threshold_margin()
    e = errors(f32, ref)
    print(f"routes: cpu-fp32-oracle {name}: {fmt(e)} threshold_margin={margin:.3f} ranks={ref.ranks}")
    assert ref.ranks == WANT_RANKS[name] and f32.ranks == WANT_RANKS[name], (ref.ranks, f32.ranks)
    assert margin >= MIN_THRESHOLD_MARGIN, margin
    check(e, name, fraction=0.1)


# --------------------------------------------------------------------------- #
# 2. the route matrix
# --------------------------------------------------------------------------- #
WATCHED_OPS = ("tridiagonalise", "tridiag_eigenvalues", "tridiag_spectrum", "tridiag_mp_rank", "tridiag_mp_rank_rank1",
               "tridiag_eigenvectors", "tridiag_apply_q", "tridiag_shifted_solve", "selector_tail", "sym_eig",
               "sort_extract", "angle_stack", "eigvec_k2", "mp_rank_device")
WATCHED_METHODS = ("_teacher_projections", "_teacher_grams_in_teacher_space", "_eigvec_adjoint_leading")


class Calls:
    """Counting wrappers around the calls that tell the routes apart.  ``log``: (name, shape of the first tensor
    argument or None, keyword / trailing arguments of interest) in call order."""

    def __init__(self, monkeypatch, selector):
        self.log = []
        for name in WATCHED_OPS:
            self._wrap(monkeypatch, ops, name)
        self._wrap(monkeypatch, losses, "_uncentred_gram")
        for name in WATCHED_METHODS:
            self._wrap(monkeypatch, selector, name)

    def _wrap(self, monkeypatch, owner, name):
        inner = getattr(owner, name)

        def counted(*args, **kwargs):
            first = next((tuple(a.shape) for a in args if isinstance(a, torch.Tensor)), None)
            extra = None
            if name == "tridiagonalise":
                extra = kwargs.get("mp_rank", args[1] if len(args) > 1 else None) is not None
            elif name == "sort_extract":
                extra = kwargs.get("kmax", args[2] if len(args) > 2 else None)
            self.log.append((name, first, extra))
            return inner(*args, **kwargs)
        monkeypatch.setattr(owner, name, counted)

    def count(self, name) -> int:
        return sum(1 for n, _, _ in self.log if n == name)

    def of(self, name) -> list:
        return [(shape, extra) for n, shape, extra in self.log if n == name]

    def factorisations(self) -> list:
        """(number of matrices, with the fused MP rank?) of every ``ops.tridiagonalise`` call, sorted."""
        return sorted((shape[0], extra) for shape, extra in self.of("tridiagonalise"))


def _students(c: Calls, fix, grad: bool, tridiagonal_backward: bool = False) -> list:
    """The student side's own factorisation launch, where there is one: with a backward the student Grams of these
    orders go through Jacobi (``small_student_jacobi``) unless the case turned that off."""
    E = len(fix.layers)
    if grad and not tridiagonal_backward:
        assert ((E, fix.shape.d_s, fix.shape.d_s), None) in c.of("angle_stack"), c.log    # [G ; I], student Grams
        assert c.count("_eigvec_adjoint_leading") == 0
        assert [shape[1] for shape, _ in c.of("eigvec_k2")] == [fix.shape.d_s], c.log        # K2 at order d_s
        return []
    if grad:
        assert c.count("_eigvec_adjoint_leading") == 1 and c.count("tridiag_shifted_solve") == 1, c.log
    return [(E, False)]


def route_merged(c, fix, grad, tridiagonal_backward=True):
    L, E = fix.shape.layers_t, len(fix.layers)
    assert c.factorisations() == [(L + E, False)], c.log         # one launch over teacher and student matrices
    assert c.count("tridiag_mp_rank_rank1") == 1 and c.count("_teacher_grams_in_teacher_space") == 1, c.log
    assert c.count("_teacher_projections") == 0 and c.count("sym_eig") == 0 and c.count("mp_rank_device") == 0, c.log
    if grad:
        assert c.count("_eigvec_adjoint_leading") == 1 and c.count("selector_tail") == 0, c.log
    else:
        assert c.count("selector_tail") == 1 and c.count("tridiag_eigenvectors") == 0, c.log


def route_rank1_unmerged(c, fix, grad, tridiagonal_backward=True):
    L = fix.shape.layers_t
    assert c.factorisations() == sorted(_students(c, fix, grad, tridiagonal_backward) + [(L, False)]), c.log
    assert c.count("tridiag_mp_rank_rank1") == 1 and c.count("_teacher_grams_in_teacher_space") == 1, c.log
    assert c.count("_teacher_projections") == 0 and c.count("mp_rank_device") == 0, c.log


def route_rank1_jacobi_students(c, fix, grad):
    assert grad
    route_rank1_unmerged(c, fix, True, tridiagonal_backward=False)


def _route_fused(c, fix, grad, teacher_space: bool):
    L = fix.shape.layers_t
    # uncentred and centred Grams in one factorisation launch whose last kernel counts the MP ranks
    assert c.factorisations() == sorted(_students(c, fix, grad) + [(2 * L, True)]), c.log
    assert c.count("tridiag_mp_rank_rank1") == 0 and c.count("tridiag_mp_rank") == 0, c.log
    assert c.count("mp_rank_device") == 0 and c.count("_uncentred_gram") == 0, c.log
    assert c.count("_teacher_grams_in_teacher_space") == int(teacher_space), c.log
    assert c.count("_teacher_projections") == int(not teacher_space), c.log
    if not grad:
        assert c.count("selector_tail") == 1, c.log


def route_fused_teacher_space(c, fix, grad):
    _route_fused(c, fix, grad, True)


def route_fused_projected(c, fix, grad):
    _route_fused(c, fix, grad, False)


def route_token_side(c, fix, grad):
    L, s = fix.shape.layers_t, fix.shape
    M = s.batch * s.n_t
    assert M < s.d_s
    assert c.count("_uncentred_gram") == L and c.count("_teacher_projections") == 1, c.log
    assert sorted(shape for shape, _ in c.of("tridiag_eigenvalues")) == [(L, M, M), (L, s.d_s, s.d_s)], c.log
    assert c.factorisations() == sorted(_students(c, fix, grad) + [(L, False), (L, False)]), c.log    # no mp_rank=
    assert c.count("mp_rank_device") == 1 and c.count("tridiag_mp_rank_rank1") == 0, c.log
    assert c.count("_teacher_grams_in_teacher_space") == 0 and c.count("sym_eig") == 0, c.log


def _route_jacobi(c, fix, grad):
    tridiagonal = [n for n, _, _ in c.log
                   if n.startswith("tridiag") or n in ("selector_tail", "_eigvec_adjoint_leading")]
    assert tridiagonal == [], tridiagonal
    assert c.count("mp_rank_device") == 1, c.log
    if grad:
        E = len(fix.layers)
        assert ((E, fix.shape.d_s, fix.shape.d_s), None) in c.of("angle_stack"), c.log
        assert [shape[1] for shape, _ in c.of("eigvec_k2")] == [fix.shape.d_s], c.log


def _route_jacobi_stacked(c, fix, grad, teacher_space: bool):
    _route_jacobi(c, fix, grad)
    L, d_s = fix.shape.layers_t, fix.shape.d_s
    assert ((L, d_s, d_s), 0) in c.of("sort_extract"), c.log   # the ranks: values only, L matrices
    assert c.count("sym_eig") == 0 and c.count("_uncentred_gram") == 0, c.log
    assert c.count("_teacher_grams_in_teacher_space") == int(teacher_space), c.log
    assert c.count("_teacher_projections") == int(not teacher_space), c.log


def route_jacobi_teacher_space(c, fix, grad):
    _route_jacobi_stacked(c, fix, grad, True)


def route_jacobi_projected(c, fix, grad):
    _route_jacobi_stacked(c, fix, grad, False)


def route_jacobi_token_side(c, fix, grad):
    _route_jacobi(c, fix, grad)
    L, s = fix.shape.layers_t, fix.shape
    M = s.batch * s.n_t
    assert [shape for shape, _ in c.of("sym_eig")] == [(L, M, M)], c.log              # ops.sym_eig on g_u
    assert c.count("_uncentred_gram") == L and c.count("_teacher_projections") == 1, c.log


def route_default(c, fix, grad):
    """What the default settings take at fixture V: merged without a backward, rank-one + Jacobi students with one."""
    if grad:
        route_rank1_jacobi_students(c, fix, True)
    else:
        route_merged(c, fix, False)


# id, fixture, settings on the selector, settings on ops, no-grad / grad runs, route proof.  The settings are the
# attributes behind BASD_TEACHER_SPACE_GRAM, BASD_RANK1_MP, BASD_MERGE_FACTORISATIONS and BASD_EIG_SOLVER.
CASES = [
    ("merged", "V", {}, {}, (False,), route_merged),
    ("merged_leading_k_backward", "V", dict(small_student_jacobi=False), {}, (True,), route_merged),
    ("rank1_unmerged", "V", dict(merge_factorisations=False), {}, (False,), route_rank1_unmerged),
    # with a backward the default sends the students through Jacobi, where the merge switch has no say (the next case):
    # the unmerged launch pair with a backward is the one with the leading-k adjoint
    ("rank1_unmerged_leading_k_backward", "V", dict(merge_factorisations=False, small_student_jacobi=False), {},
     (True,), route_rank1_unmerged),
    ("rank1_jacobi_students", "V", {}, {}, (True,), route_rank1_jacobi_students),
    ("fused_teacher_space", "V", dict(rank1_mp=False), {}, (False, True), route_fused_teacher_space),
    ("fused_projected", "V", dict(teacher_space_gram=False), {}, (False, True), route_fused_projected),
    ("fused_wide_teacher", "W", {}, {}, (False, True), route_fused_projected),
    ("token_side_gram", "F", {}, {}, (False, True), route_token_side),
    ("jacobi_teacher_space", "V", {}, dict(EIG_SOLVER="jacobi"), (False, True), route_jacobi_teacher_space),
    ("jacobi_projected", "W", {}, dict(EIG_SOLVER="jacobi"), (False, True), route_jacobi_projected),
    ("jacobi_token_side", "F", {}, dict(EIG_SOLVER="jacobi"), (False, True), route_jacobi_token_side),
]
ROUTE_RUNS = [pytest.param(*case[:4], grad, case[5], id=f"{case[0]}-{'grad' if grad else 'nograd'}")
              for case in CASES for grad in case[4]]


def _run(fix, mod, grad: bool):
    """One step of ``mod`` on the fixture's inputs -> results laid out like ``_Fixture.oracle``'s."""
    inp = fix.on_device()
    sel = mod.layer_selector
    if not grad:
        with torch.no_grad():
            loss = mod(inp.logits, inp.targets, inp.student, inp.teacher, inp.attn)
        sel.finish_pending()
        torch.cuda.synchronize()
        leaves = None
    else:
        leaves = {k: v.requires_grad_(True) for k, v in inp.student.items()}
        loss = mod(inp.logits, inp.targets, leaves, inp.teacher, inp.attn)
        loss.backward()
        torch.cuda.synchronize()
    return SimpleNamespace(
        ranks=[sel.subspace_ranks[k] for k in sorted(inp.teacher)],
        d_grass_sq=mod.last_components["d_grass_sq"].double().cpu().numpy(),
        mix=mod.last_components["mix"].double().cpu().numpy(),
        loss=float(loss.detach().double()),
        student_grads={l: leaves[l].grad.double().cpu() for l in fix.layers} if grad else None,
        temp_grad=sel.log_temperatures.grad.double().cpu().numpy() if grad else None)


def _route_case(monkeypatch, tag, name, selector_settings, ops_settings, grad, route):
    fix = fixture(name)
    ref = fix.oracle(torch.float64)
    mod = fix.module()
    for key, value in selector_settings.items():
        assert hasattr(mod.layer_selector, key)
        monkeypatch.setattr(mod.layer_selector, key, value)
    for key, value in ops_settings.items():
        monkeypatch.setattr(ops, key, value)
    calls = Calls(monkeypatch, mod.layer_selector)
    got = _run(fix, mod, grad)
    route(calls, fix, grad)
    e = errors(got, ref)
    print(f"routes: {tag}-{'grad' if grad else 'nograd'} {name}: {fmt(e)} ranks={got.ranks}")
    assert got.ranks == ref.ranks == WANT_RANKS[name], (got.ranks, ref.ranks)
    check(e, tag)


@gpu
@pytest.mark.parametrize("tag,name,selector_settings,ops_settings,grad,route", ROUTE_RUNS)
def test_route_against_fp64(monkeypatch, tag, name, selector_settings, ops_settings, grad, route):
    """One route of the matrix: the route proof first (a case that lands elsewhere fails whatever it computes), then
    ranks exactly and distances, mixing weights, loss and gradients within ``TOL`` of the fp64 oracle."""
    _route_case(monkeypatch, tag, name, selector_settings, ops_settings, grad, route)


@gpu
@pytest.mark.parametrize("grad", [False, True], ids=["nograd", "grad"])
def test_default_route_on_fp32_mfma_grams(monkeypatch, grad):
    """Fixture V with ``basd_gemm_tuning(0)`` (BASD_GEMM_SPLIT=0): every Gram launch on the fp32 MFMA instead of the
    split bf16 operands, same routes, same tolerances."""
    from basd_amd import _lib
    prev = _lib.query("basd_gemm_tuning_get")
    _lib.call("basd_gemm_tuning", 0)
    try:
        assert _lib.query("basd_gemm_tuning_get") == 0
        _route_case(monkeypatch, "fp32_mfma_grams", "V", {}, {}, grad, route_default)
    finally:
        _lib.call("basd_gemm_tuning", prev)


# --------------------------------------------------------------------------- #
# 3. scheduling switches of the single-teacher step
# --------------------------------------------------------------------------- #
def _cfg2_module():
    from basd_amd.losses import BASDLoss
    shape = synth.CONFIGS["cfg2"]
    torch.manual_seed(42)
    return BASDLoss(torch.nn.CrossEntropyLoss(label_smoothing=0.001), shape.d_s, shape.d_t, shape.depth, shape.n_s,
                    config=SimpleNamespace(num_extraction_points=shape.points),
                    teacher_has_cls_token=shape.has_cls).to(DEV)


def _four_alternating_steps(golden, mod, each_step=None):
    """cfg-2 at batch 8, seeds 1234 / 1235 / 1234 / 1235: every workspace slot and the deferred read-back carry changing
    data.  Ranks exact, d_grass_sq rtol 2e-4, loss rtol 1e-4 against the reference's values
    (test_selector_chain_layouts_agree_with_the_reference)."""
    g = golden("baseline_scalars.npz")
    shape = synth.CONFIGS["cfg2"]
    inputs = {seed: synth.make_inputs(shape, seed, batch=8, device=DEV, strided=True) for seed in (1234, 1235)}
    for step, seed in enumerate((1234, 1235, 1234, 1235)):
        tag = f"cfg2_s{seed}_b8"
        inp = inputs[seed]
        loss = mod(inp.logits, inp.targets, inp.student, inp.teacher, inp.attn)
        mod.layer_selector.finish_pending()
        torch.cuda.synchronize()
        d = mod.last_components["d_grass_sq"].cpu().numpy()
        assert list(mod.layer_selector.subspace_ranks.values()) == list(g[f"{tag}_ranks"]), (step, seed)
        np.testing.assert_allclose(d, g[f"{tag}_d_grass_sq"], rtol=2e-4, err_msg=f"step {step} seed {seed}")
        np.testing.assert_allclose(loss.item(), g[f"{tag}_loss"], rtol=1e-4, err_msg=f"step {step} seed {seed}")
        if each_step is not None:
            each_step(mod)


def _plans(mod):
    plans = list(mod._chain_plans.values())
    assert plans, "the step did not go through basd_selector_chain"
    return plans


@gpu
def test_chain_without_the_rank_certificate(golden, monkeypatch):
    """``chain.CERTIFICATE = False`` (BASD_RANK_CERT=0): no certificate kernel, the host waits for the ranks."""
    from basd_amd import chain
    monkeypatch.setattr(chain, "CERTIFICATE", False)
    mod = _cfg2_module()

    def no_certificate(mod):
        assert all(plan.cert_stream is None for plan in _plans(mod))
    _four_alternating_steps(golden, mod, no_certificate)
    assert mod.readback_deferred_steps == 0        # ``auto`` defers only behind a certificate


@gpu
def test_chain_with_two_slots(golden, monkeypatch):
    """``chain.SLOTS = 2`` (BASD_CHAIN_SLOTS=2): four steps go twice round the workspace ring."""
    from basd_amd import chain
    monkeypatch.setattr(chain, "SLOTS", 2)
    mod = _cfg2_module()

    def two_slots(mod):
        assert all(len(plan.slots) == 2 for plan in _plans(mod))
    _four_alternating_steps(golden, mod, two_slots)


@gpu
@pytest.mark.parametrize("priority", ["0", "1"])
def test_chain_stream_priorities(golden, monkeypatch, priority):
    """BASD_CHAIN_PRIORITY (read when a module creates its side streams): none / chain and student stream high."""
    monkeypatch.setenv("BASD_CHAIN_PRIORITY", priority)
    mod = _cfg2_module()
    _four_alternating_steps(golden, mod)
    _plans(mod)
    chain_stream, student_stream, tail_stream = (mod._side_streams[(DEV, i)].priority for i in range(3))
    assert chain_stream == student_stream <= tail_stream          # (lower number = higher priority)
    if priority == "0":
        assert chain_stream == tail_stream


@gpu
def test_chain_student_stream_at_default_priority(golden):
    """``student_low_priority = False`` (BASD_STUDENT_LOW_PRIORITY=0): the student stream is one of torch's."""
    mod = _cfg2_module()
    mod.student_low_priority = False
    _four_alternating_steps(golden, mod)
    _plans(mod)
    assert (DEV, "student-low") not in mod._side_streams


@gpu
def test_kernel_by_kernel_layout_without_the_student_gate(golden):
    """``gate_student_chain = False`` (BASD_STUDENT_GATE=0) in the kernel-by-kernel layout (``use_chain = False``): the
    student chain is queued beside the teacher's instead of behind its shared tridiagonalisation stage."""
    mod = _cfg2_module()
    mod.use_chain = False
    mod.layer_selector.gate_student_chain = False
    _four_alternating_steps(golden, mod)
    assert not mod._chain_plans
    assert getattr(mod.layer_selector, "_gate_event", None) is None       # no gate was ever armed
