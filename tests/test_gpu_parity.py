"""Parity of the HIP path with the CPU oracle and with the golden fixtures generated from the
reference (tests/golden).  Tolerances: loss values 1e-4 relative (north star), ranks exact."""
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

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def T(a):
    return torch.from_numpy(np.asarray(a))


def _module(shape, ls):
    from basd_amd.losses import BASDLoss
    torch.manual_seed(42)
    crit = torch.nn.CrossEntropyLoss(label_smoothing=ls)
    return BASDLoss(crit, shape.d_s, shape.d_t, shape.depth, shape.n_s,
                    config=SimpleNamespace(num_extraction_points=shape.points),
                    teacher_has_cls_token=shape.has_cls).to(DEV)


@pytest.mark.parametrize("solver", ["tridiag", "jacobi"])
def test_mp_rank_golden(golden, solver, monkeypatch):
    from basd_amd.losses import marchenko_pastur_rank
    monkeypatch.setattr(ops, "EIG_SOLVER", solver)
    g = golden("mp_rank.npz")
    cases = [("m32_d192", 32, 192, 6), ("m128_d192", 128, 192, 10), ("m1000_d384", 1000, 384, 24),
             ("m12544_d384", 12544, 384, 48)]
    for i, (tag, m, d, r) in enumerate(cases):
        gen = torch.Generator().manual_seed(100 + i)
        x = synth.structured(gen, 1, m, d, r)[0]
        assert marchenko_pastur_rank(x.to(DEV)) == int(g[f"{tag}_rank"]), tag
    gen = torch.Generator().manual_seed(200)
    noise = torch.randn(2000, 128, generator=gen)
    assert marchenko_pastur_rank(noise.to(DEV)) == int(g["noise_rank"])


def test_subspace_golden(golden):
    from basd_amd.losses import _grassmann_subspace
    g = golden("subspace.npz")
    for i in range(3):
        m, d, r, k = [int(v) for v in g[f"c{i}_shape"]]
        gen = torch.Generator().manual_seed(300 + i)
        z = synth.structured(gen, 1, m, d, r)[0] + 0.7
        basis, s = _grassmann_subspace(z.to(DEV), k=k)
        assert list(basis.shape) == list(g[f"c{i}_basis_shape"])
        if k:
            proj = (basis @ basis.T).cpu().numpy()
            assert np.abs(proj - g[f"c{i}_proj"]).max() < 5e-4      # subspace projector (sign/rotation free)
            np.testing.assert_allclose(s.cpu().numpy(), g[f"c{i}_svals"], rtol=2e-5)


@pytest.mark.parametrize("tag", ["cls_same", "cls_interp", "nocls_uniform", "nocls_attn"])
def test_relational_golden(golden, tag):
    """geometric_relational_loss on the reference's own inputs: value, per-sample terms, student grad."""
    from basd_amd import ops
    from basd_amd.losses import geometric_relational_loss
    g = golden("relational.npz")
    cls = bool(g[f"{tag}_meta"][6])
    s = T(g[f"{tag}_s"]).to(DEV).requires_grad_(True)
    t = T(g[f"{tag}_t"]).to(DEV)
    attn = T(g[f"{tag}_attn"]).to(DEV)
    loss = geometric_relational_loss(s, t, attn, has_cls_token=cls)
    np.testing.assert_allclose(loss.item(), g[f"{tag}_loss"], rtol=1e-4)
    pc = ops.procrustes_forward([s.detach()], [t], [attn], torch.ones(1, 1, device=DEV), cls, need_backward=False)
    np.testing.assert_allclose(pc.loss_b[0].cpu().numpy(), g[f"{tag}_per_sample"], rtol=1e-4)
    loss.backward()
    ref = g[f"{tag}_grad_s"]
    err = np.linalg.norm(s.grad.cpu().numpy() - ref) / np.linalg.norm(ref)
    assert err < 1e-4, (tag, err)


@pytest.mark.parametrize("tag", ["cls_same", "cls_interp", "nocls_uniform", "nocls_attn"])
def test_relational_golden_teacher_side_gradients(golden, tag):
    """geometric_relational_loss is differentiable w.r.t. the teacher tokens and the attention too
    (relational.py:18-50): gradients against the reference's autograd on its own inputs."""
    from basd_amd.losses import geometric_relational_loss
    g = golden("relational.npz")
    cls = bool(g[f"{tag}_meta"][6])
    s = T(g[f"{tag}_s"]).to(DEV).requires_grad_(True)
    t = T(g[f"{tag}_t"]).to(DEV).requires_grad_(True)
    attn = T(g[f"{tag}_attn"]).to(DEV).requires_grad_(True)
    loss = geometric_relational_loss(s, t, attn, has_cls_token=cls)
    np.testing.assert_allclose(loss.item(), g[f"{tag}_loss"], rtol=1e-4)
    gs, gt, ga = torch.autograd.grad(loss, [s, t, attn])
    for got, name in ((gs, "grad_s"), (gt, "grad_t")):
        ref = g[f"{tag}_{name}"]
        err = np.linalg.norm(got.cpu().numpy() - ref) / np.linalg.norm(ref)
        assert err < 2e-4, (tag, name, err)
    assert ga.shape == attn.shape
    np.testing.assert_allclose(ga.double().abs().sum().item(), g[f"{tag}_grad_attn_cls_row_sum"], rtol=2e-3)
    if cls:                                                  # only the CLS row (minus the CLS column) receives gradient
        mask = torch.ones_like(ga, dtype=torch.bool)
        mask[:, :, 0, 1:] = False
        assert ga[mask].abs().max().item() == 0.0


@pytest.mark.parametrize("n_s,n_t,d_s,d_t,cls", [(196, 49, 384, 2048, False), (64, 64, 192, 256, True),
                                                  (36, 9, 64, 160, False), (64, 1, 192, 512, False),
                                                  (49, 64, 96, 128, True), (196, 256, 64, 96, False)])
def test_procrustes_terms_vs_oracle(n_s, n_t, d_s, d_t, cls):
    """tr_s, tr_t, nuc per sample against the oracle's LAPACK path, including the interpolated grids."""
    from basd_amd import ops
    gen = torch.Generator().manual_seed(n_s * 7 + n_t)
    B = 6
    s = synth.structured(gen, B, n_s, d_s, 8) + 0.5
    t = synth.structured(gen, B, n_t, d_t, 6) - 0.25
    a = n_t + (1 if cls else 0)
    attn = torch.softmax(torch.randn(B, 3, a, a, generator=gen), dim=-1)
    w = O.token_weights(attn, cls, n_s)
    tr_s, tr_t, nuc = O.procrustes_terms(s, O.resample_tokens(t, n_s), w)
    pc = ops.procrustes_forward([s.to(DEV)], [t.to(DEV)], [attn.to(DEV)], torch.ones(1, 1, device=DEV), cls,
                                need_backward=False, want_sweeps=True)
    assert int(pc.sweeps.max()) < ops.MAX_SWEEPS
    np.testing.assert_allclose(pc.omega[0].cpu().numpy(), w.numpy(), rtol=2e-6, atol=1e-9)
    np.testing.assert_allclose(pc.tr_s[0].cpu().numpy(), tr_s.numpy(), rtol=1e-5)
    np.testing.assert_allclose(pc.tr_t[0].cpu().numpy(), tr_t.numpy(), rtol=1e-5, atol=1e-6)
    # atol: with a single teacher token the centred teacher is exactly 0 here, while the oracle's fp32
    # centring leaves ~1e-5 of round-off in its nuclear norm
    np.testing.assert_allclose(pc.nuc[0].cpu().numpy(), nuc.numpy(), rtol=2e-5, atol=2e-6 * float((tr_s + tr_t).max()))
    ref_loss = (tr_s + tr_t - 2 * nuc).numpy()
    np.testing.assert_allclose(pc.loss_b[0].cpu().numpy(), ref_loss, rtol=1e-4)


def test_procrustes_exactly_low_rank_inputs():
    """Rank-5 student x rank-7 teacher: the fp64 Gram/Cholesky front end keeps LAPACK-level accuracy
    where an fp32 Gram route loses three digits."""
    from basd_amd import ops
    gen = torch.Generator().manual_seed(77)
    B, n, d_s, d_t = 4, 64, 192, 256
    s = torch.randn(B, n, 5, generator=gen) @ torch.randn(5, d_s, generator=gen)
    t = torch.randn(B, n, 7, generator=gen) @ torch.randn(7, d_t, generator=gen)
    attn = torch.ones(B, 1, n, n) / n
    w = O.token_weights(attn, False, n)
    tr_s, tr_t, nuc = O.procrustes_terms(s.double(), t.double(), w.double())
    nuc64 = torch.linalg.svdvals(torch.bmm((w.unsqueeze(-1).sqrt() * (s - (w.unsqueeze(-1) * s).sum(1, keepdim=True))).double().transpose(1, 2),
                                           (w.unsqueeze(-1).sqrt() * (t - (w.unsqueeze(-1) * t).sum(1, keepdim=True))).double())).sum(-1)
    pc = ops.procrustes_forward([s.to(DEV)], [t.to(DEV)], [attn.to(DEV)], torch.ones(1, 1, device=DEV), False,
                                need_backward=False)
    np.testing.assert_allclose(pc.nuc[0].cpu().numpy(), nuc64.numpy(), rtol=2e-5)


@pytest.mark.parametrize("tag", ["cnn"])
def test_full_small_golden(golden, tag):
    g = golden("full_small.npz")
    shape, seed = S.SMALL[tag]
    mod = _module(shape, 0.01)
    inp = synth.make_inputs(shape, seed, device=DEV)
    leaves = {k: v.requires_grad_(True) for k, v in inp.student.items()}
    logits = inp.logits.requires_grad_(True)
    loss = mod(logits, inp.targets, leaves, inp.teacher, inp.attn)
    assert mod.token_layers == list(g[f"{tag}_token_layers"])
    assert [mod.layer_selector.subspace_ranks[k] for k in sorted(inp.teacher)] == list(g[f"{tag}_ranks"])
    np.testing.assert_allclose(loss.item(), g[f"{tag}_loss"], rtol=1e-4)
    loss.backward()
    np.testing.assert_allclose(logits.grad.cpu().numpy(), g[f"{tag}_grad_logits"], rtol=1e-4, atol=1e-8)
    for l in mod.token_layers:
        ref = g[f"{tag}_grad_student_{l}"]
        err = np.linalg.norm(leaves[l].grad.cpu().numpy() - ref) / np.linalg.norm(ref)
        assert err < 1e-4, (l, err)
    np.testing.assert_array_equal(mod.layer_selector.log_temperatures.grad.cpu().numpy(),
                                  g[f"{tag}_grad_log_temperatures"])


def _full_small_golden_multilayer(golden, tag, small_student_jacobi):
    g = golden("full_small.npz")
    shape, seed = S.SMALL[tag]
    mod = _module(shape, 0.01)
    mod.layer_selector.small_student_jacobi = small_student_jacobi
    adjoint = mod.layer_selector._eigvec_adjoint_leading
    leading_k_calls = []
    mod.layer_selector._eigvec_adjoint_leading = lambda *a: leading_k_calls.append(1) or adjoint(*a)
    inp = synth.make_inputs(shape, seed, device=DEV)
    leaves = {k: v.requires_grad_(True) for k, v in inp.student.items()}
    logits = inp.logits.requires_grad_(True)
    loss = mod(logits, inp.targets, leaves, inp.teacher, inp.attn)
    assert [mod.layer_selector.subspace_ranks[k] for k in sorted(inp.teacher)] == list(g[f"{tag}_ranks"])
    np.testing.assert_allclose(mod.last_components["mix"].cpu().numpy(), g[f"{tag}_mix_weights"], rtol=2e-3, atol=1e-6)
    np.testing.assert_allclose(loss.item(), g[f"{tag}_loss"], rtol=1e-4)
    loss.backward()
    # which student-eigenvector backward ran: the leading-k adjoint (shifted solves) or the full Jacobi eigenvectors
    assert bool(leading_k_calls) == (not small_student_jacobi)
    np.testing.assert_allclose(logits.grad.cpu().numpy(), g[f"{tag}_grad_logits"], rtol=1e-4, atol=1e-8)
    for l in mod.token_layers:
        ref = g[f"{tag}_grad_student_{l}"]
        err = np.linalg.norm(leaves[l].grad.cpu().numpy() - ref) / np.linalg.norm(ref)
        print(tag, "layer", l, "student grad rel err", err)
        assert err < 2e-3, (l, err)
    gt = mod.layer_selector.log_temperatures.grad.cpu().numpy()
    print(tag, "dlogtau", gt, g[f"{tag}_grad_log_temperatures"])
    np.testing.assert_allclose(gt, g[f"{tag}_grad_log_temperatures"], rtol=2e-3, atol=1e-7)


@pytest.mark.parametrize("tag", ["vit", "vit_same"])
def test_full_small_golden_multilayer(golden, tag):
    """Multi-layer (ViT) teachers: ranks, distances, mixing weights, loss value and the gradients that flow
    through the selector (route (b): principal angles -> eigenvectors of the student Gram) and the mixing
    weights (teacher tokens + attention) -- looser tolerance there, the route is ill-conditioned
    (hard part 3)."""
    _full_small_golden_multilayer(golden, tag, True)


@pytest.mark.parametrize("tag", ["vit", "vit_same"])
def test_full_small_golden_multilayer_tridiagonal_backward(golden, tag):
    """The same against the goldens on the tridiagonal route's backward (leading-k eigenvectors + shifted solves):
    the route of student orders past the LDS-resident Jacobi solver (cfg-4's 768), which the toy shapes otherwise
    leave to the Jacobi eigenvectors."""
    _full_small_golden_multilayer(golden, tag, False)


@pytest.mark.parametrize("name,seed,batch,ls,strided", [
    ("cfg1", 1234, None, 0.01, False), ("cfg2", 1234, 8, 0.001, True), ("cfg2", 1235, 8, 0.001, False),
    ("cfg5", 1234, 4, 0.001, True)])
def test_baseline_scalars(golden, name, seed, batch, ls, strided):
    g = golden("baseline_scalars.npz")
    shape = synth.CONFIGS[name]
    tag = f"{name}_s{seed}_b{batch or shape.batch}"
    mod = _module(shape, ls)
    inp = synth.make_inputs(shape, seed, batch=batch, device=DEV, strided=strided)
    leaves = {k: v.detach().requires_grad_(True) for k, v in inp.student.items()}
    loss = mod(inp.logits, inp.targets, leaves, inp.teacher, inp.attn)
    assert [mod.layer_selector.subspace_ranks[k] for k in sorted(inp.teacher)] == list(g[f"{tag}_ranks"])
    np.testing.assert_allclose(loss.item(), g[f"{tag}_loss"], rtol=1e-4)
    loss.backward()
    norms = np.array([leaves[l].grad.double().norm().item() for l in mod.token_layers])
    np.testing.assert_allclose(norms, g[f"{tag}_grad_student_norms"], rtol=1e-3)


def test_cfg4_scalar(golden):
    """cfg-4 shapes (ViT-B <- ViT-L, 24 teacher layers, CLS attention) at batch 4: ranks, loss, gradient norms."""
    g = golden("baseline_scalars.npz")
    shape = synth.CONFIGS["cfg4"]
    mod = _module(shape, 0.001)
    inp = synth.make_inputs(shape, 1234, batch=4, device=DEV, strided=True)
    leaves = {k: v.detach().requires_grad_(True) for k, v in inp.student.items()}
    loss = mod(inp.logits, inp.targets, leaves, inp.teacher, inp.attn)
    assert [mod.layer_selector.subspace_ranks[k] for k in sorted(inp.teacher)] == list(g["cfg4_s1234_b4_ranks"])
    np.testing.assert_allclose(loss.item(), g["cfg4_s1234_b4_loss"], rtol=1e-4)
    loss.backward()
    norms = np.array([leaves[l].grad.double().norm().item() for l in mod.token_layers])
    np.testing.assert_allclose(norms, g["cfg4_s1234_b4_grad_student_norms"], rtol=2e-3)
    np.testing.assert_allclose(mod.layer_selector.log_temperatures.grad.cpu().numpy(),
                               g["cfg4_s1234_b4_grad_log_temperatures"], rtol=5e-3, atol=1e-8)


def test_cfg2_full_size(golden):
    """BASELINE.json configs[1] at full size (B=256): golden loss from the reference's CPU run."""
    g = golden("baseline_scalars.npz")
    shape = synth.CONFIGS["cfg2"]
    mod = _module(shape, 0.001)
    inp = synth.make_inputs(shape, 1234, device=DEV, strided=True)
    leaves = {k: v.detach().requires_grad_(True) for k, v in inp.student.items()}
    loss = mod(inp.logits, inp.targets, leaves, inp.teacher, inp.attn)
    assert list(mod.layer_selector.subspace_ranks.values()) == list(g["cfg2_s1234_b256_ranks"])
    np.testing.assert_allclose(loss.item(), g["cfg2_s1234_b256_loss"], rtol=1e-4)
    loss.backward()
    norms = np.array([leaves[l].grad.double().norm().item() for l in mod.token_layers])
    np.testing.assert_allclose(norms, g["cfg2_s1234_b256_grad_student_norms"], rtol=1e-3)
    # size-independent properties: per-sample Procrustes loss is non-negative; total = harmonic mean
    comp = mod.last_components
    ce, geo = comp["ce"].item(), comp["geo_layers"].mean().item()
    assert abs(loss.item() - 2 * ce * geo / (ce + geo)) < 1e-4 * loss.item()


def _d_grass_sq(mod):
    """``last_components["d_grass_sq"]`` of the latest step (single-teacher steps publish it from the selector's tail
    stream: complete the step and synchronise before reading)."""
    mod.layer_selector.finish_pending()
    torch.cuda.synchronize()
    return mod.last_components["d_grass_sq"].cpu().numpy()


def _oracle_selector(state, cpu, token_layers):
    """(ranks, d_grass_sq (E, L)) of the CPU oracle's selector for the inputs ``cpu`` (synth.make_inputs on the CPU)."""
    with torch.no_grad():
        _, _, trace = O.selector_forward(state, cpu.student, cpu.teacher, cpu.attn, list(token_layers))
    return trace.ranks, np.stack([trace.d_grass_sq[l].numpy() for l in token_layers])


@pytest.mark.parametrize("chain", ["1", "0"])
def test_principal_angle_distance_single_teacher(golden, chain, monkeypatch):
    """d_grass_sq (layer_selector.py:99-105) of ONE teacher layer -- the SVD + principal-angle path of the headline
    step, whose value the loss cannot observe (softmax over one distance) -- against the reference's values at the
    cfg-1 / cfg-2 shapes and the small CNN case, through ``basd_selector_chain`` (one library call, device-side ranks)
    and through the kernel-by-kernel layout.  Two steps in a row with different inputs: the second one runs the
    speculative tail (eigenvector count from the previous step's rank)."""
    monkeypatch.setenv("BASD_SELECTOR_CHAIN", chain)
    g = golden("baseline_scalars.npz")
    for name, seed, batch, ls in [("cfg2", 1234, 8, 0.001), ("cfg2", 1235, 8, 0.001), ("cfg1", 1234, 32, 0.01)]:
        shape = synth.CONFIGS[name]
        mod = _module(shape, ls)
        tag = f"{name}_s{seed}_b{batch}"
        for rep in range(2):                                # rep 1: the tail was queued before the ranks were read
            inp = synth.make_inputs(shape, seed, batch=batch, device=DEV, strided=True)
            loss = mod(inp.logits, inp.targets, inp.student, inp.teacher, inp.attn)
            d = _d_grass_sq(mod)
            assert list(mod.layer_selector.subspace_ranks.values()) == list(g[f"{tag}_ranks"])
            np.testing.assert_allclose(d, g[f"{tag}_d_grass_sq"], rtol=2e-4, err_msg=f"{tag} rep {rep}")
            np.testing.assert_allclose(loss.item(), g[f"{tag}_loss"], rtol=1e-4)
    g = golden("full_small.npz")
    shape, seed = S.SMALL["cnn"]
    mod = _module(shape, 0.01)
    inp = synth.make_inputs(shape, seed, device=DEV)
    mod(inp.logits, inp.targets, inp.student, inp.teacher, inp.attn)
    np.testing.assert_allclose(_d_grass_sq(mod), g["cnn_d_grass_sq"], rtol=2e-4)


@pytest.mark.parametrize("n_s,n_t", [(49, 64), (196, 196)])
def test_mixing_weight_gradients_on_the_transposed_route(n_s, n_t, monkeypatch):
    """Multi-layer teachers with >= 128 cores that the plain LDS solver holds (up to 196 tokens: cfg-4) take the
    transposed route as well: the Jacobi runs on M^T alone and U Sigma -- the one piece of the SVD the backward through
    the mixing weights reads -- is rebuilt from it (basd_ustack_from_transposed).  Loss, student gradients and the
    temperature gradients must agree with the stacked cores (riding rows) on the same inputs."""
    shape = synth.LossShape("mix-t", 32, n_s, 96, 12, n_t, 128, 3, 4, True, 10, r_s=6, r_t=5)
    out = []
    for flag in (False, True):
        monkeypatch.setattr(ops, "TRANSPOSED_MIX_GRAD", flag)
        mod = _module(shape, 0.01)
        inp = synth.make_inputs(shape, 21, device=DEV, strided=True)
        leaves = {k: v.detach().requires_grad_(True) for k, v in inp.student.items()}
        loss = mod(inp.logits, inp.targets, leaves, inp.teacher, inp.attn)
        loss.backward()
        out.append((loss.item(), [leaves[l].grad.double() for l in mod.token_layers],
                    mod.layer_selector.log_temperatures.grad.double().cpu().numpy()))
    (l0, g0, t0), (l1, g1, t1) = out
    assert abs(l0 - l1) <= 2e-6 * abs(l0), (l0, l1)
    # (the two routes agree with fp64 to ~1e-5 each on the stand-alone loss: test_relational_all_gradients_at_196_tokens_
    # vs_fp64; through the selector's principal angles the gradients are held to 2e-3 against the reference elsewhere)
    for a, b in zip(g0, g1):
        assert ((a - b).norm() / a.norm()).item() < 1e-3
    np.testing.assert_allclose(t1, t0, rtol=2e-3, atol=1e-8)


def test_early_launched_factorisation_gives_up_cleanly(golden, monkeypatch):
    """The teacher's factorisation is queued ahead of its input and waits, bounded, for a device word (whole-CU
    workgroups must take their CUs before the step's throughput launches fill the chip).  With a budget of one poll it
    must give up, the step must fall back to the plain launch (a warning, not an error) and deliver the reference's
    ranks, loss and distances; the following steps stay on the plain launch."""
    from basd_amd import chain
    monkeypatch.setattr(chain, "EARLY_LAUNCH", True)          # an option (BASD_CHAIN_EARLY=1), off by default
    g = golden("baseline_scalars.npz")
    # with its normal budget the early-launched factorisation delivers the same ranks / distances
    shape = synth.CONFIGS["cfg2"]
    mod = _module(shape, 0.001)
    mod.chain_mode = 3                # the early launch belongs to the layout with the teacher matrices first
    inp = synth.make_inputs(shape, 1234, batch=8, device=DEV, strided=True)
    for _ in range(3):
        loss = mod(inp.logits, inp.targets, inp.student, inp.teacher, inp.attn)
        assert list(mod.layer_selector.subspace_ranks.values()) == list(g["cfg2_s1234_b8_ranks"])
        np.testing.assert_allclose(_d_grass_sq(mod), g["cfg2_s1234_b8_d_grass_sq"], rtol=2e-4)
    assert list(mod._chain_plans.values())[0].early is True
    monkeypatch.setattr(chain, "EARLY_BUDGET", 1)
    shape = synth.CONFIGS["cfg2"]
    mod = _module(shape, 0.001)
    mod.chain_mode = 3
    inp = synth.make_inputs(shape, 1234, batch=8, device=DEV, strided=True)
    with pytest.warns(RuntimeWarning, match="early-launched factorisation"):
        loss = mod(inp.logits, inp.targets, inp.student, inp.teacher, inp.attn)
    assert list(mod.layer_selector.subspace_ranks.values()) == list(g["cfg2_s1234_b8_ranks"])
    np.testing.assert_allclose(loss.item(), g["cfg2_s1234_b8_loss"], rtol=1e-4)
    np.testing.assert_allclose(_d_grass_sq(mod), g["cfg2_s1234_b8_d_grass_sq"], rtol=2e-4)
    plan = list(mod._chain_plans.values())[0]
    assert plan.early is False
    loss2 = mod(inp.logits, inp.targets, inp.student, inp.teacher, inp.attn)          # no warning any more
    np.testing.assert_allclose(loss2.item(), g["cfg2_s1234_b8_loss"], rtol=1e-4)


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_selector_chain_layouts_agree_with_the_reference(golden, mode):
    """``basd_selector_chain`` in each of its four layouts (where the student side sits; one factorisation launch or two):
    the reference's ranks, loss and d_grass_sq, step after step (two slots, speculative tail)."""
    g = golden("baseline_scalars.npz")
    shape = synth.CONFIGS["cfg2"]
    mod = _module(shape, 0.001)
    mod.chain_mode = mode
    inp = synth.make_inputs(shape, 1234, batch=8, device=DEV, strided=True)
    for _ in range(3):
        loss = mod(inp.logits, inp.targets, inp.student, inp.teacher, inp.attn)
        assert list(mod.layer_selector.subspace_ranks.values()) == list(g["cfg2_s1234_b8_ranks"])
        np.testing.assert_allclose(loss.item(), g["cfg2_s1234_b8_loss"], rtol=1e-4)
        np.testing.assert_allclose(_d_grass_sq(mod), g["cfg2_s1234_b8_d_grass_sq"], rtol=2e-4)
    assert list(mod._chain_plans.values())[0].mode == mode


def test_selector_tails_on_two_streams(golden, monkeypatch):
    """Teachers of high rank: alternate steps queue the selector's tail on a second stream (``chain.TAIL_STREAMS``; taken
    by itself from rank 96 on).  Forced here at the golden's shapes: ranks, loss and d_grass_sq of four consecutive steps
    (every slot, both streams) against the reference's."""
    from basd_amd import chain
    monkeypatch.setattr(chain, "TAIL_STREAMS", 2)
    g = golden("baseline_scalars.npz")
    shape = synth.CONFIGS["cfg2"]
    mod = _module(shape, 0.001)
    inp = synth.make_inputs(shape, 1234, batch=8, device=DEV, strided=True)
    seen = set()
    for _ in range(4):
        loss = mod(inp.logits, inp.targets, inp.student, inp.teacher, inp.attn)
        assert list(mod.layer_selector.subspace_ranks.values()) == list(g["cfg2_s1234_b8_ranks"])
        np.testing.assert_allclose(loss.item(), g["cfg2_s1234_b8_loss"], rtol=1e-4)
        np.testing.assert_allclose(_d_grass_sq(mod), g["cfg2_s1234_b8_d_grass_sq"], rtol=2e-4)
        for plan in mod._chain_plans.values():
            seen.update(slot.tail_stream.cuda_stream for slot in plan.slots if slot.d_out is not None)
    assert len(seen) == 2, "both tail streams must have been used"


def test_principal_angle_distance_cfg2_full_batch_vs_oracle():
    """The same at the headline size (B = 256, kmax 48, n 384): no reference value exists at this size for d (the golden
    holds the loss), so the oracle's selector is run on the CPU for the same inputs (seconds: it needs the Gram route,
    not the per-sample SVDs)."""
    shape = synth.CONFIGS["cfg2"]
    mod = _module(shape, 0.001)
    inp = synth.make_inputs(shape, 1234, device=DEV, strided=True)
    mod(inp.logits, inp.targets, inp.student, inp.teacher, inp.attn)
    d = _d_grass_sq(mod)
    torch.manual_seed(42)
    state = O.SelectorState.create(shape.points, shape.d_s, shape.d_t)
    cpu = synth.make_inputs(shape, 1234)
    ranks, d_ref = _oracle_selector(state, cpu, mod.token_layers)
    assert mod.layer_selector.subspace_ranks == ranks
    np.testing.assert_allclose(d, d_ref, rtol=2e-4)


def test_speculative_tail_follows_the_rank():
    """The selector tail is sized by the PREVIOUS step's rank: a step whose rank jumps far above the hint must re-queue
    it, a step whose rank drops must still be right -- d_grass_sq against the oracle in both."""
    shape = synth.CONFIGS["cfg2"]
    mod = _module(shape, 0.001)
    torch.manual_seed(42)
    state = O.SelectorState.create(shape.points, shape.d_s, shape.d_t)
    import dataclasses
    for r_t in (12, 70, 20):                                 # teacher rank of the synthetic features per step
        sh = dataclasses.replace(shape, r_t=r_t)
        inp = synth.make_inputs(sh, 500 + r_t, batch=8, device=DEV, strided=True)
        mod(inp.logits, inp.targets, inp.student, inp.teacher, inp.attn)
        d = _d_grass_sq(mod)
        cpu = synth.make_inputs(sh, 500 + r_t, batch=8)
        ranks, d_ref = _oracle_selector(state, cpu, mod.token_layers)
        assert mod.layer_selector.subspace_ranks == ranks, r_t
        np.testing.assert_allclose(d, d_ref, rtol=3e-4, err_msg=str(r_t))


def test_selector_tail_at_teacher_ranks_near_160():
    """Teachers of rank ~160 (what random-init / real ResNet-50 features give at D_s = 384): from the second step on the
    tail is sized by a hint past 96 -- the principal-angle matrices are zero-padded to the common order and take the
    register-resident solver, alternate steps use the second tail stream.  Ranks and d_grass_sq against the oracle while
    the rank moves up and down (150 -> 165 -> 120 -> 160)."""
    shape = synth.CONFIGS["cfg2"]
    mod = _module(shape, 0.001)
    torch.manual_seed(42)
    state = O.SelectorState.create(shape.points, shape.d_s, shape.d_t)
    import dataclasses
    for r_t in (150, 165, 120, 160):
        sh = dataclasses.replace(shape, r_t=r_t)
        inp = synth.make_inputs(sh, 900 + r_t, batch=16, device=DEV, strided=True)
        mod(inp.logits, inp.targets, inp.student, inp.teacher, inp.attn)
        d = _d_grass_sq(mod)
        cpu = synth.make_inputs(sh, 900 + r_t, batch=16)
        ranks, d_ref = _oracle_selector(state, cpu, mod.token_layers)
        assert mod.layer_selector.subspace_ranks == ranks, r_t
        assert min(ranks.values()) > 100, ranks
        np.testing.assert_allclose(d, d_ref, rtol=3e-4, err_msg=str(r_t))


def test_bf16_inputs_cfg5_shapes():
    """cfg-5 (bf16 features): tokens are consumed in place as bf16 and widened inside the kernels; the parity
    target is the fp32 oracle on the same bf16-rounded values (the reference itself has no runnable
    bf16-input CPU path: its selector matmul mixes dtypes)."""
    shape = synth.CONFIGS["cfg5"]
    mod = _module(shape, 0.001)
    inp = synth.make_inputs(shape, 77, batch=4, device=DEV, dtype=torch.bfloat16, strided=True)
    leaves = {k: v.detach().requires_grad_(True) for k, v in inp.student.items()}
    loss = mod(inp.logits, inp.targets, leaves, inp.teacher, inp.attn)
    loss.backward()
    torch.manual_seed(42)
    state = O.SelectorState.create(shape.points, shape.d_s, shape.d_t)
    cpu = synth.make_inputs(shape, 77, batch=4, dtype=torch.bfloat16)
    st = {k: v.float().requires_grad_(True) for k, v in cpu.student.items()}
    te = {k: v.float() for k, v in cpu.teacher.items()}
    at = {k: v.float() for k, v in cpu.attn.items()}
    crit = torch.nn.CrossEntropyLoss(label_smoothing=0.001)
    ref, trace = O.basd_forward(state, crit, mod.token_layers, shape.n_s, shape.has_cls, cpu.logits, cpu.targets,
                                st, te, at)
    ref.backward()
    assert mod.layer_selector.subspace_ranks == trace.selector.ranks
    np.testing.assert_allclose(loss.item(), ref.item(), rtol=1e-4)
    for l in mod.token_layers:
        assert leaves[l].grad.dtype == torch.bfloat16
        g, r = leaves[l].grad.float().cpu(), st[l].grad
        assert ((g - r).norm() / r.norm()).item() < 1e-2       # the gradient itself is rounded to bf16


@pytest.mark.parametrize("sync_ranks", [True, False, "auto"])
def test_rank_zero_raises_like_the_reference(sync_ranks):
    """A teacher whose projected Gram has a flat spectrum has Marchenko-Pastur rank 0 (no eigenvalue exceeds
    median * (1 + sqrt(q))^2); the reference then produces NaN mixing weights and torch.linalg.svd raises
    LinAlgError.  Same class here, and the oracle agrees on the rank.
    ``rank_readback`` "sync" and "auto" (the default: a flat spectrum is exactly what the rank certificate cannot
    prove anything about, so the host waits for the ranks): raised inside the call, the reference's timing; "deferred"
    (BASD_RANK_READBACK=deferred, one teacher layer): raised by the first reader of ``subspace_ranks`` or by the
    next forward."""
    shape = synth.LossShape("flat", 4, 16, 32, 12, 16, 48, 1, 1, False, 10)
    mod = _module(shape, 0.0)
    if sync_ranks == "auto":
        mod.rank_readback = "auto"          # the default (unless BASD_RANK_READBACK says otherwise)
        sync_ranks = True
    else:
        mod.sync_ranks = sync_ranks
    gen = torch.Generator().manual_seed(1)
    B = 8
    q, _ = torch.linalg.qr(torch.randn(B * 16, 48, generator=gen))      # orthonormal columns: T^T T = I
    teacher_cpu = q.reshape(B, 16, 48).contiguous()
    assert O.mp_rank(teacher_cpu.reshape(-1, 48) @ mod.layer_selector.proj_t.cpu().T) == 0
    student = {l: synth.structured(gen, B, 16, 32, 4).to(DEV) for l in mod.token_layers}
    teacher = {0: teacher_cpu.to(DEV)}
    attn = {0: (torch.ones(B, 1, 16, 16) / 16).to(DEV)}
    logits = torch.randn(B, 10, generator=gen).to(DEV)
    targets = torch.randint(0, 10, (B,), generator=gen).to(DEV)
    if sync_ranks:
        with pytest.raises(torch.linalg.LinAlgError):
            mod(logits, targets, student, teacher, attn)
    else:
        loss = mod(logits, targets, student, teacher, attn)        # the Procrustes value does not depend on the rank
        assert torch.isfinite(loss).item()
        with pytest.raises(torch.linalg.LinAlgError):
            mod(logits, targets, student, teacher, attn)           # the previous step's error surfaces here
        with pytest.raises(torch.linalg.LinAlgError):
            mod.layer_selector.subspace_ranks                      # ... and this step's on the first read
    assert mod.layer_selector.subspace_ranks == {0: 0}


def test_rank_readback_is_deferred_only_behind_a_proof():
    """``rank_readback = "auto"``: with a teacher whose spectrum has a clear signal part the certificate kernel proves
    "rank >= 1" behind the teacher Grams and forward returns without waiting for the factorisation -- same loss, same
    gradients, the same ranks and d_grass_sq (read afterwards) as with the read-back inside forward."""
    shape = synth.CONFIGS["cfg2"]
    inp = synth.make_inputs(shape, 7, batch=64, device=DEV, strided=True)
    out = {}
    for mode in ("sync", "auto"):
        mod = _module(shape, 0.0)
        mod.rank_readback = mode
        leaves = {l: inp.student[l].detach().requires_grad_(True) for l in mod.token_layers}
        for _ in range(2):       # the second step also exercises the speculative tail behind a deferred read-back
            for t in leaves.values():
                t.grad = None
            loss = mod(inp.logits, inp.targets, leaves, inp.teacher, inp.attn)
            loss.backward()
        deferred = mod.readback_deferred_steps
        ranks = dict(mod.layer_selector.subspace_ranks)              # completes a deferred read-back
        mod.layer_selector.finish_pending()
        torch.cuda.synchronize()
        out[mode] = (loss.item(), [leaves[l].grad.clone() for l in mod.token_layers], ranks,
                     mod.last_components["d_grass_sq"].clone(), deferred)
    assert out["sync"][4] == 0 and out["auto"][4] == 2, (out["sync"][4], out["auto"][4])
    # a pending read-back must not keep the step's token tensors alive: one more deferred step, then look at
    # what the pending closure still references
    loss = mod(inp.logits, inp.targets, leaves, inp.teacher, inp.attn)
    pending = mod.layer_selector._pending_tail
    assert pending is not None
    ptrs = {t.data_ptr() for t in list(inp.teacher.values()) + [leaves[l] for l in mod.token_layers]}

    def tensors_in(obj, depth=0):
        if isinstance(obj, torch.Tensor):
            yield obj
        elif isinstance(obj, (list, tuple)) and depth < 3:
            for x in obj:
                yield from tensors_in(x, depth + 1)
    held = [t for c in pending.__closure__ for t in tensors_in(c.cell_contents) if t.data_ptr() in ptrs]
    assert not held, "the deferred read-back references input tensors"
    mod.layer_selector.finish_pending()
    assert out["sync"][0] == out["auto"][0]
    for a, b in zip(out["sync"][1], out["auto"][1]):
        assert torch.equal(a, b)
    assert out["sync"][2] == out["auto"][2] and min(out["auto"][2].values()) >= 1
    # (the two modes take different chain layouts -- one factorisation launch or two -- so d_grass_sq agrees to rounding)
    torch.testing.assert_close(out["sync"][3], out["auto"][3], rtol=1e-5, atol=0)


def test_bf16_multilayer_teacher_rounds_the_mixing_weights_like_the_reference():
    """layer_selector.py:110 casts the mixing weights to the token dtype: with a bf16 multi-layer teacher they are bf16
    values.  Same here (value only: the adjoint of a cast is the identity); the loss agrees with the oracle run on the same
    bf16 inputs to bf16 accuracy (the reference also MIXES in bf16, which this library does in fp32)."""
    shape, seed = S.SMALL["vit"]
    mod = _module(shape, 0.01)
    inp = synth.make_inputs(shape, seed, dtype=torch.bfloat16)
    student = {l: inp.student[l].to(DEV).requires_grad_(True) for l in mod.token_layers}
    teacher = {k: v.to(DEV) for k, v in inp.teacher.items()}
    attn = {k: v.to(DEV) for k, v in inp.attn.items()}
    loss = mod(inp.logits.to(DEV), inp.targets.to(DEV), student, teacher, attn)
    loss.backward()
    mix = mod.last_components["mix"]
    assert torch.equal(mix, mix.to(torch.bfloat16).float()), "weights must be bf16-representable"
    assert mod.layer_selector.log_temperatures.grad is not None and torch.isfinite(mod.layer_selector.log_temperatures.grad).all()
    # the oracle on the widened inputs (torch has no bf16 linalg on the CPU): same ranks, loss to the accuracy of the rounding
    torch.manual_seed(42)
    state = O.SelectorState.create(shape.points, shape.d_s, shape.d_t)
    crit = torch.nn.CrossEntropyLoss(label_smoothing=0.01)
    ref, trace = O.basd_forward(state, crit, mod.token_layers, shape.n_s, shape.has_cls, inp.logits, inp.targets,
                                {k: v.float() for k, v in inp.student.items()}, {k: v.float() for k, v in inp.teacher.items()},
                                {k: v.float() for k, v in inp.attn.items()})
    assert mod.layer_selector.subspace_ranks == trace.selector.ranks
    np.testing.assert_allclose(loss.item(), ref.item(), rtol=1e-2)
    exact = torch.stack([trace.selector.mix_weights[l] for l in mod.token_layers])
    assert torch.equal(mix.cpu(), exact.to(torch.bfloat16).float()) or \
        torch.allclose(mix.cpu(), exact.to(torch.bfloat16).float(), atol=2 ** -8)      # a weight may sit on a rounding boundary


def test_selector_forward_api_materialises_mixed_tensors(golden):
    """GrassmannianLayerSelector.forward keeps the reference's return contract (dicts of mixed tokens and
    attention maps); values against the reference's own outputs."""
    g = golden("selector_outputs.npz")
    shape, seed = S.SMALL["vit"]
    mod = _module(shape, 0.01)
    inp = synth.make_inputs(shape, seed, device=DEV)
    with torch.no_grad():
        mixed, mixed_attn = mod.layer_selector(inp.student, inp.teacher, inp.attn, mod.token_layers)
    for l in mod.token_layers:
        assert mixed[l].shape == inp.teacher[0].shape and mixed_attn[l].shape == inp.attn[0].shape
        np.testing.assert_allclose(mixed[l][:, :5, :7].cpu().numpy(), g[f"mixed_{l}_slice"], rtol=2e-3, atol=2e-4)
        np.testing.assert_allclose(mixed_attn[l][:, :, 0, 1:].cpu().numpy(), g[f"attn_{l}_cls_row"], rtol=2e-3, atol=1e-6)
    # the reference's per-layer helper, driven the way the reference's forward drives it (layer_selector.py:131-150)
    sel = mod.layer_selector
    keys = sorted(inp.teacher)
    sub, spw = {}, {}
    with torch.no_grad():
        for k in keys:
            z_t = ops.gemm_nt(inp.teacher[k], sel.proj_t.float().contiguous())
            sub[k], spw[k] = losses._grassmann_subspace(z_t, k=sel.subspace_ranks[k])
        tok = torch.stack([inp.teacher[k] for k in keys])
        att = torch.stack([inp.attn[k] for k in keys])
        for i, l in enumerate(mod.token_layers):
            m, a = sel._mix_for_student_layer(i, inp.student[l], keys, tok, att, sub, spw)
            np.testing.assert_allclose(m[:, :5, :7].cpu().numpy(), g[f"mixed_{l}_slice"], rtol=2e-3, atol=2e-4)
            np.testing.assert_allclose(a[:, :, 0, 1:].cpu().numpy(), g[f"attn_{l}_cls_row"], rtol=2e-3, atol=1e-6)


@pytest.mark.parametrize("solver", ["tridiag", "jacobi"])
@pytest.mark.parametrize("tag", ["vit", "cnn", "vit_same"])
def test_estimate_ranks_golden(golden, tag, solver, monkeypatch):
    """GrassmannianLayerSelector._estimate_ranks (layer_selector.py:69-74) by itself: ``subspace_ranks`` against the
    ranks the imported reference produced on the same teacher tensors (exact)."""
    monkeypatch.setattr(ops, "EIG_SOLVER", solver)
    g = golden("full_small.npz")
    shape, seed = S.SMALL[tag]
    mod = _module(shape, 0.01)
    inp = synth.make_inputs(shape, seed, device=DEV)
    sel = mod.layer_selector
    assert sel.subspace_ranks == {}
    sel._estimate_ranks(inp.teacher)
    assert [sel.subspace_ranks[k] for k in sorted(inp.teacher)] == list(g[f"{tag}_ranks"])


def test_estimate_ranks_cfg4_shapes(golden):
    """... and at cfg-4 shapes (24 ViT-L layers, batch 4), strided CLS-sliced views."""
    g = golden("baseline_scalars.npz")
    shape = synth.CONFIGS["cfg4"]
    mod = _module(shape, 0.001)
    inp = synth.make_inputs(shape, 1234, batch=4, device=DEV, strided=True)
    mod.layer_selector._estimate_ranks(inp.teacher)
    assert [mod.layer_selector.subspace_ranks[k] for k in sorted(inp.teacher)] == list(g["cfg4_s1234_b4_ranks"])


@pytest.mark.parametrize("name,dtype", [("cfg4", torch.float32), ("cfg5", torch.bfloat16)])
def test_full_batch_properties(name, dtype):
    """BASELINE.json configs[3] (B=128, 24 teacher layers: the block Jacobi path on 512 stacked 392 x 196 cores) and
    configs[4] (B=64, 576 student tokens, bf16 features) at FULL batch.  The oracle needs minutes there, so the
    checks are the size-independent properties of the path: finite loss, per-sample Procrustes loss >= 0 (it is a
    squared Bures-Wasserstein distance), total = harmonic mean of CE and geo (UW-SO, combined.py:78-85), mixing
    weights on the simplex, every SVD converged below the sweep cap, eigen-solver status words clean, gradients
    finite and of the inputs' dtype."""
    shape = synth.CONFIGS[name]
    mod = _module(shape, 0.001)
    inp = synth.make_inputs(shape, 1234, device=DEV, dtype=dtype, strided=True, attn_on_device=shape.layers_t > 1)
    leaves = {k: v.detach().requires_grad_(True) for k, v in inp.student.items()}
    logits = inp.logits.requires_grad_(True)
    loss = mod(logits, inp.targets, leaves, inp.teacher, inp.attn)
    loss.backward()
    ranks = mod.layer_selector.subspace_ranks            # completes the read-back; raises on a give-up / rank 0
    assert len(ranks) == shape.layers_t and min(ranks.values()) >= 1
    assert max(ranks.values()) <= shape.d_s - 1
    comp = mod.last_components
    ce, geo = comp["ce"].item(), comp["geo_layers"].mean().item()
    assert np.isfinite(loss.item()) and geo > 0
    assert abs(loss.item() - 2 * ce * geo / (ce + geo)) < 1e-4 * loss.item()
    mix = comp["mix"].cpu().numpy()
    assert mix.shape == (shape.points, shape.layers_t) and (mix >= 0).all()
    np.testing.assert_allclose(mix.sum(axis=1), 1.0, rtol=1e-5)
    for l in mod.token_layers:
        gl = leaves[l].grad
        assert gl.dtype == dtype and torch.isfinite(gl.float()).all().item() and gl.float().norm().item() > 0
    if shape.layers_t > 1:
        gt = mod.layer_selector.log_temperatures.grad
        assert torch.isfinite(gt).all().item()
    # the Procrustes cores once more, with the sweep counts
    students = [leaves[l].detach() for l in mod.token_layers]
    keys = sorted(inp.teacher)
    pc = ops.procrustes_forward(students, [inp.teacher[k] for k in keys], [inp.attn[k] for k in keys],
                                comp["mix"].float(), shape.has_cls, need_backward=False, want_sweeps=True)
    lb = pc.loss_b.cpu().numpy()
    scale = (pc.tr_s + pc.tr_t).cpu().numpy()
    assert np.isfinite(lb).all() and (lb >= -2e-5 * scale).all()
    np.testing.assert_allclose(lb.mean(axis=1), comp["geo_layers"].cpu().numpy(), rtol=1e-5)
    if pc.sweeps is not None and int(pc.sweeps.max()) > 0:
        assert int(pc.sweeps.max()) < ops.MAX_SWEEPS


def test_reference_checkpoint_round_trip_on_gpu(golden):
    """Checkpoint interchange (reference trainer.py:84,94-123): a state file written by the REFERENCE module (with
    trained, non-default temperatures) loads into the build's module on the GPU, and a step from it reproduces the
    reference's loss, mixing weights and temperature gradient; the build's own state file loads back bit-equal."""
    import io
    g = golden("checkpoint.npz")
    shape, seed = S.SMALL["vit"]
    mod = _module(shape, 0.01)
    state = torch.load(os.path.join(os.path.dirname(__file__), "golden", "ref_basd_state.pth"), map_location=DEV,
                       weights_only=True)
    res = mod.load_state_dict(state, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    np.testing.assert_array_equal(mod.layer_selector.log_temperatures.detach().cpu().numpy(), g["log_temperatures"])
    inp = synth.make_inputs(shape, seed, device=DEV)
    leaves = {k: v.requires_grad_(True) for k, v in inp.student.items()}
    loss = mod(inp.logits, inp.targets, leaves, inp.teacher, inp.attn)
    np.testing.assert_allclose(loss.item(), g["loss"], rtol=1e-4)
    np.testing.assert_allclose(mod.last_components["mix"].cpu().numpy(), g["mix_weights"], rtol=2e-3, atol=1e-6)
    loss.backward()
    np.testing.assert_allclose(mod.layer_selector.log_temperatures.grad.cpu().numpy(), g["grad_log_temperatures"],
                               rtol=3e-3, atol=1e-7)
    # and back: save on the GPU, load into a fresh module (what accelerate's load_state does)
    buf = io.BytesIO()
    torch.save(mod.state_dict(), buf)
    buf.seek(0)
    fresh = _module(shape, 0.01)
    fresh.load_state_dict(torch.load(buf, map_location=DEV, weights_only=True), strict=True)
    for (ka, a), (kb, b) in zip(mod.state_dict().items(), fresh.state_dict().items()):
        assert ka == kb and torch.equal(a, b)
    assert int(g["reverse_load_ok"]) == 1       # recorded by make_goldens: the build's state_dict loads into the reference


@pytest.mark.parametrize("tag", ["cnn", "vit"])
def test_give_up_degrades_to_one_member(golden, tag, monkeypatch):
    """A give-up of the tridiagonalisation's shared stage (simulated: the first rank read-back reports one) must not
    kill the step: the selector is queued again with one workgroup per matrix and the step's results are the usual
    ones; the setting sticks (with a warning)."""
    from basd_amd import _lib
    g = golden("full_small.npz")
    shape, seed = S.SMALL[tag]
    mod = _module(shape, 0.01)
    inp = synth.make_inputs(shape, seed, device=DEV)
    sel = mod.layer_selector
    real = sel._read_ranks
    calls = {"n": 0}

    def flaky(st, keys):
        calls["n"] += 1
        if calls["n"] == 1:
            raise losses.TridiagGiveUp("simulated give-up")
        return real(st, keys)
    monkeypatch.setattr(sel, "_read_ranks", flaky)
    leaves = {k: v.requires_grad_(True) for k, v in inp.student.items()}
    try:
        with pytest.warns(RuntimeWarning, match="one workgroup per matrix"):
            loss = mod(inp.logits, inp.targets, leaves, inp.teacher, inp.attn)
        assert calls["n"] >= 2
        assert [sel.subspace_ranks[k] for k in sorted(inp.teacher)] == list(g[f"{tag}_ranks"])
        np.testing.assert_allclose(loss.item(), g[f"{tag}_loss"], rtol=1e-4)
        loss.backward()
    finally:
        _lib.call("basd_tridiag_tuning", -1, -1, -1, -1, -1, 1)


@pytest.mark.parametrize("n_s,n_t,d_s,d_t,cls", [
    (256, 256, 320, 384, False),     # 255 < D: cores of full rank 255, Grams past one workgroup's tile list
    (576, 576, 96, 128, True),       # a ViT teacher at 384 x 384: 576 tokens on both sides, cores of rank 96
    (324, 576, 64, 96, True),        # finer teacher grid resampled to 324 student tokens
    (400, 225, 48, 160, False),      # coarser teacher: the core grid is the teacher's 225 tokens
])
def test_cores_past_lds_vs_fp64(n_s, n_t, d_s, d_t, cls):
    """min(N_s, N_t) > 196: the Gram tile list is cut into chunks, the Cholesky factor lives in global memory
    (panels in LDS), the SVD takes the block path and K' a tiled kernel.  Per-sample terms and the student gradient
    against an fp64 evaluation of relational.py:36-50 (autograd through svdvals)."""
    from basd_amd import ops
    gen = torch.Generator().manual_seed(n_s + 3 * n_t)
    B = 2
    s = synth.structured(gen, B, n_s, d_s, 8) + 0.5
    t = synth.structured(gen, B, n_t, d_t, 6) - 0.25
    a = n_t + (1 if cls else 0)
    attn = torch.softmax(torch.randn(B, 2, a, a, generator=gen), dim=-1)
    w = O.token_weights(attn, cls, n_s).double()
    t_al = O.resample_tokens(t, n_s).double()
    s64 = s.double().requires_grad_(True)
    w3 = w.unsqueeze(-1)
    s_w = w3.sqrt() * (s64 - (w3 * s64).sum(1, keepdim=True))
    t_w = w3.sqrt() * (t_al - (w3 * t_al).sum(1, keepdim=True))
    tr_s, tr_t = s_w.square().sum((1, 2)), t_w.square().sum((1, 2))
    nuc = torch.linalg.svdvals(torch.bmm(s_w.transpose(1, 2), t_w)).sum(-1)
    ref_b = tr_s + tr_t - 2 * nuc
    ref_b.mean().backward()
    sd = s.to(DEV)
    pc = ops.procrustes_forward([sd], [t.to(DEV)], [attn.to(DEV)], torch.ones(1, 1, device=DEV), cls,
                                want_sweeps=True)
    assert int(pc.sweeps.max()) < ops.MAX_SWEEPS
    np.testing.assert_allclose(pc.tr_s[0].cpu().numpy(), tr_s.detach().numpy(), rtol=1e-5)
    np.testing.assert_allclose(pc.tr_t[0].cpu().numpy(), tr_t.detach().numpy(), rtol=1e-5)
    np.testing.assert_allclose(pc.nuc[0].cpu().numpy(), nuc.detach().numpy(), rtol=2e-5)
    np.testing.assert_allclose(pc.loss_b[0].cpu().numpy(), ref_b.detach().numpy(), rtol=1e-4)
    grads = ops.procrustes_student_grads([sd], pc, torch.ones(1, device=DEV))
    err = (grads[0].double().cpu() - s64.grad).norm() / s64.grad.norm()
    assert err < 1e-4, err


@pytest.mark.parametrize("n,d_s,d_t,cls", [(256, 320, 384, False), (576, 64, 96, True)])
def test_relational_all_gradients_past_lds_vs_fp64(n, d_s, d_t, cls):
    """geometric_relational_loss at token grids past the LDS-resident kernels (ViT teacher at 384 x 384: 576 tokens):
    loss and gradients w.r.t. student tokens, teacher tokens and attention against fp64 autograd of
    relational.py:18-50 (the teacher-side factor takes the tiled kernels there)."""
    from basd_amd.losses import geometric_relational_loss
    gen = torch.Generator().manual_seed(5 * n + d_s)
    B = 2
    s = synth.structured(gen, B, n, d_s, 8) + 0.5
    t = synth.structured(gen, B, n, d_t, 6) - 0.25
    a = n + (1 if cls else 0)
    attn = torch.softmax(torch.randn(B, 2, a, a, generator=gen), dim=-1)
    s64, t64, a64 = (x.double().requires_grad_(True) for x in (s, t, attn))
    w = (a64[:, :, 0, 1:].mean(1) if cls else a64.mean((1, 2)))
    w = w / w.sum(-1, keepdim=True)
    w3 = w.unsqueeze(-1)
    s_w = w3.sqrt() * (s64 - (w3 * s64).sum(1, keepdim=True))
    t_w = w3.sqrt() * (t64 - (w3 * t64).sum(1, keepdim=True))
    ref = (s_w.square().sum((1, 2)) + t_w.square().sum((1, 2))
           - 2 * torch.linalg.svdvals(torch.bmm(s_w.transpose(1, 2), t_w)).sum(-1)).mean()
    rs, rt, ra = torch.autograd.grad(ref, [s64, t64, a64])
    sd, td, ad = (x.to(DEV).requires_grad_(True) for x in (s, t, attn))
    loss = geometric_relational_loss(sd, td, ad, has_cls_token=cls)
    np.testing.assert_allclose(loss.item(), ref.item(), rtol=1e-4)
    gs, gt, ga = torch.autograd.grad(loss, [sd, td, ad])
    for got, want, name in ((gs, rs, "student"), (gt, rt, "teacher"), (ga, ra, "attn")):
        err = ((got.double().cpu() - want).norm() / want.norm()).item()
        assert err < (2e-3 if name == "attn" else 2e-4), (name, err)


@pytest.mark.parametrize("route", ["stacked", "transposed"])
def test_relational_all_gradients_at_196_tokens_vs_fp64(route, monkeypatch):
    """The same at cfg-4's core size (196 tokens on both sides) on BOTH SVD routes -- the stacked cores with riding rows
    (two-pass solver) and the transposed cores with U Sigma rebuilt afterwards (what cfg-4 takes at its batch) -- against
    fp64 autograd: loss, student, teacher and attention gradients."""
    from basd_amd.losses import geometric_relational_loss
    from basd_amd import _lib
    n, d_s, d_t, cls = 196, 96, 128, True
    gen = torch.Generator().manual_seed(1961)
    B = 3
    s = synth.structured(gen, B, n, d_s, 8) + 0.5
    t = synth.structured(gen, B, n, d_t, 6) - 0.25
    a = n + 1
    attn = torch.softmax(torch.randn(B, 2, a, a, generator=gen), dim=-1)
    s64, t64, a64 = (x.double().requires_grad_(True) for x in (s, t, attn))
    w = a64[:, :, 0, 1:].mean(1)
    w = w / w.sum(-1, keepdim=True)
    w3 = w.unsqueeze(-1)
    s_w = w3.sqrt() * (s64 - (w3 * s64).sum(1, keepdim=True))
    t_w = w3.sqrt() * (t64 - (w3 * t64).sum(1, keepdim=True))
    ref = (s_w.square().sum((1, 2)) + t_w.square().sum((1, 2))
           - 2 * torch.linalg.svdvals(torch.bmm(s_w.transpose(1, 2), t_w)).sum(-1)).mean()
    rs, rt, ra = torch.autograd.grad(ref, [s64, t64, a64])
    monkeypatch.setattr(ops, "TRANSPOSED_MIX_GRAD", "force" if route == "transposed" else False)
    _lib.call("basd_procrustes_tuning", 2 if route == "transposed" else 0)
    try:
        sd, td, ad = (x.to(DEV).requires_grad_(True) for x in (s, t, attn))
        loss = geometric_relational_loss(sd, td, ad, has_cls_token=cls)
        np.testing.assert_allclose(loss.item(), ref.item(), rtol=1e-4)
        gs, gt, ga = torch.autograd.grad(loss, [sd, td, ad])
    finally:
        _lib.call("basd_procrustes_tuning", 1)
    for got, want, name in ((gs, rs, "student"), (gt, rt, "teacher"), (ga, ra, "attn")):
        err = ((got.double().cpu() - want).norm() / want.norm()).item()
        print(route, name, "rel err vs fp64", err)
        assert err < (2e-3 if name == "attn" else 2e-4), (route, name, err)


def test_teacher_factor_tiled_matches_lds_kernel():
    """The tiled teacher-side factor (cores past LDS) against the LDS-resident kernel on cores that fit both."""
    from basd_amd import ops
    gen = torch.Generator().manual_seed(91)
    B, n_s, n_t, d_s, d_t = 3, 196, 100, 72, 80
    s = synth.structured(gen, B, n_s, d_s, 8).to(DEV)
    t = synth.structured(gen, B, n_t, d_t, 6).to(DEV)
    attn = torch.softmax(torch.randn(B, 2, n_t, n_t, generator=gen), dim=-1).to(DEV)
    pc = ops.procrustes_forward([s], [t], [attn], torch.ones(1, 1, device=DEV), False, need_mix_grad=True)
    kt, tn = ops.procrustes_teacher_factor(pc)
    mg = pc.mixgrad
    n = mg["n"]
    tp = mg["student_taps"]
    kt2, tn2 = torch.empty_like(kt), torch.empty_like(tn)
    scratch = torch.empty((B, n, n), device=DEV)
    ops._lib.call("basd_teacher_factor_tiled", mg["W"].data_ptr(), 2 * n * n, mg["sigma"].data_ptr(), n, n_s, B,
                  mg["l_a"].data_ptr(), mg["g_b"].data_ptr(), n * n, mg["omega_e"].data_ptr(), tp.tap0.data_ptr(),
                  tp.tap1.data_ptr(), tp.lam.data_ptr(), tp.range0.data_ptr(), tp.range1.data_ptr(), kt2.data_ptr(),
                  tn2.data_ptr(), scratch.data_ptr(), ops._stream())
    torch.cuda.synchronize()
    assert torch.equal(tn, tn2)
    err = ((kt - kt2).norm() / kt.norm()).item()
    assert err < 1e-5, err


def test_module_with_a_576_token_vit_teacher_vs_oracle():
    """BASDLoss end to end with a multi-layer ViT teacher at 384 x 384 (576 tokens on both sides, a shape the
    round-1 build refused): ranks, mixing weights and loss against the CPU oracle, student / temperature gradients
    against the oracle's autograd (multi-layer tolerance: the route through the principal angles)."""
    shape = synth.LossShape("vit-384", 3, 576, 64, 12, 576, 96, 3, 2, True, 10, points=2, r_s=8, r_t=6)
    mod = _module(shape, 0.0)
    inp = synth.make_inputs(shape, 77)
    sel = mod.layer_selector
    st = O.SelectorState(sel.proj_s.detach().cpu(), sel.proj_t.detach().cpu(),
                         sel.log_temperatures.detach().cpu().clone().requires_grad_(True))
    ref_leaves = {k: v.clone().requires_grad_(True) for k, v in inp.student.items()}
    ref, trace = O.basd_forward(st, torch.nn.CrossEntropyLoss(), mod.token_layers, shape.n_s, True, inp.logits,
                                inp.targets, ref_leaves, inp.teacher, inp.attn)
    ref.backward()
    dev_in = synth.make_inputs(shape, 77, device=DEV)
    leaves = {k: v.requires_grad_(True) for k, v in dev_in.student.items()}
    loss = mod(dev_in.logits, dev_in.targets, leaves, dev_in.teacher, dev_in.attn)
    assert {k: sel.subspace_ranks[k] for k in sorted(inp.teacher)} == dict(trace.selector.ranks)
    np.testing.assert_allclose(loss.item(), ref.item(), rtol=1e-4)
    loss.backward()
    for l in mod.token_layers:
        want = ref_leaves[l].grad
        err = ((leaves[l].grad.cpu() - want).norm() / want.norm()).item()
        assert err < 2e-3, (l, err)
    np.testing.assert_allclose(sel.log_temperatures.grad.cpu().numpy(), st.log_temperatures.grad.numpy(),
                               rtol=5e-3, atol=1e-7)
