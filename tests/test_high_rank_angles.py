"""Principal angles past order 192 for multi-layer teachers.

The k x k cosine matrices of the selector have the order of the teacher layer's Marchenko-Pastur rank; with several
teacher layers the orders differ and the one-sided Jacobi takes them per matrix (``n_arr``).  Orders past 192 no
longer fit LDS and go through the block path.  The kernel against ``torch.linalg.svdvals`` in fp64, the selector, the
loss and its gradients against the CPU oracle at teacher ranks (100, 200, 215): one batch that mixes orders below and
above the LDS limit."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from basd_amd import synth, ops
from oracle import basd_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# storage of order 215: 16 lanes per column pair, blocks of 64 columns, 4 blocks.  Orders on, just past and far inside
# the block boundaries, below and above the LDS limit (192)
STORAGE = 215
ORDERS = [215, 200, 193, 192, 129, 128, 64, 1, 0]

B, N_TOK, D_S, D_T, HEADS, DEPTH, POINTS, CLASSES = 8, 100, 448, 512, 2, 12, 2, 10
TEACHER_SIGNAL_RANKS = (100, 200, 215)
WANT_RANKS = {0: 100, 1: 200, 2: 215}
SEED = 5


def test_jacobi_per_matrix_order_on_the_block_path():
    """Singular values of the leading k x k blocks, k per matrix, in storage of order 215 (the block path).  The last
    matrix has exact rank 10 inside an order-200 problem: 190 zero singular values.  What lies outside a matrix's
    leading block stays as it was."""
    g = torch.Generator().manual_seed(215)
    orders = ORDERS + [200]
    mats = torch.randn(len(orders), STORAGE, STORAGE, generator=g)
    low = torch.randn(200, 10, generator=g) @ torch.randn(10, 200, generator=g)
    mats[-1, :200, :200] = low
    W = mats.clone().to(DEV)
    n_arr = torch.tensor(orders, dtype=torch.int32, device=DEV)
    sigma = ops.jacobi_onesided(W, STORAGE, n_arr=n_arr).cpu()
    out = W.cpu()
    for i, k in enumerate(orders):
        outside = torch.ones(STORAGE, STORAGE, dtype=torch.bool)
        outside[:k, :k] = False
        assert torch.equal(out[i][outside], mats[i][outside]), f"matrix {i} (order {k}): storage past the order changed"
        if k == 0:
            continue
        ref = torch.linalg.svdvals(mats[i, :k, :k].double())
        got = sigma[i, :k].double().sort(descending=True).values
        err = ((got - ref).abs().max() / ref[0]).item()
        print(f"order {k}: max |sigma - svdvals| / sigma_max = {err:.3e}")
        assert err < 3e-6, (i, k, err)
    tail = sigma[-1, :200].double().sort(descending=True).values[10:]
    assert float(tail.max()) < 3e-6 * float(torch.linalg.svdvals(low.double())[0])


class _Case:
    """Inputs, module state and the CPU oracle's results for the three-layer teacher, computed once."""

    def __init__(self):
        gen = torch.Generator().manual_seed(SEED)
        self.layers = synth.extraction_layers(DEPTH, POINTS)
        self.student = {l: synth.structured(gen, B, N_TOK, D_S, 24) for l in self.layers}
        self.teacher = {l: synth.structured(gen, B, N_TOK, D_T, r, snr=12.0)
                        for l, r in enumerate(TEACHER_SIGNAL_RANKS)}
        self.attn = {l: torch.softmax(torch.randn(B, HEADS, N_TOK + 1, N_TOK + 1, generator=gen), dim=-1)
                     for l in self.teacher}
        head = torch.Generator().manual_seed(SEED + 1)
        self.logits = torch.randn(B, CLASSES, generator=head)
        self.targets = torch.randint(0, CLASSES, (B,), generator=head)
        # the oracle, with the state the module draws under torch.manual_seed(42)
        mod = self.module()
        sel = mod.layer_selector
        self.state = O.SelectorState(sel.proj_s.detach().cpu(), sel.proj_t.detach().cpu(),
                                     sel.log_temperatures.detach().cpu().clone().requires_grad_(True))
        with torch.no_grad():
            self.mixed, self.mixed_attn, _ = O.selector_forward(self.state, self.student, self.teacher, self.attn,
                                                                self.layers)
        self.ref_leaves = {k: v.clone().requires_grad_(True) for k, v in self.student.items()}
        self.ref, trace = O.basd_forward(self.state, torch.nn.CrossEntropyLoss(), self.layers, N_TOK, True,
                                         self.logits, self.targets, self.ref_leaves, self.teacher, self.attn)
        self.ref.backward()
        self.ranks = dict(trace.selector.ranks)
        self.d_grass_sq = np.stack([trace.selector.d_grass_sq[l].numpy() for l in self.layers])
        self.mix = np.stack([trace.selector.mix_weights[l].numpy() for l in self.layers])

    def module(self):
        from basd_amd.losses import BASDLoss
        torch.manual_seed(42)
        return BASDLoss(torch.nn.CrossEntropyLoss(), D_S, D_T, DEPTH, N_TOK,
                        config=SimpleNamespace(num_extraction_points=POINTS), teacher_has_cls_token=True).to(DEV)

    def on_device(self):
        move = lambda d: {k: v.to(DEV) for k, v in d.items()}
        return SimpleNamespace(logits=self.logits.to(DEV), targets=self.targets.to(DEV), student=move(self.student),
                               teacher=move(self.teacher), attn=move(self.attn))


@pytest.fixture(scope="module")
def case():
    c = _Case()
    # on the CPU, before anything of the library runs: the teacher ranks are the ones this file is about
    assert c.ranks == WANT_RANKS, c.ranks
    return c


def test_selector_and_loss_without_gradients(case):
    """Orders 100, 200 and 215 in one batch of principal-angle matrices, through the one-call selector tail."""
    mod = case.module()
    inp = case.on_device()
    with torch.no_grad():
        loss = mod(inp.logits, inp.targets, inp.student, inp.teacher, inp.attn)
    mod.layer_selector.finish_pending()
    torch.cuda.synchronize()
    assert dict(mod.layer_selector.subspace_ranks) == case.ranks
    d = mod.last_components["d_grass_sq"].cpu().numpy()
    mix = mod.last_components["mix"].cpu().numpy()
    print("d_grass_sq", d, "oracle", case.d_grass_sq)
    print("mix", mix, "oracle", case.mix)
    print("loss", loss.item(), "oracle", case.ref.item())
    np.testing.assert_allclose(d, case.d_grass_sq, rtol=2e-4)
    np.testing.assert_allclose(mix, case.mix, rtol=2e-4)
    np.testing.assert_allclose(loss.item(), case.ref.item(), rtol=1e-4)


def test_loss_and_gradients(case):
    """The same shape with a backward: [cos ; I] stacks of the common order 215 on the block path."""
    mod = case.module()
    inp = case.on_device()
    leaves = {k: v.requires_grad_(True) for k, v in inp.student.items()}
    loss = mod(inp.logits, inp.targets, leaves, inp.teacher, inp.attn)
    assert dict(mod.layer_selector.subspace_ranks) == case.ranks
    print("loss", loss.item(), "oracle", case.ref.item())
    np.testing.assert_allclose(loss.item(), case.ref.item(), rtol=1e-4)
    loss.backward()
    errs = {}
    for l in case.layers:
        want = case.ref_leaves[l].grad
        errs[l] = ((leaves[l].grad.cpu() - want).norm() / want.norm()).item()
    got_t = mod.layer_selector.log_temperatures.grad.cpu().numpy()
    print("student gradient errors", errs, "temperature gradients", got_t, "oracle",
          case.state.log_temperatures.grad.numpy())
    for l, err in errs.items():
        assert err < 2e-3, (l, err)
    np.testing.assert_allclose(got_t, case.state.log_temperatures.grad.numpy(), rtol=5e-3, atol=1e-7)


def test_selector_forward_api(case):
    """GrassmannianLayerSelector.forward: the materialised mix against the oracle's."""
    mod = case.module()
    inp = case.on_device()
    with torch.no_grad():
        mixed, mixed_attn = mod.layer_selector(inp.student, inp.teacher, inp.attn, case.layers)
    assert dict(mod.layer_selector.subspace_ranks) == case.ranks
    for l in case.layers:
        assert mixed[l].shape == case.mixed[l].shape and mixed_attn[l].shape == case.mixed_attn[l].shape
        np.testing.assert_allclose(mixed[l].cpu().numpy(), case.mixed[l].numpy(), rtol=2e-3, atol=2e-4)
        np.testing.assert_allclose(mixed_attn[l].cpu().numpy(), case.mixed_attn[l].numpy(), rtol=2e-3, atol=1e-6)


def test_an_order_out_of_range_is_named():
    """Past the longest column the solver has a kernel shape for, the exception names the order and the limit."""
    limit = ops.jacobi_max_order()
    n = limit + 6
    W = torch.zeros(1, n, n, device=DEV)
    n_arr = torch.tensor([n], dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match=rf"order {n}\b.*\b{limit}\b"):
        ops.jacobi_onesided(W, n, n_arr=n_arr)
    with pytest.raises(ValueError, match=rf"order {n}\b.*\b{limit}\b"):
        ops.check_angle_order(n)
    ops.check_angle_order(limit)
