"""Validation metrics (``basd_amd.evaluation``, kernel in ``csrc/eval.hip``) against a restatement written here with torch
ops on the CPU from the same logits: ranks and counts must agree exactly (bf16 logits are widened exactly, comparisons are
exact in any wider type), the mean loss must stay within ``4 * e32 + 1e-6 * |loss|`` of the fp64 restatement, where
``e32`` is the error of the same per-row formula evaluated in fp32 by torch on the CPU (rows averaged exactly, as the
kernel's fixed-point sum does).

``torchmetrics`` is not installed where this was written: the restatement below is the specification (ties go to the
lower class position), and nothing here compares against the package itself."""
import inspect
import math
import os
import socket
import sys
from types import SimpleNamespace

import pytest
import torch
import torch.nn as nn

from basd_amd.evaluation import EvalAccumulator, evaluate_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = 2.0 ** 32


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
def _restate(logits, targets, index=None, eps=0.0, top_k=5, dt=torch.float64):
    """Per row over the selected columns: loss = lse(z) - (1 - eps) z_y - eps / K sum z (row maximum subtracted),
    rank = #{z_j > z_y} + #{j < y: z_j == z_y}; a row with a label outside [0, K), a NaN or a loss that is not finite
    (or >= 2^24) is a miss at every k and is counted in ``bad``."""
    z = logits.detach().cpu().to(dt)
    if index is not None:
        z = z[:, list(index)]
    y = targets.detach().cpu()
    B, K = z.shape
    valid = (y >= 0) & (y < K)
    yc = y.clamp(0, K - 1)[:, None]
    zy = z.gather(1, yc)
    pos = torch.arange(K)[None, :]
    rank = ((z > zy) | ((z == zy) & (pos < yc))).sum(1)
    m = z.max(1, keepdim=True).values
    v = z - m
    loss = v.exp().sum(1).log() - (1.0 - eps) * (zy - m)[:, 0]
    if eps > 0.0:                                   # without smoothing a class masked with -inf costs nothing (0 * inf)
        loss = loss - eps / K * v.sum(1)
    bad = ~valid | z.isnan().any(1) | ~loss.isfinite() | (loss >= 2.0 ** 24)
    good = ~bad
    return SimpleNamespace(rows=B, hit1=int((good & (rank == 0)).sum()), hitk=int((good & (rank < top_k)).sum()),
                           bad=int(bad.sum()), loss_sum=float(loss[good].double().sum()), rank=rank, good=good, z=z)


def _counts(acc):
    return acc.state.tolist()[1:]


def _make_batch(B, C, K, index, dtype, seed):
    """Seeded logits with the target's column raised on half of the rows (so that hits and misses both occur)."""
    g = torch.Generator().manual_seed(seed)
    logits = 2.0 * torch.randn(B, C, generator=g)
    targets = torch.randint(0, K, (B,), generator=g)
    cols = targets if index is None else torch.tensor(list(index))[targets]
    lift = (torch.rand(B, generator=g) < 0.5).float() * 4.0
    logits[torch.arange(B), cols] += lift
    return logits.to(dtype), targets


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the interface, the boundary, the host arithmetic, the reduction over ranks
# ---------------------------------------------------------------------------------------------------------------------
def test_signature_is_the_reference_call():
    params = list(inspect.signature(evaluate_model).parameters.values())
    assert [p.name for p in params[:3]] == ["model", "data_loader", "criterion"]
    assert all(p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for p in params[:3])
    by_name = {p.name: p for p in params}
    assert by_name["num_classes"].kind is inspect.Parameter.KEYWORD_ONLY
    assert by_name["num_classes"].default is inspect.Parameter.empty
    assert by_name["valid_indices"].kind is inspect.Parameter.KEYWORD_ONLY and by_name["valid_indices"].default is None


def test_shim_path_is_the_same_object():
    from src.evaluation.metrics import evaluate_model as shim
    import basd_amd
    assert shim is evaluate_model
    assert "evaluation" in basd_amd.__doc__


def test_trainer_has_the_callback():
    from basd_amd.trainer import Trainer
    assert list(inspect.signature(Trainer.evaluate).parameters) == ["self", "model", "val_loader"]
    train = inspect.signature(Trainer.train).parameters
    assert train["evaluate"].default is None and train["val_loader"].default is None


def test_update_on_cpu_tensors_raises():
    acc = EvalAccumulator(10, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        acc.update(torch.randn(4, 10), torch.zeros(4, dtype=torch.long))
    assert acc.state.tolist() == [0, 0, 0, 0, 0]


def test_constructor_errors():
    with pytest.raises(ValueError):
        EvalAccumulator(4, device="cpu")                                   # top_k = 5 > K = 4
    with pytest.raises(ValueError):
        EvalAccumulator(1000, valid_indices=[3, 1, 2], device="cpu")       # K = 3
    with pytest.raises(ValueError):
        EvalAccumulator(10, top_k=0, device="cpu")
    acc = EvalAccumulator(1000, valid_indices=[7, 3, 999, 0, 1, 2], top_k=6, device="cpu")
    assert acc.K == 6 and acc.state.dtype == torch.int64 and acc.state.shape == (5,)
    assert acc._index.dtype == torch.int32 and acc._index.tolist() == [7, 3, 999, 0, 1, 2]
    assert EvalAccumulator(7, device="cpu").K == 7


def test_non_stock_criterion_raises():
    class Mine(nn.CrossEntropyLoss):
        pass

    model = nn.Linear(3, 10)
    for criterion in (nn.NLLLoss(), Mine(), nn.CrossEntropyLoss(reduction="sum"),
                      nn.CrossEntropyLoss(weight=torch.ones(10)), lambda a, b: a.sum()):
        with pytest.raises(TypeError):
            evaluate_model(model, [], criterion, num_classes=10)


def test_compute_on_a_hand_filled_state():
    acc = EvalAccumulator(10, device="cpu")
    out = acc.compute()                                                    # nothing seen
    assert set(out) == {"val_acc", "val_acc_top5", "loss"} and math.isnan(out["loss"])
    acc.state.copy_(torch.tensor([int(2.5 * UNIT) * 8, 8, 2, 6, 0]))
    out = acc.compute()
    assert out == {"val_acc": 25.0, "val_acc_top5": 75.0, "loss": 2.5}
    acc.state.copy_(torch.tensor([3 * int(UNIT) + 1, 3, 3, 3, 0]))         # one unit of 2^-32 is kept
    assert acc.compute()["loss"] == (3 * UNIT + 1) / UNIT / 3 and acc.compute()["val_acc"] == 100.0
    acc.state.copy_(torch.tensor([int(2.5 * UNIT) * 7, 8, 2, 6, 1]))       # one row could not be represented
    out = acc.compute()
    assert math.isnan(out["loss"]) and out["val_acc"] == 25.0 and out["val_acc_top5"] == 75.0
    acc.reset()
    assert acc.state.tolist() == [0, 0, 0, 0, 0] and math.isnan(acc.compute()["loss"])


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _reduce_worker(rank, world, port, out):
    sys.path.insert(0, os.path.join(ROOT, "vit-inductive-bias-distillation_amd"))
    import torch.distributed as dist
    from basd_amd.evaluation import EvalAccumulator as Acc
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        acc = Acc(10, device="cpu")
        # words past 2^53: a sum through floating point would lose the low bits
        acc.state.copy_(torch.tensor([(1 << 60) + 3 + rank, 100 + rank, 7 * (rank + 1), 50 + rank, rank]))
        acc.all_reduce()
        out[rank] = acc.state.tolist()
    finally:
        dist.destroy_process_group()


def test_all_reduce_sums_exactly_over_two_gloo_ranks():
    import torch.multiprocessing as mp
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    with ctx.Manager() as mgr:
        out = mgr.dict()
        procs = [ctx.Process(target=_reduce_worker, args=(r, world, port, out)) for r in range(world)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(120)
            assert p.exitcode == 0
        for r in range(world):
            assert out[r] == [(1 << 61) + 7, 201, 21, 101, 1], out[r]


# ---------------------------------------------------------------------------------------------------------------------
# GPU: through the C ABI
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _subset(seed=7, n=200, C=1000):
    return torch.randperm(C, generator=torch.Generator().manual_seed(seed))[:n].tolist()


CONFIGS = {"all-1000": (1000, None, 5), "subset-200": (1000, _subset(), 5), "seven": (7, None, 5)}


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_counts_are_exact(dev, dtype, config):
    C, index, top_k = CONFIGS[config]
    K = C if index is None else len(index)
    for B in (1, 3, 256, 257):
        logits, targets = _make_batch(B, C, K, index, dtype, seed=B)
        want = _restate(logits, targets, index, top_k=top_k)
        acc = EvalAccumulator(C, valid_indices=index, top_k=top_k, device=dev)
        acc.update(logits.to(dev), targets.to(dev))
        got = _counts(acc)
        print(f"[evaluation] {config} {dtype} B={B}: rows/top1/top{top_k}/bad {got}")
        assert got == [want.rows, want.hit1, want.hitk, want.bad] and want.bad == 0
        if B >= 256:
            assert 0 < want.hit1 < want.hitk < B                              # the case distinguishes something


def _tie_free_batch(B, C, K, index, dtype, seed):
    """Every row's K selected logits are a permutation of K distinct multiples of 1 / 16 (exact in bf16 for K <= 256);
    on half of the rows the target trades places with one of the row's ten largest."""
    g = torch.Generator().manual_seed(seed)
    order = torch.rand(B, K, generator=g).argsort(1)
    targets = torch.randint(0, K, (B,), generator=g)
    for b in range(0, B, 2):
        other = int((order[b] == K - 1 - int(torch.randint(0, min(10, K), (1,), generator=g))).nonzero())
        y = int(targets[b])
        order[b, y], order[b, other] = order[b, other].clone(), order[b, y].clone()
    z = (order.float() - K // 2) / 16.0
    logits = 3.0 * torch.randn(B, C, generator=g)
    logits[:, list(range(K)) if index is None else list(index)] = z
    return logits.to(dtype), targets


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,config", [(torch.float32, "all-1000"), (torch.float32, "subset-200"),
                                          (torch.float32, "seven"), (torch.bfloat16, "subset-200"),
                                          (torch.bfloat16, "seven")])
def test_counts_match_topk_on_tie_free_logits(dev, dtype, config):
    C, index, top_k = CONFIGS[config]
    K = C if index is None else len(index)
    for B in (3, 257):
        logits, targets = _tie_free_batch(B, C, K, index, dtype, seed=B)
        want = _restate(logits, targets, index, top_k=top_k)
        assert all(row.unique().numel() == K for row in want.z)               # widened exactly, still distinct
        top = want.z.topk(top_k, dim=1).indices
        top1, topk = int((top[:, 0] == targets).sum()), int((top == targets[:, None]).any(1).sum())
        assert [want.hit1, want.hitk] == [top1, topk] and (B < 257 or 0 < top1 < topk < B)
        acc = EvalAccumulator(C, valid_indices=index, top_k=top_k, device=dev)
        acc.update(logits.to(dev), targets.to(dev))
        assert _counts(acc) == [B, top1, topk, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_strided_view_is_read_in_place(dev, dtype):
    for B, offset in ((257, 0), (64, 1)):                                     # offset 1: no row starts on 16 bytes
        g = torch.Generator().manual_seed(11 + offset)
        wide = (2.0 * torch.randn(B, 1024 + offset, generator=g)).to(dtype)
        wide[:, 1000 + offset:] = 50.0                                        # would win every row if it were read
        targets = torch.randint(0, 1000, (B,), generator=g)
        wide[torch.arange(0, B, 2), targets[::2] + offset] += 5.0
        view = wide.to(dev)[:, offset:1000 + offset]
        assert view.stride() == (1024 + offset, 1)
        want = _restate(wide[:, offset:1000 + offset], targets, eps=0.1)
        acc = EvalAccumulator(1000, label_smoothing=0.1, device=dev)
        acc.update(view, targets.to(dev))
        assert _counts(acc) == [B, want.hit1, want.hitk, 0] and want.hit1 > 0
        assert abs(acc.compute()["loss"] - want.loss_sum / B) <= 1e-5 * want.loss_sum / B


@pytest.mark.gpu
def test_update_boundary_errors(dev):
    acc = EvalAccumulator(10, device=dev)
    y = torch.zeros(4, dtype=torch.long, device=dev)
    with pytest.raises(ValueError):
        acc.update(torch.randn(4, 12, device=dev), y)                         # C != num_classes
    with pytest.raises(ValueError):
        acc.update(torch.randn(10, 4, device=dev).t(), y)                     # column stride
    with pytest.raises(ValueError):
        acc.update(torch.randn(4, 10, 1, device=dev), y)
    with pytest.raises(ValueError):
        acc.update(torch.randn(4, 10, device=dev), y[:3])
    with pytest.raises(TypeError):
        acc.update(torch.randn(4, 10, device=dev).half(), y)
    with pytest.raises(RuntimeError):
        acc.update(torch.randn(4, 10), y)
    sub = EvalAccumulator(10, valid_indices=[0, 2, 4, 6, 8, 11], device=dev)
    with pytest.raises(ValueError):
        sub.update(torch.randn(4, 10, device=dev), y)                         # index 11 of 10 columns
    sub.update(torch.randn(4, 12, device=dev), y)
    acc.update(torch.randn(0, 10, device=dev), y[:0])                         # B = 0: nothing happens
    assert acc.state.tolist() == [0, 0, 0, 0, 0] and sub.state.tolist()[1] == 4


@pytest.mark.gpu
def test_ties_nan_and_labels_out_of_range(dev):
    nan, inf = float("nan"), float("inf")
    rows = [
        ([1, 2, 9, 3, 4, 9, 0, 0], 2),        # the maximum twice, target is the first of the two: rank 0
        ([1, 2, 9, 3, 4, 9, 0, 0], 5),        # ... the second: rank 1, a top-1 miss
        ([9, 8, 7, 6, 5, 5, 0, 0], 4),        # ties for 5th place and comes first: rank 4, a top-5 hit
        ([9, 8, 7, 6, 5, 5, 0, 0], 5),        # ties for 5th place and comes second: rank 5, a top-5 miss
        ([9, 1, 2, nan, 0, 0, 0, 0], 0),      # a NaN anywhere in the row
        ([9, 1, 2, 3, 0, 0, 0, 0], 8),        # label == K
        ([9, 1, 2, 3, 0, 0, 0, 0], -1),       # label < 0
        ([9, -inf, 2, 3, 0, 0, 0, 0], 1),     # target logit -inf: the loss is +inf
    ]
    for dtype in (torch.float32, torch.bfloat16):
        logits = torch.tensor([r for r, _ in rows], dtype=torch.float32).to(dtype)
        targets = torch.tensor([y for _, y in rows])
        want = _restate(logits, targets)
        assert want.rank[:4].tolist() == [0, 1, 4, 5]
        assert [want.rows, want.hit1, want.hitk, want.bad] == [8, 1, 3, 4]     # the restatement says what is written above
        acc = EvalAccumulator(8, device=dev)
        acc.update(logits.to(dev), targets.to(dev))
        state = acc.state.tolist()
        assert state[1:] == [8, 1, 3, 4], state
        assert abs(state[0] / UNIT - want.loss_sum) <= 1e-5 * want.loss_sum    # the four good rows only
        out = acc.compute()
        assert math.isnan(out["loss"]) and out["val_acc"] == 12.5 and out["val_acc_top5"] == 37.5
    # with a class table the tie is broken by the position in the table, not by the column
    logits = torch.tensor([[0.0, 5.0, 1.0, 5.0]] * 2)
    targets = torch.tensor([1, 0])                     # table [3, 1]: z = [x3, x1] = [5, 5]
    want = _restate(logits, targets, [3, 1], top_k=1)
    assert want.rank.tolist() == [1, 0]
    acc = EvalAccumulator(4, valid_indices=[3, 1], top_k=1, device=dev)
    acc.update(logits.to(dev), targets.to(dev))
    assert _counts(acc) == [2, 1, 1, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_loss_against_fp64(dev, dtype, eps):
    for config, (C, index, top_k) in CONFIGS.items():
        K = C if index is None else len(index)
        logits, targets = _make_batch(256, C, K, index, dtype, seed=99)
        ref64 = _restate(logits, targets, index, eps=eps, top_k=top_k)
        ref32 = _restate(logits, targets, index, eps=eps, top_k=top_k, dt=torch.float32)
        want, e32 = ref64.loss_sum / 256, abs(ref32.loss_sum - ref64.loss_sum) / 256
        acc = EvalAccumulator(C, valid_indices=index, label_smoothing=eps, top_k=top_k, device=dev)
        acc.update(logits.to(dev), targets.to(dev))
        got = acc.compute()["loss"]
        err, bound = abs(got - want), 4.0 * e32 + 1e-6 * abs(want)
        print(f"[evaluation] loss {config} {dtype} eps={eps}: kernel {got:.9f} fp64 {want:.9f} err {err:.3e} "
              f"e32 {e32:.3e} ratio {err / max(e32, 1e-300):.3f} bound {bound:.3e}")
        assert err <= bound, (config, got, want, err, e32, bound)
        # the same number as torch's criterion on the gathered logits (its own fp32 evaluation: 1e-5 relative)
        z = logits.float() if index is None else logits.float()[:, index]
        torch_loss = float(nn.functional.cross_entropy(z, targets, label_smoothing=eps))
        assert abs(got - torch_loss) <= 1e-5 * abs(torch_loss), (got, torch_loss)


@pytest.mark.gpu
def test_accumulation_is_exact_and_deterministic(dev):
    index = _subset()
    sizes = (5, 130, 67)
    logits, targets = _make_batch(sum(sizes), 1000, 200, index, torch.float32, seed=5)
    logits, targets = logits.to(dev), targets.to(dev)

    def run(pieces):
        acc = EvalAccumulator(1000, valid_indices=index, label_smoothing=0.1, device=dev)
        start = 0
        for n in pieces:
            acc.update(logits[start:start + n], targets[start:start + n])
            start += n
        return acc.state.clone()

    whole, parts, again = run((sum(sizes),)), run(sizes), run(sizes)
    assert whole[1] == sum(sizes) and whole[0] > 0
    assert torch.equal(parts, whole), (parts.tolist(), whole.tolist())
    assert torch.equal(again, parts)
    for _ in range(5):
        assert torch.equal(run((sum(sizes),)), whole)


@pytest.mark.gpu
def test_one_launch_and_nothing_else_per_update(dev):
    """A steady-state ``update`` is one kernel launch: no memcpy, no memset, no allocation.  Counted with
    ``torch.profiler`` where it sees launches made through ctypes (the output says whether it does); the allocator's
    counters and the accumulated row count are checked either way."""
    from torch.profiler import ProfilerActivity, profile
    index = _subset()
    logits, targets = _make_batch(256, 1000, 200, index, torch.bfloat16, seed=3)
    logits, targets = logits.to(dev), targets.to(dev)
    acc = EvalAccumulator(1000, valid_indices=index, label_smoothing=0.1, device=dev)
    for _ in range(3):
        acc.update(logits, targets)
    torch.cuda.synchronize()
    allocations = torch.cuda.memory_stats(dev)["allocation.all.allocated"]
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(20):
            acc.update(logits, targets)
        torch.cuda.synchronize()
    assert torch.cuda.memory_stats(dev)["allocation.all.allocated"] == allocations
    assert acc.state.tolist()[1] == 23 * 256
    device_events = [e for e in prof.events() if "cuda" in str(e.device_type).lower()]
    host_names = {e.name for e in prof.events() if "cuda" not in str(e.device_type).lower()}
    others = [e for e in prof.events() if "memcpy" in e.name.lower() or "memset" in e.name.lower()]
    kernels = [e for e in device_events if e.name not in host_names and e not in others]
    ours = [e for e in kernels if "eval_batch_kernel" in e.name]
    if ours:
        print(f"[evaluation] profiler: {len(kernels)} kernels ({len(ours)} eval_batch_kernel), {len(others)} memcpy / "
              "memset in 20 updates")
        assert len(ours) == 20 and len(kernels) == 20, sorted({e.name for e in kernels})
        assert not others, sorted({e.name for e in others})
    else:
        print("[evaluation] the profiler does not see the ctypes launches here "
              f"({len(kernels)} device kernels, {len(others)} memcpy / memset events seen by it)")
        assert not kernels and not others


# ---------------------------------------------------------------------------------------------------------------------
# GPU: end to end
# ---------------------------------------------------------------------------------------------------------------------
def _images(B, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 3, 1, 1, generator=g) * 2.0 + torch.randn(B, 3, 32, 32, generator=g)


def _val_loader(n_batches, classes=10, B=24):
    return [{"pixel_values": _images(B + i, 200 + i), "label": (torch.arange(B + i) * 3 + i) % classes}
            for i in range(n_batches)]


@pytest.mark.gpu
@pytest.mark.parametrize("subset", [None, [9, 0, 4, 2, 7, 5]], ids=["all", "subset"])
def test_evaluate_model_against_the_restatement(dev, subset):
    from tools import stock_models as SM
    torch.manual_seed(3)
    model = SM.StockViT(img_size=32, patch_size=8, embed_dim=48, depth=6, num_heads=4, num_classes=10).to(dev)
    model.train()
    K = 10 if subset is None else len(subset)
    loader = _val_loader(3, classes=K)
    criterion = nn.CrossEntropyLoss(label_smoothing=0.1)
    out = evaluate_model(model, loader, criterion, num_classes=K if subset else 10, valid_indices=subset)
    assert not model.training and set(out) == {"val_acc", "val_acc_top5", "loss"}
    with torch.no_grad():
        logits = torch.cat([model(b["pixel_values"].to(dev)) for b in loader]).cpu()
    targets = torch.cat([b["label"] for b in loader])
    ref64 = _restate(logits, targets, subset, eps=0.1)
    ref32 = _restate(logits, targets, subset, eps=0.1, dt=torch.float32)
    n = targets.numel()
    assert n == 24 + 25 + 26 and ref64.bad == 0
    assert out["val_acc"] == 100.0 * ref64.hit1 / n and out["val_acc_top5"] == 100.0 * ref64.hitk / n
    want, e32 = ref64.loss_sum / n, abs(ref32.loss_sum - ref64.loss_sum) / n
    print(f"[evaluation] evaluate_model {out} fp64 loss {want:.9f} e32 {e32:.3e}")
    assert abs(out["loss"] - want) <= 4.0 * e32 + 1e-6 * want
    gathered = logits if subset is None else logits[:, subset]
    assert abs(out["loss"] - float(criterion(gathered, targets))) <= 1e-5 * want


@pytest.mark.gpu
def test_trainer_validates_with_its_own_evaluate(dev):
    from basd_amd import trainer as T
    from basd_amd.optim import AdamWScheduleFree
    from tools import stock_models as SM
    torch.manual_seed(3)
    student = SM.StockViT(img_size=32, patch_size=8, embed_dim=48, depth=6, num_heads=4, num_classes=10).to(dev)
    teacher = SM.make_teacher(SM.StockViT(img_size=32, patch_size=8, embed_dim=64, depth=3, num_heads=4,
                                          num_classes=0).to(dev), 32)
    cfg = SimpleNamespace(training=SimpleNamespace(label_smoothing=0.1, learning_rate=1e-3, weight_decay=0.05,
                                                   num_epochs=2),
                          basd=SimpleNamespace(num_extraction_points=4), model=SimpleNamespace(num_classes=10))
    torch.manual_seed(42)
    tr = T.Trainer(student, cfg, teacher, student_info=SM.probe_model(student, 32), mixup=False,
                   optimizer="schedulefree")
    assert isinstance(tr.optimizer, AdamWScheduleFree)
    train = [{"clean": _images(16, 10 + i), "augmented": _images(16, 50 + i), "label": (torch.arange(16) + i) % 10}
             for i in range(3)]
    val = _val_loader(2)
    history = tr.train(train, val, evaluate=tr.evaluate)
    print("[evaluation] trainer history:", dict(history))
    for key in ("val_acc", "val_acc_top5", "loss", "train_loss", "train_acc"):
        assert len(history[key]) == 2 and all(math.isfinite(v) for v in history[key]), key
    assert all(0.0 <= a <= t <= 100.0 for a, t in zip(history["val_acc"], history["val_acc_top5"]))
    assert all(v > 0.0 for v in history["loss"])
    assert tr.best_val_acc == max(history["val_acc"]) > 0.0
    assert all(g["train_mode"] for g in tr.optimizer.param_groups)            # back on the y sequence after validation
    # the last epoch's figures are those of a fresh call on the averaged weights the validation saw
    tr.optimizer.eval()
    again = evaluate_model(student, val, tr.criterion, num_classes=10)
    tr.optimizer.train()
    # (y -> x -> y -> x rounds the weights twice more: a logit may move in its last bits, so allow one sample)
    one = 100.0 / sum(b["label"].numel() for b in val) + 1e-9
    assert abs(again["val_acc"] - history["val_acc"][-1]) <= one
    assert abs(again["val_acc_top5"] - history["val_acc_top5"][-1]) <= one
    assert abs(again["loss"] - history["loss"][-1]) <= 1e-5 * again["loss"]
