"""``basd_amd.prefetch``: the input work of the next batch on a side stream while the step runs.

CPU: the scheduling of ``DevicePrefetcher`` (what has been prepared and how far the loader has been advanced when an
item arrives, where an exception arrives, a dropped iteration), and ``Trainer`` with the oracle as the loss: the split of
``train_step`` and whole epochs at ``prefetch`` 1 and 2 against 0, bit for bit.  GPU: the full input chain (JPEG decode,
resize and crop, TrivialAugment, fused mixing) prepares the same bytes at every depth, the consumer reading each item
on its own stream without a host wait; lifetime of held batches; which stream ``prepare`` runs on; launch, copy and
synchronise counts; serial and prefetched use of one set of stage objects; three trainer steps; validation.
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "jpeg_decode.npz")
KEYS = ("clean", "augmented", "targets", "mixed_targets")


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the scheduling
# ---------------------------------------------------------------------------------------------------------------------
class _Loader:
    """``n`` items ``0 .. n-1``; ``advanced``: how many it has handed out; raises ``error`` when asked for ``fail_at``."""

    def __init__(self, n, fail_at=None, error=None):
        self.n, self.fail_at, self.error, self.advanced = n, fail_at, error, 0

    def __iter__(self):
        for i in range(self.n):
            if i == self.fail_at:
                raise self.error
            self.advanced += 1
            yield i


class _Prepare:
    """Records the items it was called for; an item becomes ``{"item": i, "payload": [tensor, (tensor, i)]}``."""

    def __init__(self, fail_at=None, error=None):
        self.fail_at, self.error, self.seen = fail_at, error, []

    def __call__(self, i):
        self.seen.append(i)
        if i == self.fail_at:
            raise self.error
        return {"item": i, "payload": [torch.full((3,), float(i)), (torch.full((2,), float(-i)), i)]}


def _check_item(got, i):
    assert got["item"] == i and got["payload"][1][1] == i
    assert torch.equal(got["payload"][0], torch.full((3,), float(i)))
    assert torch.equal(got["payload"][1][0], torch.full((2,), float(-i)))


@pytest.mark.parametrize("depth", [0, 1, 2, 5])
@pytest.mark.parametrize("n", [0, 1, 2, 3, 7])
def test_items_arrive_in_order_with_exactly_depth_items_of_lookahead(n, depth):
    from basd_amd.prefetch import DevicePrefetcher
    prepare, loader = _Prepare(), _Loader(n)
    pf = DevicePrefetcher(prepare, device="cpu", depth=depth)
    assert pf.stream is None and pf.depth == depth
    arrived = 0
    for k, got in enumerate(pf.iterate(loader)):
        _check_item(got, k)
        ahead = min(k + depth, n - 1)
        assert prepare.seen == list(range(ahead + 1)), (k, prepare.seen)
        assert loader.advanced == ahead + 1, (k, loader.advanced)
        arrived += 1
    assert arrived == n and prepare.seen == list(range(n)) and loader.advanced == n


@pytest.mark.parametrize("depth", [0, 1, 2, 5])
@pytest.mark.parametrize("where", ["prepare", "loader"])
def test_an_exception_arrives_when_its_item_is_due(where, depth):
    from basd_amd.prefetch import DevicePrefetcher
    n = 7
    for j in range(n):
        error = KeyError(f"item {j}")
        prepare = _Prepare(j, error) if where == "prepare" else _Prepare()
        loader = _Loader(n, j, error) if where == "loader" else _Loader(n)
        pf = DevicePrefetcher(prepare, device="cpu", depth=depth)
        delivered = []
        with pytest.raises(KeyError) as caught:
            for got in pf.iterate(loader):
                _check_item(got, len(delivered))
                delivered.append(got["item"])
        assert caught.value is error
        assert delivered == list(range(j)), (j, delivered)
        # nothing behind the failing item was asked for or prepared
        assert loader.advanced == (j + 1 if where == "prepare" else j)
        assert prepare.seen == list(range(j + 1 if where == "prepare" else j))
        # nothing is pending: the same object starts clean
        pf.prepare = again = _Prepare()
        assert [g["item"] for g in pf.iterate(_Loader(3))] == [0, 1, 2] and again.seen == [0, 1, 2]


@pytest.mark.parametrize("depth", [0, 1, 2, 5])
def test_a_second_iteration_after_a_break_starts_clean(depth):
    from basd_amd.prefetch import DevicePrefetcher
    prepare, loader = _Prepare(), _Loader(7)
    pf = DevicePrefetcher(prepare, device="cpu", depth=depth)
    for got in pf.iterate(loader):
        if got["item"] == 1:
            break
    assert loader.advanced == min(1 + depth, 6) + 1
    gen = pf.iterate(_Loader(7))
    next(gen)
    gen.close()                                              # an explicit close ends an iteration too
    pf.prepare = prepare = _Prepare()
    fresh = _Loader(4)
    for k, got in enumerate(pf.iterate(fresh)):
        _check_item(got, k)
        assert prepare.seen == list(range(min(k + depth, 3) + 1)) and fresh.advanced == len(prepare.seen)
    assert prepare.seen == [0, 1, 2, 3]


@pytest.mark.parametrize("depth", [-1, 1.5, True])
def test_depth_must_be_a_non_negative_int(depth):
    import basd_amd
    from basd_amd.prefetch import DevicePrefetcher
    assert basd_amd.DevicePrefetcher is DevicePrefetcher and "DevicePrefetcher" in basd_amd.__all__
    with pytest.raises(ValueError, match="depth must be an int >= 0"):
        DevicePrefetcher(lambda b: b, device="cpu", depth=depth)


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the trainer
# ---------------------------------------------------------------------------------------------------------------------
def _config(points=4, classes=10, img_size=32, crop_ratio=0.875):
    return SimpleNamespace(training=SimpleNamespace(label_smoothing=0.1, learning_rate=1e-3, weight_decay=0.05),
                           basd=SimpleNamespace(num_extraction_points=points),
                           model=SimpleNamespace(num_classes=classes, vit=SimpleNamespace(img_size=img_size)),
                           data=SimpleNamespace(eval_crop_ratio=crop_ratio))


class OracleBASD(nn.Module):
    """The oracle behind the reference constructor's signature (test-side stand-in for the loss module on CPU)."""

    def __init__(self, base_criterion, student_dim, teacher_dim, student_depth, num_student_tokens, *, config,
                 teacher_has_cls_token):
        super().__init__()
        from oracle import basd_oracle as O
        self.O = O
        self.base_criterion, self.has_cls, self.n_s = base_criterion, teacher_has_cls_token, num_student_tokens
        self.token_layers = O.extraction_layers(student_depth, config.num_extraction_points)
        st = O.SelectorState.create(len(self.token_layers), student_dim, teacher_dim)
        self.register_buffer("proj_s", st.proj_s)
        self.register_buffer("proj_t", st.proj_t)
        self.log_temperatures = nn.Parameter(st.log_temperatures.detach().clone())

    def forward(self, logits, targets, s_tokens, t_tokens, t_attns):
        st = self.O.SelectorState(self.proj_s, self.proj_t, self.log_temperatures)
        t_attns = {k: v.contiguous() for k, v in t_attns.items()}
        return self.O.basd_forward(st, self.base_criterion, self.token_layers, self.n_s, self.has_cls, logits, targets,
                                   {k: v.float() for k, v in s_tokens.items()},
                                   {k: v.float() for k, v in t_tokens.items()}, t_attns)[0]


def _structured_images(B, size, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 3, 1, 1, generator=g) * 2.0 + torch.randn(B, 3, size, size, generator=g)


def _cpu_trainer(**kw):
    """Equal states: the models from one seed, the loss module from another."""
    from basd_amd import trainer as T
    from tools import stock_models as SM
    torch.manual_seed(3)
    student = SM.StockViT(img_size=32, patch_size=8, embed_dim=48, depth=6, num_heads=4, num_classes=10)
    teacher = SM.make_teacher(SM.StockResNet(layers=(1, 1, 1, 1), bottleneck=False, width=16), 32)
    torch.manual_seed(42)
    return T.Trainer(student, _config(), teacher, student_info=SM.probe_model(student, 32), loss_cls=OracleBASD, **kw)


def _cpu_batches(n, B=8):
    return [{"clean": _structured_images(B, 32, 10 + i), "augmented": _structured_images(B, 32, 20 + i),
             "label": (torch.arange(B) + i) % 10} for i in range(n)]


def _same_parameters(a, b):
    pa = list(a.model.parameters()) + list(a.basd_loss.parameters())
    pb = list(b.model.parameters()) + list(b.basd_loss.parameters())
    return len(pa) == len(pb) and all(torch.equal(x, y) for x, y in zip(pa, pb))


def test_train_step_is_step_prepared_of_prepare_batch():
    whole, split = _cpu_trainer(), _cpu_trainer()
    assert _same_parameters(whole, split)
    for batch in _cpu_batches(2):
        torch.manual_seed(5)
        a = whole.train_step(batch)
        torch.manual_seed(5)
        prepared = split.prepare_batch(batch)
        assert set(prepared) == set(KEYS) and prepared["mixed_targets"].shape == (8, 10)
        b = split.step_prepared(prepared)
        assert set(a) == set(b) and a["n"] == b["n"] == 8
        assert torch.equal(a["loss"], b["loss"]) and torch.equal(a["correct"], b["correct"])
    assert _same_parameters(whole, split)


@pytest.mark.parametrize("prefetch", [1, 2])
def test_a_prefetched_epoch_on_the_cpu_equals_the_serial_one(prefetch):
    batches = _cpu_batches(4)
    serial, ahead = _cpu_trainer(mixup=True), _cpu_trainer(mixup=True, prefetch=prefetch)
    assert serial.prefetch == 0 and ahead.prefetch == prefetch and ahead._prefetcher.depth == prefetch
    torch.manual_seed(9)
    want = serial._train_epoch(batches)
    torch.manual_seed(9)
    got = ahead._train_epoch(batches)
    assert got == want and np.isfinite(want["train_loss"])
    assert _same_parameters(serial, ahead)


@pytest.mark.parametrize("prefetch", [-1, 1.5, True, "1"])
def test_prefetch_must_be_a_non_negative_int(prefetch):
    with pytest.raises(ValueError, match="prefetch must be an int >= 0"):
        _cpu_trainer(prefetch=prefetch)


@pytest.mark.parametrize("prefetch", [0, 1, 2])
def test_a_bad_batch_raises_the_serial_error_after_the_steps_before_it(prefetch):
    good = _cpu_batches(3)
    bad = dict(good[1], augmented=torch.zeros(8, 3, 32, 32, dtype=torch.uint8))
    with pytest.raises(TypeError) as serial:
        _cpu_trainer().train_step(bad)
    tr = _cpu_trainer(prefetch=prefetch)
    steps = []
    plain_step = tr.optimizer.step
    tr.optimizer.step = lambda *a, **k: (steps.append(1), plain_step(*a, **k))[1]
    with pytest.raises(TypeError) as caught:
        tr._train_epoch([good[0], bad, good[2]])
    assert str(caught.value) == str(serial.value) and "uint8 batches need mixup='fused' and image_stats" in str(caught.value)
    assert len(steps) == 1


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
STATS = {"clean": ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5)), "augmented": (MEAN, STD)}
# 14 recorded streams as batches of 4, 4, 4 and 2: every sampling, with and without restart markers; the largest
# pictures sit in the second and the last batch, so the record tables and the decoder's workspace grow mid-epoch
STREAMS = (("gray_17x9_q75_rst1", "444_33x17_q75_plain", "422_31x33_q75_rstrow", "420_33x31_q75_rst2"),
           ("420_64x96_q100_noise", "gray_17x9_q75_plain", "444_33x17_q75_rst2", "422_16x16_q75_noise"),
           ("422_31x33_q75_plain", "420_33x33_q1_noise", "444_33x17_q75_rstrow", "420_33x31_q75_plain"),
           ("444_72x72_q75_81segments", "420_9x33_q75_ramp"))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def batches(dev):
    """The four pinned batches of files' bytes with their labels."""
    from basd_amd.jpeg import pack_jpegs
    g = np.load(GOLDEN, allow_pickle=False)
    out, at = [], 0
    for names in STREAMS:
        files = [g[f"stream_{n}"].tobytes() for n in names]
        out.append({"images": pack_jpegs(files).pin_memory(), "label": (torch.arange(len(files)) + at) % 10})
        at += len(files)
    assert [len(b["images"]) for b in out] == [4, 4, 4, 2]
    return out


def _gpu_trainer(dev, *, jpeg_decode=True, prefetch=0):
    from basd_amd import trainer as T
    from tools import stock_models as SM
    torch.manual_seed(3)
    student = SM.StockViT(img_size=16, patch_size=4, embed_dim=48, depth=6, num_heads=4, num_classes=10).to(dev)
    teacher = SM.make_teacher(SM.StockViT(img_size=16, patch_size=4, embed_dim=64, depth=3, num_heads=4,
                                          num_classes=0).to(dev), 16)
    torch.manual_seed(42)
    return T.Trainer(student, _config(img_size=16), teacher, student_info=SM.probe_model(student, 16), mixup="fused",
                     image_stats=STATS, resize_crop=True, trivial_augment=True, jpeg_decode=jpeg_decode,
                     prefetch=prefetch)


def _copy(prepared):
    """Copies on the current stream, queued the moment the item arrives; no host wait."""
    return {k: prepared[k].clone() for k in KEYS}


def _as_bytes(copies):
    return [{k: c[k].cpu().contiguous().view(torch.uint8).numpy().tobytes() for k in KEYS} for c in copies]


def _prepared_epoch(tr, batches, seed, keep=None):
    torch.manual_seed(seed)
    copies = []
    for prepared in tr._prefetcher.iterate(batches):
        copies.append(_copy(prepared))
        if keep is not None:
            keep.append(prepared)
    return copies


@pytest.fixture(scope="module")
def serial_bytes(dev, batches):
    """entropy -> the bytes the serial path prepares from the four batches under seed 11: computed once."""
    out = {}
    for jpeg_decode in (True, "parallel"):
        tr = _gpu_trainer(dev, jpeg_decode=jpeg_decode)
        copies = _prepared_epoch(tr, batches, 11)
        torch.cuda.synchronize()
        assert tr._decoder.status() == 0 and tr._resizer.status() == 0
        out[jpeg_decode] = _as_bytes(copies)
        assert [len(b["targets"]) // 8 for b in out[jpeg_decode]] == [4, 4, 4, 2]
    assert out[True] == out["parallel"]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("jpeg_decode", [True, "parallel"])
def test_prepared_batches_are_the_same_bytes_at_every_depth(dev, batches, serial_bytes, jpeg_decode):
    """The full chain under one seed at ``prefetch`` 0, 1 and 2.  The consumer copies each tensor on its own stream as
    soon as it arrives; the one synchronise comes after all three epochs."""
    trainers = [_gpu_trainer(dev, jpeg_decode=jpeg_decode, prefetch=p) for p in (2, 1, 0)]
    assert trainers[0]._prefetcher.stream is not None and trainers[2]._prefetcher.stream is None
    consumer = torch.cuda.Stream(device=dev)                 # not the default stream: the wait has to name the right one
    consumer.wait_stream(torch.cuda.current_stream(dev))
    copies = []
    with torch.cuda.stream(consumer):
        for tr in trainers:
            # an epoch of other draws first, so that what the memory still holds is not the answer; then the consumer's
            # stream is kept busy for some milliseconds when the epoch starts: the side stream waits for it, and a copy
            # that is not ordered behind its batch would run before the batch is made
            _prepared_epoch(tr, batches, 13)
            torch.cuda._sleep(20_000_000)
            copies.append(_prepared_epoch(tr, batches, 11))
    torch.cuda.synchronize()
    for tr, got in zip(trainers, copies):
        assert _as_bytes(got) == serial_bytes[jpeg_decode], tr.prefetch
        assert tr._decoder.status() == 0 and tr._resizer.status() == 0 and tr._augmenter.status() == 0


@pytest.mark.gpu
def test_held_batches_keep_their_bytes_and_their_memory(dev, batches, serial_bytes):
    tr = _gpu_trainer(dev, prefetch=2)
    held = []
    _prepared_epoch(tr, batches, 11, keep=held)
    # more work for the allocator while the four are alive
    _prepared_epoch(tr, batches, 12)
    torch.cuda.synchronize()
    assert len(held) == 4 and _as_bytes(held) == serial_bytes[True]
    spans = [(t.data_ptr(), t.data_ptr() + t.numel() * t.element_size(), i, k)
             for i, p in enumerate(held) for k, t in p.items() if k in KEYS]
    for a in spans:
        for b in spans:
            if a is not b:
                assert a[1] <= b[0] or b[1] <= a[0], (a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("priority", ["default", "lowest"])
def test_prepare_runs_on_the_side_stream_and_nowhere_else(dev, batches, serial_bytes, priority):
    from basd_amd.prefetch import DevicePrefetcher
    tr = _gpu_trainer(dev)
    seen = []

    def spy(batch):
        seen.append(torch.cuda.current_stream(dev))
        return tr.prepare_batch(batch)

    consumer = torch.cuda.current_stream(dev)
    results = {}
    for depth in (1, 2, 0):
        pf = DevicePrefetcher(spy, device=dev, depth=depth, priority=priority)
        del seen[:]
        torch.manual_seed(11)
        results[depth] = [_copy(p) for p in pf.iterate(batches)]
        assert len(seen) == 4
        if depth:
            assert pf.stream is not None and pf.stream != consumer
            assert all(s == pf.stream for s in seen), depth
            second = [s for s in seen]
            del seen[:]
            torch.manual_seed(11)
            for _ in pf.iterate(batches):                    # the stream is the object's: the same one again
                pass
            assert seen == second
        else:
            assert pf.stream is None and all(s == consumer for s in seen)
    torch.cuda.synchronize()
    for depth, got in results.items():
        assert _as_bytes(got) == serial_bytes[True], depth
    with pytest.raises(ValueError, match="priority must be one of"):
        DevicePrefetcher(spy, device=dev, depth=1, priority="highest")


def _profile_counts(tr, batches):
    """Kernels, copies and synchronise calls of three steady-state batches (the epoch before them warms every table up)."""
    from torch.profiler import ProfilerActivity, profile
    for _ in range(2):
        for _ in tr._prefetcher.iterate(batches[:3]):
            pass
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in tr._prefetcher.iterate(batches[:3]):
            pass
        torch.cuda.synchronize()
    events = list(prof.events())
    device_events = [e for e in events if "cuda" in str(e.device_type).lower()]
    host_names = [e.name for e in events if "cuda" not in str(e.device_type).lower()]
    copies = [e for e in device_events if "memcpy" in e.name.lower()]
    memsets = [e for e in device_events if "memset" in e.name.lower()]
    kernels = [e for e in device_events if e.name not in set(host_names) and e not in copies and e not in memsets]
    syncs = {name: host_names.count(name) for name in set(host_names)
             if "streamsynchronize" in name.lower() or "devicesynchronize" in name.lower()}
    return len(kernels), len(copies), len(memsets), syncs


@pytest.mark.gpu
def test_launches_copies_and_synchronises_do_not_grow_with_prefetch(dev, batches):
    """Counted with ``torch.profiler`` where it sees launches made through ctypes (the output says what it saw)."""
    torch.manual_seed(11)
    k0, c0, m0, s0 = _profile_counts(_gpu_trainer(dev, prefetch=0), batches)
    torch.manual_seed(11)
    k1, c1, m1, s1 = _profile_counts(_gpu_trainer(dev, prefetch=1), batches)
    print(f"[input_prefetch] profiler, three batches: depth 0: {k0} kernels, {c0} copies, {m0} memsets, syncs {s0}; "
          f"depth 1: {k1} kernels, {c1} copies, {m1} memsets, syncs {s1}")
    assert (k1, c1, m1) == (k0, c0, m0)
    for name, count in s1.items():
        assert count <= s0.get(name, 0), (name, s1, s0)


def _val_batches(batches):
    return [{"images": b["images"], "label": b["label"]} for b in batches]


@pytest.mark.gpu
def test_serial_and_prefetched_use_of_one_set_of_stage_objects(dev, batches):
    """A serial ``train_step``, a prefetched two-batch epoch and a serial ``evaluate`` on one trainer, no synchronise in
    between: every prepared input equals the all-serial run's."""
    def run(prefetch):
        tr = _gpu_trainer(dev, prefetch=prefetch)
        seen = []
        plain = tr.prepare_batch

        def spy(batch):
            prepared = plain(batch)
            seen.append(_copy(prepared))                     # on the stream the batch was prepared on
            return prepared

        tr.prepare_batch = tr._prefetcher.prepare = spy
        fed = []
        hook = tr.model.register_forward_pre_hook(lambda m, args: fed.append(args[0].clone()) if not m.training else None)
        torch.manual_seed(11)
        tr.model.train()
        tr.train_step(batches[0])
        tr._train_epoch(batches[1:3])
        tr.model.eval()
        serial_eval, tr.prefetch = tr.prefetch, 0            # the serial evaluate of the issue
        metrics = tr.evaluate(tr.model, _val_batches(batches))
        tr.prefetch = serial_eval
        tr.model.train()
        tr.train_step(batches[3])
        hook.remove()
        return tr, seen, fed, metrics

    serial, mixed = run(0), run(1)
    torch.cuda.synchronize()
    assert len(serial[1]) == len(mixed[1]) == 4 and len(serial[2]) == len(mixed[2]) == 4
    assert _as_bytes(mixed[1]) == _as_bytes(serial[1])
    for a, b in zip(serial[2], mixed[2]):
        assert torch.equal(a, b)
    for tr in (serial[0], mixed[0]):
        assert tr._decoder.status() == 0 and tr._resizer.status() == 0 and tr._augmenter.status() == 0
    assert serial[3]["val_acc"] >= 0.0 and mixed[3]["val_acc"] >= 0.0


def _three_steps(dev, batches, prefetch):
    tr = _gpu_trainer(dev, prefetch=prefetch)
    torch.manual_seed(11)
    metrics = tr._train_epoch(batches[:3])
    torch.cuda.synchronize()
    return metrics, [p.detach().clone() for p in list(tr.model.parameters()) + list(tr.basd_loss.parameters())]


def _distance(a, b):
    loss = abs(a[0]["train_loss"] - b[0]["train_loss"])
    return loss, max(float((x.double() - y.double()).abs().max()) for x, y in zip(a[1], b[1]))


@pytest.mark.gpu
def test_three_trainer_steps_with_prefetch_equal_three_without(dev, batches):
    """Two serial runs from one state first: where they agree bit for bit the prefetched run must too, else it may
    differ from a serial run by no more than they differ from each other."""
    first, second = _three_steps(dev, batches, 0), _three_steps(dev, batches, 0)
    ahead = _three_steps(dev, batches, 1)
    spread, got = _distance(first, second), _distance(first, ahead)
    print(f"[input_prefetch] three steps: serial vs serial |d loss| = {spread[0]:.3e}, max |d param| = {spread[1]:.3e}; "
          f"serial vs prefetch=1 |d loss| = {got[0]:.3e}, max |d param| = {got[1]:.3e}")
    assert np.isfinite(first[0]["train_loss"]) and first[0]["train_acc"] == ahead[0]["train_acc"]
    if spread == (0.0, 0.0):
        assert got == (0.0, 0.0) and ahead[0] == first[0]
    else:
        assert got[0] <= spread[0] and got[1] <= spread[1]


@pytest.mark.gpu
def test_validation_with_prefetch_returns_the_serial_metrics(dev, batches):
    from basd_amd.evaluation import evaluate_model
    from basd_amd.jpeg import JpegDecoder
    from basd_amd.resize import ResizeCrop
    tr = _gpu_trainer(dev)
    criterion = nn.CrossEntropyLoss(label_smoothing=0.1)
    val = _val_batches(batches)

    def run(prefetch, **kw):
        return evaluate_model(tr.model, val, criterion, num_classes=10, image_stats=(MEAN, STD),
                              resize_crop=ResizeCrop(16, 0.875, device=dev), jpeg_decode=JpegDecoder(dev),
                              prefetch=prefetch, **kw)

    first, second, ahead = run(0), run(0), run(1)
    print(f"[input_prefetch] validation: serial {first}, serial again {second}, prefetch=1 {ahead}")
    assert np.isfinite(first["loss"]) and set(ahead) == set(first)
    assert ahead["val_acc"] == first["val_acc"] and ahead["val_acc_top5"] == first["val_acc_top5"]      # counts: exact
    if first == second:
        assert ahead == first
    else:
        assert abs(ahead["loss"] - first["loss"]) <= abs(second["loss"] - first["loss"])
    # the trainer's own call: its prefetch, its one stream
    ahead_tr = _gpu_trainer(dev, prefetch=2)
    own = ahead_tr.evaluate(ahead_tr.model, val)
    assert own["val_acc"] == first["val_acc"] and own["val_acc_top5"] == first["val_acc_top5"]
    if first == second:
        assert own == tr.evaluate(tr.model, val) == first
    with pytest.raises(ValueError, match="prefetch must be an int >= 0"):
        run(-1)
