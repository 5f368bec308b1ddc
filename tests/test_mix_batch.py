"""Fused batch preparation (``basd_amd.augment``, kernel in ``csrc/mix.hip``): MixUp / CutMix with the batch rolled by
one, the soft targets and the uint8 conversion in one launch, against a restatement written here with torch ops on the
CPU.  Every step of the contract is ONE fp32 operation rounded to nearest (nothing contracted) and a bf16 destination is
rounded once at the end, so every comparison is on the raw bits (NaN positions equal): there is no tolerance.

``torchvision`` is not installed where this was written: ``draw_mix_params`` is checked against its own documented
formulas (and ``torch.distributions.Beta`` for the one draw it shares with torch), not against the package."""
import math
import os
from types import SimpleNamespace

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from basd_amd.augment import BatchMixer, MixParams, draw_mix_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
MEAN_T, STD_T = (0.5, 0.5, 0.5), (0.25, 0.5, 0.125)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
def _f32(value: float) -> torch.Tensor:
    """A host double rounded once to fp32 (what the kernel receives)."""
    return torch.tensor(value, dtype=torch.float64).to(torch.float32)


def _load(x, mean=None, std=None):
    """v(x): fp32 / bf16 widened exactly; uint8 as ((float(u) / 255) - mean_c) / std_c with true fp32 divisions."""
    x = x.detach().cpu()
    if x.dtype != torch.uint8:
        return x.float()
    C = x.shape[1]
    m = torch.tensor(mean if mean is not None else [0.0] * C, dtype=torch.float32).view(1, C, 1, 1)
    s = torch.tensor(std if std is not None else [1.0] * C, dtype=torch.float32).view(1, C, 1, 1)
    return x.float().div(255).sub(m).div(s)


def _restate_images(v, params, out_dtype=torch.float32):
    """``v``: the loaded fp32 batch on the CPU."""
    if params.kind == "mixup":
        out = v.roll(1, 0).mul(_f32(1.0 - params.lam)).add(v.mul(_f32(params.lam)))
    elif params.kind == "cutmix":
        x1, y1, x2, y2 = params.box
        out = v.clone()
        out[..., y1:y2, x1:x2] = v.roll(1, 0)[..., y1:y2, x1:x2]
    else:
        out = v.clone()
    return out.to(out_dtype)


def _restate_targets(labels, K, params):
    y = labels.detach().cpu()
    bad = (y < 0) | (y >= K)
    onehot = F.one_hot(y.clamp(0, K - 1), K).to(torch.float32)
    t = onehot.roll(1, 0).mul(_f32(1.0 - params.lam_targets)).add(onehot.mul(_f32(params.lam_targets)))
    t[bad | bad.roll(1, 0)] = float("nan")
    return t


def _assert_same_bits(got, want, what=""):
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    gn, wn = got.isnan(), want.isnan()
    assert torch.equal(gn, wn), f"{what}: NaN positions differ ({int(gn.sum())} vs {int(wn.sum())})"
    bits = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.uint8: torch.uint8}[got.dtype]
    g, w = got.contiguous().view(bits).masked_fill(gn, 0), want.contiguous().view(bits).masked_fill(wn, 0)
    if not torch.equal(g, w):
        diff = g != w
        raise AssertionError(f"{what}: {int(diff.sum())} of {diff.numel()} elements differ in their bits")


def _params_for(H, W):
    """Several fixed draws per kind: lam tiny / 0.5 / next to 1 / a generic double; an empty box, the full image, a box
    touching two edges (right and top), an interior box."""
    area = lambda b: 1.0 - (b[2] - b[0]) * (b[3] - b[1]) / (W * H)
    boxes = [(min(3, W), min(2, H), min(3, W), min(5, H)), (0, 0, W, H), (W // 2, 0, W, H // 2 + 1),
             (1, 1, max(W - 2, 1), max(H - 1, 1))]
    return ([MixParams("none")]
            + [MixParams("mixup", lam, None, lam) for lam in (1e-30, 0.5, 1.0 - 2.0 ** -20, 0.3141592653589793)]
            + [MixParams("cutmix", 0.37, b, area(b)) for b in boxes])


def _make_images(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.uint8:
        return torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)
    return (2.0 * torch.randn(shape, generator=g)).to(dtype)


def _make_labels(B, K, seed):
    y = torch.randint(0, K, (B,), generator=torch.Generator().manual_seed(seed))
    if B > 2:
        y[2] = y[1]                                   # a pair with equal labels: the entry is fadd(t_p, t_s)
    return y


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the restatement itself, the draws, the boundary, the trainer switch
# ---------------------------------------------------------------------------------------------------------------------
def test_restatement_equals_torchs_in_place_mixup():
    """``x.roll(1, 0).mul_(1 - lam).add_(x.mul(lam))`` (what torchvision's MixUp runs) bit for bit, five values of lam."""
    x = _make_images((8, 3, 16, 16), torch.float32, 0)
    for lam in (1e-30, 0.25, 0.5, 0.3141592653589793, 1.0 - 2.0 ** -20):
        theirs = x.roll(1, 0).mul_(1.0 - lam).add_(x.mul(lam))
        _assert_same_bits(_restate_images(x, MixParams("mixup", lam, None, lam)), theirs, f"lam={lam}")


def test_restatement_divides_and_a_reciprocal_would_not():
    u = torch.arange(256, dtype=torch.uint8)
    divided = u.float().div(255)
    assert torch.equal(divided, (u.double() / 255).float())            # a correctly rounded quotient
    assert int((divided != u.float() * torch.tensor(1.0 / 255, dtype=torch.float32)).sum()) > 0


def test_draws_are_reproducible_and_inside_the_image():
    H, W = 15, 17
    g1, g2 = torch.Generator().manual_seed(11), torch.Generator().manual_seed(11)
    a = [draw_mix_params(H, W, generator=g1) for _ in range(200)]
    b = [draw_mix_params(H, W, generator=g2) for _ in range(200)]
    assert a == b
    assert {p.kind for p in a} == {"mixup", "cutmix"}
    for p in a:
        assert 0.0 <= p.lam <= 1.0
        if p.kind == "mixup":
            assert p.box is None and p.lam_targets == p.lam
        else:
            x1, y1, x2, y2 = p.box
            assert 0 <= x1 <= x2 <= W and 0 <= y1 <= y2 <= H
            assert p.lam_targets == float(1.0 - (x2 - x1) * (y2 - y1) / (W * H))
            r = 0.5 * math.sqrt(1.0 - p.lam)
            assert x2 - x1 <= 2 * int(r * W) and y2 - y1 <= 2 * int(r * H)
    torch.manual_seed(11)                                               # generator=None is the global generator
    assert [draw_mix_params(H, W) for _ in range(200)] == a
    with pytest.raises(AttributeError):
        a[0].lam = 0.0                                                  # an immutable record


def test_draws_honour_p_and_alpha():
    g = torch.Generator().manual_seed(3)
    assert {draw_mix_params(8, 8, p=(1, 0), generator=g).kind for _ in range(50)} == {"mixup"}
    assert {draw_mix_params(8, 8, p=(0, 2), generator=g).kind for _ in range(50)} == {"cutmix"}
    many = [draw_mix_params(8, 8, p=(9, 1), generator=g).kind for _ in range(300)]
    assert many.count("mixup") > 220
    # Beta(alpha, alpha): concentrated at 1/2 for a large alpha, at the ends for a small one
    big = [draw_mix_params(8, 8, alpha=200.0, p=(1, 0), generator=g).lam for _ in range(100)]
    small = [draw_mix_params(8, 8, alpha=0.05, p=(1, 0), generator=g).lam for _ in range(100)]
    assert all(abs(v - 0.5) < 0.2 for v in big)
    assert sum(min(v, 1.0 - v) < 0.05 for v in small) > 60
    # the one draw shared with torch: the same global seed gives torch.distributions.Beta's sample
    torch.manual_seed(5)
    ours = draw_mix_params(8, 8, alpha=0.7, p=(1, 0)).lam
    torch.manual_seed(5)
    torch.multinomial(torch.tensor([1.0, 0.0]), 1)
    assert ours == float(torch.distributions.Beta(0.7, 0.7).sample())
    for bad in ({"alpha": 0.0}, {"p": (0, 0)}, {"p": (1, 2, 3)}, {"p": (-1, 2)}):
        with pytest.raises(ValueError):
            draw_mix_params(8, 8, **bad)


def test_cpu_tensors_raise():
    mixer = BatchMixer(10, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mixer(torch.zeros(4, 3, 8, 8), torch.zeros(4, dtype=torch.int64), MixParams("mixup", 0.5, None, 0.5))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mixer(torch.zeros(4, 3, 8, 8, dtype=torch.uint8), None, MixParams("none"))


def _argument_errors(dev):
    """Every boundary of ``BatchMixer.__call__``: raised before anything is launched, on any device."""
    x = torch.zeros(4, 3, 8, 8, device=dev)
    y = torch.zeros(4, dtype=torch.int64, device=dev)
    mixer = BatchMixer(10, device=dev)
    stats = BatchMixer(10, mean=MEAN, std=STD, device=dev)
    mix = MixParams("mixup", 0.5, None, 0.5)
    cases = [
        (ValueError, lambda: mixer(x[0], y, mix)),                                             # not (B, C, H, W)
        (ValueError, lambda: mixer(x.to(memory_format=torch.channels_last), y, mix)),
        (ValueError, lambda: mixer(x[:, :, :, ::2], y, mix)),                                  # not dense
        (ValueError, lambda: mixer(torch.zeros(4, 8, 8, 3, device=dev).permute(0, 3, 1, 2), y, mix)),
        (TypeError, lambda: mixer(x.double(), y, mix)),
        (TypeError, lambda: mixer(x.half(), y, mix)),
        (ValueError, lambda: stats(torch.zeros(4, 4, 8, 8, dtype=torch.uint8, device=dev), y, mix)),   # 3 stats, 4 channels
        (ValueError, lambda: stats(torch.zeros(4, 1, 8, 8, dtype=torch.uint8, device=dev), y, mix)),
        (TypeError, lambda: mixer(x, y.int(), mix)),
        (ValueError, lambda: mixer(x, y[:3], mix)),
        (ValueError, lambda: mixer(x, y[:, None], mix)),
        (ValueError, lambda: mixer(x, y, MixParams("cutmix", 0.5, (0, 0, 9, 4), 0.5))),       # box outside the image
        (ValueError, lambda: mixer(x, y, MixParams("cutmix", 0.5, (5, 0, 4, 4), 0.5))),
        (ValueError, lambda: mixer(x, y, MixParams("cutmix", 0.5, None, 0.5))),
        (ValueError, lambda: mixer(x, y, MixParams("blend", 0.5, None, 0.5))),
        (ValueError, lambda: mixer(x, y, mix, out=x)),                                         # dst overlaps src
        (ValueError, lambda: mixer(x, y, mix, out=torch.zeros(4, 3, 8, 9, device=dev))),
        (TypeError, lambda: mixer(x, y, mix, out=torch.zeros(4, 3, 8, 8, dtype=torch.float16, device=dev))),
    ]
    flat = torch.zeros(2 * x.numel() - 8, device=dev)
    src = flat[: x.numel()].view(4, 3, 8, 8)
    cases.append((ValueError, lambda: mixer(src, y, mix, out=flat[x.numel() - 8: 2 * x.numel() - 8].view(4, 3, 8, 8))))
    for error, call in cases:
        with pytest.raises(error):
            call()
    for error, kw in ((ValueError, {"mean": MEAN}), (ValueError, {"mean": (0.0,) * 5, "std": (1.0,) * 5}),
                      (ValueError, {"mean": MEAN, "std": (1.0, 1.0)}), (TypeError, {"out_dtype": torch.float16})):
        with pytest.raises(error):
            BatchMixer(10, device=dev, **kw)
    with pytest.raises(ValueError):
        BatchMixer(0, device=dev)
    if torch.device(dev).type == "cuda":
        with pytest.raises(ValueError):
            mixer(x, y.cpu(), mix)                                                             # labels elsewhere


def test_argument_errors_on_cpu():
    _argument_errors("cpu")


def test_messages_carry_the_shapes():
    mixer = BatchMixer(10, device="cpu")
    with pytest.raises(ValueError, match=r"\(4, 3, 8, 4\)"):
        mixer(torch.zeros(4, 3, 8, 8)[..., ::2], None, MixParams("none"))
    with pytest.raises(RuntimeError, match=r"\(4, 3, 8, 8\)"):
        mixer(torch.zeros(4, 3, 8, 8), None, MixParams("none"))


def test_exported_from_the_package():
    import basd_amd
    from basd_amd import _lib
    assert "augment" in basd_amd.__doc__
    assert "basd_mix_batch" in _lib.SIGNATURES
    with open(os.path.join(ROOT, "include", "basd_hip.h")) as f:
        header = f.read()
    assert "#define BASD_DTYPE_U8 2" in header and "int basd_mix_batch(" in header


# -- the trainer switch (the OracleBASD pattern of tests/test_trainer_step.py)
def _config(points=4, classes=10):
    return SimpleNamespace(training=SimpleNamespace(label_smoothing=0.1, learning_rate=1e-3, weight_decay=0.05),
                           basd=SimpleNamespace(num_extraction_points=points), model=SimpleNamespace(num_classes=classes))


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


def _toy_models(dev="cpu"):
    from tools import stock_models as SM
    torch.manual_seed(3)
    student = SM.StockViT(img_size=32, patch_size=8, embed_dim=48, depth=6, num_heads=4, num_classes=10).to(dev)
    teacher = SM.StockViT(img_size=32, patch_size=8, embed_dim=64, depth=3, num_heads=4, num_classes=0).to(dev)
    return student, SM.make_teacher(teacher, 32)


STATS = {"clean": (MEAN_T, STD_T), "augmented": (MEAN, STD)}


def _uint8_batch(B=8, seed=1):
    g = torch.Generator().manual_seed(seed)
    return {"clean": torch.randint(0, 256, (B, 3, 32, 32), generator=g, dtype=torch.uint8),
            "augmented": torch.randint(0, 256, (B, 3, 32, 32), generator=g, dtype=torch.uint8),
            "label": torch.arange(B) % 10}


def test_trainer_switch_on_cpu():
    from basd_amd import trainer as T
    from tools import stock_models as SM
    student, teacher = _toy_models()
    info = SM.probe_model(student, 32)
    tr = T.Trainer(student, _config(), teacher, student_info=info, loss_cls=OracleBASD, mixup="fused")
    assert isinstance(tr._mixer, BatchMixer) and tr._mixer.mean is None and tr._mixer.num_classes == 10
    with pytest.raises(TypeError, match="uint8"):
        tr.train_step(_uint8_batch())                                   # fused, but no image_stats
    tr = T.Trainer(student, _config(), teacher, student_info=info, loss_cls=OracleBASD, mixup="fused",
                   image_stats=STATS, mix_dtype=torch.bfloat16)
    assert tr._mixer.mean == MEAN and tr._clean_mixer.std == STD_T and tr._mixer.out_dtype == torch.bfloat16
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tr.train_step(_uint8_batch())                                   # everything is in order but the device
    for mixup in (True, False):
        tr = T.Trainer(student, _config(), teacher, student_info=info, loss_cls=OracleBASD, mixup=mixup,
                       image_stats=STATS)
        assert tr._mixer is None
        with pytest.raises(TypeError, match="uint8"):
            tr.train_step(_uint8_batch())
    with pytest.raises(ValueError):
        T.Trainer(student, _config(), teacher, student_info=info, loss_cls=OracleBASD, mixup="fuse")
    with pytest.raises(ValueError):
        T.Trainer(student, _config(), teacher, student_info=info, loss_cls=OracleBASD, mixup="fused",
                  image_stats={"clean": (MEAN, STD)})
    with pytest.raises(ValueError):
        T.Trainer(student, _config(), teacher, student_info=info, loss_cls=OracleBASD, mix_dtype=torch.bfloat16)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the kernel, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


SHAPES = [(8, 3, 16, 16), (5, 3, 15, 17), (1, 3, 8, 8), (3, 1, 7, 7), (256, 3, 224, 224)]
SRC = {"fp32": torch.float32, "bf16": torch.bfloat16, "uint8": torch.uint8}
DST = {"fp32": torch.float32, "bf16": torch.bfloat16}


@pytest.mark.gpu
@pytest.mark.parametrize("src", list(SRC))
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_images_and_targets_bit_exact(dev, shape, src):
    """{fp32, bf16, uint8} x {fp32, bf16} x {none, MixUp, CutMix}, several draws per kind; one launch per case."""
    B, C, H, W = shape
    K = 1000 if B == 256 else 10
    x = _make_images(shape, SRC[src], seed=B * 1000 + H)
    labels = _make_labels(B, K, seed=B)
    mean, std = (MEAN[:C], STD[:C]) if src == "uint8" else (None, None)
    v = _load(x, mean, std)
    x_dev, labels_dev = x.to(dev), labels.to(dev)
    for dst_name, dst in DST.items():
        mixer = BatchMixer(K, mean=mean, std=std, out_dtype=dst, device=dev)
        for params in _params_for(H, W):
            mixed, targets = mixer(x_dev, labels_dev, params)
            what = f"{shape} {src}->{dst_name} {params}"
            assert mixed.dtype == dst and targets.dtype == torch.float32 and targets.shape == (B, K)
            _assert_same_bits(mixed, _restate_images(v, params, dst), what)
            _assert_same_bits(targets, _restate_targets(labels, K, params), what + " targets")
    _assert_same_bits(x_dev, x, "src unchanged")
    if B > 2:                                                           # the equal pair: exactly fadd(t_p, t_s)
        p = MixParams("mixup", 0.3141592653589793, None, 0.3141592653589793)
        t = BatchMixer(K, device=dev)(x_dev.float(), labels_dev, p)[1].cpu()
        assert t[2, labels[2]] == _f32(1.0 - p.lam_targets) + _f32(p.lam_targets)


@pytest.mark.gpu
@pytest.mark.parametrize("dst", list(DST))
def test_uint8_every_byte_value_and_no_stats(dev, dst):
    """All 256 byte values in every channel; without mean / std the plain scale (any channel count)."""
    x = torch.arange(256, dtype=torch.uint8).view(1, 1, 16, 16).repeat(2, 3, 1, 1)
    x[1] = x[1].flip(-1)
    for mean, std in ((MEAN, STD), (MEAN_T, STD_T), (None, None)):
        mixer = BatchMixer(10, mean=mean, std=std, out_dtype=DST[dst], device=dev)
        for params in (MixParams("none"), MixParams("mixup", 0.3, None, 0.3), MixParams("cutmix", 0.5, (2, 3, 11, 9), 0.5)):
            got = mixer(x.to(dev), None, params)
            assert got[1] is None
            _assert_same_bits(got[0], _restate_images(_load(x, mean, std), params, DST[dst]), f"{mean} {params}")
    six = torch.randint(0, 256, (3, 6, 5, 5), dtype=torch.uint8, generator=torch.Generator().manual_seed(1))
    got = BatchMixer(10, out_dtype=DST[dst], device=dev)(six.to(dev), None, MixParams("mixup", 0.7, None, 0.7))[0]
    _assert_same_bits(got, _restate_images(_load(six), MixParams("mixup", 0.7, None, 0.7), DST[dst]), "six channels")


@pytest.mark.gpu
@pytest.mark.parametrize("src", ["fp32", "bf16"])
def test_nan_and_inf_pixels_follow_the_formula(dev, src):
    x = _make_images((5, 3, 15, 17), torch.float32, 9)
    x[0, 0, 0, :4] = torch.tensor([float("nan"), float("inf"), -float("inf"), 0.0])
    x[1, 0, 0, :4] = torch.tensor([1.0, 0.0, float("inf"), float("inf")])
    x[3, 2, 14, 16] = float("inf")
    x[4, 2, 14, 16] = -float("inf")
    x = x.to(SRC[src])
    for dst in DST.values():
        for params in (MixParams("none"), MixParams("mixup", 0.5, None, 0.5), MixParams("mixup", 1.0, None, 1.0),
                       MixParams("mixup", 0.0, None, 0.0), MixParams("cutmix", 0.5, (0, 0, 3, 1), 0.5)):
            got = BatchMixer(10, out_dtype=dst, device=dev)(x.to(dev), None, params)[0]
            want = _restate_images(_load(x), params, dst)
            _assert_same_bits(got, want, f"{src} {dst} {params}")
    # inf * 0 is NaN, as in torch
    assert _restate_images(_load(x), MixParams("mixup", 1.0, None, 1.0))[2, 0, 0, 2:4].isnan().all()


@pytest.mark.gpu
def test_labels_out_of_range_make_their_rows_nan(dev):
    B, K = 8, 10
    x = _make_images((B, 3, 16, 16), torch.float32, 4).to(dev)
    labels = torch.tensor([1, 10, 3, 3, -1, 7, 0, 9])
    for params in (MixParams("none"), MixParams("mixup", 0.25, None, 0.25), MixParams("cutmix", 0.5, (1, 1, 9, 9), 0.75)):
        mixed, targets = BatchMixer(K, device=dev)(x, labels.to(dev), params)
        want = _restate_targets(labels, K, params)
        assert want.isnan().all(1).tolist() == [False, True, True, False, True, True, False, False]
        _assert_same_bits(targets, want, str(params))
        _assert_same_bits(mixed, _restate_images(x.cpu(), params), str(params))       # the images are not affected
    big = torch.tensor([2 ** 40, 0, 1, 2, 3, 4, 5, -2 ** 40])
    targets = BatchMixer(K, device=dev)(x, big.to(dev), MixParams("mixup", 0.5, None, 0.5))[1]
    _assert_same_bits(targets, _restate_targets(big, K, MixParams("mixup", 0.5, None, 0.5)), "far out of range")


@pytest.mark.gpu
@pytest.mark.parametrize("src", list(SRC))
@pytest.mark.parametrize("dst", list(DST))
def test_views_at_odd_element_offsets(dev, src, dst):
    """A dense view that starts at an odd element of a larger buffer, as the source and as the destination: the
    narrower accesses; the elements around the destination view stay as they were."""
    shape = (5, 3, 15, 17)
    n = math.prod(shape)
    x = _make_images(shape, SRC[src], 21)
    labels = _make_labels(5, 10, 2)
    mean, std = (MEAN, STD) if src == "uint8" else (None, None)
    mixer = BatchMixer(10, mean=mean, std=std, device=dev)
    for s_off, d_off in ((1, 0), (0, 3), (5, 7)):
        src_buf = torch.zeros(n + 16, dtype=SRC[src], device=dev)
        src_view = src_buf[s_off: s_off + n].view(shape)
        src_view.copy_(x)
        for params in (MixParams("mixup", 0.3, None, 0.3), MixParams("cutmix", 0.5, (4, 2, 17, 9), 0.5), MixParams("none")):
            dst_buf = torch.full((n + 16,), 7.0, dtype=DST[dst], device=dev)
            out = dst_buf[d_off: d_off + n].view(shape)
            mixed, targets = mixer(src_view, labels.to(dev), params, out=out)
            assert mixed.data_ptr() == out.data_ptr()
            _assert_same_bits(mixed, _restate_images(_load(x, mean, std), params, DST[dst]), f"{s_off} {d_off} {params}")
            _assert_same_bits(targets, _restate_targets(labels, 10, params), "targets")
            assert (dst_buf[:d_off] == 7.0).all() and (dst_buf[d_off + n:] == 7.0).all()
        _assert_same_bits(src_view, x, "src unchanged")


@pytest.mark.gpu
def test_argument_errors_on_the_gpu(dev):
    _argument_errors(dev)


@pytest.mark.gpu
def test_overlapping_destination_is_refused_by_the_library_too(dev):
    from basd_amd import _lib
    x = torch.zeros(4, 3, 8, 8, device=dev)
    stream = torch._C._cuda_getCurrentRawStream(dev.index)
    args = [0, 4, 3, 8, 8, 1, 0.5, 0, 0, 0, 0, None, None, None, 10, 0.5, None, stream]
    with pytest.raises(RuntimeError, match="invalid argument"):
        _lib.call("basd_mix_batch", x.data_ptr(), 0, x.data_ptr() + 64, *args)
    with pytest.raises(RuntimeError, match="invalid argument"):
        _lib.call("basd_mix_batch", x.data_ptr(), 3, x.data_ptr() + 4 * x.numel(), *args)      # no such dtype


@pytest.mark.gpu
def test_one_launch_and_nothing_else_per_call(dev):
    """A steady-state call is one kernel launch: no memcpy, no memset, no allocation on the device.  Counted with
    ``torch.profiler`` where it sees launches made through ctypes (the output says whether it does); the allocator's
    counter is checked either way."""
    from torch.profiler import ProfilerActivity, profile
    x = _make_images((64, 3, 64, 64), torch.uint8, 5).to(dev)
    labels = _make_labels(64, 1000, 5).to(dev)
    mixer = BatchMixer(1000, mean=MEAN, std=STD, out_dtype=torch.bfloat16, device=dev)
    draws = [MixParams("mixup", 0.4, None, 0.4), MixParams("cutmix", 0.5, (3, 5, 40, 50), 0.6), MixParams("none")]
    for i in range(6):
        out = mixer(x, labels, draws[i % 3])
    del out
    torch.cuda.synchronize()
    device_allocations = torch.cuda.memory_stats(dev)["num_device_alloc"]
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for i in range(21):
            out = mixer(x, labels, draws[i % 3])
        torch.cuda.synchronize()
    assert torch.cuda.memory_stats(dev)["num_device_alloc"] == device_allocations
    device_events = [e for e in prof.events() if "cuda" in str(e.device_type).lower()]
    host_names = {e.name for e in prof.events() if "cuda" not in str(e.device_type).lower()}
    others = [e for e in prof.events() if "memcpy" in e.name.lower() or "memset" in e.name.lower()]
    kernels = [e for e in device_events if e.name not in host_names and e not in others]
    ours = [e for e in kernels if "mix_batch_kernel" in e.name]
    if ours:
        print(f"[mix_batch] profiler: {len(kernels)} kernels ({len(ours)} mix_batch_kernel), {len(others)} memcpy / "
              "memset in 21 calls")
        assert len(ours) == 21 and len(kernels) == 21, sorted({e.name for e in kernels})
        assert not others, sorted({e.name for e in others})
    else:
        print("[mix_batch] the profiler does not see the ctypes launches here "
              f"({len(kernels)} device kernels, {len(others)} memcpy / memset events seen by it)")
        assert not kernels and not others


# ---------------------------------------------------------------------------------------------------------------------
# GPU: inside the trainer
# ---------------------------------------------------------------------------------------------------------------------
class _Recorder:
    """What the student, the teacher and the loss receive in a step."""

    def __init__(self, trainer, teacher):
        self.student, self.teacher, self.targets = [], [], []
        trainer.model.register_forward_pre_hook(lambda m, args: self.student.append(args[0].detach().clone()))
        teacher.model.register_forward_pre_hook(lambda m, args: self.teacher.append(args[0].detach().clone()))
        trainer.basd_loss.register_forward_pre_hook(lambda m, args: self.targets.append(args[1].detach().clone()))


def _float_batch(B=16):
    g = torch.Generator().manual_seed(2)
    return {"clean": torch.randn(B, 3, 1, 1, generator=g) * 2.0 + torch.randn(B, 3, 32, 32, generator=g),
            "augmented": torch.randn(B, 3, 1, 1, generator=g) * 2.0 + torch.randn(B, 3, 32, 32, generator=g),
            "label": torch.arange(B) % 10}


@pytest.mark.gpu
@pytest.mark.parametrize("mix_dtype", [None, torch.bfloat16], ids=["fp32", "bf16"])
def test_trainer_feeds_the_restated_draw(dev, mix_dtype):
    """Under one torch seed the tensors the model and the loss receive are the restatement of the same draw; three steps
    give finite losses and move the parameters."""
    from basd_amd import trainer as T
    from tools import stock_models as SM
    student, teacher = _toy_models(dev)
    torch.manual_seed(42)
    tr = T.Trainer(student, _config(), teacher, student_info=SM.probe_model(student, 32), mixup="fused",
                   autocast_dtype=mix_dtype, mix_dtype=mix_dtype)
    rec = _Recorder(tr, teacher)
    batch = _float_batch()
    before = [p.detach().clone() for p in student.parameters()]
    kinds = set()
    for step in range(3):
        torch.manual_seed(100 + step)
        out = tr.train_step(batch)
        assert torch.isfinite(out["loss"])
        torch.manual_seed(100 + step)
        params = draw_mix_params(32, 32)
        kinds.add(params.kind)
        _assert_same_bits(rec.student[step], _restate_images(batch["augmented"], params, mix_dtype or torch.float32),
                          f"step {step} {params}")
        _assert_same_bits(rec.targets[step], _restate_targets(batch["label"], 10, params), f"step {step} targets")
        _assert_same_bits(rec.teacher[step], batch["clean"], "clean batch")
    assert any(not torch.equal(a, b) for a, b in zip(before, student.parameters()))
    print(f"[mix_batch] kinds drawn in the three steps: {sorted(kinds)}")


@pytest.mark.gpu
def test_trainer_uint8_equals_host_normalised_fp32(dev):
    """uint8 batches plus ``image_stats`` against the same run on batches normalised on the host: bitwise equal on
    the mixed images, the clean images and the targets."""
    from basd_amd import trainer as T
    from tools import stock_models as SM
    student, teacher = _toy_models(dev)
    torch.manual_seed(42)
    tr = T.Trainer(student, _config(), teacher, student_info=SM.probe_model(student, 32), mixup="fused",
                   image_stats=STATS)
    rec = _Recorder(tr, teacher)
    raw = _uint8_batch(16)
    host = {"clean": _load(raw["clean"], MEAN_T, STD_T), "augmented": _load(raw["augmented"], MEAN, STD),
            "label": raw["label"]}
    for step in range(3):
        torch.manual_seed(7 + step)
        a = tr.train_step(raw)
        torch.manual_seed(7 + step)
        b = tr.train_step(host)
        assert torch.isfinite(a["loss"]) and torch.isfinite(b["loss"])
        _assert_same_bits(rec.student[2 * step], rec.student[2 * step + 1], f"mixed images, step {step}")
        _assert_same_bits(rec.teacher[2 * step], rec.teacher[2 * step + 1], f"clean images, step {step}")
        _assert_same_bits(rec.targets[2 * step], rec.targets[2 * step + 1], f"targets, step {step}")
        torch.manual_seed(7 + step)
        params = draw_mix_params(32, 32)
        _assert_same_bits(rec.student[2 * step], _restate_images(host["augmented"], params), f"restated, step {step}")
    with pytest.raises(TypeError, match="uint8"):
        T.Trainer(student, _config(), teacher, student_info=SM.probe_model(student, 32), mixup="fused").train_step(raw)
