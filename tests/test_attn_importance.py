"""Teacher attention importance from the output of the block's own ``qkv`` projection (``csrc/attn.hip``,
``basd_amd.attention``, ``capture.make_qkv_importance_hook``): CPU tests cover the restatement against the reference-form
hook and the plumbing, GPU tests the kernel against fp64, its launch / memory contract and the loss on its captures."""
import os
from types import SimpleNamespace

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from basd_amd import _lib, capture
from basd_amd.attention import MODES, attn_importance
from basd_amd.capture import make_qkv_importance_hook
from oracle import basd_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def restate(qkv: torch.Tensor, num_heads: int, mode: str, dtype=torch.float64, scale=None) -> torch.Tensor:
    """The reference hook's expression (teacher.py:27-39) in ``dtype``, reduced to what the loss reads of it."""
    B, N, C3 = qkv.shape
    hd = C3 // (3 * num_heads)
    x = qkv.to(dtype).reshape(B, N, 3, num_heads, hd).permute(2, 0, 3, 1, 4)
    attn = ((x[0] @ x[1].transpose(-2, -1)) * (hd ** -0.5 if scale is None else scale)).softmax(dim=-1)
    return attn[:, :, 0, :] if mode == "cls_row" else attn.mean(dim=2)


class _Attn(nn.Module):
    def __init__(self, dim, heads, bias=True):
        super().__init__()
        self.num_heads = heads
        self.qkv = nn.Linear(dim, 3 * dim, bias=bias)
        self.proj = nn.Linear(dim, dim)

    def forward(self, x):
        B, N, C = x.shape
        qkv = self.qkv(x).reshape(B, N, 3, self.num_heads, C // self.num_heads).permute(2, 0, 3, 1, 4)
        # one sample at a time: whatever backend serves the product, its working set is one sample's
        y = torch.cat([F.scaled_dot_product_attention(qkv[0][b:b + 1], qkv[1][b:b + 1], qkv[2][b:b + 1])
                       for b in range(B)])
        return self.proj(y.transpose(1, 2).reshape(B, N, C))


class _Block(nn.Module):
    def __init__(self, dim, heads):
        super().__init__()
        self.norm1, self.attn = nn.LayerNorm(dim), _Attn(dim, heads)
        self.norm2, self.fc1, self.fc2 = nn.LayerNorm(dim), nn.Linear(dim, 4 * dim), nn.Linear(4 * dim, dim)

    def forward(self, x):
        x = x + self.attn(self.norm1(x))
        return x + self.fc2(F.gelu(self.fc1(self.norm2(x))))


class _NoClsViT(nn.Module):
    """A token ViT without a CLS token (global-pool head), timm attribute layout."""

    def __init__(self, *, img_size=32, patch_size=8, embed_dim=64, depth=3, num_heads=4):
        super().__init__()
        self.embed_dim = embed_dim
        self.patch_embed = nn.Conv2d(3, embed_dim, patch_size, patch_size)
        self.pos_embed = nn.Parameter(torch.randn(1, (img_size // patch_size) ** 2, embed_dim) * 0.02)
        self.blocks = nn.ModuleList([_Block(embed_dim, num_heads) for _ in range(depth)])
        self.norm = nn.LayerNorm(embed_dim)

    def forward(self, x):
        x = self.patch_embed(x).flatten(2).transpose(1, 2) + self.pos_embed
        for blk in self.blocks:
            x = blk(x)
        return self.norm(x).mean(dim=1)


def _teacher(model, depth, has_cls, dim, heads):
    return SimpleNamespace(model=model, layer_paths=[f"blocks.{i}" for i in range(depth)], attn_subpath="attn",
                           has_cls_token=has_cls, feature_format="token", embed_dim=dim, heads_per_layer=[heads] * depth,
                           depth=depth, mlp_ratio=4.0)


def _config(points=4, classes=10):
    return SimpleNamespace(training=SimpleNamespace(label_smoothing=0.1, learning_rate=1e-3, weight_decay=0.05),
                           basd=SimpleNamespace(num_extraction_points=points), model=SimpleNamespace(num_classes=classes))


def _models(has_cls, dev="cpu"):
    from tools import stock_models as SM
    torch.manual_seed(3)
    student = SM.StockViT(img_size=32, patch_size=8, embed_dim=48, depth=6, num_heads=4, num_classes=10).to(dev)
    if has_cls:
        teacher = SM.StockViT(img_size=32, patch_size=8, embed_dim=64, depth=3, num_heads=4, num_classes=0).to(dev)
    else:
        teacher = _NoClsViT().to(dev)
    return student, SM.make_teacher(teacher, 32)


def _images(B, size, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 3, 1, 1, generator=g) * 2.0 + torch.randn(B, 3, size, size, generator=g)


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the restatement and the plumbing
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [True, False])
def test_restatement_equals_the_reference_hook(bias):
    torch.manual_seed(0)
    attn = _Attn(32, 4, bias=bias)
    x = torch.randn(3, 11, 32)
    full, qkv = {}, {}
    h1 = attn.register_forward_hook(capture.make_attn_capture_hook(full, 0, cls_row_only=False))
    h2 = attn.qkv.register_forward_hook(lambda m, i, o: qkv.update(out=o))
    attn(x)
    h1.remove(), h2.remove()
    assert full[0].shape == (3, 4, 11, 11)
    torch.testing.assert_close(restate(qkv["out"], 4, "cls_row").float(), full[0][:, :, 0, :], rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(restate(qkv["out"], 4, "query_mean").float(), full[0].mean(dim=2), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("has_cls", [False, True])
def test_zero_stride_view_is_equivalent_for_the_loss(has_cls):
    torch.manual_seed(1)
    B, H, N = 3, 4, 11
    full = torch.randn(B, H, N, N).softmax(dim=-1)
    imp = full[:, :, 0, :] if has_cls else full.mean(dim=2)
    view = imp.contiguous()[:, :, None, :].expand(B, H, N, N)
    assert view.stride(2) == 0
    n = N - 1 if has_cls else N
    torch.testing.assert_close(O.token_weights(view, has_cls, n), O.token_weights(full, has_cls, n), rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(O.token_weights(view, has_cls, 7), O.token_weights(full, has_cls, 7), rtol=1e-5, atol=1e-7)


def test_cpu_tensors_raise_and_hooks_are_removed():
    torch.manual_seed(2)
    model = _NoClsViT()
    teacher = _teacher(model, 3, False, 64, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        capture.extract_intermediates(teacher, _images(2, 32, 0), attn="fused")
    assert not any(m._forward_hooks for m in model.modules())
    with pytest.raises(RuntimeError, match=r"\(2, 16, 192\)"):
        attn_importance(torch.zeros(2, 16, 192), 4, mode="query_mean")
    with pytest.raises(ValueError, match="attn must be"):
        capture.extract_intermediates(teacher, _images(2, 32, 0), attn="hip")
    hook = make_qkv_importance_hook({}, 0, 4, mode="cls_row")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hook(None, None, torch.zeros(2, 16, 192))


def test_argument_errors_carry_the_shapes():
    with pytest.raises(ValueError, match=r"\(2, 16\)"):
        attn_importance(torch.zeros(2, 16), 4, mode="cls_row")
    with pytest.raises(ValueError, match=r"\(2, 16, 190\)"):
        attn_importance(torch.zeros(2, 16, 190), 4, mode="cls_row")
    with pytest.raises(ValueError, match=r"head_dim 12 .*\(2, 16, 144\)"):
        attn_importance(torch.zeros(2, 16, 144), 4, mode="cls_row")
    with pytest.raises(ValueError, match=r"head_dim 136"):
        attn_importance(torch.zeros(1, 4, 3 * 136), 1, mode="cls_row")
    with pytest.raises(ValueError, match=r"\(2, 1026, 96\)"):
        attn_importance(torch.zeros(2, 1026, 96), 4, mode="cls_row")
    with pytest.raises(TypeError, match=r"float16.*\(2, 16, 96\)"):
        attn_importance(torch.zeros(2, 16, 96, dtype=torch.float16), 4, mode="cls_row")
    with pytest.raises(ValueError, match=r"strides \(3072, 192, 2\)"):
        attn_importance(torch.zeros(2, 16, 192)[:, :, ::2], 4, mode="cls_row")
    with pytest.raises(ValueError, match="mode must be"):
        attn_importance(torch.zeros(2, 16, 96), 4, mode="mean")
    with pytest.raises(ValueError, match=r"out must be .*\(2, 4, 16\).*\(2, 4, 15\)"):
        attn_importance(torch.zeros(2, 16, 96), 4, mode="cls_row", out=torch.zeros(2, 4, 15))


class OracleBASD(nn.Module):
    """The oracle behind the reference constructor's signature (test-side stand-in for the loss module on CPU)."""

    def __init__(self, base_criterion, student_dim, teacher_dim, student_depth, num_student_tokens, *, config,
                 teacher_has_cls_token):
        super().__init__()
        self.base_criterion, self.has_cls, self.n_s = base_criterion, teacher_has_cls_token, num_student_tokens
        self.token_layers = O.extraction_layers(student_depth, config.num_extraction_points)
        st = O.SelectorState.create(len(self.token_layers), student_dim, teacher_dim)
        self.register_buffer("proj_s", st.proj_s)
        self.register_buffer("proj_t", st.proj_t)
        self.log_temperatures = nn.Parameter(st.log_temperatures.detach().clone())

    def forward(self, logits, targets, s_tokens, t_tokens, t_attns):
        st = O.SelectorState(self.proj_s, self.proj_t, self.log_temperatures)
        return O.basd_forward(st, self.base_criterion, self.token_layers, self.n_s, self.has_cls, logits, targets,
                              {k: v.float() for k, v in s_tokens.items()}, {k: v.float() for k, v in t_tokens.items()},
                              {k: v.contiguous() for k, v in t_attns.items()})[0]


def test_trainer_switch_on_cpu():
    from basd_amd import trainer as T
    from tools import stock_models as SM
    student, teacher = _models(True)
    info = SM.probe_model(student, 32)
    with pytest.raises(ValueError, match="attn_capture must be 'torch' or 'fused', not 'x'"):
        T.Trainer(student, _config(), teacher, student_info=info, loss_cls=OracleBASD, attn_capture="x")
    batch = {"clean": _images(4, 32, 1), "augmented": _images(4, 32, 2), "label": torch.arange(4) % 10}
    tr = T.Trainer(student, _config(), teacher, student_info=info, loss_cls=OracleBASD, mixup=False)
    assert tr.attn_capture == "torch" and torch.isfinite(tr.train_step(batch)["loss"])
    tr = T.Trainer(student, _config(), teacher, student_info=info, loss_cls=OracleBASD, mixup=False,
                   attn_capture="fused")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tr.train_step(batch)                                            # everything is in order but the device
    assert not any(m._forward_hooks for m in teacher.model.modules())


def test_symbol_header_table_and_export():
    import basd_amd
    assert basd_amd.attn_importance is attn_importance and "attention" in basd_amd.__doc__
    assert _lib.SIGNATURES["basd_attn_importance"] == [_lib.vp, _lib.i32, _lib.i64, _lib.i64, _lib.i32, _lib.i32,
                                                       _lib.i32, _lib.i32, _lib.i32, _lib.f32, _lib.vp, _lib.vp]
    with open(os.path.join(ROOT, "include", "basd_hip.h")) as f:
        header = f.read()
    assert "int basd_attn_importance(const void* qkv, int dtype, long sb, long sn, int B, int N, int H, int hd," in header
    assert "#define BASD_ATTN_CLS_ROW 0" in header and "#define BASD_ATTN_QUERY_MEAN 1" in header
    assert "teacher.py:27-39" in header and "relational.py:22-27" in header
    assert MODES == {"cls_row": 0, "query_mean": 1}


@pytest.mark.parametrize("has_cls", [True, False])
def test_torch_capture_is_what_it_was(has_cls):
    """``attn="torch"`` (and no ``attn`` at all): the hooks of the attention module, same values, same strides."""
    student, teacher = _models(has_cls)
    x = _images(2, 32, 5)
    toks, attns = capture.extract_intermediates(teacher, x)
    toks2, attns2 = capture.extract_intermediates(teacher, x, attn="torch")
    manual = {}
    hooks = [teacher.model.get_submodule(f"blocks.{i}.attn").register_forward_hook(
        capture.make_attn_capture_hook(manual, i, apply_softmax=True, cls_row_only=has_cls)) for i in range(3)]
    with torch.no_grad():
        teacher.model(x)
    for h in hooks:
        h.remove()
    N = 17 if has_cls else 16
    for i in range(3):
        assert attns[i].shape == attns2[i].shape == (2, 4, N, N)
        assert attns[i].stride() == attns2[i].stride() == manual[i].stride()
        assert (attns[i].stride(2) == 0) == has_cls
        assert torch.equal(attns[i], manual[i]) and torch.equal(attns2[i], manual[i])
        assert torch.equal(toks[i], toks2[i]) and toks[i].stride() == toks2[i].stride()
    assert not any(m._forward_hooks for m in teacher.model.modules())


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


ULP = 2.0 ** -23
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


def _qkv(B, N, H, hd, dtype, seed, dev, q_gain=1.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, N, 3, H, hd, generator=g)
    x[:, :, 0] *= q_gain
    return x.reshape(B, N, 3 * H * hd).to(dtype).to(dev)


def _errors(qkv, H, mode, label):
    """(max|kernel - p64|, max|p32 - p64|, kernel output, p64) on the same, already rounded, inputs."""
    got = attn_importance(qkv, H, mode=mode)
    p64 = restate(qkv, H, mode, torch.float64)
    p32 = restate(qkv, H, mode, torch.float32)
    e_k = (got.double() - p64).abs().max().item()
    e_32 = (p32.double() - p64).abs().max().item()
    print(f"[attn] {label} {mode}: max|kernel - p64| = {e_k:.3e}, max|p32 - p64| = {e_32:.3e}, "
          f"bound = {2 * e_32 + ULP:.3e}")
    return e_k, e_32, got, p64


def _check(qkv, H, mode, label):
    e_k, e_32, got, p64 = _errors(qkv, H, mode, label)
    assert got.shape == p64.shape and got.dtype == torch.float32
    bound = 2 * e_32 + ULP
    assert e_k <= bound, (label, mode, e_k, bound)
    N = qkv.shape[1]
    s_err = (got.double().sum(dim=-1) - 1).abs().max().item()
    assert s_err <= N * bound, (label, mode, s_err, N * bound)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("H", [1, 12])
@pytest.mark.parametrize("hd", [32, 64, 72, 128])
@pytest.mark.parametrize("N", [1, 50, 196, 197, 577, 1025])
def test_accuracy_against_fp64(dev, N, hd, H, dt, mode):
    """max|p_kernel - p64| <= 2 max|p32 - p64| + 2^-23: the kernel and torch's fp32 evaluation of the reference hook's
    expression differ in summation order only (hence the 2); 2^-23 is one ulp of the largest value a probability
    takes.  Every row sums to 1 within N times that."""
    qkv = _qkv(2, N, H, hd, DTYPES[dt], 1000 * N + hd + H, dev)
    _check(qkv, H, mode, f"N={N} hd={hd} H={H} {dt}")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("dt", list(DTYPES))
def test_accuracy_on_views(dev, dt, mode):
    """A token stride larger than 3 H hd, and a view at an odd element offset (no 16-byte alignment)."""
    B, N, H, hd = 3, 197, 12, 64
    C3 = 3 * H * hd
    dense = _qkv(B, N, H, hd, DTYPES[dt], 7, dev)
    wide = torch.full((B, N, C3 + 24), float("nan"), dtype=DTYPES[dt], device=dev)
    wide[:, :, :C3] = dense
    view = wide[:, :, :C3]
    assert view.stride(1) == C3 + 24 and not view.is_contiguous()
    _check(view, H, mode, f"row stride {C3 + 24} {dt}")
    flat = torch.full((B * N * C3 + 3,), float("nan"), dtype=DTYPES[dt], device=dev)
    flat[1:1 + B * N * C3] = dense.reshape(-1)
    odd = flat[1:1 + B * N * C3].view(B, N, C3)
    assert odd.storage_offset() == 1 and odd.data_ptr() % 16 != 0
    _check(odd, H, mode, f"odd offset {dt}")
    assert torch.equal(attn_importance(odd, H, mode=mode), attn_importance(dense, H, mode=mode))
    assert torch.equal(attn_importance(view, H, mode=mode), attn_importance(dense, H, mode=mode))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("dt", list(DTYPES))
def test_accuracy_peaked(dev, dt, mode):
    """Scores spanning about +-20 (standard deviation 6): without the row maximum subtracted exp would lose the small
    probabilities' precision or overflow in the sum."""
    qkv = _qkv(2, 197, 12, 64, DTYPES[dt], 11, dev, q_gain=6.0)
    B, N, H, hd = 2, 197, 12, 64
    x = qkv.double().reshape(B, N, 3, H, hd)
    scores = torch.einsum("bihd,bjhd->bhij", x[:, :, 0], x[:, :, 1]) * hd ** -0.5
    assert scores.max() > 18 and scores.min() < -18
    _check(qkv, H, mode, f"peaked {dt}")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("dt", list(DTYPES))
def test_large_scores_nan_containment_and_determinism(dev, dt, mode):
    B, N, H, hd = 2, 197, 3, 64
    qkv = _qkv(B, N, H, hd, DTYPES[dt], 13, dev, q_gain=1e4)
    got = attn_importance(qkv, H, mode=mode)
    assert torch.isfinite(got).all()                                    # scores of about 1e4 in magnitude
    assert (got.double().sum(-1) - 1).abs().max() < 1e-4
    again = attn_importance(qkv, H, mode=mode)
    assert torch.equal(got, again)                                      # identical bits
    # a NaN in one (b, h)'s keys: that row, and no other
    qkv = _qkv(B, N, H, hd, DTYPES[dt], 14, dev)
    clean = attn_importance(qkv, H, mode=mode)
    bad = qkv.clone()
    bad.view(B, N, 3, H, hd)[1, 100, 1, 2, 5] = float("nan")
    got = attn_importance(bad, H, mode=mode)
    assert torch.isnan(got[1, 2]).all()
    mask = torch.ones(B, H, dtype=torch.bool, device=dev)
    mask[1, 2] = False
    assert torch.equal(got[mask], clean[mask]) and torch.isfinite(got[mask]).all()


@pytest.mark.gpu
def test_unsupported_shapes_launch_nothing(dev):
    lib = _lib.load()
    stream = torch._C._cuda_getCurrentRawStream(dev.index)
    qkv = torch.randn(1, 1100, 3 * 136, device=dev)
    out = torch.full((1, 1, 1100), -7.0, device=dev)
    for N, hd in [(1026, 64), (16, 12), (16, 136), (0, 64)]:
        st = lib.basd_attn_importance(qkv.data_ptr(), 0, qkv.stride(0), qkv.stride(1), 1, N, 1, hd, 0, 0.125,
                                      out.data_ptr(), stream)
        assert st == (_lib.EINVAL if N == 0 else _lib.EUNSUPPORTED), (N, hd, st)
    assert lib.basd_attn_importance(qkv.data_ptr(), 2, qkv.stride(0), qkv.stride(1), 1, 16, 1, 64, 0, 0.125,
                                    out.data_ptr(), stream) == _lib.EINVAL
    assert lib.basd_attn_importance(qkv.data_ptr(), 0, qkv.stride(0), qkv.stride(1), 1, 16, 1, 64, 2, 0.125,
                                    out.data_ptr(), stream) == _lib.EINVAL
    torch.cuda.synchronize()
    assert (out == -7.0).all()
    with pytest.raises(ValueError):
        attn_importance(qkv[:, :16, :36], 1, mode="cls_row")
    o = torch.empty(1, 2, 16, device=dev)
    assert attn_importance(qkv[:, :16, :3 * 128], 2, mode="cls_row", out=o) is o


def _device_kernels(prof):
    device_events = [e for e in prof.events() if "cuda" in str(e.device_type).lower()]
    host_names = {e.name for e in prof.events() if "cuda" not in str(e.device_type).lower()}
    others = [e for e in prof.events() if "memcpy" in e.name.lower() or "memset" in e.name.lower()]
    kernels = [e for e in device_events if e.name not in host_names and e not in others]
    return kernels, others


@pytest.mark.gpu
def test_one_launch_per_call_and_per_hooked_layer(dev):
    """One kernel launch and no memcpy / memset per call; the fused capture adds exactly one launch per hooked layer to
    the teacher's own forward (no projection beyond the model's own).  Counted with ``torch.profiler`` where it sees
    launches made through ctypes (the output says whether it does)."""
    from torch.profiler import ProfilerActivity, profile
    qkv = _qkv(4, 197, 12, 64, torch.bfloat16, 3, dev)
    out = torch.empty(4, 12, 197, device=dev)
    for mode in MODES:
        attn_importance(qkv, 12, mode=mode, out=out)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for i in range(10):
            attn_importance(qkv, 12, mode=list(MODES)[i % 2], out=out)
        torch.cuda.synchronize()
    kernels, others = _device_kernels(prof)
    ours = [e for e in kernels if "attn_importance_kernel" in e.name]
    seen = bool(ours)
    if seen:
        print(f"[attn] profiler: {len(kernels)} kernels ({len(ours)} attn_importance_kernel), {len(others)} memcpy / "
              "memset in 10 calls")
        assert len(ours) == 10 and len(kernels) == 10, sorted({e.name for e in kernels})
        assert not others, sorted({e.name for e in others})
    else:
        print(f"[attn] the profiler does not see the ctypes launches here ({len(kernels)} device kernels, "
              f"{len(others)} memcpy / memset events seen by it)")
        assert not kernels and not others

    for has_cls in (True, False):
        _, teacher = _models(has_cls, dev)
        x = _images(4, 32, 1).to(dev)
        counts = []
        for fused in (False, True):
            for _ in range(2):                                          # the second run is the counted one
                with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                    with torch.no_grad():
                        if fused:
                            capture.extract_intermediates(teacher, x, attn="fused")
                        else:
                            teacher.model(x)
                    torch.cuda.synchronize()
            kernels, others = _device_kernels(prof)
            counts.append((len(kernels), sum("attn_importance_kernel" in e.name for e in kernels), len(others)))
        (plain, _, plain_other), (fused_n, fused_ours, fused_other) = counts
        print(f"[attn] has_cls={has_cls}: model forward {plain} kernels, fused capture {fused_n} "
              f"({fused_ours} attn_importance_kernel)")
        assert fused_ours == (3 if seen else 0)
        assert fused_n - plain == fused_ours and fused_other == plain_other


@pytest.mark.gpu
def test_fused_capture_allocates_nothing_of_size_n_squared(dev):
    """CLS-less teacher, N = 576: across the whole fused capture (three hooked layers) the peak of allocated memory
    stays below the bytes of ONE layer's (B, H, N, N) fp32 map."""
    torch.manual_seed(5)
    model = _NoClsViT(img_size=96, patch_size=4, embed_dim=64, depth=3, num_heads=4).to(dev).eval()
    teacher = _teacher(model, 3, False, 64, 4)
    B, H, N = 4, 4, 576
    x = _images(B, 96, 2).to(dev)
    capture.extract_intermediates(teacher, x, attn="fused")              # warm-up: library workspaces
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    toks, attns = capture.extract_intermediates(teacher, x, attn="fused")
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - base
    one_map = B * H * N * N * 4
    print(f"[attn] fused capture of 3 layers: peak {peak / 2**20:.2f} MiB over the baseline, one map = "
          f"{one_map / 2**20:.2f} MiB")
    assert peak < one_map
    assert attns[0].shape == (B, H, N, N) and attns[0].stride(2) == 0 and attns[0].dtype == torch.float32
    full = capture.extract_intermediates(teacher, x, cls_row_only=False)[1]
    for i in range(3):
        torch.testing.assert_close(attns[i][:, :, 0, :], full[i].mean(dim=2), rtol=1e-4, atol=1e-6)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the loss and the trainer on fused captures
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("has_cls", [True, False], ids=["cls", "no_cls"])
def test_loss_on_fused_captures_equals_loss_on_full_maps(dev, has_cls):
    """BASDLoss on the fused captures and on the reference-form full maps of the same forward: loss within 1e-4,
    student gradients within 1e-3 relative norm (the parity tolerances of ``smoke()``), equal subspace ranks."""
    from basd_amd import trainer as T
    from tools import stock_models as SM
    student, teacher = _models(has_cls, dev)
    assert teacher.has_cls_token == has_cls and len(teacher.layer_paths) == 3
    torch.manual_seed(42)
    tr = T.Trainer(student, _config(), teacher, student_info=SM.probe_model(student, 32), mixup=False)
    clean, aug = _images(16, 32, 1).to(dev), _images(16, 32, 2).to(dev)
    targets = (torch.arange(16) % 10).to(dev)
    t_full = capture.extract_intermediates(teacher, clean, cls_row_only=False)
    t_fused = capture.extract_intermediates(teacher, clean, attn="fused")
    assert all(a.stride(2) == 0 for a in t_fused[1].values()) and all(a.stride(2) != 0 for a in t_full[1].values())
    results = []
    for t_tok, t_att in (t_full, t_fused):
        logits, s_tok = capture._extract_student(student, aug, tr.basd_loss.token_layers,
                                                 layer_paths=tr._student_layer_paths, has_cls_token=True)
        leaves = {k: v.detach().clone().requires_grad_(True) for k, v in s_tok.items()}
        loss = tr.basd_loss(logits.detach().float(), targets, leaves, t_tok, t_att)
        loss.backward()
        results.append((loss.item(), [leaves[l].grad.clone() for l in tr.basd_loss.token_layers],
                        dict(tr.basd_loss.layer_selector.subspace_ranks)))
    (l0, g0, r0), (l1, g1, r1) = results
    rel = abs(l1 - l0) / abs(l0)
    print(f"[attn] has_cls={has_cls}: loss full {l0:.6f} fused {l1:.6f} (rel {rel:.2e}), ranks {r1}")
    assert rel < 1e-4, (l0, l1)
    assert r0 == r1
    for a, b in zip(g0, g1):
        assert ((a - b).norm() / a.norm()).item() < 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("autocast", [None, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("has_cls", [True, False], ids=["cls", "no_cls"])
def test_train_step_fused_equals_torch(dev, has_cls, autocast):
    """``Trainer.train_step`` with ``attn_capture="fused"`` and with ``"torch"`` from the same seeds: the losses agree to
    1e-4 in fp32; under bf16 autocast the torch path rounds its map to bf16 and the fused path does not, so there the
    losses are required to be finite and are printed."""
    from basd_amd import trainer as T
    from tools import stock_models as SM
    batch = {"clean": _images(16, 32, 1), "augmented": _images(16, 32, 2), "label": torch.arange(16) % 10}
    losses = {}
    for mode in ("torch", "fused"):
        student, teacher = _models(has_cls, dev)
        torch.manual_seed(42)
        tr = T.Trainer(student, _config(), teacher, student_info=SM.probe_model(student, 32), mixup=False,
                       autocast_dtype=autocast, attn_capture=mode)
        assert tr.attn_capture == mode
        before = [p.detach().clone() for p in student.parameters()]
        losses[mode] = tr.train_step(batch)["loss"].item()
        assert any(not torch.equal(a, b) for a, b in zip(before, student.parameters()))
    rel = abs(losses["fused"] - losses["torch"]) / abs(losses["torch"])
    print(f"[attn] train_step has_cls={has_cls} autocast={autocast}: torch {losses['torch']:.6f} fused "
          f"{losses['fused']:.6f} (rel {rel:.2e})")
    assert all(torch.isfinite(torch.tensor(v)) for v in losses.values())
    if autocast is None:
        assert rel < 1e-4, losses
