"""Dataset statistics (``basd_amd.stats``, kernel in ``csrc/stats.hip``) and uint8 validation batches
(``evaluate_model(image_stats=...)``).

The kernel sums integers: every comparison of sums is ``==`` against numpy int64 sums, there is no tolerance.  Mean and
standard deviation are compared with an fp64 restatement, written here in numpy, of the running merge of the reference's
``get_channel_stats`` (``src/data/datasets.py:46-68``) to 1e-12 absolute: a few hundred merges at a relative error of
about 1e-16 each (observed on the inputs below: 3e-16).  Nothing here was run against the ``datasets`` package."""
import functools
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn

from basd_amd import _lib
from basd_amd import stats as S
from basd_amd.augment import BatchMixer, MixParams
from basd_amd.evaluation import evaluate_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
MEAN_T, STD_T = (0.5, 0.5, 0.5), (0.25, 0.5, 0.125)
OFFSETS = (0, 1, 2, 3)


# ---------------------------------------------------------------------------------------------------------------------
# the restatements
# ---------------------------------------------------------------------------------------------------------------------
def _reference_merge(arrays):
    """The loop body of the reference's ``get_channel_stats`` over HWC uint8 arrays, in fp64."""
    C = arrays[0].shape[-1]
    mean, m2, count = np.zeros(C, dtype=np.float64), np.zeros(C, dtype=np.float64), 0
    for a in arrays:
        flat = (np.asarray(a, dtype=np.float64) / 255.0).reshape(-1, C)
        n = flat.shape[0]
        batch_mean, batch_var = flat.mean(axis=0), flat.var(axis=0)
        delta = batch_mean - mean
        new_count = count + n
        mean += delta * n / new_count
        m2 += batch_var * n + delta ** 2 * count * n / new_count
        count = new_count
    return tuple(mean.tolist()), tuple(np.sqrt(m2 / count).tolist())


def _int_sums(pixels):
    """``(n, [sum x], [sum x^2])`` of a (n, C) array of uint8 values, in int64."""
    x = np.asarray(pixels).astype(np.int64)
    return x.shape[0], x.sum(axis=0).tolist(), (x * x).sum(axis=0).tolist()


@functools.lru_cache(maxsize=None)
def _ragged_arrays():
    """200 ragged random HWC images (sides 1 to 40), one all-255 image and one all-0 image."""
    rng = np.random.default_rng(20240607)
    arrays = [rng.integers(0, 256, (int(rng.integers(1, 41)), int(rng.integers(1, 41)), 3), dtype=np.uint8)
              for _ in range(200)]
    return tuple(arrays + [np.full((17, 9, 3), 255, dtype=np.uint8), np.zeros((5, 31, 3), dtype=np.uint8)])


def _close(got, want, tol=1e-12):
    assert len(got) == len(want)
    return max(abs(g - w) for g, w in zip(got, want)) <= tol


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_finish_by_hand_and_empty():
    assert S.finish(2, [255], [255 * 255]) == ((0.5,), (0.5,))                    # pixels [0, 255]
    assert S.finish(4, [4 * 255, 0], [4 * 255 * 255, 0]) == ((1.0, 0.0), (0.0, 0.0))
    mean, std = S.finish(0, [0, 0, 0], [0, 0, 0])
    assert len(mean) == len(std) == 3 and all(math.isnan(v) for v in mean + std)
    with pytest.raises(ValueError):
        S.finish(2, [255], [100])                                                 # not the sums of any two values


def test_finish_agrees_with_the_reference_merge():
    arrays = _ragged_arrays()
    n, s1, s2 = _int_sums(np.concatenate([a.reshape(-1, 3) for a in arrays]))
    mean, std = S.finish(n, s1, s2)
    ref_mean, ref_std = _reference_merge(arrays)
    print(f"[channel_stats] finish vs the fp64 merge: mean {max(abs(a - b) for a, b in zip(mean, ref_mean)):.2e}, "
          f"std {max(abs(a - b) for a, b in zip(std, ref_std)):.2e}")
    assert _close(mean, ref_mean) and _close(std, ref_std)
    assert all(0.0 <= v <= 1.0 for v in mean + std)


def test_argument_checks_on_cpu():
    cs = S.ChannelStats(3, device="cpu")
    x = torch.zeros(4, 5, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cs.update(x, "hwc")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cs.update(torch.zeros(2, 3, 4, 4, dtype=torch.uint8), "chw")
    with pytest.raises(TypeError, match="float32"):
        cs.update(x.float(), "hwc")
    for bad, layout in ((torch.zeros(4, 5, 4, dtype=torch.uint8), "hwc"),         # last axis is not `channels`
                        (torch.zeros(4, 5, 6, dtype=torch.uint8)[..., ::2], "hwc"),        # a strided view
                        (torch.zeros(4, 3, 5, dtype=torch.uint8).permute(0, 2, 1), "hwc"),
                        (torch.zeros(4, 4, 4, dtype=torch.uint8), "chw"),
                        (torch.zeros(2, 3, 4, 8, dtype=torch.uint8)[..., ::2], "chw"),
                        (torch.zeros(3, 4, dtype=torch.uint8), "chw"),
                        (x, "nhwc")):
        with pytest.raises(ValueError):
            cs.update(bad, layout)
    for channels in (0, 5):
        with pytest.raises(ValueError):
            S.ChannelStats(channels, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.channel_stats([np.zeros((2, 2, 3), dtype=np.uint8)], device="cpu")
    with pytest.raises(ValueError):
        S.channel_stats([], device="cpu", chunk_bytes=2)                          # not one pixel


def test_abi_agreement():
    with open(os.path.join(ROOT, "include", "basd_hip.h")) as f:
        header = f.read()
    assert "int basd_channel_stats(" in header
    assert "#define BASD_LAYOUT_HWC 0" in header and "#define BASD_LAYOUT_CHW 1" in header
    assert "datasets.py:46-68" in header and "max_blocks: test / tuning hook" in header
    vp, i32, i64 = _lib.vp, _lib.i32, _lib.i64
    assert _lib.SIGNATURES["basd_channel_stats"] == [vp, i32, i64, i32, i64, vp, i32, vp]
    assert S._LAYOUTS == {"hwc": 0, "chw": 1}


def test_uint8_validation_without_stats_raises_before_the_model():
    class Never(nn.Module):
        def __init__(self):
            super().__init__()
            self.w = nn.Parameter(torch.zeros(1))

        def forward(self, x):
            raise AssertionError("the model was reached")

    loader = [{"pixel_values": torch.zeros(7, 3, 8, 8, dtype=torch.uint8), "label": torch.zeros(7, dtype=torch.int64)}]
    with pytest.raises(TypeError, match=r"uint8.*\(7, 3, 8, 8\)"):
        evaluate_model(Never(), loader, nn.CrossEntropyLoss(), num_classes=10)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _launch(view, layout, images, C, pixels, state, max_blocks=0):
    _lib.call("basd_channel_stats", view.data_ptr(), S._LAYOUTS[layout], images, C, pixels, state.data_ptr(),
              max_blocks, torch._C._cuda_getCurrentRawStream(view.device.index))


def _fills(n, seed):
    rng = np.random.default_rng(seed)
    return {"random": rng.integers(0, 256, n, dtype=np.uint8), "all-255": np.full(n, 255, dtype=np.uint8),
            "all-0": np.zeros(n, dtype=np.uint8)}


def _expected_words(n, s1, s2):
    C = len(s1)
    return [n] + s1 + [0] * (4 - C) + s2 + [0] * (4 - C)


@pytest.mark.gpu
@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_hwc_exact(dev, C):
    """Views at byte offsets 0..3 (heads of 0, 15, 14, 13 bytes: every phase mod C), pixel counts around the 16-byte
    vector and the 48-byte group, up to six tiles.  The 4099-pixel cases are repeated with ``max_blocks`` 1 and 3; at
    that size the default grid is one workgroup already, so the grid changes only in the large cases below."""
    for pixels in (1, 5, 15, 16, 17, 47, 48, 49, 1000, 4099):
        n = pixels * C
        for name, data in _fills(n, 100 * C + pixels).items():
            want = _expected_words(*_int_sums(data.reshape(-1, C)))
            for off in OFFSETS:
                buf = torch.zeros(n + 16, dtype=torch.uint8)
                buf[off:off + n] = torch.from_numpy(data)
                buf = buf.to(dev)
                view = buf[off:off + n]
                assert view.data_ptr() % 4 == off
                for max_blocks in ((0, 1, 3) if pixels == 4099 else (0,)):
                    state = torch.zeros(9, dtype=torch.int64, device=dev)
                    _launch(view, "hwc", 1, C, pixels, state, max_blocks)
                    assert state.tolist() == want, (C, pixels, name, off, max_blocks)
    cs = S.ChannelStats(C, device=dev)
    cs.update(view.view(-1, C), "hwc")                                            # the class, on the last case
    assert cs.sums() == _int_sums(data.reshape(-1, C))


@pytest.mark.gpu
@pytest.mark.parametrize("C", [1, 3, 4])
def test_chw_exact(dev, C):
    """Planes whose starts fall at every byte alignment (odd plane sizes), one and three images."""
    for images in (1, 3):
        for plane in (1, 15, 16, 17, 63, 64, 65, 4099):
            n = images * C * plane
            for name, data in _fills(n, 1000 * C + 10 * plane + images).items():
                x = data.reshape(images, C, plane)
                want = _expected_words(*_int_sums(x.transpose(0, 2, 1).reshape(-1, C)))
                for off in OFFSETS:
                    buf = torch.zeros(n + 16, dtype=torch.uint8)
                    buf[off:off + n] = torch.from_numpy(data)
                    buf = buf.to(dev)
                    view = buf[off:off + n]
                    for max_blocks in ((0, 1, 3) if plane == 4099 else (0,)):
                        state = torch.zeros(9, dtype=torch.int64, device=dev)
                        _launch(view, "chw", images, C, plane, state, max_blocks)
                        assert state.tolist() == want, (C, images, plane, name, off, max_blocks)
    cs = S.ChannelStats(C, device=dev)
    cs.update(view.view(images, C, plane, 1), "chw")
    assert cs.sums() == _int_sums(x.transpose(0, 2, 1).reshape(-1, C))
    if images * C > 1:
        cs.reset()
        cs.update(view.view(images, C, plane, 1)[0], "chw")                       # (C, H, W)
        assert cs.sums() == _int_sums(x[:1].transpose(0, 2, 1).reshape(-1, C))


@pytest.mark.gpu
def test_every_head_length(dev):
    """Views at byte offsets 0..15 of a 16-byte-aligned buffer: heads of 0 and 15 down to 1 bytes, in both layouts (in
    CHW the plane size 1001 moves every plane's head as well)."""
    rng = np.random.default_rng(16)
    for layout, C, pixels in (("hwc", 3, 1100), ("hwc", 4, 777), ("hwc", 2, 50), ("chw", 3, 1001)):
        images = 2 if layout == "chw" else 1
        n = images * pixels * C
        data = rng.integers(0, 256, n, dtype=np.uint8)
        x = data.reshape(-1, C) if layout == "hwc" else data.reshape(images, C, pixels).transpose(0, 2, 1).reshape(-1, C)
        want = _expected_words(*_int_sums(x))
        for off in range(16):
            buf = torch.zeros(n + 32, dtype=torch.uint8)
            buf[off:off + n] = torch.from_numpy(data)
            buf = buf.to(dev)
            assert buf.data_ptr() % 16 == 0
            state = torch.zeros(9, dtype=torch.int64, device=dev)
            _launch(buf[off:off + n], layout, images, C, pixels, state)
            assert state.tolist() == want, (layout, C, pixels, off)


@functools.lru_cache(maxsize=None)
def _large_bytes():
    """24 MiB and a few odd bytes of random values, shared by the large cases (and their int64 view for the sums)."""
    data = np.random.default_rng(2024).integers(0, 256, (24 << 20) + 1212, dtype=np.uint8)
    return data, data.astype(np.int64)


@pytest.mark.gpu
@pytest.mark.parametrize("C", [2, 3, 4])
def test_hwc_exact_over_many_workgroups_and_tiles(dev, C):
    """About 24 MiB of interleaved pixels (8192 tiles of 3 KiB): the default grid has 512 workgroups and every
    wave walks one or two tiles with the grid stride; on 1, 5 and 64 workgroups a wave walks 512, 103 and 8 of them, so
    the 64-bit sums carried from tile to tile, the lane phase that must be the same in every iteration and the stride
    over the workgroups all count.  Views at byte offsets 0..3."""
    data, wide = _large_bytes()
    pixels = (24 << 20) // C + 101
    n = pixels * C
    assert n <= data.size - 3
    buf = torch.from_numpy(data).to(dev)
    for off in OFFSETS:
        x = wide[off:off + n].reshape(-1, C)
        want = _expected_words(pixels, x.sum(axis=0).tolist(), (x * x).sum(axis=0).tolist())
        view = buf[off:off + n]
        for max_blocks in (0, 1, 5, 64):
            state = torch.zeros(9, dtype=torch.int64, device=dev)
            _launch(view, "hwc", 1, C, pixels, state, max_blocks)
            assert state.tolist() == want, (C, off, max_blocks)
    cs = S.ChannelStats(C, device=dev)
    cs.update(view.view(-1, C), "hwc")
    assert cs.sums() == (want[0], want[1:1 + C], want[5:5 + C])


@pytest.mark.gpu
def test_chw_exact_over_many_workgroups_and_tiles(dev):
    """8 images of 3 planes of 1 000 003 bytes (326 tiles each; the odd size gives every plane another head), on the
    default grid and on 1, 5 and 64 workgroups."""
    data, wide = _large_bytes()
    images, C, plane = 8, 3, 1_000_003
    n = images * C * plane
    buf = torch.from_numpy(data).to(dev)
    for off in (0, 3):
        x = wide[off:off + n].reshape(images, C, plane)
        want = _expected_words(images * plane, x.sum(axis=(0, 2)).tolist(), (x * x).sum(axis=(0, 2)).tolist())
        for max_blocks in (0, 1, 5, 64):
            state = torch.zeros(9, dtype=torch.int64, device=dev)
            _launch(buf[off:off + n], "chw", images, C, plane, state, max_blocks)
            assert state.tolist() == want, (off, max_blocks)


@pytest.mark.gpu
def test_cpu_tensor_on_a_device_instance_raises(dev):
    """What a user hits: statistics on the GPU, a batch left on the host."""
    cs = S.ChannelStats(3, device=dev)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cs.update(torch.zeros(4, 5, 3, dtype=torch.uint8), "hwc")
    with pytest.raises(TypeError):
        cs.update(torch.zeros(4, 5, 3), "hwc")                                    # the argument is reported first
    assert cs.sums() == (0, [0, 0, 0], [0, 0, 0])


@pytest.mark.gpu
def test_updates_accumulate_and_reset_clears(dev):
    rng = np.random.default_rng(5)
    parts = [rng.integers(0, 256, (p, 3), dtype=np.uint8) for p in (7, 4099, 300)]
    cs = S.ChannelStats(3, device=dev)
    for p in parts:
        cs.update(torch.from_numpy(p).to(dev), "hwc")
    assert cs.sums() == _int_sums(np.concatenate(parts))
    batch = rng.integers(0, 256, (2, 3, 5, 7), dtype=np.uint8)
    cs.update(torch.from_numpy(batch).to(dev), "chw")                             # the layouts mix in one state
    assert cs.sums() == _int_sums(np.concatenate(parts + [batch.transpose(0, 2, 3, 1).reshape(-1, 3)]))
    mean, std = cs.compute()
    assert mean == S.finish(*cs.sums())[0] and len(std) == 3
    cs.reset()
    assert cs.sums() == (0, [0, 0, 0], [0, 0, 0])
    assert all(math.isnan(v) for v in cs.compute()[0])
    empty = torch.zeros(0, 3, dtype=torch.uint8, device=dev)
    cs.update(empty, "hwc")                                                       # nothing to add: no launch
    assert cs.sums() == (0, [0, 0, 0], [0, 0, 0])


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["hwc", "chw"])
def test_words_around_the_state_and_of_other_channels_are_untouched(dev, layout):
    rng = np.random.default_rng(9)
    C, pixels = 2, 1000
    data = rng.integers(0, 256, (pixels, C), dtype=np.uint8)
    src = torch.from_numpy(data if layout == "hwc" else np.ascontiguousarray(data.T)).to(dev)
    before = [-7, -7] + [100 + i for i in range(9)] + [-7, -7]
    big = torch.tensor(before, dtype=torch.int64, device=dev)
    _launch(src, layout, 1, C, pixels, big[2:11])
    n, s1, s2 = _int_sums(data)
    after = big.tolist()
    assert after[:2] == [-7, -7] and after[11:] == [-7, -7]
    assert after[2] == 100 + n                                                    # the launch ADDS
    assert after[3:5] == [101 + s1[0], 102 + s1[1]] and after[5:7] == [103, 104]
    assert after[7:9] == [105 + s2[0], 106 + s2[1]] and after[9:11] == [107, 108]


@pytest.mark.gpu
def test_invalid_arguments_are_refused_by_the_library(dev):
    x = torch.zeros(64, dtype=torch.uint8, device=dev)
    state = torch.zeros(9, dtype=torch.int64, device=dev)
    stream = torch._C._cuda_getCurrentRawStream(dev.index)
    for layout, images, C, pixels, max_blocks in ((0, 1, 0, 8, 0), (0, 1, 5, 8, 0), (2, 1, 3, 8, 0), (0, -1, 3, 8, 0),
                                                  (1, 1, 3, -8, 0), (0, 1, 3, 8, -1)):
        with pytest.raises(RuntimeError, match="invalid argument"):
            _lib.call("basd_channel_stats", x.data_ptr(), layout, images, C, pixels, state.data_ptr(), max_blocks, stream)
    _lib.call("basd_channel_stats", x.data_ptr(), 0, 0, 3, 8, state.data_ptr(), 0, stream)        # empty: returns 0
    _lib.call("basd_channel_stats", x.data_ptr(), 1, 4, 3, 0, state.data_ptr(), 0, stream)
    assert state.tolist() == [0] * 9


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["hwc", "chw"])
def test_narrow_partials_do_not_overflow(dev, layout):
    """96 MiB of value 255 on ONE workgroup: at least 98 304 bytes per thread for any block of up to 1024 threads, past
    the 66 052 at which a 32-bit sum of squares wraps."""
    n = 96 << 20
    x = torch.full((n,), 255, dtype=torch.uint8, device=dev)
    state = torch.zeros(9, dtype=torch.int64, device=dev)
    _launch(x, layout, 1, 1, n, state, max_blocks=1)
    assert state.tolist() == [n, n * 255, 0, 0, 0, n * 65025, 0, 0, 0]


@pytest.mark.gpu
def test_one_launch_and_no_copy_per_update(dev):
    """A steady-state ``update`` is one kernel launch: no memcpy, no memset, no allocation on the device.  Counted with
    ``torch.profiler`` where it sees launches made through ctypes (the output says whether it does); the allocator's
    counter is checked either way."""
    from torch.profiler import ProfilerActivity, profile
    g = torch.Generator().manual_seed(5)
    batches = [torch.randint(0, 256, (16, 3, 64, 64), generator=g, dtype=torch.uint8).to(dev),
               torch.randint(0, 256, (999, 3), generator=g, dtype=torch.uint8).to(dev)]
    cs = S.ChannelStats(3, device=dev)
    for i in range(6):
        cs.update(batches[i % 2], ("chw", "hwc")[i % 2])
    torch.cuda.synchronize()
    device_allocations = torch.cuda.memory_stats(dev)["num_device_alloc"]
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for i in range(20):
            cs.update(batches[i % 2], ("chw", "hwc")[i % 2])
        torch.cuda.synchronize()
    assert torch.cuda.memory_stats(dev)["num_device_alloc"] == device_allocations
    device_events = [e for e in prof.events() if "cuda" in str(e.device_type).lower()]
    host_names = {e.name for e in prof.events() if "cuda" not in str(e.device_type).lower()}
    others = [e for e in prof.events() if "memcpy" in e.name.lower() or "memset" in e.name.lower()]
    kernels = [e for e in device_events if e.name not in host_names and e not in others]
    ours = [e for e in kernels if "channel_stats_kernel" in e.name]
    if ours:
        print(f"[channel_stats] profiler: {len(kernels)} kernels ({len(ours)} channel_stats_kernel), {len(others)} "
              "memcpy / memset in 20 updates")
        assert len(ours) == 20 and len(kernels) == 20, sorted({e.name for e in kernels})
        assert not others, sorted({e.name for e in others})
    else:
        print("[channel_stats] the profiler does not see the ctypes launches here "
              f"({len(kernels)} device kernels, {len(others)} memcpy / memset events seen by it)")
        assert not kernels and not others


@pytest.mark.gpu
def test_channel_stats_over_a_ragged_list(dev):
    """numpy arrays, CPU tensors, RGB PIL images and one mode-L PIL image through chunks of 1000 bytes (999 after
    rounding to whole pixels): smaller than most images, so images are split, and only between pixels."""
    from PIL import Image
    arrays = list(_ragged_arrays()[:39])
    rng = np.random.default_rng(77)
    gray = rng.integers(0, 256, (23, 11), dtype=np.uint8)
    items, rgb = [], []
    for i, a in enumerate(arrays):
        items.append(a if i % 3 == 0 else torch.from_numpy(a.copy()) if i % 3 == 1 else Image.fromarray(a))
        rgb.append(a)
    items.insert(20, Image.fromarray(gray))
    rgb.insert(20, np.repeat(gray[:, :, None], 3, axis=2))                        # what .convert("RGB") makes of it
    assert len(items) == 40 and np.array_equal(np.asarray(items[20].convert("RGB")), rgb[20])
    want = _int_sums(np.concatenate([a.reshape(-1, 3) for a in rgb]))
    cs = S.ChannelStats(3, device=dev)
    cs.stream(iter(items), chunk_bytes=1000)
    assert cs.sums() == want
    mean, std = S.channel_stats(iter(items), device=dev, chunk_bytes=1000)
    assert (mean, std) == S.finish(*want)
    ref_mean, ref_std = _reference_merge(rgb)
    assert _close(mean, ref_mean) and _close(std, ref_std)
    one = S.ChannelStats(1, device=dev)                                           # a mode-L image as one channel
    one.stream([Image.fromarray(gray), gray[:, :, None]], chunk_bytes=100)
    n, s1, s2 = _int_sums(gray.reshape(-1, 1))
    assert one.sums() == (2 * n, [2 * s1[0]], [2 * s2[0]])


# ---------------------------------------------------------------------------------------------------------------------
# GPU: uint8 validation batches
# ---------------------------------------------------------------------------------------------------------------------
def _uint8_loader(sizes, side, seed):
    g = torch.Generator().manual_seed(seed)
    return [{"pixel_values": torch.randint(0, 256, (b, 3, side, side), generator=g, dtype=torch.uint8),
             "label": torch.randint(0, 10, (b,), generator=g)} for b in sizes]


def _converted(loader, dev, mean, std, dtype):
    mixer = BatchMixer(10, mean=mean, std=std, out_dtype=dtype, device=dev)
    return [{"pixel_values": mixer(b["pixel_values"].to(dev), None, MixParams("none"))[0], "label": b["label"]}
            for b in loader]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [None, torch.bfloat16], ids=["fp32", "bf16"])
def test_evaluate_model_uint8_equals_converted_float(dev, dtype):
    """The model sees the same bits either way and the counters are integers: the two dicts are identical."""
    torch.manual_seed(11)
    model = nn.Sequential(nn.Flatten(), nn.Linear(3 * 8 * 8, 10)).to(dev)
    if dtype is not None:
        model = model.to(dtype)
    loader = _uint8_loader((7, 5), 8, 3)
    criterion = nn.CrossEntropyLoss(label_smoothing=0.1)
    raw = evaluate_model(model, loader, criterion, num_classes=10, image_stats=(MEAN, STD), input_dtype=dtype)
    floats = _converted(loader, dev, MEAN, STD, dtype)
    assert floats[0]["pixel_values"].dtype == (dtype or torch.float32)
    # image_stats and input_dtype are ignored for float batches
    for kw in ({}, {"image_stats": (MEAN_T, STD_T), "input_dtype": dtype}):
        assert evaluate_model(model, floats, criterion, num_classes=10, **kw) == raw
    assert 0.0 <= raw["val_acc"] <= raw["val_acc_top5"] <= 100.0 and math.isfinite(raw["loss"])
    with pytest.raises(TypeError, match="uint8"):
        evaluate_model(model, loader, criterion, num_classes=10)


@pytest.mark.gpu
def test_trainer_evaluate_takes_a_uint8_loader(dev):
    from basd_amd import trainer as T
    from tools import stock_models as SM
    torch.manual_seed(3)
    student = SM.StockViT(img_size=32, patch_size=8, embed_dim=48, depth=6, num_heads=4, num_classes=10).to(dev)
    teacher = SM.make_teacher(SM.StockViT(img_size=32, patch_size=8, embed_dim=64, depth=3, num_heads=4,
                                          num_classes=0).to(dev), 32)
    cfg = SimpleNamespace(training=SimpleNamespace(label_smoothing=0.1, learning_rate=1e-3, weight_decay=0.05),
                          basd=SimpleNamespace(num_extraction_points=4), model=SimpleNamespace(num_classes=10))
    stats = {"clean": (MEAN_T, STD_T), "augmented": (MEAN, STD)}
    info = SM.probe_model(student, 32)
    tr = T.Trainer(student, cfg, teacher, student_info=info, mixup="fused", image_stats=stats)
    loader = _uint8_loader((6, 3), 32, 4)
    out = tr.evaluate(student, loader)
    # the dataset's own (augmented) statistics, not the teacher's
    assert out == evaluate_model(student, _converted(loader, dev, MEAN, STD, None), tr.criterion, num_classes=10)
    assert out != evaluate_model(student, _converted(loader, dev, MEAN_T, STD_T, None), tr.criterion, num_classes=10)
    assert math.isfinite(out["loss"])
    plain = T.Trainer(student, cfg, teacher, student_info=info, mixup="fused")
    with pytest.raises(TypeError, match="uint8"):
        plain.evaluate(student, loader)
