"""Dataset statistics: the reference's ``get_channel_stats`` (``src/data/datasets.py:46-68``) -- per-channel mean and
standard deviation of a stream of images -- with the reduction as ONE launch of ``basd_channel_stats``
(``csrc/stats.hip``) per chunk of bytes, and exact.

``ChannelStats`` owns nine int64 words on the device: ``[pixels, sum of x per channel (4 words), sum of x^2 per channel
(4 words)]`` of the raw uint8 values.  They are summed with integer atomics, so the state is the same bits whatever the
order of arrival, the launch geometry, the cutting into chunks or the number of updates.  ``finish`` forms mean and
standard deviation from them in exact integer / rational arithmetic and rounds once; the reference merges per-image
fp64 means and variances with Chan's update, which agrees to a few 1e-16 (``tests/test_channel_stats.py``).

``channel_stats`` (``ChannelStats.stream``) streams an iterable of images of any sizes through pinned staging
buffers.  Nothing here was run against the ``datasets`` package or real dataset files.  There is no CPU fallback.
"""
from __future__ import annotations

import math
from fractions import Fraction
from typing import Iterable, Sequence, Tuple

import torch

from . import _lib
from ._launch import lives_on, raw_stream, require_gpu

__all__ = ["ChannelStats", "channel_stats", "finish"]

_LAYOUTS = {"hwc": 0, "chw": 1}                 # BASD_LAYOUT_* of include/basd_hip.h
_MAX_CHANNELS = 4
_ROOT_BITS = 64                                 # extra bits the integer square root is taken at


def finish(n: int, s1: Sequence[int], s2: Sequence[int]) -> Tuple[Tuple[float, ...], Tuple[float, ...]]:
    """``(mean, std)`` in [0, 1] scale from the pixel count and the per-channel integer sums of x and x^2 over uint8
    values: ``mean = S1 / (255 n)``, ``std = sqrt(n S2 - S1^2) / (255 n)`` (the population variance, the reference's
    ``m2 / count``).  Both are formed exactly -- the square root as an integer root at 64 extra bits, below 2^-64
    relative -- and rounded to a double once.  ``n == 0`` gives NaNs."""
    n = int(n)
    if n < 0:
        raise ValueError(f"a pixel count cannot be negative (got {n})")
    if n == 0:
        return (float("nan"),) * len(s1), (float("nan"),) * len(s1)
    scale = 255 * n
    mean, std = [], []
    for a, b in zip(s1, s2):
        a, b = int(a), int(b)
        spread = n * b - a * a
        if spread < 0:
            raise ValueError(f"n = {n}, sum = {a}, sum of squares = {b} are not the sums of any {n} values")
        mean.append(float(Fraction(a, scale)))
        std.append(float(Fraction(math.isqrt(spread << (2 * _ROOT_BITS)), scale << _ROOT_BITS)))
    return tuple(mean), tuple(std)


class ChannelStats:
    """``ChannelStats(channels=3, device=...)``.

    ``update(images, layout)``: ``images`` a dense uint8 tensor on ``device``; ``layout="hwc"``: shape ``(..., C)``
    (one image, a stack, or any concatenation of ragged images flattened to ``(pixels, C)``); ``layout="chw"``: shape
    ``(C, H, W)`` or ``(N, C, H, W)``.  The layout is always named: a ``(3, 3, 3)`` tensor is both.  A view at any byte
    offset is read in place.  One launch on the current stream, no allocation, no copy, no wait for the device.
    ``sums()`` is the one device-to-host copy; ``compute()`` is ``finish(*sums())``."""

    def __init__(self, channels: int = 3, *, device) -> None:
        self.channels = int(channels)
        if not 1 <= self.channels <= _MAX_CHANNELS:
            raise ValueError(f"channels must be 1 to {_MAX_CHANNELS} (got {channels})")
        self.device = torch.device(device)
        self.state = torch.zeros(1 + 2 * _MAX_CHANNELS, dtype=torch.int64, device=self.device)

    def reset(self) -> None:
        self.state.zero_()

    def update(self, images: torch.Tensor, layout: str) -> None:
        # every argument is checked before the device is: a CPU tensor with a wrong argument reports the argument
        if layout not in _LAYOUTS:
            raise ValueError(f"layout must be 'hwc' or 'chw' (got {layout!r})")
        if images.dtype != torch.uint8:
            raise TypeError(f"images must be uint8 (got {images.dtype}, shape {tuple(images.shape)})")
        C = self.channels
        shape = tuple(images.shape)
        if layout == "hwc":
            if images.dim() < 1 or shape[-1] != C:
                raise ValueError(f"layout 'hwc' needs shape (..., {C}) (shape {shape})")
            count, pixels = 1, images.numel() // C
        else:
            if images.dim() not in (3, 4) or shape[-3] != C:
                raise ValueError(f"layout 'chw' needs shape ({C}, H, W) or (N, {C}, H, W) (shape {shape})")
            count, pixels = (shape[0] if images.dim() == 4 else 1), shape[-2] * shape[-1]
        if not images.is_contiguous():
            raise ValueError(f"images must be dense in the order of their axes (shape {shape}, strides "
                             f"{images.stride()})")
        require_gpu(images, f"images of shape {shape}")
        if not lives_on(self.device, images.device):
            raise ValueError(f"images live on {images.device}, the statistics on {self.device}")
        _lib.call("basd_channel_stats", images.data_ptr(), _LAYOUTS[layout], count, C, pixels, self.state.data_ptr(),
                  0, raw_stream(images.device.index))

    def stream(self, images: Iterable, *, chunk_bytes: int = 64 << 20) -> None:
        """Add an iterable of PIL images, HWC uint8 numpy arrays or HWC uint8 CPU tensors of any sizes.  PIL images go
        through ``.convert("RGB")`` when ``channels == 3``.  The bytes are concatenated into two pinned staging buffers
        of ``chunk_bytes`` (rounded down to whole pixels) that alternate: a filled buffer is copied to the device
        asynchronously and reduced by one launch while the host fills the other, and an event per buffer is waited on
        before it is filled again.  An image may be split across chunks, but only between pixels (a chunk that started
        inside a pixel would rotate the channels)."""
        channels = self.channels
        chunk = int(chunk_bytes) - int(chunk_bytes) % channels
        if chunk < channels:
            raise ValueError(f"chunk_bytes = {chunk_bytes} does not hold one pixel of {channels} channels")
        require_gpu(self.device, "the statistics")
        staging = [torch.empty(chunk, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
        free = [None, None]                                               # event: the buffer's copy has left it
        on_device = torch.empty(chunk, dtype=torch.uint8, device=self.device)
        cur, fill = 0, 0

        def flush():
            nonlocal cur, fill
            with torch.cuda.device(self.device):
                # one stream: the copy waits for the launch that read the previous chunk from the same device buffer
                on_device[:fill].copy_(staging[cur][:fill], non_blocking=True)
                free[cur] = torch.cuda.Event()
                free[cur].record()
                self.update(on_device[:fill].view(-1, channels), "hwc")
            cur, fill = cur ^ 1, 0

        for item in images:
            flat = _hwc_bytes(item, channels)
            done, size = 0, flat.numel()
            while done < size:
                if fill == 0 and free[cur] is not None:
                    free[cur].synchronize()
                # fill, done, size and chunk are whole pixels, so every cut falls between pixels
                take = min(chunk - fill, size - done)
                staging[cur][fill:fill + take].copy_(flat[done:done + take])
                fill, done = fill + take, done + take
                if fill == chunk:
                    flush()
        if fill:
            flush()

    def sums(self):
        """``(n, [sum of x per channel], [sum of x^2 per channel])`` as Python ints."""
        words = self.state.tolist()
        C = self.channels
        return words[0], words[1:1 + C], words[1 + _MAX_CHANNELS:1 + _MAX_CHANNELS + C]

    def compute(self):
        """``(mean, std)``: two tuples of ``channels`` floats in [0, 1] scale; NaNs before the first pixel."""
        return finish(*self.sums())


def _hwc_bytes(item, channels: int) -> torch.Tensor:
    """The bytes of one image as a flat uint8 CPU tensor, a whole number of pixels."""
    import numpy as np
    if hasattr(item, "convert") and hasattr(item, "mode"):                # a PIL image
        if channels == 3:
            item = item.convert("RGB")                                    # as the reference does
        item = np.array(item)                                             # a writable copy: np.asarray's is read-only
    if isinstance(item, np.ndarray):
        if item.dtype != np.uint8:
            raise TypeError(f"images must be uint8 (got a {item.dtype} array of shape {item.shape})")
        item = torch.from_numpy(np.ascontiguousarray(item))
    if not isinstance(item, torch.Tensor):
        raise TypeError(f"images must be PIL images, numpy arrays or tensors (got {type(item).__name__})")
    if item.dtype != torch.uint8:
        raise TypeError(f"images must be uint8 (got {item.dtype}, shape {tuple(item.shape)})")
    if item.device.type != "cpu":
        raise ValueError(f"channel_stats streams images from the host (got one on {item.device}); statistics of a "
                         "batch on the device: ChannelStats.update")
    if item.dim() == 2 and channels == 1:
        item = item.unsqueeze(-1)                                         # a mode-L image as numpy gives it
    if item.dim() != 3 or item.shape[-1] != channels:
        raise ValueError(f"images must be (H, W, {channels}) (shape {tuple(item.shape)})")
    return item.contiguous().view(-1)


def channel_stats(images: Iterable, *, device, channels: int = 3, chunk_bytes: int = 64 << 20):
    """``(mean, std)`` of an iterable of PIL images, HWC uint8 numpy arrays or HWC uint8 CPU tensors of any sizes: the
    loop of the reference's ``get_channel_stats`` (``ChannelStats.stream`` on a fresh state, then ``compute()``)."""
    stats = ChannelStats(channels, device=device)
    stats.stream(images, chunk_bytes=chunk_bytes)
    return stats.compute()
