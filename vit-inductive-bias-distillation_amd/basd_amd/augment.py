"""Batch preparation: the reference's ``RandomChoice([MixUp(alpha), CutMix(alpha)])`` (``src/training/trainer.py:89-92``),
the one-hot soft targets and -- for uint8 batches -- the loader's ``ToDtype(float32, scale=True)`` + ``Normalize`` as
ONE launch of ``basd_mix_batch`` (``csrc/mix.hip``): the image batch is read once and written once.

``draw_mix_params`` makes the random choices on the host (CPU generator); ``BatchMixer`` applies a ``MixParams`` record on
the device.  All scalars of a draw travel in the kernel arguments: a steady-state call makes no host-to-device copy,
no allocation on the device and never waits for it.  The arithmetic is fixed to single fp32 operations (contract in
``include/basd_hip.h``), so that the result equals torch's ``x.roll(1, 0).mul_(1 - lam).add_(x.mul(lam))`` bit for bit.

``torchvision`` is not installed where this was written: the order of the random draws (the choice by
``torch.multinomial``, one Beta(alpha, alpha) sample, then for CutMix ``randint(W)`` and ``randint(H)``), the box
arithmetic and the amount of RNG state each draw consumes are restated from the package's documentation and are NOT
verified against the package itself.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import math
from typing import NamedTuple, Optional, Tuple

import torch

from . import _lib
from ._launch import DTYPE_CODES, check_image_batch, check_out, lives_on, raw_stream, require_gpu

__all__ = ["MixParams", "draw_mix_params", "BatchMixer"]

_KINDS = {"none": 0, "mixup": 1, "cutmix": 2}
_OUT_DTYPES = (torch.float32, torch.bfloat16)
_MAX_STAT_CHANNELS = 4                                                      # BASD_MIX_MAX_STAT_CHANNELS


class MixParams(NamedTuple):
    """One draw.  ``kind``: ``"none"`` (convert / normalise only), ``"mixup"`` or ``"cutmix"``; ``lam``: the weight of
    the row itself (MixUp); ``box``: ``(x1, y1, x2, y2)``, half open, inside the image (CutMix); ``lam_targets``: the
    weight of the row's own label in the soft targets (``lam`` for MixUp, ``1 - box area / image area`` for CutMix, 1
    for ``"none"``)."""
    kind: str
    lam: float = 1.0
    box: Optional[Tuple[int, int, int, int]] = None
    lam_targets: float = 1.0


def draw_mix_params(height: int, width: int, *, alpha: float = 1.0, p=(0.5, 0.5), generator=None) -> MixParams:
    """``RandomChoice([MixUp(alpha), CutMix(alpha)], p=p)`` of ``torchvision.transforms.v2`` as a pure host function on
    the CPU generator (``generator=None``: the global one).  The draws, in order: the choice by ``torch.multinomial``
    over ``p`` (normalised), ONE Beta(alpha, alpha) sample (``torch.distributions.Beta``'s own sampler, a Dirichlet over
    ``[alpha, alpha]``), then for CutMix ``randint(width)`` and ``randint(height)``.  CutMix's box: ``r = 0.5 *
    sqrt(1 - lam)``, half sizes ``int(r * width)`` and ``int(r * height)`` around the drawn centre, corners clamped to
    ``[0, width]`` and ``[0, height]``, and ``lam`` adjusted to the clamped box.  Restated from the package's
    documentation; the order of draws and the RNG consumption are not verified against the package (not installed)."""
    height, width = int(height), int(width)
    if height < 1 or width < 1:
        raise ValueError(f"an image of {height} x {width} has no pixels")
    if not alpha > 0.0:
        raise ValueError(f"alpha must be positive (got {alpha})")
    weights = torch.tensor([float(v) for v in p], dtype=torch.float32)
    if weights.numel() != 2 or not (weights >= 0).all() or not weights.sum() > 0:
        raise ValueError(f"p must be two non-negative weights, not all zero (got {p})")
    choice = int(torch.multinomial(weights / weights.sum(), 1, generator=generator))
    concentration = torch.tensor([float(alpha), float(alpha)])
    lam = float(torch._sample_dirichlet(concentration, generator)[0])
    if choice == 0:
        return MixParams("mixup", lam, None, lam)
    r_x = int(torch.randint(width, (1,), generator=generator))
    r_y = int(torch.randint(height, (1,), generator=generator))
    r = 0.5 * math.sqrt(1.0 - lam)
    half_w, half_h = int(r * width), int(r * height)
    x1, y1 = max(r_x - half_w, 0), max(r_y - half_h, 0)
    x2, y2 = min(r_x + half_w, width), min(r_y + half_h, height)
    return MixParams("cutmix", lam, (x1, y1, x2, y2), float(1.0 - (x2 - x1) * (y2 - y1) / (width * height)))


class BatchMixer:
    """``BatchMixer(num_classes, mean=None, std=None, out_dtype=None, device=...)``.

    ``mixer(images, labels=None, params=None, out=None) -> (mixed, targets)``: ``images`` a dense NCHW batch, fp32 /
    bf16 / uint8, on ``device``; ``mixed`` has ``out_dtype`` (default: the images' dtype, fp32 for uint8).  uint8 images
    are scaled by 1 / 255 and normalised with the per-channel ``mean`` / ``std`` (at most 4 channels; without them:
    the plain scale); fp32 / bf16 images are taken as they are.  ``params=None`` draws with ``draw_mix_params`` (global
    CPU generator); ``MixParams("none")`` converts only.  ``labels`` (B,) int64 give the dense (B, num_classes) fp32 soft
    targets, ``labels=None`` gives ``targets = None``.  ``out``: a dense NCHW tensor to write into (it must not overlap
    ``images``: row i needs the original row i - 1).  Outputs come from torch's caching allocator; exactly one launch on
    the current stream per call, no wait for the device."""

    def __init__(self, num_classes: int, *, mean=None, std=None, out_dtype=None, alpha: float = 1.0, device) -> None:
        self.num_classes = int(num_classes)
        if self.num_classes < 1:
            raise ValueError(f"num_classes must be positive (got {num_classes})")
        if (mean is None) != (std is None):
            raise ValueError("mean and std come together")
        if out_dtype is not None and out_dtype not in _OUT_DTYPES:
            raise TypeError(f"out_dtype must be torch.float32 or torch.bfloat16 (got {out_dtype})")
        self.device = torch.device(device)
        self.out_dtype = out_dtype
        self.alpha = float(alpha)
        self.mean = self.std = None
        self._mean_c = self._std_c = None
        if mean is not None:
            self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
            if len(self.mean) != len(self.std) or not 1 <= len(self.mean) <= _MAX_STAT_CHANNELS:
                raise ValueError(f"mean / std must have the same length, 1 to {_MAX_STAT_CHANNELS} channels (got "
                                 f"{len(self.mean)} and {len(self.std)})")
            # host arrays: the values reach the kernel by value in its arguments
            self._mean_c = (ctypes.c_float * len(self.mean))(*self.mean)
            self._std_c = (ctypes.c_float * len(self.std))(*self.std)

    def __call__(self, images: torch.Tensor, labels=None, params: Optional[MixParams] = None, *, out=None):
        # every argument is checked before the device is: a CPU batch with a wrong argument reports the argument
        B, C, H, W = check_image_batch(images, DTYPE_CODES)
        if not lives_on(self.device, images.device):
            raise ValueError(f"images live on {images.device}, the mixer on {self.device}")
        use_stats = images.dtype == torch.uint8 and self.mean is not None
        if use_stats and len(self.mean) != C:
            raise ValueError(f"{len(self.mean)} channel statistics for images of shape {tuple(images.shape)}")
        out_dtype = self.out_dtype or (torch.float32 if images.dtype == torch.uint8 else images.dtype)
        if labels is not None:
            if labels.dtype != torch.int64:
                raise TypeError(f"labels must be int64 (got {labels.dtype})")
            if labels.shape != (B,) or (B > 1 and labels.stride(0) != 1):
                raise ValueError(f"labels must be a dense ({B},) tensor for images of shape {tuple(images.shape)} "
                                 f"(shape {tuple(labels.shape)})")
            if labels.device != images.device:
                raise ValueError(f"labels live on {labels.device}, images on {images.device}")
        if params is None:
            params = draw_mix_params(H, W, alpha=self.alpha)
        if params.kind not in _KINDS:
            raise ValueError(f"MixParams.kind must be one of {sorted(_KINDS)} (got {params.kind!r})")
        x1 = y1 = x2 = y2 = 0
        if params.kind == "cutmix":
            if params.box is None:
                raise ValueError("CutMix needs a box")
            x1, y1, x2, y2 = (int(v) for v in params.box)
            if not (0 <= x1 <= x2 <= W and 0 <= y1 <= y2 <= H):
                raise ValueError(f"box (x1, y1, x2, y2) = {params.box} does not lie inside a {H} x {W} image")
        if out is not None:
            check_out(out, images, _OUT_DTYPES, "row i needs the original row i - 1")
        require_gpu(images, f"images of shape {(B, C, H, W)}")
        if out is None:
            out = torch.empty((B, C, H, W), dtype=out_dtype, device=images.device)
        targets = None
        if labels is not None:
            targets = torch.empty((B, self.num_classes), dtype=torch.float32, device=images.device)
        _lib.call("basd_mix_batch", images.data_ptr(), DTYPE_CODES[images.dtype], out.data_ptr(), DTYPE_CODES[out.dtype],
                  B, C, H, W, _KINDS[params.kind], float(params.lam), y1, y2, x1, x2,
                  self._mean_c if use_stats else None, self._std_c if use_stats else None,
                  None if labels is None else labels.data_ptr(), self.num_classes, float(params.lam_targets),
                  None if targets is None else targets.data_ptr(), raw_stream(images.device.index))
        return out, targets
