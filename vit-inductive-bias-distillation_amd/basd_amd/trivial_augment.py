"""The reference's ``RandomHorizontalFlip -> TrivialAugmentWide`` of its training transform (``src/data/datasets.py:137-144``)
on uint8 batches as ONE launch of ``basd_trivial_augment`` (``csrc/taug.hip``): one workgroup per image, the image
staged in LDS, every byte of the output written once.  With it the loader decodes, crops and hands over bytes; the
``ToImage -> ToDtype -> Normalize`` tail is already part of ``basd_amd.augment.BatchMixer``'s launch.

``draw_augment_params`` makes the random choices on the host (CPU generator); ``TrivialAugment`` turns an
``AugmentParams`` record into a table of fixed-size records (``BasdTaugRecord`` of ``include/basd_hip.h``, which also
holds the specification of every operation), sends it with one non-blocking copy and launches once.

The operations are ``torchvision.transforms.v2.TrivialAugmentWide._AUGMENTATION_SPACE`` with 31 bins, nearest
interpolation and fill 0, restated from the package's documentation; ``torchvision`` is not installed where this was
written, so the order of the draws, the RNG consumption and the sign conventions of the affine operations are NOT
verified against the package.  What is verified: the specification equals Pillow (``ImageEnhance``, ``ImageOps``,
``Image.transform``, ``Image.rotate``) bit for bit -- for rotations away from rounding boundaries of the source
coordinate -- and the kernel equals the specification bit for bit (``tests/test_trivial_augment.py``).  The reference
draws per image inside its loader's worker processes, each with its own generator state: no seed reproduces its
sequence, here or there.  There is no CPU fallback.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from ._launch import RecordTable, batch_columns, check_image_batch, check_out, lives_on, raw_stream, require_gpu

__all__ = ["OPS", "AugmentParams", "draw_augment_params", "posterize_bits", "magnitude", "make_records", "RECORD_DTYPE",
           "TrivialAugment"]

OPS = ("Identity", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color", "Contrast",
       "Sharpness", "Posterize", "Solarize", "AutoContrast", "Equalize")            # BASD_TAUG_* of include/basd_hip.h
(IDENTITY, SHEAR_X, SHEAR_Y, TRANSLATE_X, TRANSLATE_Y, ROTATE, BRIGHTNESS, COLOR, CONTRAST, SHARPNESS, POSTERIZE,
 SOLARIZE, AUTOCONTRAST, EQUALIZE) = range(14)
SIGNED = frozenset((SHEAR_X, SHEAR_Y, TRANSLATE_X, TRANSLATE_Y, ROTATE, BRIGHTNESS, COLOR, CONTRAST, SHARPNESS))
NUM_BINS = 31
_RANGE = {SHEAR_X: 0.99, SHEAR_Y: 0.99, TRANSLATE_X: 32.0, TRANSLATE_Y: 32.0, ROTATE: 135.0, BRIGHTNESS: 0.99,
          COLOR: 0.99, CONTRAST: 0.99, SHARPNESS: 0.99}

# BasdTaugRecord: 64 bytes
RECORD_DTYPE = np.dtype([("op", "<i4"), ("flip", "<i4"), ("iarg", "<i4"), ("farg", "<f4"), ("a", "<f8", (6,))])
assert RECORD_DTYPE.itemsize == 64


class AugmentParams(NamedTuple):
    """Per-sample draws, (B,) each: ``op`` in [0, 14) (index into ``OPS``), ``bin`` in [0, num_bins), ``sign`` (True
    negates the magnitude of a signed op; ignored by Identity, Posterize, Solarize, AutoContrast, Equalize) and ``flip``
    (the horizontal flip, applied before the op).  int64 / bool CPU tensors, or anything ``torch.as_tensor`` takes."""
    op: torch.Tensor
    bin: torch.Tensor
    sign: torch.Tensor
    flip: torch.Tensor


def draw_augment_params(batch: int, *, flip_p: float = 0.5, num_bins: int = NUM_BINS, generator=None) -> AugmentParams:
    """``RandomHorizontalFlip(flip_p)`` and ``TrivialAugmentWide(num_magnitude_bins=num_bins)`` for ``batch`` samples as
    a pure host function on the CPU generator (``generator=None``: the global one).  Per sample, in the order of
    ``TrivialAugmentWide.forward``: ``randint(14)`` (the op), ``randint(num_bins)`` (the bin), ``rand() <= 0.5`` (negates
    a signed op), and then ``rand() < flip_p`` (the flip; the reference flips first, but no seed reproduces its
    sequence anyway: it draws per image inside worker processes).  Vectorised over the batch: four calls of the
    generator, each for all samples."""
    batch = int(batch)
    if batch < 0:
        raise ValueError(f"batch must not be negative (got {batch})")
    if not 0.0 <= float(flip_p) <= 1.0:
        raise ValueError(f"flip_p must lie in [0, 1] (got {flip_p})")
    if int(num_bins) != NUM_BINS:
        raise ValueError(f"the magnitude tables are those of {NUM_BINS} bins (got num_bins={num_bins})")
    op = torch.randint(len(OPS), (batch,), generator=generator)
    bin_ = torch.randint(NUM_BINS, (batch,), generator=generator)
    sign = torch.rand(batch, generator=generator) <= 0.5
    flip = torch.rand(batch, generator=generator) < float(flip_p)
    return AugmentParams(op, bin_, sign, flip)


def posterize_bits() -> torch.Tensor:
    """The bits kept by Posterize per bin: ``(8 - (arange(31) / ((31 - 1) / 6))).round().int()``."""
    return (8 - (torch.arange(NUM_BINS) / ((NUM_BINS - 1) / 6))).round().int()


_LINSPACE = {}


def _linspace(lo: float, hi: float) -> list:
    key = (lo, hi)
    if key not in _LINSPACE:
        _LINSPACE[key] = [float(v) for v in torch.linspace(lo, hi, NUM_BINS)]
    return _LINSPACE[key]


def magnitude(op: int, bin_: int, sign: bool) -> float:
    """The magnitude of ``(op, bin, sign)`` as torchvision forms it: ``float(torch.linspace(0, range, 31)[bin])``
    (an fp32 value read as a Python float), negated by ``sign`` for the signed ops; Posterize: the bits; Solarize:
    ``255 * float(linspace(1, 0, 31)[bin])`` (the threshold for uint8); 0 for ops without a magnitude."""
    op, bin_ = int(op), int(bin_)
    if not 0 <= op < len(OPS) or not 0 <= bin_ < NUM_BINS:
        raise ValueError(f"op must lie in [0, {len(OPS)}) and bin in [0, {NUM_BINS}) (got {op}, {bin_})")
    if op in SIGNED:
        m = _linspace(0.0, _RANGE[op])[bin_]
        return -m if sign else m
    if op == POSTERIZE:
        if "bits" not in _LINSPACE:
            _LINSPACE["bits"] = posterize_bits().tolist()
        return float(_LINSPACE["bits"][bin_])
    if op == SOLARIZE:
        return 255.0 * _linspace(1.0, 0.0)[bin_]
    return 0.0


def rotation_matrix(degrees: float, height: int, width: int) -> tuple:
    """The inverse map of ``PIL.Image.rotate(degrees, NEAREST, expand=False)`` for a ``height`` x ``width`` image.
    0: the identity; 180, and 90 / 270 on a square image (Pillow transposes there): exact integer maps."""
    angle = degrees % 360.0
    w, h = float(width), float(height)
    if angle == 0.0:
        return (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
    if angle == 180.0:
        return (-1.0, 0.0, w, 0.0, -1.0, h)
    if angle == 90.0 and height == width:
        return (0.0, -1.0, w, 1.0, 0.0, 0.0)
    if angle == 270.0 and height == width:
        return (0.0, 1.0, 0.0, -1.0, 0.0, h)
    r = -math.radians(angle)
    m = [round(math.cos(r), 15), round(math.sin(r), 15), 0.0, round(-math.sin(r), 15), round(math.cos(r), 15), 0.0]
    cx, cy = w / 2.0, h / 2.0
    m[2] = (m[0] * -cx + m[1] * -cy + m[2]) + cx
    m[5] = (m[3] * -cx + m[4] * -cy + m[5]) + cy
    return tuple(m)


def affine_matrix(op: int, m: float, height: int, width: int) -> tuple:
    """The inverse affine map ``(a0..a5)`` of ops 0-5 at magnitude ``m`` (doubles; the table in include/basd_hip.h)."""
    if op == SHEAR_X:
        return (1.0, m, 0.0, 0.0, 1.0, 0.0)
    if op == SHEAR_Y:
        return (1.0, 0.0, 0.0, m, 1.0, 0.0)
    if op == TRANSLATE_X:
        return (1.0, 0.0, -float(int(m)), 0.0, 1.0, 0.0)
    if op == TRANSLATE_Y:
        return (1.0, 0.0, 0.0, 0.0, 1.0, -float(int(m)))
    if op == ROTATE:
        return rotation_matrix(m, height, width)
    return (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def _check_params(params: AugmentParams, batch: int):
    cols = batch_columns(params, batch, {"op": torch.int64, "bin": torch.int64, "sign": torch.bool, "flip": torch.bool})
    for name, limit in (("op", len(OPS)), ("bin", NUM_BINS)):
        if batch and (min(cols[name]) < 0 or max(cols[name]) >= limit):
            raise ValueError(f"AugmentParams.{name} must lie in [0, {limit}) (got {min(cols[name])}..{max(cols[name])})")
    return cols["op"], cols["bin"], cols["sign"], cols["flip"]


def make_records(params: AugmentParams, height: int, width: int, out: Optional[np.ndarray] = None) -> np.ndarray:
    """The record table of ``params`` for images of ``height`` x ``width``: a ``RECORD_DTYPE`` array of B entries
    (written into ``out`` if given).  Matrices come from ``math`` in double, magnitudes from ``magnitude``."""
    return _records_of(*_check_params(params, int(torch.as_tensor(params.op).numel())), height, width, out)


def _records_of(ops: list, bins: list, signs: list, flips: list, height: int, width: int, out) -> np.ndarray:
    batch = len(ops)
    rec = np.zeros(batch, dtype=RECORD_DTYPE) if out is None else out
    if rec.shape != (batch,) or rec.dtype != RECORD_DTYPE:
        raise ValueError(f"out must hold {batch} records")
    iargs, fargs, mats = [0] * batch, [0.0] * batch, [None] * batch
    for i, (op, bin_, sign) in enumerate(zip(ops, bins, signs)):
        m = magnitude(op, bin_, sign)
        if op in (BRIGHTNESS, COLOR, CONTRAST, SHARPNESS):
            fargs[i] = 1.0 + m
        elif op == POSTERIZE:
            iargs[i] = int(m)
        elif op == SOLARIZE:
            fargs[i] = m
        mats[i] = affine_matrix(op, m, height, width)
    if batch:
        rec["op"], rec["flip"], rec["iarg"], rec["farg"], rec["a"] = ops, flips, iargs, fargs, mats
    return rec


class TrivialAugment:
    """``TrivialAugment(device=..., flip_p=0.5)``.

    ``aug(images, params=None, *, out=None) -> uint8 batch``: ``images`` a dense NCHW uint8 batch with 1 or 3
    channels on ``device``; ``params=None`` draws with ``draw_augment_params`` (global CPU generator).  ``out``: a dense
    uint8 tensor of the same shape to write into; it must not overlap ``images``.  The record table is built in a
    pinned host buffer and sent with one non-blocking copy into a persistent device table (both grow to the largest
    batch seen); then exactly one launch on the current stream, no wait for the device.  ``status()`` reads the
    kernel's status word back (0: clean; it waits for the device)."""

    def __init__(self, *, device, flip_p: float = 0.5) -> None:
        self.device = torch.device(device)
        self.flip_p = float(flip_p)
        if not 0.0 <= self.flip_p <= 1.0:
            raise ValueError(f"flip_p must lie in [0, 1] (got {flip_p})")
        self._records = RecordTable(RECORD_DTYPE)

    def status(self) -> int:
        return self._records.status()

    def __call__(self, images: torch.Tensor, params: Optional[AugmentParams] = None, *, out=None) -> torch.Tensor:
        # every argument is checked before the device is: a CPU batch with a wrong argument reports the argument
        B, C, H, W = check_image_batch(images, (torch.uint8,), channels=(1, 3))
        if not lives_on(self.device, images.device):
            raise ValueError(f"images live on {images.device}, the augmenter on {self.device}")
        if out is not None:
            check_out(out, images, (torch.uint8,), "an output pixel reads source pixels anywhere in its image")
        if params is None:
            params = draw_augment_params(B, flip_p=self.flip_p)
        columns = _check_params(params, B)
        require_gpu(images, f"images of shape {(B, C, H, W)}")
        if out is None:
            out = torch.empty_like(images)
        if B == 0 or images.numel() == 0:
            return out
        _records_of(*columns, H, W, self._records.stage(B, images.device))
        _lib.call("basd_trivial_augment", images.data_ptr(), out.data_ptr(), B, C, H, W, self._records.upload(),
                  self._records.status_ptr, raw_stream(images.device.index))
        return out
