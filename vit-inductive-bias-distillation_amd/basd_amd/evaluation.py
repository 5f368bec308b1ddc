"""Validation metrics: the reference's ``evaluate_model`` (``src/evaluation/metrics.py:19-55``) with the work of a batch
-- the column gather ``outputs[:, valid_indices]``, the (label-smoothed) cross entropy and the top-1 / top-5 counts --
as ONE launch of ``basd_eval_batch`` (``csrc/eval.hip``), and one read-back per epoch.

``EvalAccumulator`` owns five int64 words on the device: ``[loss in units of 2^-32, rows, top-1 hits, top-k hits, rows
that could not be represented]`` (a label outside ``[0, K)``, a NaN logit, a loss that is not finite).  They are summed
with integer atomics, so the result is the same bits whatever the order of arrival, and across ranks it is one
``all_reduce(SUM)``.  Ties go to the lower class position: a row whose target shares the maximum with a class before it
is a top-1 miss.

The reference counts with ``torchmetrics.MulticlassAccuracy``, which is not installed where this was written: the
semantics above are restated in ``tests/test_evaluation.py`` with torch ops, and fidelity to the package itself (its
handling of ties in particular) is unverified.  There is no CPU fallback.
"""
from __future__ import annotations

import torch
import torch.distributed as dist
import torch.nn as nn

from . import _lib
from ._launch import DTYPE_CODES, raw_stream, require_gpu

__all__ = ["EvalAccumulator", "evaluate_model"]

_LOSS_UNIT = 2.0 ** -32


class EvalAccumulator:
    """``EvalAccumulator(num_classes, valid_indices=None, label_smoothing=0.0, top_k=5, device=...)``.

    ``update(logits, targets)``: ``logits`` (B, C) fp32 / bf16 with unit column stride (any row stride: a view is read
    in place), ``targets`` (B,) int64 positions among the ``K`` evaluated classes -- ``K = len(valid_indices)`` columns
    of the logits when given (never gathered into a tensor), else all ``num_classes``.  One launch on the current
    stream, no allocation, no wait for the device.  ``compute()`` is the one device-to-host copy."""

    def __init__(self, num_classes: int, *, valid_indices=None, label_smoothing: float = 0.0, top_k: int = 5,
                 device) -> None:
        self.num_classes = int(num_classes)
        self.device = torch.device(device)
        self.label_smoothing = float(label_smoothing)
        self.top_k = int(top_k)
        self._index = None
        self._max_index = -1
        if valid_indices is not None:
            indices = [int(i) for i in valid_indices]
            if not indices or min(indices) < 0:
                raise ValueError("valid_indices must be a non-empty list of column indices >= 0")
            self._max_index = max(indices)
            self._index = torch.tensor(indices, dtype=torch.int32).to(self.device)       # uploaded once
        self.K = self.num_classes if self._index is None else len(indices)
        if self.K < 1:
            raise ValueError(f"num_classes must be positive (got {num_classes})")
        if not 1 <= self.top_k <= self.K:
            raise ValueError(f"top_k = {top_k} needs 1 <= top_k <= {self.K} evaluated classes")
        if not 0.0 <= self.label_smoothing <= 1.0:
            raise ValueError(f"label_smoothing must be in [0, 1] (got {label_smoothing})")
        self.state = torch.zeros(5, dtype=torch.int64, device=self.device)

    def reset(self) -> None:
        self.state.zero_()

    def update(self, logits: torch.Tensor, targets: torch.Tensor) -> None:
        for t in (logits, targets, self.state):
            require_gpu(t)
        if logits.dim() != 2 or logits.stride(1) != 1:
            raise ValueError(f"logits must be (B, C) with unit column stride (shape {tuple(logits.shape)}, strides "
                             f"{logits.stride()})")
        B, C = logits.shape
        if self._index is None:
            if C != self.num_classes:
                raise ValueError(f"{C} logit columns for num_classes = {self.num_classes}")
        elif self._max_index >= C:
            raise ValueError(f"valid_indices reach column {self._max_index} of {C}")
        if logits.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"logits must be fp32 or bf16 (got {logits.dtype})")
        if targets.dtype != torch.int64:
            raise TypeError(f"targets must be int64 class positions (got {targets.dtype})")
        if targets.shape != (B,) or (B > 1 and targets.stride(0) != 1):
            raise ValueError(f"targets must be a dense ({B},) tensor (shape {tuple(targets.shape)})")
        if logits.device != self.state.device or targets.device != self.state.device:
            raise ValueError("logits, targets and the accumulator must live on one device")
        _lib.call("basd_eval_batch", logits.data_ptr(), DTYPE_CODES[logits.dtype], logits.stride(0), B, C,
                  None if self._index is None else self._index.data_ptr(), self.K, targets.data_ptr(),
                  self.label_smoothing, self.top_k, self.state.data_ptr(), raw_stream(self.state.device.index))

    def all_reduce(self, group=None) -> None:
        """Sum the five words over the ranks of ``group`` (every rank evaluated its own shard: ``shard_loader``)."""
        dist.all_reduce(self.state, op=dist.ReduceOp.SUM, group=group)

    def compute(self) -> dict:
        """``{"val_acc", "val_acc_top5", "loss"}``: percentages of the rows seen and the mean loss; the loss is NaN when
        no row was seen or when a row could not be represented (such a row also counts as a miss)."""
        fixed, rows, hit1, hitk, bad = self.state.tolist()
        if rows == 0:
            return {"val_acc": float("nan"), "val_acc_top5": float("nan"), "loss": float("nan")}
        return {"val_acc": 100.0 * hit1 / rows, "val_acc_top5": 100.0 * hitk / rows,
                "loss": float("nan") if bad > 0 else fixed * _LOSS_UNIT / rows}


def _label_smoothing_of(criterion) -> float:
    """The kernel evaluates the stock criterion only: mean-reduced, unweighted ``nn.CrossEntropyLoss`` with the default
    ``ignore_index`` (subclasses and anything else would silently be given a different loss)."""
    if (type(criterion) is not nn.CrossEntropyLoss or criterion.weight is not None or criterion.reduction != "mean"
            or criterion.ignore_index != -100):
        raise TypeError("evaluate_model needs a stock torch.nn.CrossEntropyLoss (mean reduction, no class weights); "
                        f"got {criterion!r}")
    return float(criterion.label_smoothing)


@torch.no_grad()
def evaluate_model(model: nn.Module, data_loader, criterion: nn.Module, *, num_classes: int, valid_indices=None,
                   distributed: bool = False, image_stats=None, input_dtype=None, resize_crop=None,
                   jpeg_decode=None, png_decode=None, prefetch: int = 0, prefetch_stream=None) -> dict:
    """The reference's ``evaluate_model``: batches are dicts with ``pixel_values`` and ``label``; returns ``val_acc``,
    ``val_acc_top5`` (percent) and ``loss`` (mean of ``criterion`` over the samples); fewer than 5 evaluated classes
    raise ``ValueError``.  ``distributed=True``: every rank iterates its own shard and the counts are summed over the
    default process group before they are read.
    ``image_stats``: ``(mean, std)`` per channel; with it the loader may hand over uint8 ``pixel_values`` (a
    ``ToImage()``-only pipeline): they are scaled and normalised on the device by one convert-only launch of
    ``basd_amd.augment.BatchMixer`` (``MixParams("none")``) that writes ``input_dtype`` (default fp32).  A uint8 batch
    without ``image_stats`` raises ``TypeError`` before the model sees it.  Float batches go to the model as they are,
    whatever ``image_stats`` and ``input_dtype`` say.
    ``resize_crop``: a ``basd_amd.resize.ResizeCrop``; with it a batch may carry ``images`` (a ``RaggedBatch`` of decoded
    images, ``collate_fn=collate_ragged``) instead of ``pixel_values``: one launch makes the clean view (``Resize ->
    CenterCrop``, resampled with the instance's ``interpolation["clean"]``: validation is the clean geometry), which
    then takes the uint8 path above, so ``image_stats`` is needed (``ValueError`` otherwise).
    ``jpeg_decode``: a ``basd_amd.jpeg.JpegDecoder`` (it needs ``resize_crop``); with it ``images`` may be a ``JpegBatch``
    of the files' bytes (``collate_fn=collate_jpeg``), decoded on the device ahead of the resize launch (progressive files
    too where the batch was packed with ``collate_jpeg(..., progressive=True)``: the choice is the collate function's).
    ``png_decode``: a ``basd_amd.png.PngDecoder``, the same for a ``PngBatch`` (``collate_fn=collate_png``).
    ``prefetch``: an int >= 0 (``ValueError`` otherwise); the input half of up to that many batches (transfer, decode,
    resize, conversion, labels) runs ahead on a side stream (``basd_amd.prefetch.DevicePrefetcher``) while the model
    and the metrics launch of the batch before stay on the caller's; 0, the default, is the serial loop.
    ``prefetch_stream``: a ``DevicePrefetcher``'s ``.stream`` to use for it instead of a new one.  ``resize_crop``,
    ``jpeg_decode`` and ``png_decode`` belong to this call until it returns."""
    label_smoothing = _label_smoothing_of(criterion)
    if isinstance(prefetch, bool) or not isinstance(prefetch, int) or prefetch < 0:
        raise ValueError(f"prefetch must be an int >= 0 (got {prefetch!r})")
    if resize_crop is not None and image_stats is None:
        raise ValueError("resize_crop needs image_stats=(mean, std): its uint8 batches are converted and normalised on "
                         "the device; got image_stats=None")
    if jpeg_decode is not None and resize_crop is None:
        raise ValueError("jpeg_decode needs resize_crop=ResizeCrop(...): the decoded images are a ragged batch; got "
                         "resize_crop=None")
    if png_decode is not None and resize_crop is None:
        raise ValueError("png_decode needs resize_crop=ResizeCrop(...): the decoded images are a ragged batch; got "
                         "resize_crop=None")
    model.eval()
    device = next(model.parameters()).device
    acc = EvalAccumulator(num_classes, valid_indices=valid_indices, label_smoothing=label_smoothing, top_k=5,
                          device=device)
    converter = None
    if image_stats is not None:
        from .augment import BatchMixer, MixParams
        mean, std = image_stats
        converter = BatchMixer(num_classes, mean=mean, std=std, out_dtype=input_dtype, device=device)

    def prepare(batch):
        """The input half of a batch: transfer, optional decode, resize of the clean view, conversion, labels."""
        if "images" in batch and "pixel_values" not in batch:
            if resize_crop is None:
                raise TypeError("a batch of decoded 'images' needs resize_crop=ResizeCrop(...); got resize_crop=None")
            images = batch["images"].to(device, non_blocking=True)
            if jpeg_decode is not None:
                from .jpeg import JpegBatch
                if isinstance(images, JpegBatch):
                    images = jpeg_decode(images)
            if png_decode is not None:
                from .png import PngBatch
                if isinstance(images, PngBatch):
                    images = png_decode(images)
            inputs = resize_crop(images, views=("clean",))["clean"]
        else:
            inputs = batch["pixel_values"]
        if inputs.dtype == torch.uint8 and converter is None:
            raise TypeError("uint8 pixel_values need image_stats=(mean, std): the conversion and the normalisation run "
                            f"on the device; got {inputs.dtype} of shape {tuple(inputs.shape)} and image_stats=None")
        inputs = inputs.to(device, non_blocking=True)
        targets = batch["label"].to(device, non_blocking=True)
        if inputs.dtype == torch.uint8:
            inputs, _ = converter(inputs, None, MixParams("none"))
        return inputs, targets

    from .prefetch import DevicePrefetcher
    prefetcher = DevicePrefetcher(prepare, device=device, depth=prefetch, stream=prefetch_stream if prefetch else None)
    for inputs, targets in prefetcher.iterate(data_loader):
        acc.update(model(inputs), targets)
    if distributed:
        acc.all_reduce()
    return acc.compute()
