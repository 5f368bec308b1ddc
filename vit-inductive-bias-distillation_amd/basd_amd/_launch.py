"""What the one-launch stages share on the host (``augment``, ``trivial_augment``, ``resize``, ``stats``, ``attention``,
``evaluation``, ``optim``, ``ops``): the raw stream, the ``BASD_DTYPE_*`` codes, the checks an image batch and its
``out=`` pass before a launch, and the uploader of a per-sample record table.  Private to the package."""
from __future__ import annotations

import numpy as np
import torch

DTYPE_CODES = {torch.float32: 0, torch.bfloat16: 1, torch.uint8: 2}         # BASD_DTYPE_* of include/basd_hip.h
_NAMES = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.uint8: "uint8"}


def raw_stream(device_index=None) -> int:
    """The raw ``hipStream_t`` of the current stream of that device (``None``: the current device) in one C call:
    ``torch.cuda.current_stream()`` builds a Stream object through three layers of Python (~10 us, ~20 calls a step)."""
    return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice() if device_index is None else device_index)


def require_gpu(device_or_tensor, what=None) -> None:
    """The one "no CPU fallback" error: raised unless the device (a tensor's, if a tensor is given) is a GPU."""
    device = getattr(device_or_tensor, "device", device_or_tensor)
    if device.type != "cuda":
        raise RuntimeError("basd_amd kernels need CUDA/HIP tensors (there is no CPU fallback)"
                           + ("" if what is None else f"; {what} live on {device}"))


def retire(state) -> None:
    """Called on persistent device state (``None``: nothing yet) right before it is replaced by a larger one: the last
    launches that read it may be on another stream than the one it was allocated on (a ``DevicePrefetcher``'s), so the
    allocator is told to hand the memory out again only behind the current stream's work.  Nothing is done for a
    tensor allocated on the current stream."""
    if state is not None and state.is_cuda:
        state.record_stream(torch.cuda.current_stream(state.device))


def lives_on(owner: torch.device, device: torch.device) -> bool:
    """An owner without an index (``cuda``) takes every device of its type."""
    return device.type == owner.type and owner.index in (None, device.index)


def dense(t: torch.Tensor) -> bool:
    """Row-major without gaps, axes of size 1 aside (their strides are free)."""
    expected = 1
    for size, stride in zip(reversed(t.shape), reversed(t.stride())):
        if size != 1 and stride != expected:
            return False
        expected *= size
    return True


def check_image_batch(images: torch.Tensor, dtypes, channels=None) -> tuple:
    """``(B, C, H, W)`` of a dense NCHW batch of one of ``dtypes`` (with one of ``channels`` channels, if given);
    otherwise the first of: rank, density (``ValueError``), dtype (``TypeError``), channels (``ValueError``)."""
    shape = tuple(images.shape)
    if len(shape) != 4:
        raise ValueError(f"images must be (B, C, H, W) (shape {shape})")
    if not dense(images):
        raise ValueError(f"images must be a dense NCHW batch, not channels-last or strided (shape {shape}, strides "
                         f"{images.stride()})")
    if images.dtype not in dtypes:
        raise TypeError(f"images must be {' / '.join(_NAMES[d] for d in dtypes)} (got {images.dtype}, shape {shape})")
    if channels is not None and shape[1] not in channels:
        raise ValueError(f"images must have {' or '.join(str(c) for c in channels)} channels (shape {shape})")
    return shape


def check_out(out: torch.Tensor, images: torch.Tensor, dtypes, why_no_overlap: str) -> None:
    """An ``out=`` for ``images``: the first of shape and density (``ValueError``), dtype (``TypeError``), device,
    overlap of the two byte ranges (``ValueError``; ``why_no_overlap`` ends the message)."""
    if out.shape != images.shape or not dense(out):
        raise ValueError(f"out must be a dense NCHW tensor of shape {tuple(images.shape)} (shape {tuple(out.shape)}, "
                         f"strides {out.stride()})")
    if out.dtype not in dtypes:
        raise TypeError(f"out must be {' / '.join(_NAMES[d] for d in dtypes)} (got {out.dtype})")
    if out.device != images.device:
        raise ValueError(f"out lives on {out.device}, images on {images.device}")
    s0, d0 = images.data_ptr(), out.data_ptr()
    s1, d1 = s0 + images.numel() * images.element_size(), d0 + out.numel() * out.element_size()
    if s0 < d1 and d0 < s1:
        raise ValueError(f"out overlaps images (shape {tuple(images.shape)}): {why_no_overlap}")


def batch_columns(record, batch: int, kinds: dict) -> dict:
    """The fields ``kinds`` (name -> dtype) of a record of per-sample columns as flat lists of exactly ``batch``
    entries; a field holds anything ``torch.as_tensor`` takes."""
    columns = {}
    for name, dtype in kinds.items():
        t = torch.as_tensor(getattr(record, name)).to(dtype).reshape(-1)
        if t.numel() != batch:
            raise ValueError(f"{type(record).__name__}.{name} has {t.numel()} entries for a batch of {batch}")
        columns[name] = t.tolist()
    return columns


class RecordTable:
    """A table of fixed-size records on the device, refilled from the host once per launch without waiting for it.

    ``stage(count, device)`` hands out ``count`` records of the next of ``ring`` pinned buffers to be written;
    ``upload()`` sends them with one non-blocking copy into the device table on the current stream, records an event
    behind the copy and returns the table's address.  A pinned buffer is handed out again only after the event behind
    the last copy made from it has completed -- ``ring`` calls ago, done long since: in the steady state nothing waits,
    nothing is allocated and nothing is cleared.  ``table`` (uint8) and ring grow together to the largest count seen.
    ``status_ptr``: one int32 word for the kernel's status, zero when it is created (with the table); ``status()`` reads
    it back (0 before the first use; it waits for the device)."""

    def __init__(self, record_dtype: np.dtype, ring: int = 4) -> None:
        self.record_dtype = np.dtype(record_dtype)
        self.ring = int(ring)
        self._host = []          # ring of (pinned buffer, event recorded behind its last copy)
        self._slot = 0
        self._staged = 0         # bytes of the current slot that upload() sends
        self.table = self._status = self.status_ptr = None

    def stage(self, count: int, device: torch.device) -> np.ndarray:
        nbytes = max(count, 1) * self.record_dtype.itemsize
        if self.table is None or self.table.numel() < nbytes:
            retire(self.table)
            self.table =torch.empty(nbytes, dtype=torch.uint8, device=device)
            self._host = [(torch.empty(nbytes, dtype=torch.uint8).pin_memory(), torch.cuda.Event())
                          for _ in range(self.ring)]
        if self._status is None:
            self._status = torch.zeros(1, dtype=torch.int32, device=device)
            self.status_ptr = self._status.data_ptr()
        self._slot = (self._slot + 1) % self.ring
        buffer, event = self._host[self._slot]
        if not event.query():          # true of an event never recorded
            event.synchronize()
        self._staged = count * self.record_dtype.itemsize
        return buffer.numpy()[:self._staged].view(self.record_dtype)

    def upload(self) -> int:
        buffer, event = self._host[self._slot]
        self.table[:self._staged].copy_(buffer[:self._staged], non_blocking=True)
        event.record()
        return self.table.data_ptr()

    def status(self) -> int:
        return 0 if self._status is None else int(self._status.item())
