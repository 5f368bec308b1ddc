"""The teacher side of a single-layer teacher, kept on the device per dataset image.

A frozen teacher in eval mode sees the clean view (``Resize -> CenterCrop``: not cropped at random, not flipped, not
mixed), so image *i* gives it the same tokens in every epoch.  With ONE teacher layer the mixing weight is exactly 1
(layer_selector.py:110-112) and the Procrustes loss (relational.py:22-39) reads of those tokens only ``ops.TeacherSide``:
the fp64 Gram of the centred, weighted tokens on the core grid and the two token-weight vectors --
``record_bytes(n, n_s)`` bytes per image (19,600 at 49 tokens) instead of the tokens themselves.  ``TeacherCache`` holds
those rows; ``store`` and ``load`` are one HIP launch each (basd_teacher_cache_store / _load, csrc/teacher_cache.hip).
There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._launch import lives_on, raw_stream, require_gpu
from .ops import TeacherSide

__all__ = ["TeacherCache", "CachedTeacherSide"]


class CachedTeacherSide:
    """Rows of a ``TeacherCache`` that ``load`` found filled, not gathered yet: ``into(g, omega, omega_t)`` queues the
    one gather launch on the current stream into tensors of the right shape (``ops.procrustes_forward_cached`` hands
    over the slots its call reads, so the rows are moved once); ``g`` / ``omega`` / ``omega_t`` gather into fresh
    tensors.  Either reads the cache when it is called: call it on the stream the rows were stored on."""

    def __init__(self, cache: "TeacherCache", index: torch.Tensor) -> None:
        self.cache, self.index = cache, index
        self.B, self.n, self.n_s = index.numel(), cache.n, cache.n_s
        self._side = None

    def into(self, g: torch.Tensor, omega: torch.Tensor, omega_t: torch.Tensor) -> None:
        c, B = self.cache, self.index.numel()
        for name, t, shape, dtype in (("g", g, (B, c.n, c.n), torch.float64), ("omega", omega, (B, c.n_s), torch.float32),
                                      ("omega_t", omega_t, (B, c.n), torch.float32)):
            require_gpu(t, name)
            if tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous {dtype} tensor of shape {shape} (got {t.dtype} "
                                 f"{tuple(t.shape)}, strides {t.stride()})")
        _lib.call("basd_teacher_cache_load", c.g.data_ptr(), c.omega.data_ptr(), c.omega_t.data_ptr(),
                  self.index.data_ptr(), B, c.n, c.n_s, c.capacity, g.data_ptr(), omega.data_ptr(), omega_t.data_ptr(),
                  raw_stream(c.device.index))

    def tensors(self) -> TeacherSide:
        if self._side is None:
            c, B = self.cache, self.index.numel()
            side = TeacherSide(torch.empty((B, c.n, c.n), device=c.device, dtype=torch.float64),
                               torch.empty((B, c.n_s), device=c.device, dtype=torch.float32),
                               torch.empty((B, c.n), device=c.device, dtype=torch.float32))
            self.into(*side)
            self._side = side
        return self._side

    @property
    def g(self) -> torch.Tensor:
        return self.tensors().g

    @property
    def omega(self) -> torch.Tensor:
        return self.tensors().omega

    @property
    def omega_t(self) -> torch.Tensor:
        return self.tensors().omega_t


class TeacherCache:
    """``TeacherCache(capacity, n, n_s, device)``: three device tensors, ``g (capacity, n, n)`` fp64, ``omega
    (capacity, n_s)`` and ``omega_t (capacity, n)`` fp32 -- ``n`` the core grid (the smaller of the two token grids),
    ``n_s`` the student's -- and a HOST bitmap of the filled rows, updated when a store is QUEUED: ``has`` never waits
    for the device, and a ``load`` queued behind the store on the same stream finds the rows.

    ``store(index, teacher_side)`` scatters the rows of ``ops.TeacherSide`` tensors (``BASDLoss.last_teacher_side()``)
    to the cache rows ``index`` ((B,) int64 dataset indices, on the host or on the device; give a host tensor where you
    have one: a device tensor is read back for the bitmap, which waits for it).  The same index twice in one call must
    come with equal rows (it does: the teacher side is a function of the image); the launches race on that row and
    leave the same bytes.  ``load(index)`` checks ON THE HOST that every row was stored -- ``KeyError`` naming the first
    that was not -- and returns a ``CachedTeacherSide``; a repeated index is legal.  Both run on the current stream;
    rows are visible to loads queued behind their store on that stream (or ordered behind it by an event).
    ``has(index)``: whether all those rows are filled, plain Python; ``filled(index)``: which of them.  ``clear()`` empties the bitmap (the device
    memory is kept).  Arguments are checked before anything is queued: the index (1-D int64, within ``[0, capacity)``,
    as long as the batch), shapes and dtypes (``ValueError``), then the devices -- CPU tensors, or a cache made on a
    CPU device, raise the package's "no CPU fallback" ``RuntimeError`` in ``store`` and ``load``.

    VALIDITY IS THE CALLER'S: the rows are right for one teacher (its weights, eval mode), one clean transform (size,
    crop ratio, filter), one set of clean statistics and one autocast dtype.  The cache never invalidates itself: when
    any of those changes, call ``clear()``.  It is not part of a checkpoint."""

    def __init__(self, capacity: int, n: int, n_s: int, device) -> None:
        for name, v in (("capacity", capacity), ("n", n), ("n_s", n_s)):
            if isinstance(v, bool) or not isinstance(v, int) or v <= 0:
                raise ValueError(f"{name} must be an int > 0 (got {v!r})")
        if n > n_s:
            raise ValueError(f"n is the core grid, the smaller of the two token grids: n={n} > n_s={n_s}")
        # (a cache on a CPU device can be made and asked -- the bookkeeping is the host's; store and load raise there)
        self.device = torch.device(device)
        self.capacity, self.n, self.n_s = capacity, n, n_s
        self.g = torch.empty((capacity, n, n), device=self.device, dtype=torch.float64)
        self.omega = torch.empty((capacity, n_s), device=self.device, dtype=torch.float32)
        self.omega_t = torch.empty((capacity, n), device=self.device, dtype=torch.float32)
        self._filled = np.zeros(capacity, dtype=bool)

    @staticmethod
    def record_bytes(n: int, n_s: int) -> int:
        """Bytes of one image's row: the (n, n) fp64 Gram and the two fp32 weight vectors."""
        return 8 * n * n + 4 * n_s + 4 * n

    @property
    def nbytes(self) -> int:
        return self.capacity * self.record_bytes(self.n, self.n_s)

    def clear(self) -> None:
        self._filled[:] = False

    def _host_index(self, index, batch=None) -> np.ndarray:
        if not isinstance(index, torch.Tensor) or index.dtype != torch.int64 or index.dim() != 1:
            got = f"{index.dtype} {tuple(index.shape)}" if isinstance(index, torch.Tensor) else type(index).__name__
            raise ValueError(f"index must be a 1-D int64 tensor of dataset indices (got {got})")
        if batch is not None and index.numel() != batch:
            raise ValueError(f"index has {index.numel()} entries for a batch of {batch}")
        if index.numel() == 0:
            raise ValueError("index is empty")
        host = index.detach().cpu().numpy()
        if host.min() < 0 or host.max() >= self.capacity:
            bad = host[(host < 0) | (host >= self.capacity)][0]
            raise ValueError(f"index {int(bad)} is outside [0, capacity={self.capacity})")
        return host

    def _device_index(self, index: torch.Tensor) -> torch.Tensor:
        if index.is_cuda:
            if not lives_on(self.device, index.device):
                raise ValueError(f"index lives on {index.device}, the cache on {self.device}")
            return index.contiguous()
        return index.contiguous().to(self.device, non_blocking=True)

    def has(self, index) -> bool:
        """Whether every row of ``index`` has been stored (host only; give a host tensor)."""
        return bool(self._filled[self._host_index(index)].all())

    def filled(self, index) -> torch.Tensor:
        """Per entry of ``index`` whether its row has been stored: a host bool tensor (host only; give a host tensor)."""
        return torch.from_numpy(self._filled[self._host_index(index)])

    def store(self, index, teacher_side, *, device_index=None) -> None:
        """``device_index``: the same indices already on the device (saves the upload)."""
        g, omega, omega_t = teacher_side
        B = g.shape[0] if g.dim() else 0
        host = self._host_index(index, B)
        named = (("g", g, (B, self.n, self.n), torch.float64), ("omega", omega, (B, self.n_s), torch.float32),
                 ("omega_t", omega_t, (B, self.n), torch.float32))
        for name, t, shape, dtype in named:
            if tuple(t.shape) != shape or t.dtype != dtype:
                raise ValueError(f"teacher side {name} must be {dtype} of shape {shape} for this cache (got {t.dtype} "
                                 f"{tuple(t.shape)})")
        require_gpu(self.device, "the cache's rows")
        for name, t, _, _ in named:
            require_gpu(t, f"teacher side {name}")
            if not lives_on(self.device, t.device):
                raise ValueError(f"teacher side {name} lives on {t.device}, the cache on {self.device}")
        g, omega, omega_t = g.contiguous(), omega.contiguous(), omega_t.contiguous()
        dev_index = self._device_index(index if device_index is None else device_index)
        _lib.call("basd_teacher_cache_store", g.data_ptr(), omega.data_ptr(), omega_t.data_ptr(), dev_index.data_ptr(), B,
                  self.n, self.n_s, self.capacity, self.g.data_ptr(), self.omega.data_ptr(), self.omega_t.data_ptr(),
                  raw_stream(self.device.index))
        self._filled[host] = True

    def load(self, index, *, device_index=None) -> CachedTeacherSide:
        host = self._host_index(index)
        missing = ~self._filled[host]
        if missing.any():
            raise KeyError(f"teacher cache row {int(host[missing][0])} was never stored")
        require_gpu(self.device, "the cache's rows")
        return CachedTeacherSide(self, self._device_index(index if device_index is None else device_index))
