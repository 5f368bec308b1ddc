"""Schedule-free AdamW (Defazio et al., "The Road Less Scheduled") behind the constructor, the ``train()`` / ``eval()``
switch and the ``state_dict`` layout of ``schedulefree.AdamWScheduleFree`` -- the optimizer the reference's trainer
builds (``src/training/trainer.py:7,54-58,74-76,180,184``).

The update of ALL tensors of ALL parameter groups is ONE launch of ``basd_sfadamw_step`` (``csrc/optim.hip``):

* ``z`` and ``exp_avg_sq`` of every parameter are views into two flat fp32 buffers (16-byte aligned segments);
* a device table ``{y, z, v, grad, numel, group}`` plus a chunk list is uploaded once (stream-ordered, from pinned
  memory) and again only when a ``data_ptr`` or the set of gradients that are ``None`` changes;
* the per-group scalars of a step (``schedule``: plain Python, no GPU) travel in the kernel arguments, so a steady-state
  ``step()`` issues no host-to-device copy and never waits for the device;
* ``zero_grad_in_step=True`` clears the gradients in the same pass (use it with gradients that stay in place, such as
  ``ddp.FlatGradBucket`` views), ``grad_scale`` folds a ``1 / world`` into it;
* opt-in, ``max_grad_norm`` / ``skip_nonfinite``: global-norm clipping and a guard against inf / NaN gradients, decided
  on the device.  ``step()`` is then TWO launches (``basd_grad_sqnorm``: fp64 partial sums of squares;
  ``basd_sfadamw_step_clipped``: the same update behind a prologue that sums them), still without a copy or a wait.

fp32 parameters, state and gradients only; dense contiguous tensors on ONE device.  There is no CPU fallback.

``schedulefree`` is not available where this was written: the recurrence was restated from the paper and the package's
published source, and fidelity to an installed ``schedulefree`` (the ``state_dict`` key set included) is unverified.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib
from ._launch import raw_stream as _stream, require_gpu

__all__ = ["AdamWScheduleFree", "schedule", "MAX_GROUPS"]

MAX_GROUPS = 8          # BASD_SFADAMW_MAX_GROUPS of include/basd_hip.h
_ALIGN = 4              # elements: every state segment starts on a 16-byte boundary
_UNSET = object()       # step(max_grad_norm=...): "as the optimizer was built" (None means: no clipping in this call)


def _checked_max_norm(value):
    """``None`` (no clipping) or a finite number > 0 as a float; anything else is a ``ValueError``."""
    if value is None:
        return None
    norm = float(value)
    if not (math.isfinite(norm) and norm > 0.0):
        raise ValueError(f"max_grad_norm must be None or a finite number greater than 0, not {value!r}")
    return norm


class _GroupScalars(C.Structure):
    """BasdSfAdamwGroup of include/basd_hip.h."""
    _fields_ = [(n, C.c_double) for n in ("lr", "ckp1", "bias_correction2", "beta1", "beta2", "eps", "weight_decay")]


def schedule(group: dict) -> tuple[dict, dict]:
    """The host side of one ``step()`` for one parameter group: ``(scalars, new_state)``.  ``scalars`` =
    ``{lr, ckp1, bias_correction2}`` for the kernel, ``new_state`` = ``{k, weight_sum, lr_max, scheduled_lr}`` to be
    written back into the group.  Pure: ``group`` is not modified."""
    k = group["k"]
    warmup_steps = group["warmup_steps"]
    sched = (k + 1) / warmup_steps if k < warmup_steps else 1.0
    bias_correction2 = 1.0 - group["betas"][1] ** (k + 1)
    lr = group["lr"] * sched
    lr_max = max(lr, group["lr_max"])
    weight = ((k + 1) ** group["r"]) * (lr_max ** group["weight_lr_power"])
    weight_sum = group["weight_sum"] + weight
    ckp1 = weight / weight_sum if weight_sum != 0.0 else 0.0
    return ({"lr": lr, "ckp1": ckp1, "bias_correction2": bias_correction2},
            {"k": k + 1, "weight_sum": weight_sum, "lr_max": lr_max, "scheduled_lr": lr})


class AdamWScheduleFree(torch.optim.Optimizer):
    """``AdamWScheduleFree(params, lr=0.0025, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, warmup_steps=0, r=0.0,
    weight_lr_power=2.0, foreach=True)`` (``foreach`` is accepted and ignored).

    As in the package, a fresh optimizer is in eval mode: call ``.train()`` before the first ``step()`` and ``.eval()``
    before validation or a checkpoint; ``step()`` in eval mode raises.  Keyword-only additions: ``zero_grad_in_step``
    and ``grad_scale``, both overridable per call (``step(grad_scale=..., zero_grad_in_step=...)``).

    Keyword-only as well, and overridable per call: ``max_grad_norm`` (``None`` or a finite number > 0) and
    ``skip_nonfinite``.  The package has neither, so they are attributes of the optimizer and not entries of the
    parameter groups: the ``state_dict`` is unchanged.  ``max_grad_norm``: the gradients of ALL groups together, times ``grad_scale``, are
    scaled by ``min(1, max_grad_norm / (norm + 1e-6))`` as by ``torch.nn.utils.clip_grad_norm_`` -- inside the update:
    the stored gradients are not rewritten.  ``skip_nonfinite``: a step whose gradients hold an inf or a NaN leaves
    the parameters, ``z`` and ``exp_avg_sq`` untouched (the gradients are still zeroed with ``zero_grad_in_step``).
    The host cannot know of a skipped step without waiting for the device, so ``k``, ``weight_sum`` and ``lr_max``
    advance as for any step and only the device state stands still (``torch.amp.GradScaler`` does wait, and does not
    count a skipped step).  ``last_grad_norm()``, ``last_clip_coef()`` and ``last_step_skipped()`` return 0-dim device
    tensors without waiting; ``skipped_steps()`` returns an ``int`` and is the one call that waits."""

    def __init__(self, params, lr=0.0025, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, warmup_steps=0, r=0.0,
                 weight_lr_power=2.0, foreach=True, *, zero_grad_in_step: bool = False, grad_scale: float = 1.0,
                 max_grad_norm: float | None = None, skip_nonfinite: bool = False):
        defaults = dict(lr=lr, betas=betas, eps=eps, r=r, k=0, warmup_steps=warmup_steps, train_mode=False,
                        weight_sum=0.0, lr_max=-1.0, scheduled_lr=0.0, weight_lr_power=weight_lr_power,
                        weight_decay=weight_decay, foreach=foreach)
        self.zero_grad_in_step = bool(zero_grad_in_step)
        self.grad_scale = float(grad_scale)
        self.max_grad_norm = _checked_max_norm(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self._partials = self._verdict = None   # the norm pass's fp64 partial sums; BasdGradVerdict as 4 x 8 bytes
        self.table_uploads = 0          # how often the device table was (re)written: 1 in the steady state
        self._zbuf = self._vbuf = None  # the flat state buffers; None = state not built (or stale)
        self._params: list = []
        self._chunks = self._table = None
        self._signature = None
        super().__init__(params, defaults)

    # ---- groups and state --------------------------------------------------------------------------------------
    def add_param_group(self, param_group) -> None:
        super().add_param_group(param_group)
        group = self.param_groups[-1]
        if len(self.param_groups) > MAX_GROUPS:
            self.param_groups.pop()
            raise ValueError(f"at most {MAX_GROUPS} parameter groups (their scalars travel in the kernel arguments)")
        for p in group["params"]:
            if p.dtype != torch.float32:
                self.param_groups.pop()
                raise TypeError(f"AdamWScheduleFree updates fp32 parameters only (got {p.dtype}): keep fp32 master "
                                "weights under autocast")
        # a group added later joins the mode the optimizer is in (its z starts at p: x = y = z, nothing to move)
        group["train_mode"] = self.param_groups[0]["train_mode"]
        self._zbuf = None               # the flat buffers are rebuilt (existing state is carried over)

    def _build_state(self) -> None:
        """Two flat buffers for z / exp_avg_sq with 16-byte aligned segments; ``state[p]`` holds views.  State that
        exists already (an earlier layout, or tensors ``load_state_dict`` put there) is copied in; a parameter
        without state starts at ``z = p``, ``exp_avg_sq = 0``."""
        params = [p for g in self.param_groups for p in g["params"]]
        if not params:
            raise ValueError("no parameters")
        device = params[0].device
        offsets, total = [], 0
        for p in params:
            if p.device != device:
                raise ValueError("all parameters must live on one device")
            if p.is_sparse or not p.is_contiguous():
                raise ValueError("dense contiguous parameters only")
            offsets.append(total)
            total += (p.numel() + _ALIGN - 1) // _ALIGN * _ALIGN
        zbuf = torch.zeros(total, dtype=torch.float32, device=device)
        vbuf = torch.zeros(total, dtype=torch.float32, device=device)
        with torch.no_grad():
            for p, off in zip(params, offsets):
                z = zbuf[off:off + p.numel()].view_as(p)
                v = vbuf[off:off + p.numel()].view_as(p)
                old = self.state.get(p, {})
                z.copy_(old["z"] if "z" in old else p)
                if "exp_avg_sq" in old:
                    v.copy_(old["exp_avg_sq"])
                self.state[p] = {"z": z, "exp_avg_sq": v}
        self._zbuf, self._vbuf, self._params = zbuf, vbuf, params
        self._group_of = [gi for gi, g in enumerate(self.param_groups) for _ in g["params"]]
        self._chunks = self._table = self._signature = None

    def _ensure_state(self) -> None:
        if self._zbuf is None:
            self._build_state()

    def state_dict(self):
        """The package's layout: per parameter ``{"z", "exp_avg_sq"}``, per group ``lr, betas, eps, r, k, warmup_steps,
        train_mode, weight_sum, lr_max, scheduled_lr, weight_lr_power, weight_decay, foreach``.  A checkpoint taken
        before the first step already carries ``z = p``, ``exp_avg_sq = 0``.  Call ``.eval()`` first if the model's
        weights saved next to it are meant to be the averaged ones."""
        self._ensure_state()
        return super().state_dict()

    def load_state_dict(self, state_dict) -> None:
        super().load_state_dict(state_dict)
        self._zbuf = None               # the loaded tensors are moved into fresh flat buffers
        self._build_state()

    # ---- device table ------------------------------------------------------------------------------------------
    def _upload(self, rows: list, device) -> torch.Tensor:
        host = torch.empty((len(rows), len(rows[0])), dtype=torch.int64, pin_memory=True)
        host.copy_(torch.tensor(rows, dtype=torch.int64))
        dev = torch.empty(host.shape, dtype=torch.int64, device=device)
        dev.copy_(host, non_blocking=True)          # stream-ordered; the pinned block is recycled behind the copy
        return dev

    def _sync_table(self) -> None:
        """Compare every ``data_ptr`` (and which gradients are ``None``) with what the device table holds; rewrite the
        table when something moved.  The chunk list depends on the sizes only and is written once per layout."""
        self._ensure_state()
        params = self._params
        require_gpu(params[0])
        signature = tuple((p.data_ptr(), 0 if p.grad is None else p.grad.data_ptr()) for p in params)
        if signature == self._signature:
            return
        device = params[0].device
        rows = []
        for p, gi, (yp, gp) in zip(params, self._group_of, signature):
            g = p.grad
            if g is not None:
                if g.dtype != torch.float32:
                    raise TypeError(f"AdamWScheduleFree reads fp32 gradients only (got {g.dtype})")
                if g.is_sparse or g.device != device or not g.is_contiguous() or g.numel() != p.numel():
                    raise ValueError("gradients must be dense, contiguous and on the parameters' device")
            if not p.is_contiguous():
                raise ValueError("dense contiguous parameters only")
            st = self.state[p]
            rows.append([yp, st["z"].data_ptr(), st["exp_avg_sq"].data_ptr(), gp, p.numel(), gi])
        if self._chunks is None:
            chunk = _lib.query("basd_sfadamw_chunk")
            pairs = [[ti, ci] for ti, p in enumerate(params) for ci in range((p.numel() + chunk - 1) // chunk)]
            self._n_chunks = len(pairs)
            host = torch.tensor(pairs if pairs else [[0, 0]], dtype=torch.int32).pin_memory()
            self._chunks = torch.empty(host.shape, dtype=torch.int32, device=device)
            self._chunks.copy_(host, non_blocking=True)
            self._partials = torch.zeros(_lib.query("basd_grad_sqnorm_parts", self._n_chunks), dtype=torch.float64,
                                         device=device)
            if self._verdict is None:       # kept over a new layout: ``skipped_total`` counts for the optimizer's life
                self._verdict = torch.zeros(4, dtype=torch.float64, device=device)
        self._table = self._upload(rows, device)
        self._signature = signature
        self.table_uploads += 1

    # ---- the public interface ----------------------------------------------------------------------------------
    def step(self, closure=None, *, grad_scale: float | None = None, zero_grad_in_step: bool | None = None,
             max_grad_norm=_UNSET, skip_nonfinite: bool | None = None):
        """One update of every parameter that has a gradient (a parameter whose ``.grad`` is ``None`` is skipped; its
        group's ``k`` still advances).  One kernel launch, queued on the current stream; two with ``max_grad_norm`` or
        ``skip_nonfinite`` (for this call: ``max_grad_norm=None`` switches the clipping off, leaving the argument out
        keeps the optimizer's setting).  A step the guard skips on the device still advances ``k``."""
        max_norm = self.max_grad_norm if max_grad_norm is _UNSET else _checked_max_norm(max_grad_norm)
        guard = self.skip_nonfinite if skip_nonfinite is None else bool(skip_nonfinite)
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if not self.param_groups[0]["train_mode"]:
            raise RuntimeError("Optimizer was not in train mode when step is called. Please insert .train() and "
                               ".eval() calls on the optimizer.")
        self._sync_table()
        scalars = (_GroupScalars * len(self.param_groups))()
        for s, group in zip(scalars, self.param_groups):
            now, new_state = schedule(group)
            group.update(new_state)
            s.lr, s.ckp1, s.bias_correction2 = now["lr"], now["ckp1"], now["bias_correction2"]
            s.beta1, s.beta2 = group["betas"]
            s.eps, s.weight_decay = group["eps"], group["weight_decay"]
        scale = self.grad_scale if grad_scale is None else float(grad_scale)
        zero = int(self.zero_grad_in_step if zero_grad_in_step is None else zero_grad_in_step)
        table, chunks, stream = self._table.data_ptr(), self._chunks.data_ptr(), _stream()
        if max_norm is None and not guard:
            _lib.call("basd_sfadamw_step", table, chunks, self._n_chunks, C.addressof(scalars), len(self.param_groups),
                      scale, zero, stream)
            return loss
        parts = self._partials
        _lib.call("basd_grad_sqnorm", table, chunks, self._n_chunks, parts.data_ptr(), parts.numel(), stream)
        _lib.call("basd_sfadamw_step_clipped", table, chunks, self._n_chunks, C.addressof(scalars),
                  len(self.param_groups), scale, zero, parts.data_ptr(), parts.numel(),
                  0.0 if max_norm is None else max_norm, int(guard), self._verdict.data_ptr(), stream)
        return loss

    # ---- what the last clipped / guarded step decided (BasdGradVerdict of include/basd_hip.h) ---------------------
    def _verdict_field(self, dtype, index: int) -> torch.Tensor:
        if self._verdict is None:
            raise RuntimeError("no step has run yet: there is no verdict to read")
        return self._verdict.view(dtype)[index].clone()

    def last_grad_norm(self) -> torch.Tensor:
        """The 2-norm of all gradients of the last step made with ``max_grad_norm`` or ``skip_nonfinite``, as the
        update saw them (times ``grad_scale``, before clipping): a 0-dim fp32 device tensor, a copy.  Does not wait."""
        return self._verdict_field(torch.float32, 2)

    def last_clip_coef(self) -> torch.Tensor:
        """The coefficient that step multiplied the gradients by (1 = not clipped): 0-dim fp32, a copy, no wait."""
        return self._verdict_field(torch.float32, 3)

    def last_step_skipped(self) -> torch.Tensor:
        """1 if the guard skipped that step, else 0: 0-dim int32, a copy, no wait."""
        return self._verdict_field(torch.int32, 4)

    def skipped_steps(self) -> int:
        """How many steps the guard has skipped over this optimizer's life.  The one call here that WAITS for the
        device: call it at an epoch's end."""
        return 0 if self._verdict is None else int(self._verdict.view(torch.int32)[5].item())

    def _swap(self, to_train: bool) -> None:
        if self.param_groups[0]["train_mode"] == to_train:
            return
        # before the first step there is no state and x = y = z: only the flag moves (as in the package)
        if len(self.state) > 0:
            self._sync_table()
            beta1 = [g["betas"][0] for g in self.param_groups]
            weights = (C.c_float * len(beta1))(*[1.0 - b if to_train else 1.0 - 1.0 / b for b in beta1])
            _lib.call("basd_sfadamw_swap", self._table.data_ptr(), self._chunks.data_ptr(), self._n_chunks,
                      C.addressof(weights), len(beta1), _stream())
        for group in self.param_groups:
            group["train_mode"] = to_train

    @torch.no_grad()
    def train(self) -> None:
        """x -> y: ``p <- lerp(p, z, 1 - beta1)`` when in eval mode."""
        self._swap(True)

    @torch.no_grad()
    def eval(self) -> None:
        """y -> x: ``p <- lerp(p, z, 1 - 1 / beta1)`` when in train mode."""
        self._swap(False)
