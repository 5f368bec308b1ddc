"""Teacher attention importance from the output of a block's own fused ``qkv`` projection: ONE launch of
``basd_attn_importance`` (``csrc/attn.hip``) per layer.

The loss reads very little of a ViT teacher's attention maps (reference ``src/losses/relational.py:22-27``): with a CLS
token the CLS query's row, without one the mean over the queries, both averaged over the heads.  ``attn_importance``
computes exactly that per head from ``qkv`` -- ``softmax(scale * Q K^T)`` reduced over the queries inside the kernel --
so neither the (B, H, N, N) map nor a second projection of the block's input exists.  There is no CPU fallback.
"""
from __future__ import annotations

import torch

from . import _lib
from ._launch import DTYPE_CODES, raw_stream, require_gpu

__all__ = ["attn_importance", "MODES"]

MODES = {"cls_row": 0, "query_mean": 1}                  # BASD_ATTN_CLS_ROW / BASD_ATTN_QUERY_MEAN of include/basd_hip.h
MAX_TOKENS, MAX_HEAD_DIM = 1025, 128


def attn_importance(qkv: torch.Tensor, num_heads: int, *, mode: str, scale=None, out=None) -> torch.Tensor:
    """``qkv``: (B, N, 3 * num_heads * hd) fp32 / bf16 on the GPU, the output of a timm-style fused projection (last axis
    laid out ``[3][num_heads][hd]``, unit stride; batch and token strides are free: a view is read in place).
    ``mode="cls_row"``: ``out[b, h, j] = softmax_j(scale * q[b, h, 0] . k[b, h, j])``; ``mode="query_mean"``: the mean
    of the softmax rows over all N queries.  ``scale`` defaults to ``hd ** -0.5``.  Returns (B, num_heads, N) fp32
    (``out`` if given: dense, fp32, that shape).  1 <= N <= 1025, hd a multiple of 8 up to 128.  One launch on the
    current stream, no workspace, no wait for the device."""
    # every argument is checked before the device is: a CPU tensor with a wrong argument reports the argument
    if mode not in MODES:
        raise ValueError(f"mode must be one of {sorted(MODES)} (got {mode!r})")
    if qkv.dim() != 3:
        raise ValueError(f"qkv must be (B, N, 3 * num_heads * head_dim) (shape {tuple(qkv.shape)})")
    B, N, C3 = qkv.shape
    num_heads = int(num_heads)
    if num_heads < 1 or C3 % (3 * num_heads) != 0 or C3 == 0:
        raise ValueError(f"the last axis of qkv (shape {tuple(qkv.shape)}) is not 3 * num_heads * head_dim for "
                         f"num_heads = {num_heads}")
    hd = C3 // (3 * num_heads)
    if qkv.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"qkv must be fp32 or bf16 (got {qkv.dtype}, shape {tuple(qkv.shape)})")
    if B < 1 or not 1 <= N <= MAX_TOKENS:
        raise ValueError(f"qkv of shape {tuple(qkv.shape)}: need B >= 1 and 1 <= N <= {MAX_TOKENS}")
    if hd % 8 != 0 or hd > MAX_HEAD_DIM:
        raise ValueError(f"head_dim {hd} (qkv of shape {tuple(qkv.shape)}, num_heads {num_heads}) must be a multiple of 8 "
                         f"up to {MAX_HEAD_DIM}")
    if qkv.stride(2) != 1:
        raise ValueError(f"the last axis of qkv must have unit stride (shape {tuple(qkv.shape)}, strides {qkv.stride()})")
    if out is not None:
        if out.shape != (B, num_heads, N) or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError(f"out must be a dense fp32 tensor of shape {(B, num_heads, N)} (shape {tuple(out.shape)}, "
                             f"{out.dtype}, strides {out.stride()})")
        if out.device != qkv.device:
            raise ValueError(f"out lives on {out.device}, qkv on {qkv.device}")
    require_gpu(qkv, f"the qkv activations of shape {(B, N, C3)}")
    if out is None:
        out = torch.empty((B, num_heads, N), dtype=torch.float32, device=qkv.device)
    _lib.call("basd_attn_importance", qkv.data_ptr(), DTYPE_CODES[qkv.dtype], qkv.stride(0), qkv.stride(1), B, N,
              num_heads, hd, MODES[mode], float(hd ** -0.5 if scale is None else scale), out.data_ptr(),
              raw_stream(qkv.device.index))
    return out
