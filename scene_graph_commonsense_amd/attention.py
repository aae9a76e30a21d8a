"""Fused multi-head attention forward for head dim 32 (``sgc_mha_fwd``, csrc/kernels_attn.hip): the attention of the DETR-101
extractor's 18 blocks (``detr.py``) without the ``[B*H, L, L]`` score matrix in HBM.

``fused_mha`` is the operator between the input and output projections; ``mha_forward`` is the whole block for an existing
``nn.MultiheadAttention``.  Forward only (the extractor is frozen); key-padding mask only; there is no CPU or eager fallback.
A query whose keys are all masked gets zeros, where ``nn.MultiheadAttention`` gives NaN."""
from __future__ import annotations

import ctypes
import math
from typing import Optional

import torch
import torch.nn.functional as F
from torch import Tensor, nn

from . import _lib

HEAD_DIM = 32
_DTYPES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
_FN = None


def _fn():
    global _FN
    if _FN is None:
        f = _lib.load().sgc_mha_fwd
        vp, ci, cl = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
        f.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ci, cl, cl, cl, cl, cl, cl, cl, cl, ci, ctypes.c_float, vp]
        f.restype = ci
        _FN = f
    return _FN


def _check_args(q, k, v, num_heads, key_padding_mask):
    for name, t in (("q", q), ("k", k), ("v", v)):
        if not torch.is_tensor(t) or t.dim() != 3:
            raise ValueError("%s must be a [L, B, E] tensor" % name)
    if q.dtype not in _DTYPES or k.dtype != q.dtype or v.dtype != q.dtype:
        raise ValueError("q, k and v must share one dtype of float32 / float16 / bfloat16, got %s, %s, %s" % (q.dtype, k.dtype, v.dtype))
    if k.device != q.device or v.device != q.device:
        raise ValueError("q, k and v must be on one device")
    if not isinstance(num_heads, int) or num_heads < 1:
        raise ValueError("num_heads must be a positive int")
    for name, t in (("q", q), ("k", k), ("v", v)):
        if t.shape[2] != HEAD_DIM * num_heads:
            raise ValueError("%s has E = %d, the kernel needs E = 32 * num_heads = %d" % (name, t.shape[2], HEAD_DIM * num_heads))
    if k.shape[1] != q.shape[1] or v.shape[1] != q.shape[1]:
        raise ValueError("q, k and v differ in the batch size: %d, %d, %d" % (q.shape[1], k.shape[1], v.shape[1]))
    if k.shape[0] != v.shape[0]:
        raise ValueError("k has %d keys, v %d" % (k.shape[0], v.shape[0]))
    if key_padding_mask is not None:
        m = key_padding_mask
        if not torch.is_tensor(m) or m.dtype not in (torch.bool, torch.uint8):
            raise ValueError("key_padding_mask must be a bool / uint8 tensor")
        if tuple(m.shape) != (q.shape[1], k.shape[0]):
            raise ValueError("key_padding_mask must have shape [B, Lk] = [%d, %d], got %s" % (q.shape[1], k.shape[0], tuple(m.shape)))
        if m.device != q.device:
            raise ValueError("key_padding_mask must be on the tensors' device")


def _kernel_view(t: Tensor) -> Tensor:
    """``t`` itself when the kernel can read it in place (contiguous last dim, strides a multiple of 16 bytes, 16-byte aligned base),
    else one contiguous copy."""
    mult = 16 // t.element_size()
    ok = t.stride(2) == 1 or t.shape[2] == 1
    ok = ok and all(s >= 0 and s % mult == 0 for s in (t.stride(0), t.stride(1))) and t.data_ptr() % 16 == 0
    return t if ok else t.contiguous()


def fused_mha(q: Tensor, k: Tensor, v: Tensor, num_heads: int, key_padding_mask: Optional[Tensor] = None,
              scale: Optional[float] = None) -> Tensor:
    """``softmax(scale * q k^T) v`` per image and head over the keys ``key_padding_mask`` (``[B, Lk]``, True / nonzero = excluded) leaves.
    ``q [Lq, B, E]``, ``k`` / ``v [Lk, B, E]`` with ``E = 32 * num_heads``, float32 / float16 / bfloat16, possibly strided views with a
    contiguous last dim (column slices of a packed projection are read in place); returns a contiguous ``[Lq, B, E]`` tensor of the
    inputs' dtype.  ``scale`` defaults to ``1 / sqrt(32)``."""
    _check_args(q, k, v, num_heads, key_padding_mask)
    scale = 1.0 / math.sqrt(HEAD_DIM) if scale is None else float(scale)
    if not math.isfinite(scale):
        raise ValueError("scale must be finite")
    if not q.is_cuda:
        raise RuntimeError("fused_mha runs on the GPU only (there is no CPU fallback)")
    if torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad):
        raise RuntimeError("fused_mha is forward-only: call it under torch.no_grad() or on detached tensors")
    q, k, v = _kernel_view(q), _kernel_view(k), _kernel_view(v)
    Lq, B, E = q.shape
    Lk = k.shape[0]
    out = torch.empty((Lq, B, E), dtype=q.dtype, device=q.device)
    mask = None
    if key_padding_mask is not None:
        mask = key_padding_mask.contiguous()
        mask = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
    with torch.cuda.device(q.device):
        st = _fn()(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(mask), _lib.ptr(out), Lq, Lk, B, num_heads,
                   q.stride(0), q.stride(1), k.stride(0), k.stride(1), v.stride(0), v.stride(1), out.stride(0), out.stride(1),
                   _DTYPES[q.dtype], scale, _lib.stream_ptr())
    _lib.check(st, "sgc_mha_fwd")
    return out


def mha_forward(mha: nn.MultiheadAttention, query: Tensor, key: Tensor, value: Tensor, key_padding_mask: Optional[Tensor] = None) -> Tensor:
    """The attention output of ``mha(query, key, value, key_padding_mask=...)[0]`` through ``fused_mha``: input projections as views of
    ``in_proj_weight`` / ``in_proj_bias`` (one GEMM for q and k when ``query is key``, so that both are column slices of one tensor),
    the kernel, ``out_proj``.  Runs under whatever autocast is active.  The module's parameters are untouched."""
    if mha.in_proj_weight is None or mha.batch_first or mha.bias_k is not None or mha.add_zero_attn:
        raise ValueError("mha_forward needs a packed in_proj_weight, batch_first=False, no bias_k / bias_v and no add_zero_attn")
    E = mha.embed_dim
    w, b = mha.in_proj_weight, mha.in_proj_bias
    bs = (lambda lo, hi: None) if b is None else (lambda lo, hi: b[lo:hi])
    if query is key:
        qk = F.linear(query, w[:2 * E], bs(0, 2 * E))
        q, k = qk[..., :E], qk[..., E:]
    else:
        q, k = F.linear(query, w[:E], bs(0, E)), F.linear(key, w[E:2 * E], bs(E, 2 * E))
    v = F.linear(value, w[2 * E:], bs(2 * E, 3 * E))
    return mha.out_proj(fused_mha(q, k, v, mha.num_heads, key_padding_mask))


def fused_route(mha: nn.MultiheadAttention, attn_mask, *tensors: Tensor) -> bool:
    """Whether an attention call of the extractor may take ``mha_forward``: GPU tensors, no gradient needed, no attention mask,
    no active attention dropout, head dim 32."""
    if attn_mask is not None or mha.head_dim != HEAD_DIM or (mha.training and mha.dropout != 0.0):
        return False
    if not all(t.is_cuda for t in tensors):
        return False
    if torch.is_grad_enabled() and (any(t.requires_grad for t in tensors) or any(p.requires_grad for p in mha.parameters())):
        return False
    return True
