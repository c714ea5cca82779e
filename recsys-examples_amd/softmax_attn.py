"""Softmax attention of the semantic-ID generative-retrieval family on MI355X, differentiable: the training surface.

`flash_attn_func` and `flash_attn_varlen_func` have the signatures, the validation and the refusals of prefill_attn.py (the
inference surface, which stays forward-only) and run the same forward kernel with the same bits; under autograd they carry
q.grad, k.grad and v.grad through `mi355_softmax_attn_bwd` (csrc/softmax_attn_bwd.hip): two launches, no atomics, bitwise
reproducible, dk / dv of a kv head summed over its query heads inside one workgroup.  This is what
examples/sid_gr/model/jagged_flash_attn_block.py trains through; the import names of the reference (`flash_attn`,
`flash_attn.flash_attn_interface`, `flash_attn.cute.interface`) under flash_attn_gfx950/ resolve to this module.

    dense:   q [B, Sq, Hq, D], k / v [B, Sk, Hkv, D] (any batch / row / head strides: the unbind(2) views of a packed
             [B, S, 3, H, D] leaf are read in place and the leaf receives one gradient)
    jagged:  q [total_q, Hq, D], k / v [total_k, Hkv, D], cu_seqlens_q / _k int32 [B+1]; max_seqlen_q AND max_seqlen_k bound
             the launches: each must be at least the longest sequence of its side
    arbitrary_func (aux_tensors[0], dense only): int32 [B, 1 or Hq, n_func (odd, <= 129), >= Sq]

There is no eager fallback: without the library or a GPU the call raises.
"""
from __future__ import annotations

from typing import Optional

import torch

import mi355_native as N
import prefill_attn as _P
from mi355_native import rows_aligned as _rows_aligned
from prefill_attn import MASK_CAUSAL, MASK_FUNC, MASK_NONE, PrefillAttnError  # noqa: F401

MAX_N_FUNC = 129   # csrc/softmax_attn_bwd.hip: kBwMaxFunc


def _backward(q, k, v, out, lse, dout, cu_q, cu_k, max_q, max_k, mask, func, scale, skip_tiles=True, grads=None):
    """dq, dk, dv (contiguous, the shapes and dtype of q, k, v) of the forward that returned (out, lse).  grads: an optional
    preallocated contiguous (dq, dk, dv); every element is written by the kernels, whatever they held."""
    jagged = cu_q is not None
    q, k, v, dout = _rows_aligned(q), _rows_aligned(k), _rows_aligned(v), _rows_aligned(dout)
    if dout.numel() and dout.stride(-1) != 1:
        dout = dout.contiguous()
    out = out.contiguous()
    lse = lse.contiguous()
    Hq, D, Hkv = q.shape[-2], q.shape[-1], k.shape[-2]
    if grads is None:
        grads = tuple(torch.empty(t.shape, device=t.device, dtype=t.dtype) for t in (q, k, v))
    dq, dk, dv = grads
    for name, g, t in (("dq", dq, q), ("dk", dk, k), ("dv", dv, v)):
        if g.shape != t.shape or g.dtype != t.dtype or g.device != t.device or not g.is_contiguous():
            raise PrefillAttnError(f"{name} must be contiguous with the shape, dtype and device of its input, got "
                                   f"{tuple(g.shape)} {g.dtype} strides {tuple(g.stride())}")
    delta = torch.empty_like(lse)
    if jagged:
        B, Sq, Sk, total_q, total_k = cu_q.shape[0] - 1, int(max_q), int(max_k), q.shape[0], k.shape[0]
    else:
        B, Sq, Sk, total_q, total_k = q.shape[0], q.shape[1], k.shape[1], 0, 0
    qs, ks, vs, ds = _P._strides(jagged, q, k, v, dout)
    N.check(N.lib().mi355_softmax_attn_bwd(
        N.ptr(q), *qs, N.ptr(k), *ks, N.ptr(v), *vs, N.ptr(cu_q), N.ptr(cu_k),
        B, Sq, Sk, total_q, total_k, Hq, Hkv, D, mask, *_P._func_args(func), float(scale), int(skip_tiles),
        N.ptr(out), N.ptr(dout), *ds, N.ptr(lse), N.ptr(delta), N.ptr(dq), N.ptr(dk), N.ptr(dv), N.dt(q), N.stream()),
        "mi355_softmax_attn_bwd")
    return dq, dk, dv


class SoftmaxAttn(torch.autograd.Function):
    """Softmax attention: the forward of prefill_attn.py (same kernel, same bits) with its backward."""

    @staticmethod
    def forward(ctx, q, k, v, cu_q, cu_k, max_q, max_k, mask, func, scale, skip_tiles):
        out, lse = _P._forward(q.detach(), k.detach(), v.detach(), cu_q, cu_k, max_q, mask, func, scale, skip_tiles)
        ctx.save_for_backward(q, k, v, out, lse, cu_q, cu_k, func)
        ctx.call = (max_q, max_k, mask, scale, skip_tiles)
        ctx.mark_non_differentiable(lse)
        return out, lse

    @staticmethod
    def backward(ctx, dout, _dlse):
        q, k, v, out, lse, cu_q, cu_k, func = ctx.saved_tensors
        max_q, max_k, mask, scale, skip_tiles = ctx.call
        dq, dk, dv = _backward(q.detach(), k.detach(), v.detach(), out, lse, dout, cu_q, cu_k, max_q, max_k, mask, func,
                               scale, skip_tiles)
        return dq, dk, dv, None, None, None, None, None, None, None, None


def flash_attn_func(q, k, v, softmax_scale: Optional[float] = None, causal: bool = False, arbitrary: bool = False,
                    linear_k_block_sparse_tensors=None, linear_q_block_sparse_tensors=None, aux_tensors=None,
                    return_lse: bool = False, skip_tiles: bool = True, **unsupported):
    """Dense softmax attention, differentiable in q, k, v.  q [B, Sq, Hq, D], k / v [B, Sk, Hkv, D] -> out [B, Sq, Hq, D]
    (and lse [B, Hq, Sq] fp32 with return_lse; lse carries no gradient).  causal is aligned bottom-right.  arbitrary=True
    takes aux_tensors=[arbitrary_func].  The two linear_*_block_sparse_tensors are accepted and not read: the kernels derive
    their own tile skipping, forward and backward, from the function."""
    mask, func = _P._validate_dense(q, k, v, causal, arbitrary, aux_tensors, unsupported, max_n_func=MAX_N_FUNC)
    out, lse = SoftmaxAttn.apply(q, k, v, None, None, 0, 0, mask, func, _P._scale(softmax_scale, q.shape[-1]), skip_tiles)
    return (out, lse) if return_lse else out


def flash_attn_varlen_func(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k,
                           softmax_scale: Optional[float] = None, causal: bool = False, return_lse: bool = False,
                           skip_tiles: bool = True, **unsupported):
    """Softmax attention over a flattened jagged batch, differentiable in q, k, v.  q [total_q, Hq, D], k / v
    [total_k, Hkv, D], cu_seqlens int32 [B + 1] -> out [total_q, Hq, D] (and lse [Hq, total_q] fp32 with return_lse).
    causal holds inside each sequence, aligned bottom-right.  max_seqlen_q bounds the forward and the dQ launch,
    max_seqlen_k the dK / dV launch: keys of a sequence at or past max_seqlen_k receive no gradient, so it must be at least
    the longest key sequence, as max_seqlen_q must be at least the longest query sequence."""
    cu_q, cu_k = _P._validate_varlen(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, unsupported)
    out, lse = SoftmaxAttn.apply(q, k, v, cu_q, cu_k, max_seqlen_q, max_seqlen_k,
                                 MASK_CAUSAL if causal else MASK_NONE, None, _P._scale(softmax_scale, q.shape[-1]), skip_tiles)
    return (out, lse) if return_lse else out
