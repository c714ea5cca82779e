"""Softmax prefill attention of the semantic-ID generative-retrieval family on MI355X (forward only).

`flash_attn_func` and `flash_attn_varlen_func` take the arguments the reference passes to flash-attention
(examples/sid_gr/model/jagged_flash_attn_block.py, sid-gr-inference's gr_kernels/prefill/flash_attn_backend.py); the work is
done by `mi355_prefill_attn` (csrc/prefill_attn.hip): one launch of a flash-attention forward on the MFMA with GQA, a causal
mask aligned bottom-right, the interval masks of `arbitrary_func`, and key tiles skipped from the rows' extents.

    dense:   q [B, Sq, Hq, D], k / v [B, Sk, Hkv, D] (any batch / row / head strides)  -> out [B, Sq, Hq, D], lse [B, Hq, Sq]
    jagged:  q [total_q, Hq, D], k / v [total_k, Hkv, D], cu_seqlens_q / _k int32 [B+1] -> out [total_q, Hq, D], lse [Hq, total_q]
    arbitrary_func (aux_tensors[0], dense only): int32 [B, 1 or Hq, n_func (odd), >= Sq]; query i sees key j iff
        j < F[0][i], or F[2p-1][i] <= j < F[2p][i] for some p >= 1

The import names of the reference (`flash_attn`, `flash_attn.flash_attn_interface`, `flash_attn.cute.interface`) are the
package under flash_attn_gfx950/.  There is no eager fallback: without the library or a GPU the call raises.
"""
from __future__ import annotations

import math
from typing import Optional

import torch

import mi355_native as N
from mi355_native import rows_aligned as _rows_aligned

KEY_TILE = 64      # keys per tile (csrc/softmax_tile_dev.h: kSmKeys)
ROW_TILE = 128     # query rows per workgroup (kSmRows)
MASK_NONE, MASK_CAUSAL, MASK_FUNC = 0, 1, 2


class PrefillAttnError(N.NativeError, ValueError):
    """An argument the kernel cannot take.  Both a NativeError (like every refusal of this package) and a ValueError."""


def _bad(msg):
    raise PrefillAttnError(msg)


def _refuse_unsupported(kw):
    """flash-attn arguments this kernel does not carry: accepted at their defaults, refused otherwise (never ignored)"""
    defaults = {"dropout_p": (0.0, 0), "window_size": ((-1, -1), (None, None), None, [-1, -1]), "softcap": (0.0, 0, None),
                "alibi_slopes": (None,), "deterministic": (False, True), "return_attn_probs": (False,),
                "learnable_sink": (None,), "mask_mod": (None,), "score_mod": (None,), "block_table": (None,),
                "seqused_q": (None,), "seqused_k": (None,), "pack_gqa": (None,), "num_splits": (1, 0, None)}
    for name, val in kw.items():
        if name not in defaults:
            raise TypeError(f"unexpected keyword argument {name!r}")
        if not any(val is d or (not isinstance(val, torch.Tensor) and val == d) for d in defaults[name]):
            _bad(f"{name}={val!r} is not supported by the gfx950 prefill attention (only its default is)")


def _validate_qkv(q, k, v, jagged):
    for name, t in (("q", q), ("k", k), ("v", v)):
        if not isinstance(t, torch.Tensor):
            _bad(f"{name} must be a tensor, got {type(t).__name__}")
    nd = 3 if jagged else 4
    form = "[total, H, D] (jagged)" if jagged else "[B, S, H, D]"
    for name, t in (("q", q), ("k", k), ("v", v)):
        if t.dim() != nd:
            _bad(f"{name} must be {nd}-D {form}, got shape {tuple(t.shape)}")
    if v.shape != k.shape:
        _bad(f"v shape {tuple(v.shape)} differs from k shape {tuple(k.shape)}")
    if not jagged and k.shape[0] != q.shape[0]:
        _bad(f"k batch: expected {q.shape[0]}, got shape {tuple(k.shape)}")
    D, Hq, Hkv = q.shape[-1], q.shape[-2], k.shape[-2]
    if k.shape[-1] != D:
        _bad(f"k head dim: expected {D}, got shape {tuple(k.shape)}")
    if Hkv == 0 or Hq % Hkv != 0:
        _bad(f"head_q {Hq} is no multiple of head_kv {Hkv}")
    if q.dtype not in (torch.float16, torch.bfloat16):
        _bad(f"q must be fp16 or bf16, got {q.dtype}")
    if not (q.dtype == k.dtype == v.dtype):
        _bad(f"q / k / v dtypes differ: {q.dtype}, {k.dtype}, {v.dtype}")
    if D not in (64, 128):
        _bad(f"head dim must be 64 or 128, got q shape {tuple(q.shape)}")
    for name, t in (("q", q), ("k", k), ("v", v)):
        if t.numel() and t.stride(-1) != 1:
            _bad(f"{name} must have stride(-1) == 1, got strides {tuple(t.stride())}")


def _require_gpu(**tensors):
    for name, t in tensors.items():
        if t is not None and not t.is_cuda:
            raise PrefillAttnError(f"{name} must be a GPU tensor (there is no CPU path), got device {t.device}")


def _validate_dense(q, k, v, causal, arbitrary, aux_tensors, unsupported, max_n_func=None):
    """The checks of flash_attn_func, here and in softmax_attn.py: returns (mask, func).  max_n_func: the backward's limit."""
    _refuse_unsupported(unsupported)
    _validate_qkv(q, k, v, jagged=False)
    func = None
    mask = MASK_CAUSAL if causal else MASK_NONE
    if arbitrary:
        if causal:
            _bad("arbitrary=True with causal=True: put the causal bound into the arbitrary_func instead")
        if aux_tensors is None or len(aux_tensors) != 1:
            _bad(f"arbitrary=True needs exactly one aux tensor (the arbitrary_func), got "
                 f"{'None' if aux_tensors is None else len(aux_tensors)}")
        func = aux_tensors[0]
        if not isinstance(func, torch.Tensor) or func.dtype != torch.int32 or func.dim() != 4:
            _bad("arbitrary_func must be an int32 tensor [B, 1 or Hq, n_func, >= Sq], got "
                 f"{getattr(func, 'dtype', type(func).__name__)} {tuple(getattr(func, 'shape', ()))}")
        B, Sq, Hq = q.shape[0], q.shape[1], q.shape[2]
        if func.shape[0] != B or func.shape[1] not in (1, Hq) or func.shape[2] % 2 != 1 or func.shape[3] < Sq:
            _bad(f"arbitrary_func must be [B={B}, 1 or Hq={Hq}, n_func (odd), >= Sq={Sq}], got shape {tuple(func.shape)}")
        if max_n_func is not None and func.shape[2] > max_n_func:   # refused before the forward, not at backward time
            _bad(f"arbitrary_func with n_func={func.shape[2]} > {max_n_func} is not supported by the backward")
        mask = MASK_FUNC
    elif aux_tensors:
        _bad("aux_tensors are given but arbitrary=False")
    _require_gpu(q=q, k=k, v=v, arbitrary_func=func)
    return mask, func


def _validate_varlen(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, unsupported):
    """The checks of flash_attn_varlen_func, here and in softmax_attn.py: returns the contiguous (cu_seqlens_q, cu_seqlens_k)."""
    _refuse_unsupported(unsupported)
    _validate_qkv(q, k, v, jagged=True)
    for name, cu in (("cu_seqlens_q", cu_seqlens_q), ("cu_seqlens_k", cu_seqlens_k)):
        if not isinstance(cu, torch.Tensor) or cu.dim() != 1 or cu.dtype != torch.int32 or cu.shape[0] < 1:
            _bad(f"{name} must be an int32 tensor [B + 1], got {getattr(cu, 'dtype', type(cu).__name__)} "
                 f"{tuple(getattr(cu, 'shape', ()))}")
    if cu_seqlens_q.shape != cu_seqlens_k.shape:
        _bad(f"cu_seqlens_q {tuple(cu_seqlens_q.shape)} and cu_seqlens_k {tuple(cu_seqlens_k.shape)} differ in length")
    if not isinstance(max_seqlen_q, int) or max_seqlen_q < 0 or not isinstance(max_seqlen_k, int) or max_seqlen_k < 0:
        _bad(f"max_seqlen_q / max_seqlen_k must be non-negative ints, got {max_seqlen_q!r}, {max_seqlen_k!r}")
    _require_gpu(q=q, k=k, v=v, cu_seqlens_q=cu_seqlens_q, cu_seqlens_k=cu_seqlens_k)
    return cu_seqlens_q.contiguous(), cu_seqlens_k.contiguous()


def _strides(jagged, *tensors):
    """(batch, row, head) strides of each tensor as the C ABI takes them; a jagged tensor has no batch stride"""
    return [(0, t.stride(0), t.stride(1)) if jagged else t.stride()[:3] for t in tensors]


def _func_args(func):
    """func, n_func, func_heads and the four func strides of the C ABI"""
    if func is None:
        return (N.ptr(None), 0, 0, 0, 0, 0, 0)
    return (N.ptr(func), func.shape[2], func.shape[1], *func.stride())


def _forward(q, k, v, cu_q, cu_k, max_q, mask, func, scale, skip_tiles):
    jagged = cu_q is not None
    q, k, v = _rows_aligned(q), _rows_aligned(k), _rows_aligned(v)
    dev = q.device
    Hq, D, Hkv = q.shape[-2], q.shape[-1], k.shape[-2]
    if jagged:
        B, Sq, Sk, total_q, total_k = cu_q.shape[0] - 1, int(max_q), 0, q.shape[0], k.shape[0]
        out = torch.empty(total_q, Hq, D, device=dev, dtype=q.dtype)
        lse = torch.empty(Hq, total_q, device=dev, dtype=torch.float32)
    else:
        B, Sq, Sk, total_q, total_k = q.shape[0], q.shape[1], k.shape[1], 0, 0
        out = torch.empty(B, Sq, Hq, D, device=dev, dtype=q.dtype)
        lse = torch.empty(B, Hq, Sq, device=dev, dtype=torch.float32)
    qs, ks, vs = _strides(jagged, q, k, v)
    N.check(N.lib().mi355_prefill_attn(
        N.ptr(q), *qs, N.ptr(k), *ks, N.ptr(v), *vs, N.ptr(cu_q), N.ptr(cu_k),
        B, Sq, Sk, total_q, total_k, Hq, Hkv, D, mask, *_func_args(func), float(scale), int(skip_tiles),
        N.ptr(out), N.ptr(lse), N.dt(q), N.stream()), "mi355_prefill_attn")
    return out, lse


class PrefillAttn(torch.autograd.Function):
    """Softmax prefill attention (forward only)."""

    @staticmethod
    def forward(ctx, q, k, v, cu_q, cu_k, max_q, mask, func, scale, skip_tiles):
        out, lse = _forward(q.detach(), k.detach(), v.detach(), cu_q, cu_k, max_q, mask, func, scale, skip_tiles)
        ctx.mark_non_differentiable(lse)
        return out, lse

    @staticmethod
    def backward(ctx, *args):
        raise NotImplementedError("Prefill attention is forward-only")


def _scale(softmax_scale, D):
    return 1.0 / math.sqrt(D) if softmax_scale is None else float(softmax_scale)


def flash_attn_func(q, k, v, softmax_scale: Optional[float] = None, causal: bool = False, arbitrary: bool = False,
                    linear_k_block_sparse_tensors=None, linear_q_block_sparse_tensors=None, aux_tensors=None,
                    return_lse: bool = False, skip_tiles: bool = True, **unsupported):
    """Dense softmax attention.  q [B, Sq, Hq, D], k / v [B, Sk, Hkv, D] -> out [B, Sq, Hq, D] (and lse [B, Hq, Sq] fp32
    with return_lse).  causal is aligned bottom-right.  arbitrary=True takes aux_tensors=[arbitrary_func].  The two
    linear_*_block_sparse_tensors are accepted and not read: the kernel derives its own tile skipping from the function."""
    mask, func = _validate_dense(q, k, v, causal, arbitrary, aux_tensors, unsupported)
    out, lse = PrefillAttn.apply(q, k, v, None, None, 0, mask, func, _scale(softmax_scale, q.shape[-1]), skip_tiles)
    return (out, lse) if return_lse else out


def flash_attn_varlen_func(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k,
                           softmax_scale: Optional[float] = None, causal: bool = False, return_lse: bool = False,
                           skip_tiles: bool = True, **unsupported):
    """Softmax attention over a flattened jagged batch.  q [total_q, Hq, D], k / v [total_k, Hkv, D], cu_seqlens int32
    [B + 1] -> out [total_q, Hq, D] (and lse [Hq, total_q] fp32 with return_lse).  causal holds inside each sequence,
    aligned bottom-right.  max_seqlen_q bounds the launch: rows of a sequence at or past it are not computed.
    max_seqlen_k is not needed."""
    cu_q, cu_k = _validate_varlen(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, unsupported)
    out, lse = PrefillAttn.apply(q, k, v, cu_q, cu_k, max_seqlen_q,
                                 MASK_CAUSAL if causal else MASK_NONE, None, _scale(softmax_scale, q.shape[-1]), skip_tiles)
    return (out, lse) if return_lse else out


class MI355PrefillBackend:
    """A callable with the shape of sid-gr-inference's PrefillBackend (gr_kernels/prefill/base.py): takes an object with
    .q [B, S, Hq, D], .k, .v [B, S, Hkv, D] and .causal, returns the hidden tensor [B, S, Hq, D]."""

    name = "mi355"

    def __call__(self, inputs):
        scale = getattr(inputs, "softmax_scale", None)
        return flash_attn_func(inputs.q, inputs.k, inputs.v, softmax_scale=scale, causal=bool(inputs.causal))
