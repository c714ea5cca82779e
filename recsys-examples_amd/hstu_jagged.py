"""`commons.ops.triton_ops.triton_jagged` of the reference on MI355X: the seven public functions of
examples/commons/ops/triton_ops/triton_jagged.py:1247-1360 with their names, argument names, order and defaults, over the
kernels of csrc/jagged_bmm.hip and csrc/jagged_ops.hip.  Every name is also bound without its `triton_` prefix.

* `triton_jagged_dense_bmm` / `triton_jagged_dense_bmm_broadcast_add`: out[rows of b] = jagged[rows of b] @ dense[b] (+ bias[b]),
  MFMA with fp32 accumulation.  The backward is the same kernel on dense[b]^T (read in place through its strides) for d_jagged
  and a jagged^T x jagged kernel for d_dense, whose column sum is d_bias.
* `triton_jagged_dense_broadcast_add`: out[rows of b] = jagged[rows of b] + dense[b]; d_jagged is d_out, d_dense a per-sample
  row sum.
* `triton_concat_2D_jagged`, `triton_concat_2D_jagged_jagged`, `triton_concat_2D_dense_jagged`: the mirror image of
  `split_2D_jagged` of hstu_cuda_ops over the same launch of mi355_jagged_concat.  `triton_split_2D_jagged` is that function.

Departures from the reference, all deliberate:
* `max_seq_len` is accepted and unused: the grids are sized from jagged.size(0) and the batch, so every row of a sample is
  computed however long the sample is, nothing is read back from an offset, and forward and backward capture into a graph.
* rows of `jagged` at or past seq_offsets[-1] are never read; the matching rows of the output and of d_jagged are zero.
* d_dense and d_bias are summed in an order fixed by the length of the sample: no atomics, bitwise reproducible.
* `is_replace=True` and `n_prefix_from_right != 0` (and `n_prefix_to_right != 0` of the split) raise NotImplementedError.
* There is no Triton here and no eager fallback: CPU tensors raise NativeError.
"""
from typing import Optional, Tuple

import torch

import mi355_native as N
from hstu_cuda_ops import _concat_launch, _offsets_i64, split_2D_jagged, triton_split_2D_jagged

__all__ = ["triton_jagged_dense_bmm", "triton_jagged_dense_bmm_broadcast_add", "triton_jagged_dense_broadcast_add",
           "triton_concat_2D_jagged", "triton_concat_2D_jagged_jagged", "triton_concat_2D_dense_jagged", "triton_split_2D_jagged",
           "jagged_dense_bmm", "jagged_dense_bmm_broadcast_add", "jagged_dense_broadcast_add", "concat_2D_jagged",
           "concat_2D_jagged_jagged", "concat_2D_dense_jagged", "split_2D_jagged"]


def _rows(t: torch.Tensor) -> torch.Tensor:
    """a 2-D tensor the kernels can read through its row stride: unit inner stride, else a copy"""
    return t if t.stride(1) == 1 or t.size(1) <= 1 else t.contiguous()


def _row_stride(t: torch.Tensor) -> int:
    return t.stride(0) if t.size(0) > 1 else max(t.stride(0), t.size(1))


def _check_jagged_dense(seq_offsets, jagged, dense, bias, dense_dims, what):
    if jagged.dim() != 2:
        raise ValueError(f"jagged must be 2-D, got {jagged.dim()}-D")
    if dense.dim() != dense_dims:
        raise ValueError(f"dense must be {dense_dims}-D, got {dense.dim()}-D")
    if seq_offsets.dim() != 1 or seq_offsets.numel() < 2:
        raise ValueError("seq_offsets must be 1-D with batch + 1 entries, batch >= 1")
    if seq_offsets.dtype.is_floating_point or seq_offsets.dtype == torch.bool:
        raise ValueError(f"seq_offsets must hold integers, got {seq_offsets.dtype}")
    B = seq_offsets.numel() - 1
    if dense.size(0) != B:
        raise ValueError(f"dense holds {dense.size(0)} samples, seq_offsets {B}")
    if dense.size(1) != jagged.size(1):
        raise ValueError(f"jagged is {tuple(jagged.shape)} and dense {tuple(dense.shape)}: the inner sizes differ")
    if bias is not None and (bias.dim() != 2 or bias.size(0) != B or bias.size(1) != dense.size(2)):
        raise ValueError(f"bias must be [{B}, {dense.size(2)}], got {tuple(bias.shape)}")
    ts = [t for t in (jagged, dense, bias) if t is not None]
    if not all(t.is_cuda for t in ts) or not seq_offsets.is_cuda:
        raise N.NativeError(f"{what} expects GPU tensors (no CPU fallback exists)")
    if jagged.dtype not in N._DT:
        raise N.NativeError(f"unsupported dtype {jagged.dtype}")
    if any(t.dtype != jagged.dtype for t in ts):
        raise ValueError("jagged, dense and bias must share one dtype")
    if any(t.device != jagged.device for t in ts) or seq_offsets.device != jagged.device:
        raise ValueError("all tensors must be on one device")
    return B


def _dense_bmm(offsets, B, rows, dense, transpose, bias, out):
    """out[r] = rows[r] @ dense[b] (or dense[b]^T) (+ bias[b]) for the rows of sample b; rows past offsets[-1] become zero"""
    sk, sn = (dense.stride(2), dense.stride(1)) if transpose else (dense.stride(1), dense.stride(2))
    n = dense.size(1) if transpose else dense.size(2)
    N.check(N.lib().mi355_jagged_dense_bmm(
        N.ptr(rows), _row_stride(rows), N.ptr(offsets), B, rows.size(0), rows.size(1), n, N.ptr(dense), dense.stride(0), sk, sn,
        N.ptr(bias), 0 if bias is None else _row_stride(bias), N.ptr(out), _row_stride(out), N.dt(rows), N.stream()),
        "mi355_jagged_dense_bmm")


class _JaggedDenseBmm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, offsets, jagged, dense, bias):
        # (the public functions have validated the arguments: int64 contiguous offsets, one dtype, one GPU)
        B, L = dense.size(0), jagged.size(0)
        out = jagged.new_empty((L, dense.size(2)))
        if L > 0:
            _dense_bmm(offsets, B, jagged, dense, False, bias, out)
        ctx.save_for_backward(offsets, jagged, dense)
        ctx.has_bias = bias is not None
        return out

    @staticmethod
    def backward(ctx, d_out):
        offsets, jagged, dense = ctx.saved_tensors
        B, L = dense.size(0), jagged.size(0)
        d_out = _rows(d_out)
        d_jagged = jagged.new_empty((L, jagged.size(1)))
        if L > 0:
            _dense_bmm(offsets, B, d_out, dense, True, None, d_jagged)
        d_dense = dense.new_empty(dense.shape)
        d_bias = dense.new_empty((B, dense.size(2))) if ctx.has_bias else None
        lib = N.lib()
        ws = torch.empty(int(lib.mi355_jagged_jagged_bmm_workspace_bytes(B, L, dense.size(1), dense.size(2))), dtype=torch.uint8,
                         device=dense.device)
        N.check(lib.mi355_jagged_jagged_bmm(
            N.ptr(jagged), _row_stride(jagged), N.ptr(d_out), _row_stride(d_out), N.ptr(offsets), B, L, dense.size(1),
            dense.size(2), N.ptr(d_dense), d_dense.stride(0), d_dense.stride(1), N.ptr(d_bias),
            0 if d_bias is None else d_bias.stride(0), N.dt(jagged), N.ptr(ws), ws.numel(), N.stream()), "mi355_jagged_jagged_bmm")
        return None, d_jagged, d_dense, d_bias


class _JaggedDenseBroadcastAdd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, offsets, jagged, dense):
        B, L, D = dense.size(0), jagged.size(0), jagged.size(1)
        out = torch.empty((L, D), dtype=jagged.dtype, device=jagged.device)
        if L > 0 and D > 0:
            N.check(N.lib().mi355_jagged_broadcast_add(
                N.ptr(jagged), _row_stride(jagged), N.ptr(offsets), B, L, D, N.ptr(dense), _row_stride(dense), N.ptr(out),
                _row_stride(out), N.dt(jagged), N.stream()), "mi355_jagged_broadcast_add")
        ctx.save_for_backward(offsets)
        return out

    @staticmethod
    def backward(ctx, d_out):
        (offsets,) = ctx.saved_tensors
        B, (L, D) = offsets.numel() - 1, d_out.shape
        rows = _rows(d_out)
        d_dense = d_out.new_empty((B, D))
        if D > 0:
            N.check(N.lib().mi355_jagged_row_sum(N.ptr(rows), _row_stride(rows), N.ptr(offsets), B, L, D, N.ptr(d_dense),
                                                 _row_stride(d_dense), N.dt(rows), N.stream()), "mi355_jagged_row_sum")
        return None, d_out, d_dense


def triton_jagged_dense_bmm(max_seq_len: int, seq_offsets: torch.Tensor, jagged: torch.Tensor,
                            dense: torch.Tensor) -> torch.Tensor:
    """out [L, N]: out[rows of b] = jagged[rows of b] @ dense[b], with jagged [L, K], dense [B, K, N] (read through its three
    strides) and seq_offsets [B + 1].  Differentiable in jagged and dense.  max_seq_len is unused."""
    _check_jagged_dense(seq_offsets, jagged, dense, None, 3, "jagged_dense_bmm")
    return _JaggedDenseBmm.apply(_offsets_i64(seq_offsets), _rows(jagged), dense, None)


def triton_jagged_dense_bmm_broadcast_add(max_seq_len: int, seq_offsets: torch.Tensor, jagged: torch.Tensor, dense: torch.Tensor,
                                          bias: torch.Tensor) -> torch.Tensor:
    """triton_jagged_dense_bmm with bias[b] ([B, N]) added to every row of sample b in fp32, before the one rounding"""
    _check_jagged_dense(seq_offsets, jagged, dense, bias, 3, "jagged_dense_bmm_broadcast_add")
    return _JaggedDenseBmm.apply(_offsets_i64(seq_offsets), _rows(jagged), dense, _rows(bias))


def triton_jagged_dense_broadcast_add(max_seq_len: int, seq_offsets: torch.Tensor, jagged: torch.Tensor,
                                      dense: torch.Tensor) -> torch.Tensor:
    """out [L, D]: out[rows of b] = jagged[rows of b] + dense[b], with dense [B, D].  max_seq_len is unused."""
    _check_jagged_dense(seq_offsets, jagged, dense, None, 2, "jagged_dense_broadcast_add")
    return _JaggedDenseBroadcastAdd.apply(_offsets_i64(seq_offsets), _rows(jagged), _rows(dense))


# ---------------------------------------------------------------------------------------------------------------------
# two-tensor concat: split_2D_jagged of hstu_cuda_ops run the other way
# ---------------------------------------------------------------------------------------------------------------------
class _Concat2DJagged(torch.autograd.Function):
    @staticmethod
    def forward(ctx, values_a, values_b, offsets_a, offsets_b):
        # (the public function has validated the arguments: int64 contiguous offsets, contiguous 2-D values on one GPU)
        merged_offsets = offsets_a + offsets_b
        merged = values_a.new_empty((values_a.size(0) + values_b.size(0), values_a.size(1)))
        if merged.size(0) > 0:
            _concat_launch([values_a, values_b], [offsets_a, offsets_b], merged_offsets, merged, 0, checked=True)
        ctx.save_for_backward(merged_offsets, offsets_a, offsets_b)
        ctx.shapes = (values_a.shape, values_b.shape)
        return merged

    @staticmethod
    def backward(ctx, grad):
        merged_offsets, offsets_a, offsets_b = ctx.saved_tensors
        grads = [grad.new_empty(s) for s in ctx.shapes]
        if grad.size(0) > 0:
            _concat_launch(grads, [offsets_a, offsets_b], merged_offsets, grad.contiguous(), 1, checked=True)
        return grads[0], grads[1], None, None


def triton_concat_2D_jagged(max_seq_len: int, values_a: torch.Tensor, values_b: torch.Tensor,
                            offsets_a: Optional[torch.Tensor] = None, offsets_b: Optional[torch.Tensor] = None,
                            is_replace: bool = False, n_prefix_from_right: int = 0) -> torch.Tensor:
    """Sample b of the result is sample b of values_a followed by sample b of values_b: [rows_a + rows_b, D].  A side whose
    offsets are None is dense, [B, dense_size, D], and gets its gradient back in that shape; at most one side may be.
    max_seq_len is unused.  is_replace and n_prefix_from_right are not implemented."""
    if is_replace:
        raise NotImplementedError("concat_2D_jagged: is_replace=True is not implemented")
    if n_prefix_from_right != 0:
        raise NotImplementedError("concat_2D_jagged: n_prefix_from_right != 0 is not implemented")
    if offsets_a is None and offsets_b is None:
        raise ValueError("offsets_a and offsets_b cannot both be None")
    for v, o, name in ((values_a, offsets_a, "values_a"), (values_b, offsets_b, "values_b")):
        want = 3 if o is None else 2
        if v.dim() != want:
            raise ValueError(f"{name} must be {want}-D, got {v.dim()}-D")
        if o is not None and (o.dim() != 1 or o.numel() < 2):
            raise ValueError("every offsets tensor must be 1-D with batch + 1 entries, batch >= 1")
    if values_a.size(-1) != values_b.size(-1):
        raise ValueError("values_a and values_b must have the same hidden dim")
    if offsets_a is not None and offsets_b is not None and offsets_a.numel() != offsets_b.numel():
        raise ValueError("offsets_a and offsets_b must hold the same number of entries")
    given = offsets_b if offsets_a is None else offsets_a
    if not (values_a.is_cuda and values_b.is_cuda and given.is_cuda):
        raise N.NativeError("concat_2D_jagged expects GPU tensors (no CPU fallback exists)")
    if values_a.dtype not in N._DT:
        raise N.NativeError(f"unsupported dtype {values_a.dtype}")
    if values_a.dtype != values_b.dtype:
        raise ValueError("values_a and values_b must share one dtype")
    if any(t.device != values_a.device for t in (values_b, offsets_a, offsets_b) if t is not None):
        raise ValueError("all tensors must be on one device")
    B, D = given.numel() - 1, values_a.size(-1)
    for v, o, name in ((values_a, offsets_a, "values_a"), (values_b, offsets_b, "values_b")):
        if o is None and v.size(0) != B:
            raise ValueError(f"{name} holds {v.size(0)} samples, the offsets {B}")
    dense = values_a if offsets_a is None else values_b if offsets_b is None else None
    if dense is not None:
        dense_offsets = torch.arange(B + 1, dtype=torch.int64, device=dense.device) * dense.size(1)
        offsets_a = dense_offsets if offsets_a is None else offsets_a
        offsets_b = dense_offsets if offsets_b is None else offsets_b
    # (reshape of a contiguous dense side is a view whose gradient autograd folds back to [B, dense_size, D])
    return _Concat2DJagged.apply(values_a.contiguous().reshape(-1, D), values_b.contiguous().reshape(-1, D),
                                 _offsets_i64(offsets_a), _offsets_i64(offsets_b))


def triton_concat_2D_jagged_jagged(max_seq_len_left: int, offsets_left: torch.Tensor, values_left: torch.Tensor,
                                   max_seq_len_right: int, offsets_right: torch.Tensor, values_right: torch.Tensor,
                                   is_replace: bool, n_prefix_from_right: int) -> torch.Tensor:
    return triton_concat_2D_jagged(max_seq_len=max_seq_len_left + max_seq_len_right, values_a=values_left,
                                   values_b=values_right, offsets_a=offsets_left, offsets_b=offsets_right,
                                   is_replace=is_replace, n_prefix_from_right=n_prefix_from_right)


def triton_concat_2D_dense_jagged(jagged_max_seq_len: int, jagged_offsets: torch.Tensor, jagged_values: torch.Tensor,
                                  dense_values: torch.Tensor) -> torch.Tensor:
    """dense_values [B, dense_size, D] in front of every sample of jagged_values"""
    if dense_values.dim() != 3:
        raise ValueError(f"dense_values must be 3-D, got {dense_values.dim()}-D")
    return triton_concat_2D_jagged(max_seq_len=jagged_max_seq_len + dense_values.size(1), values_a=dense_values,
                                   values_b=jagged_values, offsets_a=None, offsets_b=jagged_offsets)


jagged_dense_bmm = triton_jagged_dense_bmm
jagged_dense_bmm_broadcast_add = triton_jagged_dense_bmm_broadcast_add
jagged_dense_broadcast_add = triton_jagged_dense_broadcast_add
concat_2D_jagged = triton_concat_2D_jagged
concat_2D_jagged_jagged = triton_concat_2D_jagged_jagged
concat_2D_dense_jagged = triton_concat_2D_dense_jagged
