"""The FBGEMM sparse / jagged ops that the reference's examples/hstu calls directly as `torch.ops.fbgemm.*`, on MI355X.

`fbgemm_gpu` is not part of the ROCm image and a hipified FBGEMM is out of the question, so importing this module (or the
`fbgemm_gpu` package next to it, which does nothing else) registers these ops with FBGEMM's own schemas:

    asynchronous_complete_cumsum / asynchronous_inclusive_cumsum / asynchronous_exclusive_cumsum
    jagged_to_padded_dense, jagged_2d_to_dense, dense_to_jagged
    keyed_jagged_index_select_dim1

* "CUDA" runs the kernels of csrc/fbgemm_jagged.hip through the C ABI.  A dtype the kernels do not cover raises; there is no
  eager fallback on the GPU.  One measured exception: asynchronous_inclusive_cumsum of more than 8192 elements is torch.cumsum,
  which is faster than the clear-and-look-back launches of the scan there (see _cumsum_cuda).  The library is loaded on first use, so the import itself needs no GPU.
* "CPU" is a composition of torch statements (datasets and the host side of the batch shuffler call these ops on CPU tensors).
  The compositions are device-agnostic: tools/bench_fbgemm_jagged.py times them on GPU tensors as the yardstick.
* "Meta" where the output shape is static: the cumsums, the two to-dense ops, dense_to_jagged with total_L.
* jagged_to_padded_dense, jagged_2d_to_dense and dense_to_jagged are differentiable in the values / dense argument; each
  backward is the opposite op with padding 0.  keyed_jagged_index_select_dim1 is not differentiable and says so.
* An op that is already registered (a real fbgemm_gpu imported first) is left alone.

Differences from FBGEMM, all on undefined or unused ground: one offsets level only (no caller passes more); an index outside
[0, batch) of the select yields an empty bag instead of undefined behaviour.  dense_to_jagged without total_L and the select
without selected_lengths_sum read one scalar on the host to size their output, as FBGEMM does; with the size given nothing is
read and the ops capture into a graph."""
import functools
from typing import List, Optional, Sequence

import torch

import mi355_native as N

SCHEMAS = {
    "asynchronous_complete_cumsum": "asynchronous_complete_cumsum(Tensor t_in) -> Tensor",
    "asynchronous_inclusive_cumsum": "asynchronous_inclusive_cumsum(Tensor t_in) -> Tensor",
    "asynchronous_exclusive_cumsum": "asynchronous_exclusive_cumsum(Tensor t_in) -> Tensor",
    "jagged_to_padded_dense": "jagged_to_padded_dense(Tensor values, Tensor[] offsets, SymInt[] max_lengths, "
                              "float padding_value=0.0) -> Tensor",
    "jagged_2d_to_dense": "jagged_2d_to_dense(Tensor values, Tensor offsets, SymInt max_sequence_length) -> Tensor",
    "dense_to_jagged": "dense_to_jagged(Tensor dense, Tensor[] x_offsets, SymInt? total_L=None) -> (Tensor, Tensor[])",
    "keyed_jagged_index_select_dim1": "keyed_jagged_index_select_dim1(Tensor values, Tensor lengths, Tensor offsets, "
                                      "Tensor indices, SymInt batch_size, Tensor? weights=None, "
                                      "SymInt? selected_lengths_sum=None) -> Tensor[]",
}

_ITYPE = {torch.int32: 0, torch.int64: 1}
_BITS_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
COMPLETE, INCLUSIVE, EXCLUSIVE = 0, 1, 2
ONE_BLOCK_SCAN = 8192   # the longest row mi355_cumsum scans with one block and no workspace (mi355_cumsum_workspace_bytes)


def _already_there(name: str) -> bool:
    try:
        getattr(torch.ops.fbgemm, name)
        return True
    except (AttributeError, RuntimeError):
        return False


def _check(cond, msg):
    if not cond:
        raise RuntimeError(msg)


def _itype(t: torch.Tensor, what: str) -> int:
    try:
        return _ITYPE[t.dtype]
    except KeyError:
        raise N.NativeError(f"{what} must be int32 or int64, got {t.dtype}")


def _one_level(offsets: Sequence[torch.Tensor], lengths: Optional[Sequence[int]] = None) -> torch.Tensor:
    if len(offsets) != 1 or (lengths is not None and len(lengths) != 1):
        raise NotImplementedError("only one level of jagged offsets is implemented (no caller of examples/hstu passes more)")
    off = offsets[0]
    _check(off.dim() == 1 and off.numel() >= 1, "offsets must be 1-D with batch + 1 entries")
    return off


def _pad_bits(dtype: torch.dtype, value: float) -> int:
    """the padding element as raw bits (host only: a one-element CPU tensor)"""
    t = torch.tensor([value], dtype=dtype)
    return int(t.view(_BITS_VIEW[t.element_size()]).item()) & ((1 << (8 * t.element_size())) - 1)


# ---------------------------------------------------------------------------------------------------------------------
# cumulative sums
# ---------------------------------------------------------------------------------------------------------------------
def _cumsum_check(mode, t):
    if mode == COMPLETE:
        _check(t.dim() in (1, 2), f"asynchronous_complete_cumsum takes a 1-D or 2-D tensor, got {t.dim()}-D")
    else:
        _check(t.dim() == 1, f"the inclusive / exclusive cumsum takes a 1-D tensor, got {t.dim()}-D")


def _cumsum_shape(mode, t):
    return tuple(t.shape[:-1]) + (t.size(-1) + 1,) if mode == COMPLETE else tuple(t.shape)


def _cumsum_torch(mode, t):
    _cumsum_check(mode, t)
    inc = torch.cumsum(t, -1, dtype=t.dtype)
    if mode == INCLUSIVE:
        return inc
    if mode == EXCLUSIVE:
        return inc - t
    out = t.new_zeros(_cumsum_shape(mode, t))
    out[..., 1:] = inc
    return out


_CUMSUM = None


def _bind_cumsum():
    global _CUMSUM
    _CUMSUM = N.lib().mi355_cumsum
    return _CUMSUM


def _cumsum_cuda(mode, t, kernel_only=False):
    """kernel_only: the tests' and the benchmark's way to the look-back kernel in inclusive mode (see below).
    The whole call is host-bound at the example's sizes, so the common case -- a short contiguous vector -- goes first and
    straight to the launch."""
    it = _ITYPE.get(t.dtype)
    if t.dim() == 1 and it is not None:
        n = t.numel()
        if 0 < n <= ONE_BLOCK_SCAN and t.is_contiguous():
            out = t.new_empty(n + 1) if mode == COMPLETE else torch.empty_like(t)
            rc = (_CUMSUM or _bind_cumsum())(t.data_ptr(), out.data_ptr(), 1, n, it, mode, None, 0, N.stream())
            if rc != 0:
                N.check(rc, "mi355_cumsum")
            return out
        if mode == INCLUSIVE and n > ONE_BLOCK_SCAN and not kernel_only:
            return torch.cumsum(t, 0, dtype=t.dtype)   # (why: below)
    _cumsum_check(mode, t)
    it = _itype(t, "the input of a cumsum")
    n = t.size(-1)
    if mode == INCLUSIVE and n > ONE_BLOCK_SCAN and not kernel_only:
        # Past one block's reach the scan is a clearing launch and one or more look-back launches, and rocPRIM's scan is
        # faster on the GPU (10.4 us against 12.6 us at 1 M int64 inside a graph, profiles/fbgemm_jagged_bench.txt); for the
        # inclusive sum torch.cumsum IS the whole composition, with no zeros / copy / subtract launch to save.  The complete and
        # exclusive sums keep the kernel there (1.5-1.6x and 1.0-1.2x the composition at 1 M).
        return torch.cumsum(t, 0, dtype=t.dtype)
    rows = t.numel() // n if n else (t.size(0) if t.dim() == 2 else 1)
    if n == 0 or rows == 0:
        return t.new_zeros(_cumsum_shape(mode, t))
    t = t if t.is_contiguous() else t.contiguous()
    out = t.new_empty(_cumsum_shape(mode, t))
    lib = N.lib()
    # (up to ONE_BLOCK_SCAN elements a row is one block's: no look-back, no workspace)
    ws_bytes = lib.mi355_cumsum_workspace_bytes(rows, n) if n > ONE_BLOCK_SCAN else 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=t.device) if ws_bytes else None
    rc = lib.mi355_cumsum(t.data_ptr(), out.data_ptr(), rows, n, it, mode, ws.data_ptr() if ws_bytes else None, ws_bytes,
                          N.stream())
    if rc != 0:
        N.check(rc, "mi355_cumsum")
    return out


def _cumsum_meta(mode, t):
    _cumsum_check(mode, t)
    return t.new_empty(_cumsum_shape(mode, t))


# ---------------------------------------------------------------------------------------------------------------------
# jagged <-> padded dense
# ---------------------------------------------------------------------------------------------------------------------
def _as_rows(values: torch.Tensor) -> torch.Tensor:
    _check(values.dim() in (1, 2), f"values must be 1-D or 2-D, got {values.dim()}-D")
    return values.unsqueeze(-1) if values.dim() == 1 else values


def _to_padded_torch(values, off, max_len, padding_value):
    """[T, D] -> [B, max_len, D] by an index gather"""
    T, D = values.shape
    B = off.numel() - 1
    o = off.to(torch.int64)
    ar = torch.arange(max_len, dtype=torch.int64, device=values.device)
    idx = o[:-1].unsqueeze(1) + ar.unsqueeze(0)
    valid = (ar.unsqueeze(0) < (o[1:] - o[:-1]).unsqueeze(1)) & (idx >= 0) & (idx < T)
    pad = torch.full((), padding_value, dtype=values.dtype, device=values.device)
    if T == 0 or B * max_len == 0:
        return pad.expand(B, max_len, D).clone()
    rows = values.index_select(0, torch.where(valid, idx, torch.zeros_like(idx)).reshape(-1)).view(B, max_len, D)
    return torch.where(valid.unsqueeze(-1), rows, pad)


def _to_padded_cuda(values, off, max_len, padding_value):
    T, D = values.shape
    B = off.numel() - 1
    eb = values.element_size()
    if eb not in (2, 4, 8) or values.is_complex():
        raise N.NativeError(f"jagged_to_padded_dense: unsupported dtype {values.dtype}")
    _check(D >= 1, "jagged_to_padded_dense: the inner dimension must not be empty")
    _check(off.device == values.device, "offsets must be on the device of the values")
    it = _itype(off, "offsets")
    values = values if values.is_contiguous() else values.contiguous()
    off = off if off.is_contiguous() else off.contiguous()
    out = values.new_empty((B, max_len, D))
    if out.numel():
        rc = N.lib().mi355_jagged_to_padded(values.data_ptr(), T, off.data_ptr(), it, B, max_len, D, eb,
                                            _pad_bits(values.dtype, padding_value), out.data_ptr(), N.stream())
        if rc != 0:
            N.check(rc, "mi355_jagged_to_padded")
    return out


def _to_jagged_torch(dense, off, total):
    """[B, N, D] -> [total, D] by an index gather; rows past N and rows of no sample are zeros"""
    B, Nn, D = dense.shape
    out_shape = (total, D)
    if B == 0 or Nn == 0 or total == 0:
        return dense.new_zeros(out_shape)
    o = off.to(torch.int64)
    rows = torch.arange(total, dtype=torch.int64, device=dense.device)
    b = (torch.searchsorted(o, rows, right=True) - 1).clamp(0, B - 1)
    pos = rows - o[b]
    valid = (pos >= 0) & (pos < Nn) & (rows < o[b + 1])
    flat = dense.reshape(B * Nn, D)
    picked = flat.index_select(0, torch.where(valid, b * Nn + pos, torch.zeros_like(pos)))
    return torch.where(valid.unsqueeze(-1), picked, torch.zeros((), dtype=dense.dtype, device=dense.device))


def _to_jagged_cuda(dense, off, total):
    B, Nn, D = dense.shape
    eb = dense.element_size()
    if eb not in (2, 4, 8) or dense.is_complex():
        raise N.NativeError(f"dense_to_jagged: unsupported dtype {dense.dtype}")
    _check(D >= 1, "dense_to_jagged: the inner dimension must not be empty")
    _check(off.device == dense.device, "offsets must be on the device of the dense tensor")
    it = _itype(off, "offsets")
    if dense.stride(2) != 1 and D > 1:
        dense = dense.contiguous()   # the slices the reference passes keep the inner dimension contiguous: no copy for them
    off = off if off.is_contiguous() else off.contiguous()
    out = dense.new_empty((total, D))
    if out.numel():
        rc = N.lib().mi355_padded_to_jagged(dense.data_ptr(), dense.stride(0), dense.stride(1), B, Nn, off.data_ptr(), it, D, eb,
                                            out.data_ptr(), total, N.stream())
        if rc != 0:
            N.check(rc, "mi355_padded_to_jagged")
    return out


def _total_rows(off: torch.Tensor, total_L) -> int:
    # FBGEMM reads the last offset here too
    return int(off[-1].item()) if total_L is None else int(total_L)


def _dense_rows(dense: torch.Tensor) -> torch.Tensor:
    _check(dense.dim() in (2, 3), f"dense must be [B, N] or [B, N, D], got {dense.dim()}-D")
    return dense.unsqueeze(-1) if dense.dim() == 2 else dense


def _jagged_to_padded_dense(cuda, values, offsets, max_lengths, padding_value=0.0):
    off = _one_level(offsets, max_lengths)
    rows = _as_rows(values)
    out = (_to_padded_cuda if cuda else _to_padded_torch)(rows, off, int(max_lengths[0]), padding_value)
    return out.squeeze(-1) if values.dim() == 1 else out


def _jagged_2d_to_dense(cuda, values, offsets, max_sequence_length):
    _check(values.dim() == 2, f"jagged_2d_to_dense: values must be 2-D, got {values.dim()}-D")
    return _jagged_to_padded_dense(cuda, values, [offsets], [max_sequence_length], 0.0)


def _dense_to_jagged(cuda, dense, x_offsets, total_L=None):
    off = _one_level(x_offsets)
    rows = _dense_rows(dense)
    _check(off.numel() == rows.size(0) + 1, "x_offsets must hold batch + 1 entries")
    out = (_to_jagged_cuda if cuda else _to_jagged_torch)(rows, off, _total_rows(off, total_L))
    return (out.squeeze(-1) if dense.dim() == 2 else out), list(x_offsets)


def _jagged_to_padded_dense_meta(values, offsets, max_lengths, padding_value=0.0):
    off = _one_level(offsets, max_lengths)
    rows = _as_rows(values)
    out = rows.new_empty((off.numel() - 1, max_lengths[0], rows.size(1)))
    return out.squeeze(-1) if values.dim() == 1 else out


def _jagged_2d_to_dense_meta(values, offsets, max_sequence_length):
    return _jagged_to_padded_dense_meta(values, [offsets], [max_sequence_length])


def _dense_to_jagged_meta(dense, x_offsets, total_L=None):
    _one_level(x_offsets)
    if total_L is None:
        raise RuntimeError("dense_to_jagged without total_L has a data-dependent output shape: pass total_L to trace it")
    rows = _dense_rows(dense)
    out = rows.new_empty((total_L, rows.size(2)))
    return (out.squeeze(-1) if dense.dim() == 2 else out), list(x_offsets)


def _below_autograd():
    return torch._C._AutoDispatchBelowAutograd()


class _ToPadded(torch.autograd.Function):
    @staticmethod
    def forward(ctx, values, off, max_len, padding_value):
        with _below_autograd():
            out = torch.ops.fbgemm.jagged_to_padded_dense(values, [off], [max_len], padding_value)
        ctx.save_for_backward(off)
        ctx.rows = values.size(0)
        return out

    @staticmethod
    def backward(ctx, grad):
        # truncated rows and value rows of no sample get zeros
        (off,) = ctx.saved_tensors
        return torch.ops.fbgemm.dense_to_jagged(grad, [off], ctx.rows)[0], None, None, None


class _ToJagged(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dense, off, total_L):
        with _below_autograd():
            out = torch.ops.fbgemm.dense_to_jagged(dense, [off], total_L)[0]
        ctx.save_for_backward(off)
        ctx.max_len = dense.size(1)
        return out

    @staticmethod
    def backward(ctx, grad):
        # padded positions of dense get zeros
        (off,) = ctx.saved_tensors
        return torch.ops.fbgemm.jagged_to_padded_dense(grad, [off], [ctx.max_len], 0.0), None, None


def _jagged_to_padded_dense_autograd(values, offsets, max_lengths, padding_value=0.0):
    off = _one_level(offsets, max_lengths)
    return _ToPadded.apply(values, off, max_lengths[0], padding_value)


def _jagged_2d_to_dense_autograd(values, offsets, max_sequence_length):
    _check(values.dim() == 2, f"jagged_2d_to_dense: values must be 2-D, got {values.dim()}-D")
    return _ToPadded.apply(values, offsets, max_sequence_length, 0.0)


def _dense_to_jagged_autograd(dense, x_offsets, total_L=None):
    off = _one_level(x_offsets)
    return _ToJagged.apply(dense, off, total_L), list(x_offsets)


# ---------------------------------------------------------------------------------------------------------------------
# KeyedJaggedTensor batch select
# ---------------------------------------------------------------------------------------------------------------------
def _select_check(values, lengths, offsets, indices, batch_size, weights):
    _check(values.dim() == 1 and lengths.dim() == 1 and offsets.dim() == 1 and indices.dim() == 1,
           "keyed_jagged_index_select_dim1: values, lengths, offsets and indices must be 1-D")
    _check(batch_size >= 0 and (lengths.numel() % batch_size == 0 if batch_size else lengths.numel() == 0),
           f"lengths.numel()={lengths.numel()} must be a multiple of batch_size={batch_size}")
    _check(offsets.numel() == lengths.numel() + 1, "offsets must hold lengths.numel() + 1 entries")
    _check(weights is None or weights.shape == values.shape, "weights must have the shape of values")
    for t in (lengths, offsets, indices, weights):
        _check(t is None or t.device == values.device, "every tensor must be on the device of the values")
    return lengths.numel() // batch_size if batch_size else 0


def _select_torch(values, lengths, offsets, indices, batch_size, weights=None, selected_lengths_sum=None):
    F = _select_check(values, lengths, offsets, indices, batch_size, weights)
    B, S = batch_size, indices.numel()
    idx = indices.to(torch.int64)
    ok = (idx >= 0) & (idx < B)
    idx = idx.clamp(0, max(B - 1, 0))
    if F == 0 or S == 0:
        out_lengths = lengths.new_zeros(F * S)
        empty = [values.new_empty(0), out_lengths]
        return empty + [weights.new_empty(0)] if weights is not None else empty
    picked = lengths.view(F, B).index_select(1, idx)
    out_lengths = torch.where(ok.unsqueeze(0), picked, torch.zeros_like(picked)).reshape(-1)
    starts = offsets[:-1].view(F, B).index_select(1, idx).reshape(-1).to(torch.int64)
    ol = out_lengths.to(torch.int64)
    out_starts = torch.cumsum(ol, 0) - ol
    total = int(ol.sum().item()) if selected_lengths_sum is None else int(selected_lengths_sum)
    delta = torch.repeat_interleave(starts - out_starts, ol, output_size=total)
    src = torch.arange(total, dtype=torch.int64, device=values.device) + delta
    out = [values.index_select(0, src), out_lengths]
    if weights is not None:
        out.append(weights.index_select(0, src))
    return out


def _select_cuda(values, lengths, offsets, indices, batch_size, weights=None, selected_lengths_sum=None):
    F = _select_check(values, lengths, offsets, indices, batch_size, weights)
    B, S = batch_size, indices.numel()
    eb = values.element_size()
    if eb not in (1, 2, 4, 8) or values.is_complex():
        raise N.NativeError(f"keyed_jagged_index_select_dim1: unsupported values dtype {values.dtype}")
    wb = 0
    if weights is not None:
        wb = weights.element_size()
        if wb not in (2, 4, 8) or weights.is_complex():
            raise N.NativeError(f"keyed_jagged_index_select_dim1: unsupported weights dtype {weights.dtype}")
        weights = weights if weights.is_contiguous() else weights.contiguous()
    lt, ot, xt = _itype(lengths, "lengths"), _itype(offsets, "offsets"), _itype(indices, "indices")
    values, lengths, offsets, indices = (t if t.is_contiguous() else t.contiguous() for t in (values, lengths, offsets, indices))
    lib, stream = N.lib(), N.stream()
    out_lengths = lengths.new_empty(F * S)
    if F * S:
        rc = lib.mi355_kjt_select_lengths(lengths.data_ptr(), lt, indices.data_ptr(), xt, F, B, S, out_lengths.data_ptr(), stream)
        if rc != 0:
            N.check(rc, "mi355_kjt_select_lengths")
    out_offsets = _cumsum_cuda(COMPLETE, out_lengths)
    # FBGEMM reads the last output offset here too
    total = int(out_offsets[-1].item()) if selected_lengths_sum is None else int(selected_lengths_sum)
    # (no bags at all: the kernel has nothing to do, and a non-zero selected_lengths_sum still gets defined -- zero -- elements)
    alloc = torch.Tensor.new_empty if F * S else torch.Tensor.new_zeros
    out_values = alloc(values, total)
    out_weights = alloc(weights, total) if weights is not None else None
    if total and F * S:
        rc = lib.mi355_kjt_select_values(values.data_ptr(), values.numel(), eb, weights.data_ptr() if wb else None, wb,
                                         offsets.data_ptr(), ot, indices.data_ptr(), xt, F, B, S, out_offsets.data_ptr(), lt,
                                         out_values.data_ptr(), out_weights.data_ptr() if wb else None, total, stream)
        if rc != 0:
            N.check(rc, "mi355_kjt_select_values")
    return [out_values, out_lengths] + ([out_weights] if weights is not None else [])


def _select_autograd(values, lengths, offsets, indices, batch_size, weights=None, selected_lengths_sum=None):
    if values.requires_grad:
        raise RuntimeError("keyed_jagged_index_select_dim1 is not differentiable here: values.requires_grad is set "
                           "(every caller of examples/ passes ids)")
    with _below_autograd():
        return torch.ops.fbgemm.keyed_jagged_index_select_dim1(values, lengths, offsets, indices, batch_size, weights,
                                                               selected_lengths_sum)


# ---------------------------------------------------------------------------------------------------------------------
# registration
# ---------------------------------------------------------------------------------------------------------------------
def _bind_backend(fn, first):
    return functools.partial(fn, first)   # (no Python frame of its own: these calls are host-bound)


# op -> (CPU, CUDA, Meta or None, Autograd or None)
_IMPLS = {
    "asynchronous_complete_cumsum": (_bind_backend(_cumsum_torch, COMPLETE), _bind_backend(_cumsum_cuda, COMPLETE),
                                     _bind_backend(_cumsum_meta, COMPLETE), None),
    "asynchronous_inclusive_cumsum": (_bind_backend(_cumsum_torch, INCLUSIVE), _bind_backend(_cumsum_cuda, INCLUSIVE),
                                      _bind_backend(_cumsum_meta, INCLUSIVE), None),
    "asynchronous_exclusive_cumsum": (_bind_backend(_cumsum_torch, EXCLUSIVE), _bind_backend(_cumsum_cuda, EXCLUSIVE),
                                      _bind_backend(_cumsum_meta, EXCLUSIVE), None),
    "jagged_to_padded_dense": (_bind_backend(_jagged_to_padded_dense, False), _bind_backend(_jagged_to_padded_dense, True),
                               _jagged_to_padded_dense_meta, _jagged_to_padded_dense_autograd),
    "jagged_2d_to_dense": (_bind_backend(_jagged_2d_to_dense, False), _bind_backend(_jagged_2d_to_dense, True),
                           _jagged_2d_to_dense_meta, _jagged_2d_to_dense_autograd),
    "dense_to_jagged": (_bind_backend(_dense_to_jagged, False), _bind_backend(_dense_to_jagged, True),
                        _dense_to_jagged_meta, _dense_to_jagged_autograd),
    "keyed_jagged_index_select_dim1": (_select_torch, _select_cuda, None, _select_autograd),
}

# what the CPU implementations are made of, for the benchmark's "composition" column
COMPOSITIONS = {name: impls[0] for name, impls in _IMPLS.items()}

REGISTERED: List[str] = []
_lib = None
for _name, (_cpu, _cuda, _meta, _autograd) in _IMPLS.items():
    if _already_there(_name):
        continue   # a real fbgemm_gpu wins
    if _lib is None:
        _lib = torch.library.Library("fbgemm", "FRAGMENT")
    _lib.define(SCHEMAS[_name])
    _lib.impl(_name, _cpu, "CPU")
    _lib.impl(_name, _cuda, "CUDA")
    if _meta is not None:
        _lib.impl(_name, _meta, "Meta")
    if _autograd is not None:
        _lib.impl(_name, _autograd, "Autograd")
    REGISTERED.append(_name)
