"""The HSTU positional encoder on MI355X: `add_position_embeddings`, `add_timestamp_positional_embeddings` and the module
`HSTUPositionalEncoder` of the reference (examples/hstu/ops/triton_ops/triton_position.py:659-699 and
examples/hstu/modules/position_encoder.py:71-178), over the kernels of csrc/position_ops.hip.

* Both functions are autograd functions with the reference's argument names and order; they are also exported under the
  reference's names `triton_add_position_embeddings` / `triton_add_timestamp_positional_embeddings`, so binding them is a
  one-line import change in position_encoder.py.  There is no Triton here and no eager fallback: CPU
  tensors raise.
* Offsets, lengths, high indices, index offsets and target counts of any integer dtype are converted to int64 with device ops;
  nothing is read back to the host, so the forward is capturable into a graph.
* Inputs may be row-strided (a column slice of a wider tensor); only a strided LAST dimension is copied.
* Where the reference reads a table row out of bounds (an index past the table), the kernels clamp the row index.
"""
from math import sqrt
from typing import Optional

import torch

import mi355_native as N

__all__ = ["add_position_embeddings", "add_timestamp_positional_embeddings", "triton_add_position_embeddings",
           "triton_add_timestamp_positional_embeddings", "HSTUPositionalEncoder"]

# the constants the reference passes to its kernel (triton_position.py:541-544)
NUM_TIME_BUCKETS = 2048
TIME_BUCKET_INCREMENTS = 60.0
TIME_BUCKET_SCALE = 1.0
TIME_DELTA = 0
_BUCKET_FN = {"sqrt": 0, "log": 1}
_INT_DTYPES = (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8)


def _i64(t: torch.Tensor) -> torch.Tensor:
    return t if t.dtype == torch.int64 and t.is_contiguous() else t.to(torch.int64).contiguous()


def _rows(t: torch.Tensor) -> torch.Tensor:
    """a 2-D tensor whose last dimension is contiguous (any row stride)"""
    return t if t.stride(1) == 1 and t.stride(0) >= t.size(1) else t.contiguous()


def _stride(t: torch.Tensor) -> int:
    return t.stride(0) if t.size(0) > 1 else t.size(1)


def _workspace(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 32), dtype=torch.uint8, device=device)


def _check_int(t, name, numel=None):
    if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.dtype not in _INT_DTYPES:
        raise ValueError(f"{name} must be a 1-D integer tensor")
    if numel is not None and t.numel() != numel:
        raise ValueError(f"{name} must hold {numel} entries, got {t.numel()}")


def _check_table(table, name, D, dtype):
    if table.dim() != 2:
        raise ValueError(f"{name} must be 2-D, got {table.dim()}-D")
    if table.size(1) != D:
        raise ValueError(f"shape[1] of {name} ({table.size(1)}) must match the embedding dim ({D})")
    if table.size(0) < 1:
        raise ValueError(f"{name} must hold at least one row")
    if table.dtype not in (torch.float32, dtype):
        raise ValueError(f"{name} must be float32 or {dtype}, got {table.dtype}")


def _require_gpu(*ts):
    dev = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise N.NativeError("the positional encoder expects GPU tensors (no CPU fallback exists)")
        if dev is not None and t.device != dev:
            raise ValueError("all tensors must be on one device")
        dev = t.device


def _check_position_args(jagged, jagged_offsets, high_inds, dense, ind_offsets):
    if jagged.dim() != 2:
        raise ValueError(f"jagged must be 2-D, got {jagged.dim()}-D")
    if jagged.dtype not in N._DT:
        raise N.NativeError(f"unsupported dtype {jagged.dtype}")
    _check_table(dense, "dense", jagged.size(1), jagged.dtype)
    _check_int(jagged_offsets, "jagged_offsets")
    _check_int(high_inds, "high_inds")
    if jagged_offsets.numel() - 1 != high_inds.numel() or high_inds.numel() < 1:
        raise ValueError("wrong jagged_offsets shape[0]: it must hold high_inds.numel() + 1 entries (batch >= 1)")
    if ind_offsets is not None:
        _check_int(ind_offsets, "ind_offsets", high_inds.numel())
    _require_gpu(jagged, jagged_offsets, high_inds, dense, ind_offsets)


class _AddPositionEmbeddings(torch.autograd.Function):
    @staticmethod
    def forward(ctx, jagged, jagged_offsets, high_inds, max_seq_len, dense, scale, ind_offsets):
        jagged, dense = _rows(jagged), _rows(dense)
        offsets, high = _i64(jagged_offsets), _i64(high_inds)
        ind = None if ind_offsets is None else _i64(ind_offsets)
        rows, D = jagged.shape
        out = torch.empty((rows, D), dtype=jagged.dtype, device=jagged.device)
        N.check(N.lib().mi355_hstu_add_position_embeddings(
            N.ptr(jagged), _stride(jagged), rows, D, N.dt(jagged), N.ptr(offsets), N.ptr(high), N.ptr(ind), high.numel(),
            N.ptr(dense), _stride(dense), dense.size(0), N.dt(dense), float(scale), N.ptr(out), D, N.stream()),
            "mi355_hstu_add_position_embeddings")
        ctx.save_for_backward(offsets, high)
        ctx.scale = float(scale)
        ctx.dense_shape, ctx.dense_dtype = dense.shape, dense.dtype
        ctx.no_ind_offsets = ind_offsets is None
        return out

    @staticmethod
    def backward(ctx, d_out):
        if not ctx.no_ind_offsets:
            raise AssertionError("No backward support for position encoder with incremental input")
        offsets, high = ctx.saved_tensors
        d_out = _rows(d_out)
        rows, D = d_out.shape
        K = ctx.dense_shape[0]
        d_dense = torch.empty((K, D), dtype=ctx.dense_dtype, device=d_out.device)
        d_jagged = torch.empty((rows, D), dtype=d_out.dtype, device=d_out.device) if ctx.scale != 1.0 else None
        lib = N.lib()
        ws = _workspace(lib.mi355_hstu_add_position_embeddings_bwd_workspace_bytes(rows, high.numel(), D), d_out.device)
        N.check(lib.mi355_hstu_add_position_embeddings_bwd(
            N.ptr(d_out), _stride(d_out), rows, D, N.dt(d_out), N.ptr(offsets), N.ptr(high), high.numel(), ctx.scale,
            N.ptr(d_jagged), D, N.ptr(d_dense), D, K, N.dt(d_dense), N.ptr(ws), ws.numel(), N.stream()),
            "mi355_hstu_add_position_embeddings_bwd")
        return (d_out if d_jagged is None else d_jagged), None, None, None, d_dense, None, None


def add_position_embeddings(jagged: torch.Tensor, jagged_offsets: torch.Tensor, high_inds: torch.Tensor, max_seq_len: int,
                            dense: torch.Tensor, scale: float = 1.0,
                            ind_offsets: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[s_b + n] = jagged[s_b + n] * scale + dense[idx], idx = min(n + ind_offsets[b], high_inds[b]) clamped into the table,
    for every row n of every sequence b (triton_position.py:659-670).  fp32 arithmetic, one rounding to the dtype of `jagged`;
    `dense` [K, D] is float32 or of that dtype.  Differentiable in `jagged` and `dense` when `ind_offsets` is None; the
    gradient of `dense` is summed in fp32 in a fixed order (bitwise reproducible) and rounded once to the dtype of `dense`.

    `max_seq_len` is part of the reference's signature (its launch grid); it is accepted and unused: the kernels split their
    work by rows."""
    _check_position_args(jagged, jagged_offsets, high_inds, dense, ind_offsets)
    return _AddPositionEmbeddings.apply(jagged, jagged_offsets, high_inds, max_seq_len, dense, scale, ind_offsets)


def _index_rows_sum(d_out, keys, rows_of, K, dtype):
    n, D = d_out.shape
    d_table = torch.empty((K, D), dtype=dtype, device=d_out.device)
    lib = N.lib()
    ws = _workspace(lib.mi355_hstu_index_rows_sum_workspace_bytes(keys.numel(), K, D), d_out.device)
    N.check(lib.mi355_hstu_index_rows_sum(N.ptr(d_out), _stride(d_out), n, D, N.dt(d_out), N.ptr(keys), N.ptr(rows_of),
                                          keys.numel(), N.ptr(d_table), D, K, N.dt(d_table), N.ptr(ws), ws.numel(),
                                          N.stream()), "mi355_hstu_index_rows_sum")
    return d_table


class _AddTimestampPositionEmbeddings(torch.autograd.Function):
    @staticmethod
    def forward(ctx, seq_embeddings, seq_offsets, pos_embeddings, ts_embeddings, timestamps, max_seq_len,
                max_contextual_seq_len, seq_lengths, num_targets, interleave_targets, time_bucket_fn, training):
        seq, pos, ts = _rows(seq_embeddings), _rows(pos_embeddings), _rows(ts_embeddings)
        offsets, lengths, stamps = _i64(seq_offsets), _i64(seq_lengths), _i64(timestamps)
        targets = None if num_targets is None else _i64(num_targets)
        rows, D = seq.shape
        out = torch.empty((rows, D), dtype=seq.dtype, device=seq.device)
        pos_inds = torch.empty(rows, dtype=torch.int32, device=seq.device) if training else None
        ts_inds = torch.empty(rows, dtype=torch.int32, device=seq.device) if training else None
        N.check(N.lib().mi355_hstu_add_timestamp_position_embeddings(
            N.ptr(seq), _stride(seq), rows, D, N.dt(seq), N.ptr(offsets), N.ptr(lengths), lengths.numel(),
            N.ptr(pos), _stride(pos), pos.size(0), N.ptr(ts), _stride(ts), ts.size(0), N.dt(pos),
            N.ptr(stamps), N.ptr(targets), int(bool(interleave_targets)), int(max_contextual_seq_len),
            _BUCKET_FN[time_bucket_fn], NUM_TIME_BUCKETS, TIME_BUCKET_INCREMENTS, TIME_BUCKET_SCALE, TIME_DELTA,
            N.ptr(out), D, N.ptr(pos_inds), N.ptr(ts_inds), N.stream()), "mi355_hstu_add_timestamp_position_embeddings")
        if training:
            # a stable sort of the table rows saved for the backward, as the reference does (:557-573)
            pos_keys, pos_rows = torch.sort(pos_inds, stable=True)
            ts_keys, ts_rows = torch.sort(ts_inds, stable=True)
            ctx.save_for_backward(pos_keys, pos_rows, ts_keys, ts_rows)
        ctx.training = training
        ctx.pos_meta = (pos.size(0), pos.dtype)
        ctx.ts_meta = (ts.size(0), ts.dtype)
        return out

    @staticmethod
    def backward(ctx, d_out):
        d_pos = d_ts = None
        if ctx.training:
            pos_keys, pos_rows, ts_keys, ts_rows = ctx.saved_tensors
            rows = _rows(d_out)
            if ctx.needs_input_grad[2]:
                d_pos = _index_rows_sum(rows, pos_keys, pos_rows, *ctx.pos_meta)
            if ctx.needs_input_grad[3]:
                d_ts = _index_rows_sum(rows, ts_keys, ts_rows, *ctx.ts_meta)
        return d_out, None, d_pos, d_ts, None, None, None, None, None, None, None, None


def add_timestamp_positional_embeddings(seq_embeddings: torch.Tensor, seq_offsets: torch.Tensor,
                                        pos_embeddings: torch.Tensor, ts_embeddings: torch.Tensor, timestamps: torch.Tensor,
                                        max_seq_len: int, max_contextual_seq_len: int, seq_lengths: torch.Tensor,
                                        num_targets: Optional[torch.Tensor], interleave_targets: bool,
                                        time_bucket_fn: str) -> torch.Tensor:
    """out = seq_embeddings + (pos_embeddings[p] + ts_embeddings[t]).to(seq dtype) per row (triton_position.py:673-699): p counts
    back from the first target of the sequence, t is the sqrt / log bucket of the time to the sequence's last timestamp (the
    index maps are spelled out in include/recsys_amd.h).  The tables share one dtype, float32 or that of `seq_embeddings`.
    Differentiable: the gradient of `seq_embeddings` is the incoming gradient itself, the tables' gradients are fp32 sums in a
    fixed order (bitwise reproducible, no atomics) rounded once to the table dtype.

    `max_seq_len` is part of the reference's signature (its launch grid); it is accepted and unused."""
    if seq_embeddings.dim() != 2:
        raise ValueError(f"seq_embeddings must be 2-D, got {seq_embeddings.dim()}-D")
    if seq_embeddings.dtype not in N._DT:
        raise N.NativeError(f"unsupported dtype {seq_embeddings.dtype}")
    rows, D = seq_embeddings.shape
    _check_table(pos_embeddings, "pos_embeddings", D, seq_embeddings.dtype)
    _check_table(ts_embeddings, "ts_embeddings", D, seq_embeddings.dtype)
    if pos_embeddings.dtype != ts_embeddings.dtype:
        raise ValueError("pos_embeddings and ts_embeddings must share one dtype")
    if time_bucket_fn not in _BUCKET_FN:
        raise ValueError(f"unknown time_bucket_fn {time_bucket_fn!r}: expected 'sqrt' or 'log'")
    _check_int(seq_lengths, "seq_lengths")
    if seq_lengths.numel() < 1:
        raise ValueError("seq_lengths must hold at least one sequence")
    _check_int(seq_offsets, "seq_offsets", seq_lengths.numel() + 1)
    _check_int(timestamps, "timestamps", rows)
    if num_targets is not None:
        _check_int(num_targets, "num_targets", seq_lengths.numel())
    if max_contextual_seq_len < 0:
        raise ValueError("max_contextual_seq_len must be >= 0")
    _require_gpu(seq_embeddings, seq_offsets, pos_embeddings, ts_embeddings, timestamps, seq_lengths, num_targets)
    # the index vectors and their sort are the backward's: only a call that autograd records for a table pays for them
    training = torch.is_grad_enabled() and (pos_embeddings.requires_grad or ts_embeddings.requires_grad)
    return _AddTimestampPositionEmbeddings.apply(seq_embeddings, seq_offsets, pos_embeddings, ts_embeddings, timestamps,
                                                 max_seq_len, max_contextual_seq_len, seq_lengths, num_targets,
                                                 interleave_targets, time_bucket_fn, training)


triton_add_position_embeddings = add_position_embeddings
triton_add_timestamp_positional_embeddings = add_timestamp_positional_embeddings


def _get_high_inds(high_inds: torch.Tensor, position_embeddings_weight: torch.Tensor, num_targets: Optional[torch.Tensor],
                   interleave_targets: bool) -> torch.Tensor:
    """first table row that a sequence's targets share: its length less its targets, capped at the last row of the table"""
    if num_targets is not None:
        high_inds = high_inds - (num_targets * 2 if interleave_targets else num_targets)
    return torch.clamp(high_inds, max=position_embeddings_weight.size(0) - 1)


class HSTUPositionalEncoder(torch.nn.Module):
    """Drop-in for the reference's module (position_encoder.py:71-178): same constructor, parameters and `forward`.
    `static_max_seq_len` fixes the launch grid of the reference's Triton kernels; it is accepted and ignored here."""

    def __init__(self, num_position_buckets: int, num_time_buckets: int, embedding_dim: int, training_dtype: torch.dtype,
                 is_inference: bool = True, use_time_encoding: bool = True, static_max_seq_len: Optional[int] = None) -> None:
        super().__init__()
        self._is_inference = is_inference
        self._training_dtype = training_dtype
        self._use_time_encoding: bool = use_time_encoding
        self._embedding_dim: int = embedding_dim
        bound = sqrt(1.0 / num_position_buckets)
        self._position_embeddings_weight = torch.nn.Parameter(
            torch.empty(num_position_buckets, embedding_dim).uniform_(-bound, bound))
        if self._use_time_encoding:
            bound = sqrt(1.0 / num_time_buckets)
            self._timestamp_embeddings_weight = torch.nn.Parameter(
                torch.empty(num_time_buckets + 1, embedding_dim).uniform_(-bound, bound))

    def forward(self, max_seq_len: int, seq_lengths: torch.Tensor, seq_offsets: torch.Tensor, seq_embeddings: torch.Tensor,
                num_targets: Optional[torch.Tensor], seq_timestamps: Optional[torch.Tensor] = None,
                seq_start_position: Optional[torch.Tensor] = None) -> torch.Tensor:
        alpha = self._embedding_dim ** 0.5
        if self._use_time_encoding:
            return add_timestamp_positional_embeddings(
                seq_embeddings=seq_embeddings * alpha, seq_offsets=seq_offsets,
                pos_embeddings=self._position_embeddings_weight, ts_embeddings=self._timestamp_embeddings_weight,
                timestamps=seq_timestamps, max_seq_len=max_seq_len, max_contextual_seq_len=0, seq_lengths=seq_lengths,
                num_targets=num_targets, interleave_targets=False, time_bucket_fn="sqrt")
        incremental = self._is_inference and seq_start_position is not None
        high_inds = _get_high_inds(seq_lengths + seq_start_position if incremental else seq_lengths,
                                   self._position_embeddings_weight, num_targets, False)
        return add_position_embeddings(jagged=seq_embeddings, jagged_offsets=seq_offsets, high_inds=high_inds,
                                       max_seq_len=max_seq_len, dense=self._position_embeddings_weight, scale=alpha,
                                       ind_offsets=seq_start_position if incremental else None)
