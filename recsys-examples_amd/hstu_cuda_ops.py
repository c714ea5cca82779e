"""`hstu_cuda_ops` of the reference (examples/commons/ops/cuda_ops/csrc/jagged_tensor_op_cuda.cpp:242-256 and
csrc/kjt_aux_op.cpp:344-366) on MI355X: importing this module registers the ten ops of `torch.ops.hstu_cuda_ops` with the
reference's schemas, so `commons/ops/cuda_ops/JaggedTensorOpFunction.py`, `examples/hstu/modules/hstu_processor.py` and
`examples/sid_gr/model/gpt_model.py` import and run unchanged.

* The concat / workload / preprocess ops run the kernels of csrc/jagged_ops.hip through the C ABI ("CUDA" key only: there is
  no CPU or eager fallback).  The library is loaded on first use, so the import itself needs no GPU.
* The five KJT helpers are narrow / view / cat / index_select compositions in the reference and are plain torch statements
  here too, registered for "CPU" and "CUDA".
* NO fake / meta implementation is registered here, for any of the ten ops: the reference's `fake_hstu_cuda_ops.py` registers
  them itself when the examples import it, and a second registration of the same op raises.
* `jagged_2D_tensor_concat` is the library's own one-call form of the concat: one launch forward, one backward, no workload
  array and no cumulative sum.
* `split_2D_jagged` (alias `triton_split_2D_jagged`, the name `examples/hstu/modules/hstu_processor.py` imports from the
  reference's Triton package) is the inverse of the two-tensor concat over the same kernel; it is a Python function, not an
  eleventh op schema.
"""
import ctypes
from typing import List, Optional, Sequence, Tuple

import torch

import mi355_native as N

MAX_TENSORS = 128  # pointer-table slots of one launch (csrc/jagged_ops.hip: kJagMaxN)
_DT = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2, torch.float64: 3}

_lib = torch.library.Library("hstu_cuda_ops", "FRAGMENT")
_lib.define("concat_2D_jagged_tensors_forward(Tensor[] values_list, Tensor[] offsets_list, int seqlen_per_block, "
            "int max_seqlen, int total_blocks, int blocks, int threads, Tensor workload_offset, "
            "Tensor(a!) merged_values, Tensor(b!) merged_offsets) -> ()")
_lib.define("concat_2D_jagged_tensors_backward(Tensor grad_output, Tensor grad_lengths, int seqlen_per_block, "
            "int max_seqlen, int total_blocks, int blocks, int threads, Tensor workload_offset, "
            "Tensor(a!)[] grad_inputs, Tensor[] offsets_list, Tensor merged_offsets) -> ()")
_lib.define("compute_block_workloads(Tensor[] offsets_list, int seqlen_per_block, int max_seqlen, "
            "Tensor(a!) block_workloads) -> ()")
_lib.define("concat_2D_jagged_tensors_fwd_exportable(Tensor[] values_list, Tensor[] offsets_list, int seqlen_per_block, "
            "int max_seqlen, Tensor total_blocks, Tensor blocks, int threads, Tensor workload_offset, "
            "Tensor(a!) merged_values, Tensor(b!) merged_offsets) -> ()")
_lib.define("hstu_inference_preprocess(Tensor item_values, Tensor item_lengths, Tensor action_values, "
            "Tensor action_lengths, Tensor num_candidates) -> (Tensor, Tensor, Tensor, Tensor)")
_lib.define("split_by_lengths(Tensor values, Tensor lengths_1d, int num_splits) -> Tensor[]")
_lib.define("lengths_reduce_dim1(Tensor lengths_1d, int num_splits) -> Tensor")
_lib.define("lengths_splits(Tensor lengths_1d, int num_splits) -> Tensor[]")
_lib.define("permute_and_split(Tensor jagged_features, Tensor jagged_lengths, Tensor jagged_offsets, "
            "int num_static_features, int num_dynamic_features, int[] features_order) -> Tensor[]")
_lib.define("strip_cached_tokens(Tensor values, Tensor lengths, Tensor length_offsets, Tensor num_cached, "
            "int[] feature_order) -> (Tensor, Tensor)")


def _check(cond, msg):
    if not cond:
        raise RuntimeError(msg)


# ---------------------------------------------------------------------------------------------------------------------
# concat over the C ABI
# ---------------------------------------------------------------------------------------------------------------------
def _offsets_i64(o: torch.Tensor) -> torch.Tensor:
    return o if o.dtype == torch.int64 and o.is_contiguous() else o.to(torch.int64).contiguous()


def _concat_launch(values: Sequence[torch.Tensor], offsets: Sequence[torch.Tensor], merged_offsets: torch.Tensor,
                   merged: torch.Tensor, direction: int, checked: bool = False) -> None:
    """One launch of mi355_jagged_concat.  direction 0 fills `merged` from `values`, 1 fills every tensor of `values` from
    `merged`.  Every tensor is a contiguous [rows, D] GPU tensor of one dtype.  checked: the caller has validated the
    arguments (jagged_2D_tensor_concat does it once for forward and backward; this call is host-bound at the HSTU shapes)."""
    n = len(values)
    if not checked:
        if n == 0 or n != len(offsets):
            raise ValueError("values_list and offsets_list must be non-empty and of equal length")
        if merged.dim() != 2:
            raise ValueError("merged values must be 2-D")
        for v in values:
            if v.dim() != 2 or v.size(1) != merged.size(1):
                raise ValueError("all tensors must be 2-D with the same hidden dim")
            if v.dtype != merged.dtype or v.device != merged.device:
                raise ValueError("all tensors must share one dtype and one device")
        if not merged.is_cuda:
            raise N.NativeError("librecsys_amd expects GPU tensors (no CPU fallback exists)")
        if merged.dtype not in _DT:
            raise N.NativeError(f"unsupported dtype {merged.dtype}")
        N.require_contiguous(merged, *values)
        B = offsets[0].numel() - 1
        if B < 1 or any(o.numel() != B + 1 or o.device != merged.device for o in offsets) \
                or merged_offsets.numel() != B + 1 or merged_offsets.device != merged.device:
            raise ValueError("every offsets tensor must hold batch + 1 entries (batch >= 1) on the device of the values")
        offsets = [_offsets_i64(o) for o in offsets]
        merged_offsets = _offsets_i64(merged_offsets)
    vp = (ctypes.c_void_p * n)(*[v.data_ptr() for v in values])
    op = (ctypes.c_void_p * n)(*[o.data_ptr() for o in offsets])
    rows = (ctypes.c_int64 * n)(*[v.size(0) for v in values])
    rc = N.lib().mi355_jagged_concat(n, vp, op, rows, merged_offsets.numel() - 1, merged_offsets.data_ptr(),
                                     merged.data_ptr(), merged.size(0), merged.size(1), _DT[merged.dtype], direction,
                                     N.stream())
    if rc != 0:
        N.check(rc, "mi355_jagged_concat")


def _fwd_impl(values_list, offsets_list, seqlen_per_block, max_seqlen, total_blocks, blocks, threads, workload_offset,
              merged_values, merged_offsets):
    # blocks / threads / workload_offset are launch hints of the reference's kernel; the row layout they imply is the
    # concatenation order, which is all this kernel needs
    _concat_launch([v.contiguous() for v in values_list], offsets_list, merged_offsets, merged_values, 0)


def _fwd_exportable_impl(values_list, offsets_list, seqlen_per_block, max_seqlen, total_blocks, blocks, threads,
                         workload_offset, merged_values, merged_offsets):
    _concat_launch([v.contiguous() for v in values_list], offsets_list, merged_offsets, merged_values, 0)


def _bwd_impl(grad_output, grad_lengths, seqlen_per_block, max_seqlen, total_blocks, blocks, threads, workload_offset,
              grad_inputs, offsets_list, merged_offsets):
    _concat_launch(grad_inputs, offsets_list, merged_offsets, grad_output.contiguous(), 1)


def _workloads_impl(offsets_list, seqlen_per_block, max_seqlen, block_workloads):
    n = len(offsets_list)
    _check(n > 0, "offsets_list cannot be empty")
    _check(block_workloads.dtype == torch.int64 and block_workloads.is_contiguous(),
           "block_workloads must be a contiguous int64 tensor")
    B = offsets_list[0].numel() - 1
    _check(all(o.numel() == B + 1 for o in offsets_list), "every offsets tensor must hold batch + 1 entries")
    offs = [_offsets_i64(o) for o in offsets_list]
    op = (ctypes.c_void_p * n)(*[N.ptr(o).value for o in offs])
    N.check(N.lib().mi355_jagged_block_workloads(n, op, B, seqlen_per_block, max_seqlen, N.ptr(block_workloads),
                                                 block_workloads.numel(), N.stream()), "mi355_jagged_block_workloads")


def _exclusive_offsets(lengths_i64: torch.Tensor) -> torch.Tensor:
    out = lengths_i64.new_zeros(lengths_i64.numel() + 1)
    torch.cumsum(lengths_i64, 0, out=out[1:])
    return out


def _preprocess_impl(item_values, item_lengths, action_values, action_lengths, num_candidates):
    for t, name in ((item_values, "item_values"), (item_lengths, "item_lengths"), (action_values, "action_values"),
                    (action_lengths, "action_lengths"), (num_candidates, "num_candidates")):
        _check(t.is_cuda, f"{name} must be a CUDA tensor")
    _check(item_values.dim() == 2, "item_values must be 2D")
    _check(action_values.dim() == 2, "action_values must be 2D")
    _check(action_lengths.dim() == 1, "action_lengths must be 1D")
    _check(item_lengths.dim() == 1, "item_lengths must be 1D")
    _check(num_candidates.dim() == 1, "num_candidates must be 1D")
    _check(item_values.size(1) == action_values.size(1), "item/action embedding dims must match")
    _check(item_values.dtype == action_values.dtype, "item/action dtypes must match")
    _check(item_lengths.size(0) == action_lengths.size(0), "item/action length batch sizes must match")
    _check(item_lengths.size(0) == num_candidates.size(0), "num_candidates batch size must match")
    if item_values.dtype not in _DT:
        raise N.NativeError(f"unsupported dtype {item_values.dtype}")
    il, al, nc = (t.to(torch.int64) for t in (item_lengths, action_lengths, num_candidates))
    hist, ahist, extra = il - nc, al - nc, al - il
    out_lengths = hist + ahist + nc
    # the three validity checks and the output size in ONE host read (the output is sized by it)
    bad_h, bad_a, bad_e, total = torch.stack([(hist < 0).any().to(torch.int64), (ahist < 0).any().to(torch.int64),
                                              ((extra != 0) & (extra != 1)).any().to(torch.int64),
                                              out_lengths.sum()]).tolist()
    _check(not bad_h, "item history lengths must be non-negative after removing candidates")
    _check(not bad_a, "action history lengths must be non-negative after removing candidates")
    _check(not bad_e, "each action length must equal item length or item length + 1")
    io, ao, oo = _exclusive_offsets(il), _exclusive_offsets(al), _exclusive_offsets(out_lengths)
    co = _exclusive_offsets(nc).to(torch.int32)
    B, D = il.numel(), item_values.size(1)
    out = item_values.new_empty((total, D))
    if B > 0 and total > 0:
        iv, av = item_values.contiguous(), action_values.contiguous()
        N.check(N.lib().mi355_hstu_inference_preprocess(N.ptr(iv), iv.size(0), N.ptr(io), N.ptr(av), av.size(0), N.ptr(ao),
                                                        N.ptr(oo), B, N.ptr(out), total, D, _DT[out.dtype], N.stream()),
                "mi355_hstu_inference_preprocess")
    return out, out_lengths, oo, co


_lib.impl("concat_2D_jagged_tensors_forward", _fwd_impl, "CUDA")
_lib.impl("concat_2D_jagged_tensors_backward", _bwd_impl, "CUDA")
_lib.impl("compute_block_workloads", _workloads_impl, "CUDA")
_lib.impl("concat_2D_jagged_tensors_fwd_exportable", _fwd_exportable_impl, "CUDA")
_lib.impl("hstu_inference_preprocess", _preprocess_impl, "CUDA")


# ---------------------------------------------------------------------------------------------------------------------
# KJT helpers: torch statements, no kernels (kjt_aux_op.cpp)
# ---------------------------------------------------------------------------------------------------------------------
def _on(t: torch.Tensor, cuda: bool) -> bool:
    return t.is_cuda if cuda else t.device.type == "cpu"


def _kind(cuda: bool) -> str:
    return "CUDA" if cuda else "CPU"


def _check_splits(lengths_1d, num_splits):
    _check(lengths_1d.dim() == 1, f"lengths_1d must be 1D, got dim={lengths_1d.dim()}")
    _check(num_splits > 0, "num_splits must be > 0")
    _check(lengths_1d.numel() % num_splits == 0,
           f"lengths_1d.numel()={lengths_1d.numel()} must be divisible by num_splits={num_splits}")


def _split_by_lengths(cuda, values, lengths_1d, num_splits):
    _check(_on(values, cuda), f"values must be a {_kind(cuda)} tensor")
    _check(lengths_1d.is_cuda or lengths_1d.device.type == "cpu", f"lengths_1d must be CPU or CUDA, got {lengths_1d.device}")
    _check(values.dim() in (1, 2), f"values must be 1D or 2D, got dim={values.dim()}")
    _check_splits(lengths_1d, num_splits)
    sizes = lengths_1d.to("cpu", torch.int64).reshape(num_splits, -1).sum(1).tolist()
    _check(sum(sizes) == values.size(0), f"sum(lengths_1d)={sum(sizes)} must equal values.size(0)={values.size(0)}")
    out, start = [], 0
    for s in sizes:
        out.append(values.narrow(0, start, s))
        start += s
    return out


def _lengths_reduce_dim1(cuda, lengths_1d, num_splits):
    _check_splits(lengths_1d, num_splits)
    _check(_on(lengths_1d, cuda), f"lengths_1d must be a {_kind(cuda)} tensor for {_kind(cuda)} impl")
    return lengths_1d.view(num_splits, -1).sum(1)


def _lengths_splits(cuda, lengths_1d, num_splits):
    _check_splits(lengths_1d, num_splits)
    _check(_on(lengths_1d, cuda), f"lengths_1d must be a {_kind(cuda)} tensor for {_kind(cuda)} impl")
    batch = lengths_1d.numel() // num_splits
    return [lengths_1d.narrow(0, i * batch, batch) for i in range(num_splits)]


def _permute_and_split(cuda, jagged_features, jagged_lengths, jagged_offsets, num_static_features, num_dynamic_features,
                       features_order):
    nf = num_static_features + num_dynamic_features
    _check(jagged_features.dim() == 1, f"jagged_features must be 1D, got dim={jagged_features.dim()}")
    _check(jagged_lengths.dim() == 1, f"jagged_lengths must be 1D, got dim={jagged_lengths.dim()}")
    _check(num_static_features > 0, "num_static_features must be > 0")
    _check(num_dynamic_features > 0, "num_dynamic_features must be > 0")
    _check(jagged_lengths.numel() % nf == 0,
           f"jagged_lengths.numel()={jagged_lengths.numel()} must be divisible by num_features={nf}")
    _check(_on(jagged_features, cuda), f"jagged_features must be a {_kind(cuda)} tensor for {_kind(cuda)} impl")
    _check(_on(jagged_lengths, cuda), f"jagged_lengths must be a {_kind(cuda)} tensor for {_kind(cuda)} impl")
    _check(nf == len(features_order), "features_order size must match total number of features")
    batch = jagged_lengths.numel() // nf
    _check(all(0 <= f < nf for f in features_order), "features_order contains an invalid index")
    sizes = jagged_lengths.view(nf, batch).sum(1).tolist()
    offsets = jagged_offsets.to("cpu").tolist()
    lengths = [jagged_lengths.narrow(0, f * batch, batch) for f in features_order]
    feats = [jagged_features.narrow(0, offsets[f * batch], sizes[f]) for f in features_order]
    ns = num_static_features
    return [torch.cat(feats[:ns], 0), torch.cat(feats[ns:], 0), torch.cat(lengths[:ns], 0), torch.cat(lengths[ns:], 0)]


def _strip_cached_tokens(cuda, values, lengths, length_offsets, num_cached, feature_order):
    F = len(feature_order)
    _check(values.dim() == 1, f"values must be 1D, got dim={values.dim()}")
    _check(lengths.dim() == 1, f"lengths must be 1D, got dim={lengths.dim()}")
    _check(length_offsets.dim() == 1, f"length_offsets must be 1D, got dim={length_offsets.dim()}")
    _check(num_cached.dim() == 1, f"num_cached must be 1D, got dim={num_cached.dim()}")
    _check(F >= 2, "feature_order must have at least item and action features")
    B = num_cached.numel()
    _check(B > 0, "batch_size must be > 0")
    _check(lengths.numel() == B * F, "lengths must have shape [batch_size * feature_order.size()]")
    _check(length_offsets.numel() == lengths.numel() + 1, "length_offsets must have shape [lengths.numel() + 1]")
    for t, name in ((lengths, "lengths"), (length_offsets, "length_offsets"), (num_cached, "num_cached")):
        _check(t.device == values.device, f"{name} must be on the same device as values")
    _check(_on(values, cuda), f"values must be a {_kind(cuda)} tensor for {_kind(cuda)} impl")
    for f in feature_order:
        _check(0 <= f < F, f"feature_order contains invalid index: {f}")
    L = lengths.to(torch.int64).view(F, B)
    starts = length_offsets.to(torch.int64)[:-1].view(F, B)
    remaining = num_cached.to(torch.int64)
    strip = torch.zeros_like(L)
    # the cached prefix is taken off the leading features in order; what is left is split between item and action, the item
    # side taking the extra one of an odd remainder
    for f in feature_order[:-2]:
        strip[f] = torch.minimum(remaining, L[f])
        remaining = remaining - strip[f]
    item_f, action_f = feature_order[-2], feature_order[-1]
    strip[item_f] = torch.minimum((remaining + 1) // 2, L[item_f])
    strip[action_f] = torch.minimum(remaining // 2, L[action_f])
    order = torch.tensor(list(feature_order), dtype=torch.int64, device=values.device)
    new_lengths = (L - strip).index_select(0, order).reshape(-1)
    src_starts = (starts + strip).index_select(0, order).reshape(-1)
    new_offsets = _exclusive_offsets(new_lengths)
    delta = torch.repeat_interleave(src_starts - new_offsets[:-1], new_lengths)
    index = torch.arange(delta.numel(), dtype=torch.int64, device=values.device) + delta
    return values.index_select(0, index), new_lengths.to(lengths.dtype)


def _bind_backend(fn, cuda):
    def impl(*args, **kwargs):
        return fn(cuda, *args, **kwargs)

    return impl


for _name, _fn in (("split_by_lengths", _split_by_lengths), ("lengths_reduce_dim1", _lengths_reduce_dim1),
                   ("lengths_splits", _lengths_splits), ("permute_and_split", _permute_and_split),
                   ("strip_cached_tokens", _strip_cached_tokens)):
    for _cuda in (False, True):
        _lib.impl(_name, _bind_backend(_fn, _cuda), _kind(_cuda))


# ---------------------------------------------------------------------------------------------------------------------
# the library's own one-call concat
# ---------------------------------------------------------------------------------------------------------------------
class _JaggedConcat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, offsets_list: List[torch.Tensor], *values_list: torch.Tensor):
        ctx.n = len(values_list)
        if ctx.n == 1:
            lengths = offsets_list[0][1:] - offsets_list[0][:-1]
            ctx.mark_non_differentiable(lengths)
            return values_list[0], lengths
        # (the public function has validated the arguments: int64 contiguous offsets, contiguous values of one dtype on one GPU)
        merged_offsets = offsets_list[0] + offsets_list[1] if ctx.n == 2 else torch.stack(offsets_list).sum(0)
        merged_lengths = torch.diff(merged_offsets)
        ctx.mark_non_differentiable(merged_lengths)
        v0 = values_list[0]
        merged = v0.new_empty((sum(v.size(0) for v in values_list), v0.size(1)))
        if merged.size(0) > 0:
            _concat_launch(values_list, offsets_list, merged_offsets, merged, 0, checked=True)
        ctx.save_for_backward(merged_offsets, *offsets_list)
        ctx.shapes = [v.shape for v in values_list]
        return merged, merged_lengths

    @staticmethod
    def backward(ctx, grad_output, grad_lengths):
        if ctx.n == 1:
            return None, grad_output
        merged_offsets, *offsets_list = ctx.saved_tensors
        grads = [grad_output.new_empty(s) for s in ctx.shapes]
        if grad_output.size(0) > 0:
            _concat_launch(grads, offsets_list, merged_offsets, grad_output.contiguous(), 1, checked=True)
        return (None, *grads)


def _complete_offsets(lengths: torch.Tensor) -> torch.Tensor:
    return _exclusive_offsets(lengths.to(torch.int64))


def jagged_2D_tensor_concat(values_list: List[torch.Tensor], offsets_list: List[torch.Tensor],
                            max_seqlens: List[int]) -> Tuple[torch.Tensor, torch.Tensor]:
    """Concatenates n jagged 2-D tensors sample by sample (the reference wrapper's jagged_2D_tensor_concat,
    commons/ops/cuda_ops/JaggedTensorOpFunction.py:199-250): sample b of the result is sample b of values_list[0], then of
    values_list[1], ...  Returns (merged_values [sum of rows, D], merged_lengths [B]); differentiable in the values.

    `max_seqlens` is part of the reference's signature; the kernel splits its work by rows of the merged buffer and has no use
    for it.  More than 128 tensors are concatenated in groups of 128 whose results are merged pairwise.  Inputs that are not
    contiguous are copied."""
    if len(values_list) == 0 or len(offsets_list) == 0:
        raise ValueError("offsets_list and values_list cannot be empty")
    if len(values_list) != len(offsets_list):
        raise ValueError("values_list and offsets_list must have the same length")
    v0 = values_list[0]
    for v in values_list:
        if v.dtype != v0.dtype:
            raise ValueError("all values must have the same dtype")
        if v.device != v0.device:
            raise ValueError("all values must be on the same device")
        if v.dim() != 2 or v.size(1) != v0.size(1):
            raise ValueError("all values must be 2-D with the same hidden dim")
    if not v0.is_cuda:
        raise N.NativeError("jagged_2D_tensor_concat expects GPU tensors (no CPU fallback exists)")
    if v0.dtype not in _DT:
        raise N.NativeError(f"unsupported dtype {v0.dtype}")
    numel = offsets_list[0].numel()
    for o in offsets_list:
        if o.device != v0.device:
            raise ValueError("offsets must be on the device of the values")
        if o.dim() != 1 or o.numel() != numel or numel < 2:
            raise ValueError("every offsets tensor must be 1-D with batch + 1 entries, batch >= 1")
    values_list = [v if v.is_contiguous() else v.contiguous() for v in values_list]
    offsets_list = [_offsets_i64(o) for o in offsets_list]
    if len(values_list) <= MAX_TENSORS:
        return _JaggedConcat.apply(offsets_list, *values_list)
    result = None
    for i in range(0, len(values_list), MAX_TENSORS):
        part = _JaggedConcat.apply(offsets_list[i:i + MAX_TENSORS], *values_list[i:i + MAX_TENSORS])
        if result is None:
            result = part
        else:
            result = _JaggedConcat.apply([_complete_offsets(result[1]), _complete_offsets(part[1])], result[0], part[0])
    return result


# ---------------------------------------------------------------------------------------------------------------------
# split of a merged jagged tensor into its two parts: the inverse of the two-tensor concat
# ---------------------------------------------------------------------------------------------------------------------
class _Split2DJagged(torch.autograd.Function):
    @staticmethod
    def forward(ctx, values, offsets_a, offsets_b, rows_a, rows_b):
        # (the public function has validated the arguments: int64 contiguous offsets, contiguous 2-D values on the GPU)
        merged_offsets = offsets_a + offsets_b
        values_a = values.new_empty((rows_a, values.size(1)))
        values_b = values.new_empty((rows_b, values.size(1)))
        if values.size(0) > 0:
            _concat_launch([values_a, values_b], [offsets_a, offsets_b], merged_offsets, values, 1, checked=True)
        ctx.save_for_backward(merged_offsets, offsets_a, offsets_b)
        ctx.rows = values.size(0)
        return values_a, values_b

    @staticmethod
    def backward(ctx, grad_a, grad_b):
        merged_offsets, offsets_a, offsets_b = ctx.saved_tensors
        d_values = grad_a.new_empty((ctx.rows, grad_a.size(1)))
        if ctx.rows > 0:
            _concat_launch([grad_a.contiguous(), grad_b.contiguous()], [offsets_a, offsets_b], merged_offsets, d_values, 0,
                           checked=True)
        return d_values, None, None, None, None


def split_2D_jagged(values: torch.Tensor, max_seq_len: int, offsets_a: Optional[torch.Tensor] = None,
                    offsets_b: Optional[torch.Tensor] = None, dense_size: int = 0, n_prefix_to_right: int = 0,
                    seq_len_a=None, seq_len_b=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Cuts every sample of the jagged `values` [rows, D] into its leading part A and its trailing part B (the reference's
    triton_split_2D_jagged, commons/ops/triton_ops/triton_jagged.py:1330-1349): the inverse of the two-tensor concat, one
    launch of mi355_jagged_concat forward (direction 1) and one backward (direction 0).  Differentiable in `values`.

    A side whose offsets are None is dense: `dense_size` rows per sample, returned as [B, dense_size, D]; at most one side may
    be.  With both sides jagged, `seq_len_a` / `seq_len_b` (int or one-element tensor: the row count of each part) spare the
    host read of the last offset.  `max_seq_len` is part of the reference's signature (its launch grid) and is unused here.
    `n_prefix_to_right` != 0 (a prefix of A moved behind B) is not implemented; no caller in examples/hstu passes it."""
    if n_prefix_to_right != 0:
        raise NotImplementedError("split_2D_jagged: n_prefix_to_right != 0 is not implemented")
    if values.dim() != 2:
        raise ValueError(f"values must be 2-D, got {values.dim()}-D")
    if offsets_a is None and offsets_b is None:
        raise ValueError("offsets_a and offsets_b cannot both be None")
    for o in (offsets_a, offsets_b):
        if o is not None and (o.dim() != 1 or o.numel() < 2):
            raise ValueError("every offsets tensor must be 1-D with batch + 1 entries, batch >= 1")
    if offsets_a is not None and offsets_b is not None and offsets_a.numel() != offsets_b.numel():
        raise ValueError("offsets_a and offsets_b must hold the same number of entries")
    if (offsets_a is None or offsets_b is None) and dense_size < 0:
        raise ValueError("dense_size must be >= 0")
    if not values.is_cuda:
        raise N.NativeError("split_2D_jagged expects GPU tensors (no CPU fallback exists)")
    if values.dtype not in _DT:
        raise N.NativeError(f"unsupported dtype {values.dtype}")
    given = offsets_b if offsets_a is None else offsets_a
    if given.device != values.device or (offsets_b is not None and offsets_b.device != values.device):
        raise ValueError("offsets must be on the device of the values")
    B, rows = given.numel() - 1, values.size(0)
    dense_a, dense_b = offsets_a is None, offsets_b is None
    if dense_a or dense_b:
        dense_offsets = torch.arange(B + 1, dtype=torch.int64, device=values.device) * dense_size
        if B * dense_size > rows:
            raise ValueError(f"values holds {rows} rows, fewer than batch * dense_size = {B * dense_size}")
    if dense_a:
        offsets_a, rows_a, rows_b = dense_offsets, B * dense_size, rows - B * dense_size
    elif dense_b:
        offsets_b, rows_b, rows_a = dense_offsets, B * dense_size, rows - B * dense_size
    else:
        rows_a = int(offsets_a[-1].item() if seq_len_a is None else seq_len_a)
        rows_b = int(offsets_b[-1].item() if seq_len_b is None else seq_len_b)
    values = values if values.is_contiguous() else values.contiguous()
    values_a, values_b = _Split2DJagged.apply(values, _offsets_i64(offsets_a), _offsets_i64(offsets_b), rows_a, rows_b)
    if dense_a:
        values_a = values_a.reshape(B, dense_size, values.size(1))
    if dense_b:
        values_b = values_b.reshape(B, dense_size, values.size(1))
    return values_a, values_b


triton_split_2D_jagged = split_2D_jagged
