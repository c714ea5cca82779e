"""CPU checks of the `hstu_cuda_ops` binding: the module imports without a GPU, registers the reference's ten op schemas and
no fake implementation, the five KJT helpers compute what the direct torch statements compute, and the three jagged entry
points of the C ABI answer bad arguments with an error code."""
import pytest
import torch

SCHEMAS = {
    "concat_2D_jagged_tensors_forward":
        "hstu_cuda_ops::concat_2D_jagged_tensors_forward(Tensor[] values_list, Tensor[] offsets_list, int seqlen_per_block, "
        "int max_seqlen, int total_blocks, int blocks, int threads, Tensor workload_offset, Tensor(a!) merged_values, "
        "Tensor(b!) merged_offsets) -> ()",
    "concat_2D_jagged_tensors_backward":
        "hstu_cuda_ops::concat_2D_jagged_tensors_backward(Tensor grad_output, Tensor grad_lengths, int seqlen_per_block, "
        "int max_seqlen, int total_blocks, int blocks, int threads, Tensor workload_offset, Tensor(a!)[] grad_inputs, "
        "Tensor[] offsets_list, Tensor merged_offsets) -> ()",
    "compute_block_workloads":
        "hstu_cuda_ops::compute_block_workloads(Tensor[] offsets_list, int seqlen_per_block, int max_seqlen, "
        "Tensor(a!) block_workloads) -> ()",
    "concat_2D_jagged_tensors_fwd_exportable":
        "hstu_cuda_ops::concat_2D_jagged_tensors_fwd_exportable(Tensor[] values_list, Tensor[] offsets_list, "
        "int seqlen_per_block, int max_seqlen, Tensor total_blocks, Tensor blocks, int threads, Tensor workload_offset, "
        "Tensor(a!) merged_values, Tensor(b!) merged_offsets) -> ()",
    "hstu_inference_preprocess":
        "hstu_cuda_ops::hstu_inference_preprocess(Tensor item_values, Tensor item_lengths, Tensor action_values, "
        "Tensor action_lengths, Tensor num_candidates) -> (Tensor, Tensor, Tensor, Tensor)",
    "split_by_lengths": "hstu_cuda_ops::split_by_lengths(Tensor values, Tensor lengths_1d, int num_splits) -> Tensor[]",
    "lengths_reduce_dim1": "hstu_cuda_ops::lengths_reduce_dim1(Tensor lengths_1d, int num_splits) -> Tensor",
    "lengths_splits": "hstu_cuda_ops::lengths_splits(Tensor lengths_1d, int num_splits) -> Tensor[]",
    "permute_and_split":
        "hstu_cuda_ops::permute_and_split(Tensor jagged_features, Tensor jagged_lengths, Tensor jagged_offsets, "
        "int num_static_features, int num_dynamic_features, int[] features_order) -> Tensor[]",
    "strip_cached_tokens":
        "hstu_cuda_ops::strip_cached_tokens(Tensor values, Tensor lengths, Tensor length_offsets, Tensor num_cached, "
        "int[] feature_order) -> (Tensor, Tensor)",
}


def _ops():
    import hstu_cuda_ops  # noqa: F401

    return torch.ops.hstu_cuda_ops


def _offsets(lengths):
    return torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(lengths.to(torch.int64), 0)])


def test_import_registers_the_ten_schemas():
    ops = _ops()
    for name, schema in SCHEMAS.items():
        assert hasattr(ops, name), name
        assert str(getattr(ops, name).default._schema) == schema


def test_module_registers_no_fake_implementations():
    """the reference's fake_hstu_cuda_ops.py registers the fakes itself; a second registration of one op raises"""
    _ops()

    @torch.library.register_fake("hstu_cuda_ops::split_by_lengths")
    def _fake_split(values, lengths_1d, num_splits):
        return [values.new_empty((0,)) for _ in range(num_splits)]

    @torch.library.register_fake("hstu_cuda_ops::lengths_reduce_dim1")
    def _fake_reduce(lengths_1d, num_splits):
        return lengths_1d.new_empty((num_splits,))


def test_split_by_lengths_cpu():
    ops = _ops()
    lengths = torch.tensor([2, 0, 1, 3, 1, 0], dtype=torch.int32)   # 3 splits x batch 2
    for values in (torch.arange(7.0), torch.arange(21.0).view(7, 3)):
        out = ops.split_by_lengths(values, lengths, 3)
        want = torch.split(values, [2, 4, 1], 0)
        assert len(out) == 3 and all(torch.equal(a, b) for a, b in zip(out, want))
    with pytest.raises(RuntimeError, match="must equal values.size"):
        ops.split_by_lengths(torch.arange(8.0), lengths, 3)
    with pytest.raises(RuntimeError, match="divisible"):
        ops.split_by_lengths(torch.arange(7.0), lengths, 4)
    with pytest.raises(RuntimeError, match="num_splits must be > 0"):
        ops.split_by_lengths(torch.arange(7.0), lengths, 0)
    with pytest.raises(RuntimeError, match="1D or 2D"):
        ops.split_by_lengths(torch.zeros(7, 1, 1), lengths, 3)
    with pytest.raises(RuntimeError, match="lengths_1d must be 1D"):
        ops.split_by_lengths(torch.arange(7.0), lengths.view(3, 2), 3)


def test_lengths_reduce_and_splits_cpu():
    ops = _ops()
    lengths = torch.tensor([2, 0, 1, 3, 1, 0])
    assert torch.equal(ops.lengths_reduce_dim1(lengths, 3), lengths.view(3, 2).sum(1))
    parts = ops.lengths_splits(lengths, 2)
    assert len(parts) == 2 and torch.equal(parts[0], lengths[:3]) and torch.equal(parts[1], lengths[3:])
    for op in (ops.lengths_reduce_dim1, ops.lengths_splits):
        with pytest.raises(RuntimeError, match="divisible"):
            op(lengths, 4)
        with pytest.raises(RuntimeError, match="num_splits must be > 0"):
            op(lengths, 0)
        with pytest.raises(RuntimeError, match="must be 1D"):
            op(lengths.view(2, 3), 2)


def test_permute_and_split_cpu():
    ops = _ops()
    batch = 2
    lengths = torch.tensor([1, 2, 0, 3, 2, 2, 1, 0])   # 4 features x batch 2
    offsets = _offsets(lengths)
    feats = torch.arange(int(lengths.sum())) * 10
    order = [2, 0, 3, 1]                               # static: features 2, 0; dynamic: 3, 1
    per_feature = [feats[offsets[f * batch]:offsets[(f + 1) * batch]] for f in range(4)]
    per_length = [lengths[f * batch:(f + 1) * batch] for f in range(4)]
    out = ops.permute_and_split(feats, lengths, offsets, 2, 2, order)
    assert len(out) == 4
    assert torch.equal(out[0], torch.cat([per_feature[2], per_feature[0]]))
    assert torch.equal(out[1], torch.cat([per_feature[3], per_feature[1]]))
    assert torch.equal(out[2], torch.cat([per_length[2], per_length[0]]))
    assert torch.equal(out[3], torch.cat([per_length[3], per_length[1]]))
    with pytest.raises(RuntimeError, match="features_order size"):
        ops.permute_and_split(feats, lengths, offsets, 2, 2, [0, 1, 2])
    with pytest.raises(RuntimeError, match="num_static_features must be > 0"):
        ops.permute_and_split(feats, lengths, offsets, 0, 4, order)
    with pytest.raises(RuntimeError, match="divisible"):
        ops.permute_and_split(feats, lengths, offsets, 2, 1, [0, 1, 2])
    with pytest.raises(RuntimeError, match="jagged_features must be 1D"):
        ops.permute_and_split(feats.view(-1, 1), lengths, offsets, 2, 2, order)


def _strip_by_hand(values, lengths, offsets, num_cached, order):
    """per sample and feature in python: the cached prefix comes off the leading features in order, the rest is split between
    the last two (item, action), the item side taking the extra one of an odd remainder"""
    F, B = len(order), len(num_cached)
    strip = [[0] * B for _ in range(F)]
    for b in range(B):
        left = int(num_cached[b])
        for f in order[:-2]:
            strip[f][b] = min(left, int(lengths[f * B + b]))
            left -= strip[f][b]
        strip[order[-2]][b] = min((left + 1) // 2, int(lengths[order[-2] * B + b]))
        strip[order[-1]][b] = min(left // 2, int(lengths[order[-1] * B + b]))
    rows, new_lengths = [], []
    for f in order:
        for b in range(B):
            s, n = int(offsets[f * B + b]), int(lengths[f * B + b])
            rows.append(values[s + strip[f][b]:s + n])
            new_lengths.append(n - strip[f][b])
    return torch.cat(rows), torch.tensor(new_lengths, dtype=lengths.dtype)


def test_strip_cached_tokens_cpu():
    ops = _ops()
    # 3 features (context, item, action) x batch 3; sample 0: 5 cached > 2 context rows -> 3 spill: item 2, action 1
    lengths = torch.tensor([2, 1, 0, 4, 3, 2, 4, 3, 2], dtype=torch.int32)
    offsets = _offsets(lengths)
    values = torch.arange(int(lengths.sum())) + 100
    num_cached = torch.tensor([5, 0, 1])
    for order in ([0, 1, 2], [0, 2, 1]):
        got_v, got_l = ops.strip_cached_tokens(values, lengths, offsets, num_cached, order)
        want_v, want_l = _strip_by_hand(values, lengths, offsets, num_cached, order)
        assert torch.equal(got_v, want_v) and torch.equal(got_l, want_l) and got_l.dtype == lengths.dtype
    got_v, got_l = ops.strip_cached_tokens(values, lengths, offsets, num_cached, [0, 1, 2])
    assert got_l.tolist() == [0, 1, 0, 2, 3, 1, 3, 3, 2]   # sample 0: context 2 -> 0, item 4 -> 2, action 4 -> 3
    with pytest.raises(RuntimeError, match="at least item and action"):
        ops.strip_cached_tokens(values, lengths, offsets, num_cached, [0])
    with pytest.raises(RuntimeError, match="lengths must have shape"):
        ops.strip_cached_tokens(values, lengths, offsets, num_cached, [0, 1])
    with pytest.raises(RuntimeError, match="length_offsets must have shape"):
        ops.strip_cached_tokens(values, lengths, offsets[:-1], num_cached, [0, 1, 2])
    with pytest.raises(RuntimeError, match="invalid index"):
        ops.strip_cached_tokens(values, lengths, offsets, num_cached, [0, 1, 3])
    with pytest.raises(RuntimeError, match="values must be 1D"):
        ops.strip_cached_tokens(values.view(-1, 1), lengths, offsets, num_cached, [0, 1, 2])


def test_jagged_entry_points_reject_bad_arguments():
    import mi355_native as N

    lib = N.lib()
    for n, D, dt, word in ((0, 8, 1, b"1..128"), (129, 8, 1, b"1..128"), (2, 0, 1, b"D must be > 0"), (2, 8, 9, b"dtype")):
        rc = lib.mi355_jagged_concat(n, None, None, None, 4, None, None, 16, D, dt, 0, None)
        assert rc == -1 and word in lib.mi355_last_error()
    rc = lib.mi355_jagged_concat(2, None, None, None, 4, None, None, 16, 8, 1, 0, None)   # null tables with rows to move
    assert rc == -1 and b"null" in lib.mi355_last_error()
    for n in (0, 129):
        rc = lib.mi355_jagged_block_workloads(n, None, 4, 8, 20, None, 0, None)
        assert rc == -1 and b"1..128" in lib.mi355_last_error()
    rc = lib.mi355_jagged_block_workloads(2, None, 4, 0, 20, None, 0, None)
    assert rc == -1 and b"seqlen_per_block" in lib.mi355_last_error()
    rc = lib.mi355_jagged_block_workloads(2, None, 4, 8, 20, None, 0, None)               # 4 x 2 x 3 entries do not fit 0
    assert rc == -1 and b"smaller" in lib.mi355_last_error()
    for D, dt, word in ((0, 1, b"D must be > 0"), (8, 9, b"dtype")):
        rc = lib.mi355_hstu_inference_preprocess(None, 0, None, None, 0, None, None, 4, None, 0, D, dt, None)
        assert rc == -1 and word in lib.mi355_last_error()
    rc = lib.mi355_hstu_inference_preprocess(None, 4, None, None, 4, None, None, 4, None, 8, 8, 1, None)
    assert rc == -1 and b"null" in lib.mi355_last_error()


def test_jagged_2D_tensor_concat_refuses_bad_inputs():
    import hstu_cuda_ops as H
    import mi355_native as N

    off = torch.tensor([0, 1, 2])
    with pytest.raises(ValueError):
        H.jagged_2D_tensor_concat([], [], [])
    with pytest.raises(N.NativeError):
        H.jagged_2D_tensor_concat([torch.zeros(2, 4), torch.zeros(2, 4)], [off, off], [1, 1])
    with pytest.raises(ValueError):
        H.jagged_2D_tensor_concat([torch.zeros(2, 4), torch.zeros(2, 4).half()], [off, off], [1, 1])
    with pytest.raises(ValueError):
        H.jagged_2D_tensor_concat([torch.zeros(2, 4), torch.zeros(2, 8)], [off, off], [1, 1])
