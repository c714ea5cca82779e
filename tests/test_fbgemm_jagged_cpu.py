"""CPU checks of fbgemm_jagged_ops: the loop twin (tests/fbgemm_jagged_twin.py) and the "CPU" implementations of the ops on
worked cases, the schemas, the `fbgemm_gpu` import name, Meta shapes, the refusals, the shift-by-n chain of the reference's
jagged_tensors_shift_n, and the argument checks of the C entry points."""
import ctypes
import importlib

import pytest
import torch

import fbgemm_jagged_twin as T

fbgemm_gpu = importlib.import_module("fbgemm_gpu")   # the reference's `import fbgemm_gpu`: registers the ops
import fbgemm_jagged_ops as J  # noqa: E402

ops = torch.ops.fbgemm
I64 = torch.int64


def _t(x, dtype=I64):
    return torch.tensor(x, dtype=dtype)


def test_import_registers_every_op_with_fbgemms_schema():
    assert sorted(J.REGISTERED) == sorted(J.SCHEMAS)   # no real fbgemm_gpu here: every op is ours
    for name, schema in J.SCHEMAS.items():
        op = getattr(ops, name)
        # (compared as parsed schemas: printing normalises the default 0.0 to "0.")
        assert str(op.default._schema) == str(torch._C.parse_schema("fbgemm::" + schema))


SCHEMA_STRINGS = [
    "asynchronous_complete_cumsum(Tensor t_in) -> Tensor",
    "asynchronous_inclusive_cumsum(Tensor t_in) -> Tensor",
    "asynchronous_exclusive_cumsum(Tensor t_in) -> Tensor",
    "jagged_to_padded_dense(Tensor values, Tensor[] offsets, SymInt[] max_lengths, float padding_value=0.0) -> Tensor",
    "jagged_2d_to_dense(Tensor values, Tensor offsets, SymInt max_sequence_length) -> Tensor",
    "dense_to_jagged(Tensor dense, Tensor[] x_offsets, SymInt? total_L=None) -> (Tensor, Tensor[])",
    "keyed_jagged_index_select_dim1(Tensor values, Tensor lengths, Tensor offsets, Tensor indices, SymInt batch_size, "
    "Tensor? weights=None, SymInt? selected_lengths_sum=None) -> Tensor[]",
]


def test_schema_strings():
    assert sorted(J.SCHEMAS.values()) == sorted(SCHEMA_STRINGS)


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_cumsum_worked_case(dtype):
    x = _t([3, 0, 2, 5], dtype)
    want = {"complete": [0, 3, 3, 5, 10], "inclusive": [3, 3, 5, 10], "exclusive": [0, 3, 3, 5]}
    for mode, op in (("complete", ops.asynchronous_complete_cumsum), ("inclusive", ops.asynchronous_inclusive_cumsum),
                     ("exclusive", ops.asynchronous_exclusive_cumsum)):
        w = _t(want[mode], dtype)
        assert torch.equal(T.cumsum(x, mode), w)
        got = op(x)
        assert got.dtype == dtype and torch.equal(got, w)


def test_cumsum_2d_empty_and_wrap():
    x = _t([[1, 2, 3], [4, 0, 6]])
    want = _t([[0, 1, 3, 6], [0, 4, 4, 10]])
    assert torch.equal(T.cumsum(x, "complete"), want) and torch.equal(ops.asynchronous_complete_cumsum(x), want)
    e = torch.empty(0, dtype=I64)
    assert torch.equal(ops.asynchronous_complete_cumsum(e), _t([0])) and torch.equal(T.cumsum(e, "complete"), _t([0]))
    assert ops.asynchronous_inclusive_cumsum(e).shape == (0,) and ops.asynchronous_exclusive_cumsum(e).shape == (0,)
    big = _t([2 ** 31 - 1, 1, 5], torch.int32)
    want = _t([0, 2 ** 31 - 1, -2 ** 31, -2 ** 31 + 5], torch.int32)
    assert torch.equal(T.cumsum(big, "complete"), want) and torch.equal(ops.asynchronous_complete_cumsum(big), want)
    with pytest.raises(RuntimeError):
        ops.asynchronous_inclusive_cumsum(x)   # only the complete sum takes 2-D


OFF = [0, 3, 3, 5, 10]
PADDED = [[0, 1, 2, -1], [-1, -1, -1, -1], [3, 4, -1, -1], [5, 6, 7, 8]]


@pytest.mark.parametrize("off_dtype", [torch.int32, torch.int64])
def test_to_padded_and_back_worked_case(off_dtype):
    values, off = torch.arange(10), _t(OFF, off_dtype)
    want = _t(PADDED)
    assert torch.equal(T.jagged_to_padded_dense(values, off, 4, -1), want)
    got = ops.jagged_to_padded_dense(values, [off], [4], -1)
    assert got.dtype == I64 and torch.equal(got, want)   # element 9 is truncated
    back = _t([0, 1, 2, 3, 4, 5, 6, 7, 8, 0])             # the last row is beyond N: zero
    assert torch.equal(T.dense_to_jagged(want, off), back)
    out, out_offsets = ops.dense_to_jagged(want, [off])
    assert torch.equal(out, back) and len(out_offsets) == 1 and torch.equal(out_offsets[0], off)
    assert torch.equal(ops.dense_to_jagged(want, [off], 10)[0], back)
    assert torch.equal(ops.dense_to_jagged(want, [off], 12)[0], _t(back.tolist() + [0, 0]))   # rows of no sample: zeros
    assert torch.equal(T.dense_to_jagged(want, off, 12), _t(back.tolist() + [0, 0]))


def test_to_dense_2d_values_and_float_padding():
    g = torch.Generator().manual_seed(3)
    values, off = torch.randn(10, 3, generator=g), _t(OFF)
    want = T.jagged_to_padded_dense(values, off, 4, 0.5)
    assert want.shape == (4, 4, 3) and torch.equal(want[1], torch.full((4, 3), 0.5))
    assert torch.equal(ops.jagged_to_padded_dense(values, [off], [4], 0.5), want)
    assert torch.equal(ops.jagged_2d_to_dense(values, off, 4), T.jagged_to_padded_dense(values, off, 4, 0.0))
    mask = ops.jagged_to_padded_dense(torch.ones(10, 1, dtype=I64), [off], [4], 0).to(torch.bool)   # the reference's mask
    assert mask.shape == (4, 4, 1) and mask.sum().item() == 9
    strided = want[:, 1:]
    assert torch.equal(ops.dense_to_jagged(strided, [_t([0, 2, 2, 3, 6])])[0], T.dense_to_jagged(strided, _t([0, 2, 2, 3, 6])))


def test_autograd_cpu_matches_the_adjoints():
    g = torch.Generator().manual_seed(4)
    off = _t(OFF)
    values = torch.randn(11, 3, generator=g, requires_grad=True)   # row 10 belongs to no sample
    out = ops.jagged_to_padded_dense(values, [off], [4], 0.25)
    go = torch.randn(out.shape, generator=g)
    (gv,) = torch.autograd.grad(out, values, go)
    assert torch.equal(gv, T.jagged_to_padded_dense_grad(go, off, 11))
    assert gv[9].abs().sum() == 0 and gv[10].abs().sum() == 0      # truncated row, row of no sample
    dense = torch.randn(4, 4, 3, generator=g, requires_grad=True)
    jag = ops.dense_to_jagged(dense, [off])[0]
    gj = torch.randn(jag.shape, generator=g)
    (gd,) = torch.autograd.grad(jag, dense, gj)
    assert torch.equal(gd, T.dense_to_jagged_grad(gj, off, 4, 4))
    assert gd[1].abs().sum() == 0                                   # an empty sample: all padding
    ints = ops.jagged_to_padded_dense(torch.arange(10), [off], [4], 0)
    assert not ints.requires_grad


def test_select_worked_case():
    lengths, values, indices = _t([2, 0, 1, 1, 3, 0]), torch.arange(100, 107), _t([2, 0, 2])
    offsets = ops.asynchronous_complete_cumsum(lengths)
    want_v, want_l = _t([102, 100, 101, 102, 103]), _t([1, 2, 1, 0, 1, 0])
    for got in (T.keyed_jagged_index_select_dim1(values, lengths, offsets, indices, 3),
                ops.keyed_jagged_index_select_dim1(values, lengths, offsets, indices, 3),
                ops.keyed_jagged_index_select_dim1(values, lengths, offsets, indices, 3, None, 5)):
        assert len(got) == 2 and torch.equal(got[0], want_v) and torch.equal(got[1], want_l)
    w = torch.arange(7, dtype=torch.float32) / 8
    for got in (T.keyed_jagged_index_select_dim1(values, lengths, offsets, indices, 3, w),
                ops.keyed_jagged_index_select_dim1(values, lengths, offsets, indices, 3, w)):
        assert len(got) == 3 and torch.equal(got[0], want_v) and torch.equal(got[2], w[want_v - 100])
    # an index outside [0, B): an empty bag
    bad = _t([2, 7, -1, 0])
    twin = T.keyed_jagged_index_select_dim1(values, lengths, offsets, bad, 3)
    got = ops.keyed_jagged_index_select_dim1(values, lengths, offsets, bad, 3)
    assert torch.equal(twin[1], _t([1, 0, 0, 2, 0, 0, 0, 1])) and torch.equal(got[1], twin[1]) and torch.equal(got[0], twin[0])


def test_meta_shapes():
    m = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device="meta")   # noqa: E731
    assert ops.asynchronous_complete_cumsum(m(7, dtype=I64)).shape == (8,)
    assert ops.asynchronous_complete_cumsum(m(3, 7, dtype=I64)).shape == (3, 8)
    assert ops.asynchronous_inclusive_cumsum(m(7, dtype=I64)).shape == (7,)
    assert ops.asynchronous_exclusive_cumsum(m(7, dtype=torch.int32)).dtype == torch.int32
    off = m(5, dtype=I64)
    out = ops.jagged_to_padded_dense(m(10, 3, dtype=torch.bfloat16), [off], [6], 0.0)
    assert out.shape == (4, 6, 3) and out.dtype == torch.bfloat16 and out.device.type == "meta"
    assert ops.jagged_to_padded_dense(m(10), [off], [6]).shape == (4, 6)
    assert ops.jagged_2d_to_dense(m(10, 3), off, 6).shape == (4, 6, 3)
    jag, offs = ops.dense_to_jagged(m(4, 6, 3), [off], 9)
    assert jag.shape == (9, 3) and len(offs) == 1
    with pytest.raises(RuntimeError):
        ops.dense_to_jagged(m(4, 6, 3), [off])


def test_refusals():
    off = _t(OFF)
    with pytest.raises(NotImplementedError):
        ops.jagged_to_padded_dense(torch.arange(10), [off, off], [4, 4], 0)
    with pytest.raises(NotImplementedError):
        ops.dense_to_jagged(torch.zeros(4, 4), [off, off])
    lengths = _t([2, 0, 1, 1, 3, 0])
    offsets = ops.asynchronous_complete_cumsum(lengths)
    values = torch.arange(7, dtype=torch.float32).requires_grad_(True)
    with pytest.raises(RuntimeError, match="requires_grad"):
        ops.keyed_jagged_index_select_dim1(values, lengths, offsets, _t([0]), 3)


@pytest.mark.parametrize("n", [1, 2])
def test_shift_by_n_chain(n):
    """What the reference's jagged_tensors_shift_n computes: every sample loses its last n rows (history) or its first n
    (supervision).  The chain is the complete cumsum of the shortened lengths, the padded form of the values, the two
    slices of it along the sequence axis, and each slice back to jagged."""
    g = torch.Generator().manual_seed(5)
    seqlen = _t([0, 1, 5, 2, 7])
    max_seqlen = 7
    off = ops.asynchronous_complete_cumsum(seqlen)
    total = int(off[-1])
    for values in (torch.randn(total, 3, generator=g), torch.arange(total).unsqueeze(-1)):
        short = torch.clamp(seqlen - n, min=0)
        short_off = ops.asynchronous_complete_cumsum(short)
        assert torch.equal(short_off, T.cumsum(short, "complete"))
        dense = ops.jagged_2d_to_dense(values, off, max_seqlen)
        history = ops.dense_to_jagged(dense[:, :-n], [short_off])[0]
        supervision = ops.dense_to_jagged(dense[:, n:], [short_off])[0]
        want_h = torch.cat([values[int(off[b]):int(off[b + 1]) - n] for b in range(5) if seqlen[b] > n])
        want_s = torch.cat([values[int(off[b]) + n:int(off[b + 1])] for b in range(5) if seqlen[b] > n])
        assert torch.equal(history, want_h) and torch.equal(supervision, want_s)
        # and the twin walks the same chain to the same rows
        td = T.jagged_to_padded_dense(values, off, max_seqlen)
        assert torch.equal(T.dense_to_jagged(td[:, :-n], short_off), want_h)
        assert torch.equal(T.dense_to_jagged(td[:, n:], short_off), want_s)


def test_entry_points_answer_bad_arguments_with_an_error_code():
    import mi355_native as N

    lib = N.lib()
    buf = (ctypes.c_uint64 * 32)()
    p = ctypes.addressof(buf)

    def refused(rc, word):
        assert rc == -1 and word in lib.mi355_last_error(), (rc, lib.mi355_last_error())

    refused(lib.mi355_cumsum(p, p, 1, 4, 7, 0, None, 0, None), b"dtype")
    refused(lib.mi355_cumsum(p, p, 1, -4, 1, 0, None, 0, None), b"negative")
    refused(lib.mi355_cumsum(None, p, 1, 4, 1, 0, None, 0, None), b"null")
    refused(lib.mi355_cumsum(p, p, 1, 4, 1, 3, None, 0, None), b"mode")
    refused(lib.mi355_cumsum(p, p, 2, 4, 1, 1, None, 0, None), b"2-D")
    refused(lib.mi355_cumsum(p, p, 1, 1 << 20, 1, 0, None, 0, None), b"workspace")
    assert lib.mi355_cumsum_workspace_bytes(1, 8192) == 0 and lib.mi355_cumsum_workspace_bytes(2, 1 << 20) == 16 + 2 * 256 * 16
    assert lib.mi355_cumsum_workspace_bytes(1, J.ONE_BLOCK_SCAN) == 0 and lib.mi355_cumsum_workspace_bytes(1, J.ONE_BLOCK_SCAN + 1) > 0
    assert lib.mi355_cumsum(None, None, 1, 0, 1, 0, None, 0, None) == 0   # nothing to do: no launch, no error

    refused(lib.mi355_jagged_to_padded(p, 4, p, 1, 2, 3, 4, 3, 0, p, None), b"dtype")
    refused(lib.mi355_jagged_to_padded(p, 4, p, 5, 2, 3, 4, 4, 0, p, None), b"offsets dtype")
    refused(lib.mi355_jagged_to_padded(p, -4, p, 1, 2, 3, 4, 4, 0, p, None), b"negative")
    refused(lib.mi355_jagged_to_padded(p, 4, None, 1, 2, 3, 4, 4, 0, p, None), b"null")
    refused(lib.mi355_jagged_to_padded(p, 4, p, 1, 2, 3, 0, 4, 0, p, None), b"D must be")

    refused(lib.mi355_padded_to_jagged(p, 12, 4, 2, 3, p, 1, 4, 1, p, 5, None), b"dtype")
    refused(lib.mi355_padded_to_jagged(p, 12, 4, 2, 3, p, 1, 4, 4, p, -5, None), b"negative")
    refused(lib.mi355_padded_to_jagged(p, -12, 4, 2, 3, p, 1, 4, 4, p, 5, None), b"stride")
    refused(lib.mi355_padded_to_jagged(p, 12, 4, 2, 3, p, 1, 4, 4, None, 5, None), b"null")

    refused(lib.mi355_kjt_select_lengths(p, 2, p, 1, 2, 3, 3, p, None), b"dtype")
    refused(lib.mi355_kjt_select_lengths(p, 1, p, 1, 2, -3, 3, p, None), b"negative")
    refused(lib.mi355_kjt_select_lengths(p, 1, None, 1, 2, 3, 3, p, None), b"null")

    refused(lib.mi355_kjt_select_values(p, 7, 3, None, 0, p, 1, p, 1, 2, 3, 3, p, 1, p, None, 5, None), b"dtype")
    refused(lib.mi355_kjt_select_values(p, 7, 8, None, 0, p, 1, p, 9, 2, 3, 3, p, 1, p, None, 5, None), b"dtype")
    refused(lib.mi355_kjt_select_values(p, -7, 8, None, 0, p, 1, p, 1, 2, 3, 3, p, 1, p, None, 5, None), b"negative")
    refused(lib.mi355_kjt_select_values(p, 7, 8, None, 0, None, 1, p, 1, 2, 3, 3, p, 1, p, None, 5, None), b"null")
    refused(lib.mi355_kjt_select_values(p, 7, 8, p, 4, p, 1, p, 1, 2, 3, 3, p, 1, p, None, 5, None), b"out_weights")


def test_gpu_implementations_refuse_what_the_kernels_do_not_cover():
    """no eager fallback behind the "CUDA" key: the launchers refuse before they touch the library"""
    import mi355_native as N

    with pytest.raises(N.NativeError):
        J._cumsum_cuda(J.COMPLETE, torch.zeros(4))                              # a float cumsum has no kernel
    with pytest.raises(N.NativeError):
        J._to_padded_cuda(torch.zeros(4, 2, dtype=torch.uint8), _t([0, 4]), 4, 0.0)   # 1-byte elements
    with pytest.raises(N.NativeError):
        J._to_padded_cuda(torch.zeros(4, 2), torch.tensor([0.0, 4.0]), 4, 0.0)        # float offsets
