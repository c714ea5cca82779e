"""CPU checks of hstu_jagged (the jagged x dense ops and the two-tensor concat):
1. the float64 twin of tests/jagged_dense_twin.py against a padded-dense torch.baddbmm and its autograd;
2. the signatures of the seven public functions against tests/golden/jagged_dense_signatures.json;
3. every argument error that is raised before a kernel runs, and the refusal of CPU tensors;
4. the C entry points of csrc/jagged_bmm.hip answer null and negative arguments with an error code and a message."""
import inspect
import json
import os

import pytest
import torch

import jagged_dense_twin as T

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "jagged_dense_signatures.json")
NAMES = ["triton_jagged_dense_bmm", "triton_jagged_dense_bmm_broadcast_add", "triton_jagged_dense_broadcast_add",
         "triton_concat_2D_jagged", "triton_concat_2D_jagged_jagged", "triton_concat_2D_dense_jagged", "triton_split_2D_jagged"]


def _offsets(lengths):
    return [0] + torch.tensor(lengths).cumsum(0).tolist()


def _padded(offsets, rows, max_len):
    B = len(offsets) - 1
    idx = []
    for b in range(B):
        idx += [b * max_len + i for i in range(offsets[b + 1] - offsets[b])]
    idx = torch.tensor(idx, dtype=torch.int64)
    n = offsets[-1]
    flat = torch.zeros(B * max_len, rows.size(1), dtype=rows.dtype).index_add(0, idx, rows[:n])
    return flat.view(B, max_len, rows.size(1)), idx


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("surplus", [0, 3])
def test_twin_agrees_with_padded_baddbmm(with_bias, surplus):
    lengths, K, N = [0, 1, 5, 9, 0, 3], 7, 5
    off = _offsets(lengths)
    B, L = len(lengths), off[-1] + surplus
    jagged = torch.randn(L, K, dtype=torch.float64, requires_grad=True)
    dense = torch.randn(B, K, N, dtype=torch.float64, requires_grad=True)
    bias = torch.randn(B, N, dtype=torch.float64, requires_grad=True) if with_bias else None
    d_out = torch.randn(L, N, dtype=torch.float64)
    pad, idx = _padded(off, jagged, max(lengths))
    if with_bias:
        full = torch.baddbmm(bias[:, None, :], pad, dense)
    else:
        full = torch.bmm(pad, dense)
    ref = full.reshape(B * max(lengths), N)[idx]
    fwd = T.bmm_fwd(off, jagged, dense, bias)
    assert fwd.n == K + (1 if with_bias else 0)
    torch.testing.assert_close(fwd.out[:off[-1]], ref.detach(), rtol=1e-12, atol=1e-12)
    assert (fwd.out[off[-1]:] == 0).all() and (fwd.mag[off[-1]:] == 0).all()
    assert (fwd.mag >= fwd.out.abs() - 1e-12).all()
    ref.backward(d_out[:off[-1]])
    bwd = T.bmm_bwd(off, jagged, dense, d_out, with_bias)
    torch.testing.assert_close(bwd.d_jagged, jagged.grad, rtol=1e-12, atol=1e-12)
    assert (bwd.d_jagged[off[-1]:] == 0).all()
    torch.testing.assert_close(bwd.d_dense, dense.grad, rtol=1e-12, atol=1e-12)
    assert (bwd.d_dense[0] == 0).all() and (bwd.d_dense_mag >= bwd.d_dense.abs() - 1e-12).all()
    assert bwd.lengths.tolist() == [float(v) for v in lengths] and bwd.n_jagged == N
    if with_bias:
        torch.testing.assert_close(bwd.d_bias, bias.grad, rtol=1e-12, atol=1e-12)
    else:
        assert bwd.d_bias is None


def test_twin_broadcast_add_and_row_sum_agree_with_autograd():
    lengths, D = [2, 0, 4, 1], 6
    off = _offsets(lengths)
    jagged = torch.randn(off[-1] + 2, D, dtype=torch.float64, requires_grad=True)
    dense = torch.randn(len(lengths), D, dtype=torch.float64, requires_grad=True)
    ref = jagged[:off[-1]] + torch.repeat_interleave(dense, torch.tensor(lengths), 0)
    out = T.broadcast_add(off, jagged, dense)
    torch.testing.assert_close(out[:off[-1]], ref.detach(), rtol=0, atol=0)
    assert (out[off[-1]:] == 0).all()
    g = torch.randn(off[-1] + 2, D, dtype=torch.float64)
    ref.backward(g[:off[-1]])
    st = T.row_sum(off, g)
    torch.testing.assert_close(st.sum, dense.grad, rtol=1e-12, atol=1e-12)
    assert (st.sum[1] == 0).all() and (st.mag >= st.sum.abs() - 1e-12).all()


def test_bounds_are_functions_of_the_reference_alone():
    ref, mag = torch.tensor([1.0, -2.0, 0.0]).double(), torch.tensor([3.0, 2.0, 0.0]).double()
    b = T.bound_gemm(ref, mag, 8, torch.bfloat16)
    assert torch.allclose(b, 2.0 ** -8 * ref.abs() + 16 * 2.0 ** -24 * mag + 2.0 ** -134, rtol=1e-15, atol=0)
    b32 = T.bound_gemm(ref, mag, 8, torch.float32)
    assert torch.allclose(b32, 2.0 ** -24 * ref.abs() + 18 * 2.0 ** -24 * mag + 2.0 ** -150, rtol=1e-15, atol=0)
    assert torch.equal(T.bound_add(ref, torch.float16), 2.0 ** -11 * ref.abs() + 2.0 ** -25)
    n = torch.tensor([2.0, 0.0])[:, None, None]
    assert T.bound_gemm(torch.zeros(2, 1, 1).double(), torch.ones(2, 1, 1).double(), n, torch.float16).flatten().tolist() == \
        [4 * 2.0 ** -24 + 2.0 ** -25, 2.0 ** -25]


def _signature(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]


def test_signatures_are_the_reference_s():
    import hstu_cuda_ops
    import hstu_jagged as J

    golden = json.load(open(GOLDEN))
    assert sorted(golden) == sorted(NAMES)
    for name, want in golden.items():
        fn = getattr(J, name)
        assert getattr(J, name[len("triton_"):]) is fn, name
        got = _signature(fn)
        assert [g[0] for g in got] == [w[0] for w in want], name
        for (pname, ours), (_, literal) in zip(got, want):
            assert (ours is not inspect.Parameter.empty) == (literal is not None), (name, pname)
            if literal is not None:
                assert repr(ours) == literal, (name, pname, ours, literal)
    assert J.triton_split_2D_jagged is hstu_cuda_ops.split_2D_jagged
    assert set(NAMES) <= set(J.__all__)


def test_argument_errors_come_before_any_kernel():
    import hstu_jagged as J
    import mi355_native as N

    off = torch.tensor([0, 2, 5])
    jagged, dense, bias = torch.randn(5, 4), torch.randn(2, 4, 3), torch.randn(2, 3)
    with pytest.raises(ValueError, match="samples"):
        J.triton_jagged_dense_bmm(3, off, jagged, torch.randn(3, 4, 3))
    with pytest.raises(ValueError, match="inner sizes"):
        J.triton_jagged_dense_bmm(3, off, jagged, torch.randn(2, 5, 3))
    with pytest.raises(ValueError, match="samples"):
        J.triton_jagged_dense_bmm_broadcast_add(3, off, jagged, torch.randn(1, 4, 3), bias)
    with pytest.raises(ValueError, match="inner sizes"):
        J.triton_jagged_dense_bmm_broadcast_add(3, off, jagged, torch.randn(2, 6, 3), bias)
    with pytest.raises(ValueError, match="bias"):
        J.triton_jagged_dense_bmm_broadcast_add(3, off, jagged, dense, torch.randn(2, 4))
    with pytest.raises(ValueError, match="samples"):
        J.triton_jagged_dense_broadcast_add(3, off, jagged, torch.randn(3, 4))
    with pytest.raises(ValueError, match="inner sizes"):
        J.triton_jagged_dense_broadcast_add(3, off, jagged, torch.randn(2, 5))
    with pytest.raises(ValueError, match="batch >= 1"):
        J.triton_jagged_dense_bmm(3, torch.tensor([0]), jagged, torch.randn(0, 4, 3))
    with pytest.raises(ValueError, match="integers"):
        J.triton_jagged_dense_bmm(3, off.float(), jagged, dense)
    with pytest.raises(ValueError, match="2-D"):
        J.triton_jagged_dense_bmm(3, off, jagged[None], dense)
    # the two refusals name their argument, whatever else is passed
    a, b = torch.randn(5, 4), torch.randn(3, 4)
    off_b = torch.tensor([0, 1, 3])
    with pytest.raises(NotImplementedError, match="is_replace"):
        J.triton_concat_2D_jagged(8, a, b, off, off_b, is_replace=True)
    with pytest.raises(NotImplementedError, match="n_prefix_from_right"):
        J.triton_concat_2D_jagged(8, a, b, off, off_b, n_prefix_from_right=1)
    with pytest.raises(NotImplementedError, match="is_replace"):
        J.triton_concat_2D_jagged_jagged(4, off, a, 4, off_b, b, True, 0)
    with pytest.raises(NotImplementedError, match="n_prefix_from_right"):
        J.triton_concat_2D_jagged_jagged(4, off, a, 4, off_b, b, False, 2)
    with pytest.raises(NotImplementedError, match="n_prefix_to_right"):
        J.triton_split_2D_jagged(torch.randn(8, 4), 8, off, off_b, n_prefix_to_right=1)
    with pytest.raises(ValueError, match="both be None"):
        J.triton_concat_2D_jagged(8, a, b)
    with pytest.raises(ValueError, match="3-D"):
        J.triton_concat_2D_jagged(8, a, b, None, off_b)
    with pytest.raises(ValueError, match="hidden dim"):
        J.triton_concat_2D_jagged(8, a, torch.randn(3, 5), off, off_b)
    with pytest.raises(ValueError, match="3-D"):
        J.triton_concat_2D_dense_jagged(4, off, a, torch.randn(2, 4))
    assert N.NativeError is not None


def test_cpu_tensors_and_other_dtypes_are_refused():
    import hstu_jagged as J
    import mi355_native as N

    off = torch.tensor([0, 2, 5])
    jagged, dense, bias = torch.randn(5, 4), torch.randn(2, 4, 3), torch.randn(2, 3)
    with pytest.raises(N.NativeError):
        J.triton_jagged_dense_bmm(3, off, jagged, dense)
    with pytest.raises(N.NativeError):
        J.triton_jagged_dense_bmm_broadcast_add(3, off, jagged, dense, bias)
    with pytest.raises(N.NativeError):
        J.triton_jagged_dense_broadcast_add(3, off, jagged, torch.randn(2, 4))
    with pytest.raises(N.NativeError):
        J.triton_concat_2D_jagged(8, jagged, torch.randn(3, 4), off, torch.tensor([0, 1, 3]))
    with pytest.raises(N.NativeError):
        J.triton_concat_2D_dense_jagged(4, off, jagged, torch.randn(2, 2, 4))
    with pytest.raises(N.NativeError):
        J.triton_jagged_dense_bmm(3, off, jagged.double(), dense.double())


def test_entry_points_answer_bad_arguments_with_error_codes():
    import ctypes

    import mi355_native as N

    lib = N.lib()
    off = (ctypes.c_int64 * 3)(0, 2, 5)
    buf = (ctypes.c_uint8 * 8192)()
    o, p = ctypes.addressof(off), (ctypes.addressof(buf) + 15) & ~15
    bmm, jj, add, rs = lib.mi355_jagged_dense_bmm, lib.mi355_jagged_jagged_bmm, lib.mi355_jagged_broadcast_add, lib.mi355_jagged_row_sum

    def err(rc, word):
        assert rc == -1 and word in lib.mi355_last_error(), (rc, lib.mi355_last_error())

    # (a)
    err(bmm(p, 4, None, 2, 5, 4, 3, p, 12, 3, 1, None, 0, p, 3, 1, None), b"null offsets")
    err(bmm(None, 4, o, 2, 5, 4, 3, p, 12, 3, 1, None, 0, p, 3, 1, None), b"null buffer")
    err(bmm(p, 4, o, 2, 5, 4, 3, None, 12, 3, 1, None, 0, p, 3, 1, None), b"null buffer")
    err(bmm(p, 4, o, 2, 5, 4, 3, p, 12, 3, 1, None, 0, None, 3, 1, None), b"null buffer")
    err(bmm(p, 4, o, 2, 5, 4, 3, p, 12, 3, 1, None, 0, p, 3, 7, None), b"unsupported dtype")
    err(bmm(p, 4, o, 2, -1, 4, 3, p, 12, 3, 1, None, 0, p, 3, 1, None), b"rows must be")
    err(bmm(p, 4, o, 0, 5, 4, 3, p, 12, 3, 1, None, 0, p, 3, 1, None), b"batch must be")
    err(bmm(p, 4, o, 2, 5, -4, 3, p, 12, 3, 1, None, 0, p, 3, 1, None), b"K must be")
    err(bmm(p, 4, o, 2, 5, 4, 0, p, 12, 3, 1, None, 0, p, 3, 1, None), b"K must be")
    err(bmm(p, 3, o, 2, 5, 4, 3, p, 12, 3, 1, None, 0, p, 3, 1, None), b"smaller than the width")
    err(bmm(p, 4, o, 2, 5, 4, 3, p, 12, 3, 1, None, 0, p, 2, 1, None), b"smaller than the width")
    err(bmm(p, 4, o, 2, 5, 4, 3, p, 12, 0, 1, None, 0, p, 3, 1, None), b"stride of dense")
    err(bmm(p, 4, o, 2, 5, 4, 3, p, 12, 3, 1, p, 2, p, 3, 1, None), b"stride of bias")
    err(bmm(p + 1, 4, o, 2, 5, 4, 3, p, 12, 3, 1, None, 0, p, 3, 1, None), b"not aligned")
    assert bmm(None, 4, o, 2, 0, 4, 3, None, 12, 3, 1, None, 0, None, 3, 1, None) == 0   # no rows: nothing to do
    # (b)
    err(jj(p, 4, p, 3, None, 2, 5, 4, 3, p, 12, 3, None, 0, 1, p, 4096, None), b"null offsets")
    err(jj(p, 4, p, 3, o, 2, 5, 4, 3, None, 12, 3, None, 0, 1, p, 4096, None), b"null out")
    err(jj(None, 4, p, 3, o, 2, 5, 4, 3, p, 12, 3, None, 0, 1, p, 4096, None), b"null buffer")
    err(jj(p, 4, p, 3, o, 2, 5, 4, 3, p, 12, 3, None, 0, 9, p, 4096, None), b"unsupported dtype")
    err(jj(p, 4, p, 3, o, 2, 5, -1, 3, p, 12, 3, None, 0, 1, p, 4096, None), b"M and N")
    err(jj(p, 4, p, 3, o, 2, -5, 4, 3, p, 12, 3, None, 0, 1, p, 4096, None), b"rows must be")
    err(jj(p, 3, p, 3, o, 2, 5, 4, 3, p, 12, 3, None, 0, 1, p, 4096, None), b"smaller than the width")
    err(jj(p, 4, p, 3, o, 2, 5, 4, 3, p, 12, 2, None, 0, 1, p, 4096, None), b"smaller than the width")
    err(jj(p, 4, p, 3, o, 2, 5, 4, 3, p, 11, 3, None, 0, 1, p, 4096, None), b"batch stride")
    err(jj(p, 4, p, 3, o, 2, 5, 4, 3, p, 12, 3, p, 2, 1, p, 4096, None), b"batch stride")
    err(jj(p, 4, p, 3, o, 2, 5, 4, 3, p, 12, 3, None, 0, 1, None, 4096, None), b"workspace")
    err(jj(p, 4, p, 3, o, 2, 5, 4, 3, p, 12, 3, None, 0, 1, p + 4, 4096, None), b"workspace")
    err(jj(p, 4, p, 3, o, 2, 5, 4, 3, p, 12, 3, None, 0, 1, p, 8, None), b"workspace")
    ws = lib.mi355_jagged_jagged_bmm_workspace_bytes
    # (L // chunk + batch) slots of M N + N floats; a chunk is 64 rows per 64 x 64 tile of out, within 256 .. 4096
    assert ws(2, 5, 4, 3) == 2 * 15 * 4 and ws(2, 1000, 4, 3) == (1000 // 256 + 2) * 60
    assert ws(2, 9000, 512, 512) == (9000 // 4096 + 2) * (512 * 512 + 512) * 4 and ws(1, 0, 1, 1) == 16
    assert ws(0, 5, 4, 3) == 0 and ws(2, -1, 4, 3) == 0 and ws(2, 5, 0, 3) == 0
    # (c)
    err(add(p, 4, None, 2, 5, 4, p, 4, p, 4, 1, None), b"null offsets")
    err(add(None, 4, o, 2, 5, 4, p, 4, p, 4, 1, None), b"null buffer")
    err(add(p, 4, o, 2, 5, 4, None, 4, p, 4, 1, None), b"null buffer")
    err(add(p, 4, o, 2, 5, 4, p, 4, p, 4, -2, None), b"unsupported dtype")
    err(add(p, 4, o, 2, 5, -4, p, 4, p, 4, 1, None), b"D must be")
    err(add(p, 4, o, 2, 5, 4, p, 4, p, 3, 1, None), b"smaller than the width")
    err(add(p, 4, o, 2, 5, 4, p, 3, p, 4, 1, None), b"smaller than the width")
    err(add(p, 4, o, -2, 5, 4, p, 4, p, 4, 1, None), b"batch must be")
    # (d)
    err(rs(p, 4, None, 2, 5, 4, p, 4, 1, None), b"null offsets")
    err(rs(p, 4, o, 2, 5, 4, None, 4, 1, None), b"null out")
    err(rs(None, 4, o, 2, 5, 4, p, 4, 1, None), b"null buffer")
    err(rs(p, 4, o, 2, 5, 4, p, 4, 3, None), b"unsupported dtype")
    err(rs(p, 4, o, 2, 5, 0, p, 4, 1, None), b"D must be")
    err(rs(p, 2, o, 2, 5, 4, p, 4, 1, None), b"smaller than the width")
    err(rs(p, 4, o, 2, -1, 4, p, 4, 1, None), b"rows must be")
