"""GPU checks of hstu_jagged: the jagged x dense product (with and without bias), the broadcast add and the two-tensor concat,
forward and every gradient, element by element against the float64 twin of tests/jagged_dense_twin.py under its derived bounds.
Each comparison prints its worst |err| / bound."""
import pytest
import torch

import jagged_dense_twin as T

pytestmark = pytest.mark.gpu

LENGTHS = {
    "tiles": [0, 1, 31, 32, 33, 64, 129, 0],   # leading and trailing empty samples, both sides of one and of four 32-row tiles
    "one": [5],
    "late": [0, 0, 7],
    "long": [1, 1, 1100, 1, 1],                # the long reduction of d_dense; most tile slots leave at once
}
KN = [(8, 8), (40, 24), (64, 64), (136, 200), (1, 3)]
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
CASES = [(ln, dt) for ln in LENGTHS for dt in DTYPES if dt != "fp32" or ln in ("tiles", "one")]


def _offsets(lengths, dtype=torch.int64):
    return torch.tensor([0] + torch.tensor(lengths).cumsum(0).tolist(), dtype=dtype, device="cuda")


def _inputs(lengths, K, N, dtype, surplus=0):
    L = sum(lengths) + surplus
    g = torch.Generator().manual_seed(1000 * K + N + len(lengths))
    mk = lambda *s: torch.randn(*s, generator=g).to(dtype).cuda()   # noqa: E731
    return mk(L, K), mk(len(lengths), K, N), mk(len(lengths), N), mk(L, N)


def _run(J, lengths, jagged, dense, bias, d_out, offsets=None, max_seq_len=None):
    """(out, d_jagged, d_dense, d_bias) of one forward + backward"""
    offsets = _offsets(lengths) if offsets is None else offsets
    msl = max(lengths) if max_seq_len is None else max_seq_len
    jagged, dense = jagged.detach().requires_grad_(True), dense.detach().requires_grad_(True)
    if bias is None:
        out = J.triton_jagged_dense_bmm(msl, offsets, jagged, dense)
        grads = torch.autograd.grad(out, [jagged, dense], d_out) + (None,)
    else:
        bias = bias.detach().requires_grad_(True)
        out = J.triton_jagged_dense_bmm_broadcast_add(msl, offsets, jagged, dense, bias)
        grads = torch.autograd.grad(out, [jagged, dense, bias], d_out)
    return (out.detach(),) + tuple(grads)


def _check(name, got, ref, bound):
    ratio = T.worst(got, ref, bound)
    print(f"{name}: worst |err| / bound = {ratio:.4f}")
    assert ratio <= 1.0, name


def _bit_equal(a, b):
    return all((x is None and y is None) or (x.dtype == y.dtype and x.shape == y.shape and
                                             torch.equal(x.view(torch.uint8), y.view(torch.uint8))) for x, y in zip(a, b))


@pytest.mark.parametrize("with_bias", [False, True], ids=["plain", "bias"])
@pytest.mark.parametrize("K,N", KN)
@pytest.mark.parametrize("lengths,dt", CASES)
def test_bmm_forward_and_gradients_against_the_twin(lengths, dt, K, N, with_bias):
    import hstu_jagged as J

    lens, dtype = LENGTHS[lengths], DTYPES[dt]
    jagged, dense, bias, d_out = _inputs(lens, K, N, dtype)
    bias = bias if with_bias else None
    out, d_jagged, d_dense, d_bias = _run(J, lens, jagged, dense, bias, d_out)
    assert out.dtype == dtype and out.shape == (sum(lens), N) and d_jagged.shape == jagged.shape and d_dense.shape == dense.shape
    off = _offsets(lens).tolist()
    fwd = T.bmm_fwd(off, jagged, dense, bias)
    bwd = T.bmm_bwd(off, jagged, dense, d_out, with_bias)
    tag = f"{lengths} {dt} K{K} N{N} {'bias' if with_bias else 'plain'}"
    _check(f"out       {tag}", out, fwd.out, T.bound_gemm(fwd.out, fwd.mag, fwd.n, dtype))
    _check(f"d_jagged  {tag}", d_jagged, bwd.d_jagged, T.bound_gemm(bwd.d_jagged, bwd.d_jagged_mag, bwd.n_jagged, dtype))
    _check(f"d_dense   {tag}", d_dense, bwd.d_dense, T.bound_gemm(bwd.d_dense, bwd.d_dense_mag, bwd.lengths[:, None, None], dtype))
    if with_bias:
        assert d_bias.shape == bias.shape and d_bias.dtype == dtype
        _check(f"d_bias    {tag}", d_bias, bwd.d_bias, T.bound_gemm(bwd.d_bias, bwd.d_bias_mag, bwd.lengths[:, None], dtype))
    else:
        assert d_bias is None


@pytest.mark.parametrize("dt", list(DTYPES))
def test_d_dense_on_both_sides_of_a_sequence_chunk(dt):
    """d_dense of a sample longer than one chunk of the sequence (256 rows at these K, N) is folded from chunk sums"""
    import hstu_jagged as J

    lens, (K, N), dtype = [256, 257, 0, 513, 255], (40, 24), DTYPES[dt]
    jagged, dense, bias, d_out = _inputs(lens, K, N, dtype)
    _, _, d_dense, d_bias = _run(J, lens, jagged, dense, bias, d_out)
    bwd = T.bmm_bwd(_offsets(lens).tolist(), jagged, dense, d_out, True)
    _check(f"d_dense   chunks {dt}", d_dense, bwd.d_dense, T.bound_gemm(bwd.d_dense, bwd.d_dense_mag, bwd.lengths[:, None, None], dtype))
    _check(f"d_bias    chunks {dt}", d_bias, bwd.d_bias, T.bound_gemm(bwd.d_bias, bwd.d_bias_mag, bwd.lengths[:, None], dtype))
    # the order of the additions belongs to the sample's length: the same sample alone gives the same bits
    for b in (1, 3):
        s, e = sum(lens[:b]), sum(lens[:b + 1])
        alone = _run(J, [lens[b]], jagged[s:e], dense[b:b + 1], bias[b:b + 1], d_out[s:e])
        assert torch.equal(alone[2][0], d_dense[b]) and torch.equal(alone[3][0], d_bias[b])


@pytest.mark.parametrize("dt", list(DTYPES))
def test_jagged_as_a_column_slice_of_a_wider_buffer(dt):
    import hstu_jagged as J

    lens, (K, N), dtype = LENGTHS["tiles"], (40, 24), DTYPES[dt]
    jagged, dense, bias, d_out = _inputs(lens, K, N, dtype)
    wide = torch.full((jagged.size(0), 8 + K + 8), 777.0, dtype=dtype, device="cuda")
    wide[:, 8:8 + K] = jagged
    view = wide[:, 8:8 + K]
    assert not view.is_contiguous() and view.data_ptr() != wide.data_ptr()
    for b in (None, bias):
        assert _bit_equal(_run(J, lens, view, dense, b, d_out), _run(J, lens, jagged, dense, b, d_out))
    assert (wide[:, :8] == 777.0).all() and (wide[:, 8 + K:] == 777.0).all() and torch.equal(wide[:, 8:8 + K], jagged)
    # d_out as a column slice too (the backward reads it through its row stride)
    wide_g = torch.full((d_out.size(0), 8 + N + 8), 777.0, dtype=dtype, device="cuda")
    wide_g[:, 8:8 + N] = d_out
    assert _bit_equal(_run(J, lens, jagged, dense, bias, wide_g[:, 8:8 + N]), _run(J, lens, jagged, dense, bias, d_out))
    assert (wide_g[:, :8] == 777.0).all() and (wide_g[:, 8 + N:] == 777.0).all()


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("K,N", [(40, 24), (136, 200), (1, 3)])
def test_dense_as_a_transposed_view(dt, K, N):
    import hstu_jagged as J

    lens, dtype = LENGTHS["tiles"], DTYPES[dt]
    jagged, dense, bias, d_out = _inputs(lens, K, N, dtype)
    view = torch.empty_like(dense).view(dense.size(0), N, K).transpose(1, 2)   # [B, K, N] with strides (K N, 1, K)
    view.copy_(dense)
    assert (view.stride(1), view.stride(2)) == (1, K) and torch.equal(view, dense)
    assert _bit_equal(_run(J, lens, jagged, view, bias, d_out), _run(J, lens, jagged, dense, bias, d_out))


@pytest.mark.parametrize("dt", list(DTYPES))
def test_rows_past_the_last_offset_are_zero_and_never_read(dt):
    import hstu_jagged as J

    lens, (K, N), dtype = LENGTHS["tiles"], (40, 24), DTYPES[dt]
    jagged, dense, bias, d_out = _inputs(lens, K, N, dtype, surplus=5)
    n = sum(lens)
    jagged[n:] = float("nan")
    d_out[n:] = float("nan")
    for b in (None, bias):
        out, d_jagged, d_dense, d_bias = _run(J, lens, jagged, dense, b, d_out)
        assert out.shape[0] == n + 5 and (out[n:] == 0).all() and (d_jagged[n:] == 0).all()
        for t in (out, d_jagged, d_dense, d_bias):
            assert t is None or not torch.isnan(t).any()
        want = _run(J, lens, jagged[:n], dense, b, d_out[:n])
        assert _bit_equal((out[:n], d_jagged[:n], d_dense, d_bias), want)


def test_max_seq_len_and_offset_dtype_do_not_matter():
    import hstu_jagged as J

    lens, (K, N), dtype = LENGTHS["tiles"], (64, 64), torch.bfloat16
    jagged, dense, bias, d_out = _inputs(lens, K, N, dtype)
    exact = _run(J, lens, jagged, dense, bias, d_out)
    for msl in (7, max(lens) + 1000):
        assert _bit_equal(_run(J, lens, jagged, dense, bias, d_out, max_seq_len=msl), exact), msl
    assert _bit_equal(_run(J, lens, jagged, dense, bias, d_out, offsets=_offsets(lens, torch.int32)), exact)


@pytest.mark.parametrize("lengths", ["tiles", "long"])
def test_backward_is_bitwise_reproducible(lengths):
    import hstu_jagged as J

    lens, (K, N), dtype = LENGTHS[lengths], (136, 200), torch.bfloat16
    jagged, dense, bias, d_out = _inputs(lens, K, N, dtype)
    first = _run(J, lens, jagged, dense, bias, d_out)
    assert _bit_equal(_run(J, lens, jagged, dense, bias, d_out), first)


def test_an_empty_jagged_tensor_needs_no_launch():
    import hstu_jagged as J

    off = _offsets([0, 0])
    jagged = torch.empty(0, 8, dtype=torch.bfloat16, device="cuda", requires_grad=True)
    dense = torch.randn(2, 8, 4, device="cuda").bfloat16().requires_grad_(True)
    bias = torch.randn(2, 4, device="cuda").bfloat16().requires_grad_(True)
    out = J.triton_jagged_dense_bmm_broadcast_add(0, off, jagged, dense, bias)
    assert out.shape == (0, 4)
    gj, gd, gb = torch.autograd.grad(out, [jagged, dense, bias], torch.empty(0, 4, dtype=torch.bfloat16, device="cuda"))
    assert gj.shape == (0, 8) and (gd == 0).all() and (gb == 0).all()


@pytest.mark.parametrize("D", [8, 72, 2050])
@pytest.mark.parametrize("lengths,dt", CASES)
def test_broadcast_add_and_its_row_sum(lengths, dt, D):
    import hstu_jagged as J

    lens, dtype = LENGTHS[lengths], DTYPES[dt]
    g = torch.Generator().manual_seed(D + len(lens))
    L, B = sum(lens) + 2, len(lens)
    jagged = torch.randn(L, D, generator=g).to(dtype).cuda().requires_grad_(True)
    dense = torch.randn(B, D, generator=g).to(dtype).cuda().requires_grad_(True)
    d_out = torch.randn(L, D, generator=g).to(dtype).cuda()
    offsets = _offsets(lens)
    out = J.triton_jagged_dense_broadcast_add(max(lens), offsets, jagged, dense)
    d_jagged, d_dense = torch.autograd.grad(out, [jagged, dense], d_out)
    off = offsets.tolist()
    ref = T.broadcast_add(off, jagged, dense)
    tag = f"{lengths} {dt} D{D}"
    _check(f"add       {tag}", out, ref, T.bound_add(ref, dtype))
    assert (out[sum(lens):] == 0).all()
    assert torch.equal(d_jagged, d_out)
    st = T.row_sum(off, d_out)
    _check(f"row sum   {tag}", d_dense, st.sum, T.bound_row_sum(st, dtype))
    # a column slice of a wider buffer is read in place and gives the same bits
    wide = torch.full((L, D + 16), 777.0, dtype=dtype, device="cuda")
    wide[:, 8:8 + D] = jagged.detach()
    assert torch.equal(J.triton_jagged_dense_broadcast_add(max(lens), offsets, wide[:, 8:8 + D], dense.detach()), out.detach())
    assert (wide[:, :8] == 777.0).all() and (wide[:, 8 + D:] == 777.0).all()


def _cat_per_sample(a, off_a, b, off_b):
    parts = []
    for i in range(len(off_a) - 1):
        parts += [a[off_a[i]:off_a[i + 1]], b[off_b[i]:off_b[i + 1]]]
    return torch.cat(parts, 0)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("kind", ["jagged_jagged", "dense_a", "dense_b"])
def test_concat_is_torch_cat_per_sample_and_split_undoes_it(kind, dt):
    import hstu_jagged as J

    dtype, D, dense_size = DTYPES[dt], 72, 3
    lens_a, lens_b = [0, 1, 31, 33, 0, 7], [2, 0, 5, 64, 0, 1]
    B = len(lens_a)
    if kind == "dense_a":
        lens_a = [dense_size] * B
    if kind == "dense_b":
        lens_b = [dense_size] * B
    off_a, off_b = _offsets(lens_a), _offsets(lens_b)
    a = torch.randn(sum(lens_a), D, device="cuda").to(dtype).requires_grad_(True)
    b = torch.randn(sum(lens_b), D, device="cuda").to(dtype).requires_grad_(True)
    va = a.view(B, dense_size, D) if kind == "dense_a" else a
    vb = b.view(B, dense_size, D) if kind == "dense_b" else b
    msl = max(x + y for x, y in zip(lens_a, lens_b))
    if kind == "jagged_jagged":
        out = J.triton_concat_2D_jagged_jagged(max(lens_a), off_a, va, max(lens_b), off_b, vb, False, 0)
        assert torch.equal(out, J.triton_concat_2D_jagged(msl, va, vb, off_a, off_b))
    elif kind == "dense_a":
        out = J.triton_concat_2D_dense_jagged(max(lens_b), off_b, vb, va)
    else:
        out = J.triton_concat_2D_jagged(msl, va, vb, off_a, None)
    want = _cat_per_sample(a, off_a.tolist(), b, off_b.tolist())
    assert torch.equal(out, want)
    g = torch.randn_like(want)
    ga, gb = torch.autograd.grad(out, [a, b], g)
    wa, wb = torch.autograd.grad(want, [a, b], g)
    assert torch.equal(ga, wa) and torch.equal(gb, wb)
    back_a, back_b = J.triton_split_2D_jagged(out.detach(), msl, None if kind == "dense_a" else off_a,
                                              None if kind == "dense_b" else off_b, dense_size=dense_size)
    assert back_a.shape == va.shape and back_b.shape == vb.shape
    assert torch.equal(back_a, va.detach()) and torch.equal(back_b, vb.detach())


def test_forward_and_backward_capture_into_a_graph():
    import hstu_jagged as J

    lens, (K, N), dtype = LENGTHS["tiles"], (40, 24), torch.bfloat16
    jagged, dense, bias, d_out = _inputs(lens, K, N, dtype)
    offsets = _offsets(lens)
    eager = _run(J, lens, jagged, dense, bias, d_out, offsets=offsets)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(graph, stream=side):
        captured = _run(J, lens, jagged, dense, bias, d_out, offsets=offsets)
    for t in captured:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert _bit_equal(captured, eager)
