"""GPU checks of fbgemm_jagged_ops: every op against the loop twin of tests/fbgemm_jagged_twin.py with torch.equal (the ops
move data: there is no tolerance), over the sizes at which the kernels change path -- wave and tile edges of the scan, its
one-block and look-back forms, every access width of the row movers, truncation / exact fit / all padding, both offsets
types -- plus the backward of both directions, the select's edge cases and one graph capture."""
import pytest
import torch

import fbgemm_gpu  # noqa: F401  (registers the ops)
import fbgemm_jagged_ops as J
import fbgemm_jagged_twin as T

pytestmark = pytest.mark.gpu

ops = torch.ops.fbgemm
I32, I64 = torch.int32, torch.int64
INT = {"i32": I32, "i64": I64}
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32, "i64": I64}
CUMSUM = {"complete": "asynchronous_complete_cumsum", "inclusive": "asynchronous_inclusive_cumsum",
          "exclusive": "asynchronous_exclusive_cumsum"}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and torch.equal(got.cpu(), want)


def _offsets(lengths, dtype=I64):
    return T.cumsum(torch.tensor(lengths, dtype=dtype), "complete")


def _rand(shape, dtype, g):
    if dtype == I64:
        return torch.randint(-2 ** 40, 2 ** 40, shape, generator=g, dtype=I64)
    return torch.randn(shape, generator=g).to(dtype)


# ---------------------------------------------------------------------------------------------------------------------
# cumulative sums
# ---------------------------------------------------------------------------------------------------------------------
# wave edges (63 / 64 / 65), block edges (256 / 257), a part of a tile and a tile and a bit (1025, 4097), the last one-block
# size and the first look-back size (8192 / 8193), and a look-back over 18 tiles
SCAN_N = [0, 1, 63, 64, 65, 256, 257, 1025, 4097, 8192, 8193, 70001]


@pytest.mark.parametrize("dtype", list(INT), ids=list(INT))
@pytest.mark.parametrize("n", SCAN_N)
def test_cumsum(n, dtype):
    x = torch.randint(0, 1000, (n,), generator=_gen(n), dtype=INT[dtype])
    xg = x.cuda()
    for mode, name in CUMSUM.items():
        assert _same(getattr(ops, name)(xg), T.cumsum(x, mode)), mode
    # (the inclusive op hands rows past one block's reach to torch.cumsum: the kernel's inclusive mode is checked there too)
    assert _same(J._cumsum_cuda(J.INCLUSIVE, xg, kernel_only=True), T.cumsum(x, "inclusive"))


@pytest.mark.parametrize("n", [1025, 70001])
def test_cumsum_carries_all_64_bits(n):
    x = torch.randint(-2 ** 62, 2 ** 62, (n,), generator=_gen(n), dtype=I64)   # the sum wraps many times
    for mode, name in CUMSUM.items():
        assert _same(getattr(ops, name)(x.cuda()), T.cumsum(x, mode)), mode


def test_cumsum_looks_back_over_more_than_one_round():
    """300 tiles in one launch (an MI355X holds 512): the look-back of the late tiles passes the 256 tiles of one round"""
    n = 4096 * 300 + 5
    x = torch.randint(-2 ** 40, 2 ** 40, (n,), generator=_gen(n), dtype=I64)
    assert _same(ops.asynchronous_exclusive_cumsum(x.cuda()), T.cumsum(x, "exclusive"))


BIG_SCAN = {}


def _big_scan(n):
    """one input and one twin pass per size, shared by the cases below"""
    if n not in BIG_SCAN:
        x = torch.randint(-2 ** 40, 2 ** 40, (n,), generator=_gen(n), dtype=I64)
        BIG_SCAN[n] = (x, T.cumsum(x, "inclusive"))
    return BIG_SCAN[n]


@pytest.mark.parametrize("mode", list(CUMSUM))
def test_cumsum_longer_than_one_launch_holds(mode):
    """1100 tiles: more than the 512 blocks an MI355X keeps resident, so the scan is three launches, the second and third
    beginning inside the row and continuing from the output of the one before -- in each mode's own way"""
    x, inc = _big_scan(4096 * 1100 - 3)
    want = {"inclusive": inc, "exclusive": inc - x, "complete": torch.cat([torch.zeros(1, dtype=I64), inc])}[mode]
    got = J._cumsum_cuda({"complete": J.COMPLETE, "inclusive": J.INCLUSIVE, "exclusive": J.EXCLUSIVE}[mode], x.cuda(),
                         kernel_only=True)
    assert _same(got, want)


def test_cumsum_2d_rows_times_tiles_exceed_one_launch():
    """3 rows of 367 tiles, 1101 work items: launch boundaries fall inside rows 1 and 2, and rows begin inside launches"""
    x, inc = _big_scan(4096 * 1100 - 3)
    n = 4096 * 366 + 5
    x2 = x[:3 * n].view(3, n)
    # (each row's sums from the one twin pass over the flat input: minus what came before the row; nothing wraps at these sizes)
    before = torch.tensor([0, int(inc[n - 1]), int(inc[2 * n - 1])]).view(3, 1)
    want = torch.cat([torch.zeros(3, 1, dtype=I64), inc[:3 * n].view(3, n) - before], 1)
    assert _same(ops.asynchronous_complete_cumsum(x2.cuda()), want)
    assert _same(ops.asynchronous_complete_cumsum(x2.cuda().to(I32)), want.to(I32))


def test_cumsum_int32_wraps_like_torch():
    x = torch.tensor([2 ** 31 - 1, 1, 5] + [2 ** 30] * 70, dtype=I32)
    got = ops.asynchronous_complete_cumsum(x.cuda())
    assert _same(got, T.cumsum(x, "complete"))
    assert torch.equal(got[1:].cpu(), torch.cumsum(x, 0, dtype=I32))
    big = torch.full((20000,), 2 ** 30 + 7, dtype=I32)                         # wraps across look-back tiles too
    assert _same(J._cumsum_cuda(J.INCLUSIVE, big.cuda(), kernel_only=True), T.cumsum(big, "inclusive"))


@pytest.mark.parametrize("shape", [(3, 130), (2, 20000), (4, 0), (0, 5)], ids=str)
def test_cumsum_2d(shape):
    x = torch.randint(0, 1000, shape, generator=_gen(shape[1]), dtype=I64)
    got = ops.asynchronous_complete_cumsum(x.cuda())
    want = T.cumsum(x, "complete") if x.numel() else torch.zeros(shape[0], shape[1] + 1, dtype=I64)
    assert _same(got, want)
    assert _same(ops.asynchronous_complete_cumsum(x.cuda().t().contiguous().t()), want)   # a non-contiguous input


def test_cumsum_agrees_with_hstu_cuda_ops_offsets():
    import hstu_cuda_ops as H

    lengths = torch.randint(0, 50, (777,), generator=_gen(7)).cuda()
    assert torch.equal(ops.asynchronous_complete_cumsum(lengths), H._complete_offsets(lengths))
    assert torch.equal(ops.asynchronous_complete_cumsum(lengths.to(I32)).to(I64), H._complete_offsets(lengths))


# ---------------------------------------------------------------------------------------------------------------------
# jagged <-> padded dense
# ---------------------------------------------------------------------------------------------------------------------
LENGTHS = [0, 1, 7, 64, 65]
MAX_LENS = [0, 1, 7, 64, 70]   # all padding, truncation of most, exact fit of 7 and of 64, no truncation
DIMS = [1, 3, 8, 130, 256]     # 2-byte to 16-byte accesses in every dtype, rows of more than one 16-byte piece
PAD = {"bf16": 0.5, "fp32": -3.25, "i64": -1}


@pytest.mark.parametrize("off_dtype", list(INT), ids=list(INT))
@pytest.mark.parametrize("dtype", list(DTYPES), ids=list(DTYPES))
@pytest.mark.parametrize("D", DIMS)
def test_to_padded_and_back(D, dtype, off_dtype):
    dt = DTYPES[dtype]
    off = _offsets(LENGTHS, INT[off_dtype])
    rows = int(off[-1]) + 2                                   # two value rows that belong to no sample
    values = _rand((rows, D), dt, _gen(D))
    vg, og = values.cuda(), off.cuda()
    for max_len in MAX_LENS:
        for pad in (0.0, PAD[dtype]):
            dense = ops.jagged_to_padded_dense(vg, [og], [max_len], pad)
            assert _same(dense, T.jagged_to_padded_dense(values, off, max_len, pad)), (max_len, pad)
        assert _same(ops.jagged_2d_to_dense(vg, og, max_len), T.jagged_to_padded_dense(values, off, max_len, 0.0))
        # back: `dense` holds the padding where a sample is short, and samples longer than max_len get zero rows
        back, back_off = ops.dense_to_jagged(dense, [og])
        want = T.dense_to_jagged(dense.cpu(), off)
        assert _same(back, want) and len(back_off) == 1 and torch.equal(back_off[0], og), max_len
        assert _same(ops.dense_to_jagged(dense, [og], rows)[0], T.dense_to_jagged(dense.cpu(), off, rows)), max_len
        assert _same(ops.dense_to_jagged(dense, [og], 5)[0], T.dense_to_jagged(dense.cpu(), off, 5)), max_len


@pytest.mark.parametrize("dtype", list(DTYPES), ids=list(DTYPES))
@pytest.mark.parametrize("D", [1, 8, 130])
def test_dense_to_jagged_takes_the_slices_of_shift_n(D, dtype):
    """dense[:, :-1] and dense[:, 1:] keep the strides of the full tensor: no copy, and 16-byte accesses only where the
    sliced base still allows them"""
    dt = DTYPES[dtype]
    dense = _rand((5, 66, D), dt, _gen(D + 1))
    dg = dense.cuda()
    short = _offsets([max(n - 1, 0) for n in LENGTHS])
    full = _offsets(LENGTHS)
    for sl in (slice(None, -1), slice(1, None)):
        for off in (short, full):
            got = ops.dense_to_jagged(dg[:, sl], [off.cuda()])[0]
            assert _same(got, T.dense_to_jagged(dense[:, sl], off))
    if D > 1:
        assert _same(ops.dense_to_jagged(dg[:, :, 1:], [full.cuda()])[0], T.dense_to_jagged(dense[:, :, 1:], full))


@pytest.mark.parametrize("dtype", ["bf16", "i64"])
def test_one_dimensional_values(dtype):
    dt = DTYPES[dtype]
    off = _offsets(LENGTHS)
    values = _rand((int(off[-1]),), dt, _gen(11))
    for max_len in (7, 70):
        dense = ops.jagged_to_padded_dense(values.cuda(), [off.cuda()], [max_len], PAD[dtype])
        assert dense.dim() == 2 and _same(dense, T.jagged_to_padded_dense(values, off, max_len, PAD[dtype]))
        back = ops.dense_to_jagged(dense, [off.cuda()])[0]
        assert back.dim() == 1 and _same(back, T.dense_to_jagged(dense.cpu(), off))


def test_empty_batch_and_empty_values():
    none = torch.zeros(1, dtype=I64)
    v0 = torch.zeros(0, 8)
    assert ops.jagged_to_padded_dense(v0.cuda(), [none.cuda()], [4], 1.0).shape == (0, 4, 8)
    off = torch.zeros(4, dtype=I64)
    assert _same(ops.jagged_to_padded_dense(v0.cuda(), [off.cuda()], [4], 1.5), torch.full((3, 4, 8), 1.5))
    d0 = torch.zeros(0, 4, 8)
    assert ops.dense_to_jagged(d0.cuda(), [none.cuda()])[0].shape == (0, 8)
    assert _same(ops.dense_to_jagged(d0.cuda(), [none.cuda()], 3)[0], torch.zeros(3, 8))
    assert _same(ops.dense_to_jagged(torch.ones(3, 4, 8).cuda(), [off.cuda()], 2)[0], torch.zeros(2, 8))
    assert ops.dense_to_jagged(torch.ones(3, 4, 8).cuda(), [off.cuda()])[0].shape == (0, 8)
    assert _same(ops.dense_to_jagged(torch.ones(2, 0, 8).cuda(), [_offsets([2, 1]).cuda()])[0], torch.zeros(3, 8))


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("D", [3, 256])
def test_backward_of_both_directions(D, dtype):
    dt = DTYPES[dtype]
    off = _offsets(LENGTHS)
    rows = int(off[-1]) + 2
    og = off.cuda()
    for max_len in (7, 64, 70):
        g = _gen(D + max_len)
        values = _rand((rows, D), dt, g).cuda().requires_grad_(True)
        dense = ops.jagged_to_padded_dense(values, [og], [max_len], 0.5)
        go = _rand(tuple(dense.shape), dt, g)
        (gv,) = torch.autograd.grad(dense, values, go.cuda())
        assert _same(gv, T.jagged_to_padded_dense_grad(go, off, rows)), max_len          # truncated rows: zero gradient
        (gv2,) = torch.autograd.grad(ops.jagged_2d_to_dense(values, og, max_len), values, go.cuda())
        assert torch.equal(gv2, gv)
        full = _rand((5, max_len + 1, D), dt, g).cuda().requires_grad_(True)
        for total_L in (None, rows):
            jag = ops.dense_to_jagged(full[:, 1:], [og], total_L)[0]
            gj = _rand(tuple(jag.shape), dt, g)
            (gd,) = torch.autograd.grad(jag, full, gj.cuda())
            want = torch.zeros(5, max_len + 1, D, dtype=dt)
            want[:, 1:] = T.dense_to_jagged_grad(gj, off, 5, max_len)                    # padded positions: zero gradient
            assert _same(gd, want), (max_len, total_L)
    ints = ops.jagged_to_padded_dense(torch.arange(rows).cuda(), [og], [7], 0)
    assert not ints.requires_grad


# ---------------------------------------------------------------------------------------------------------------------
# KeyedJaggedTensor batch select
# ---------------------------------------------------------------------------------------------------------------------
def _select_case(lengths, indices, B, *, values_dtype=I64, index_dtype=I64, offsets_dtype=None, weights=False, seed=0):
    lengths = torch.tensor(lengths, dtype=I64 if offsets_dtype is not None else index_dtype)
    offsets = T.cumsum(lengths, "complete").to(offsets_dtype or index_dtype)
    n = int(offsets[-1])
    g = _gen(seed)
    values = torch.randint(0, 2 ** 31 - 1, (n,), generator=g).to(values_dtype)
    w = torch.randn(n, generator=g) if weights else None
    indices = torch.tensor(indices, dtype=index_dtype)
    want = T.keyed_jagged_index_select_dim1(values, lengths, offsets, indices, B, w)
    args = (values.cuda(), lengths.cuda(), offsets.cuda(), indices.cuda(), B, None if w is None else w.cuda())
    got = ops.keyed_jagged_index_select_dim1(*args)
    assert len(got) == len(want) and all(_same(a, b) for a, b in zip(got, want))
    total = want[0].numel()
    given = ops.keyed_jagged_index_select_dim1(*args, total)           # selected_lengths_sum: nothing read on the host
    assert all(_same(a, b) for a, b in zip(given, want))
    return want


def test_select_worked_case():
    want = _select_case([2, 0, 1, 1, 3, 0], [2, 0, 2], 3)
    assert want[1].tolist() == [1, 2, 1, 0, 1, 0] and want[0].numel() == 5


@pytest.mark.parametrize("index_dtype", list(INT), ids=list(INT))
@pytest.mark.parametrize("values_dtype", [I64, I32, torch.int16, torch.uint8], ids=str)
def test_select_ragged_bags(values_dtype, index_dtype):
    g = _gen(21)
    F, B = 3, 37
    lengths = torch.randint(0, 11, (F * B,), generator=g).tolist()
    repeated = torch.randint(0, B, (50,), generator=g).tolist()        # S != B, indices repeat
    _select_case(lengths, repeated, B, values_dtype=values_dtype, index_dtype=INT[index_dtype], weights=True, seed=1)
    _select_case(lengths, [5], B, values_dtype=values_dtype, index_dtype=INT[index_dtype], seed=2)
    # int64 lengths with offsets and indices of either type
    _select_case(lengths, repeated, B, values_dtype=values_dtype, index_dtype=INT[index_dtype], offsets_dtype=I32, seed=4)
    _select_case(lengths, repeated, B, values_dtype=values_dtype, index_dtype=INT[index_dtype], offsets_dtype=I64, seed=5)


def test_select_out_of_range_index_gives_an_empty_bag():
    want = _select_case([2, 0, 1, 1, 3, 0], [2, 3, -1, 0, 1000], 3, weights=True)
    assert want[1].tolist() == [1, 0, 0, 2, 0, 0, 0, 0, 1, 0]


def test_select_all_empty_bags_and_no_indices():
    want = _select_case([0] * 12, [1, 1, 3, 0, 2], 4)
    assert want[0].numel() == 0 and want[1].tolist() == [0] * 15
    _select_case([1, 2, 3, 4], [], 2)


def test_select_one_long_bag_among_short_ones():
    g = _gen(22)
    F, B = 2, 40
    lengths = torch.randint(0, 4, (F * B,), generator=g).tolist()
    lengths[B + 17] = 3000
    indices = torch.randperm(B, generator=g).tolist() + [17, 17]
    want = _select_case(lengths, indices, B, weights=True, seed=3)
    assert want[0].numel() > 9000


# ---------------------------------------------------------------------------------------------------------------------
# one graph over all of it
# ---------------------------------------------------------------------------------------------------------------------
def test_ops_capture_into_a_graph_and_replay_on_new_contents():
    B, D, N = 6, 24, 9
    F = 2

    def contents(seed):
        g = _gen(seed)
        perm = torch.randperm(B, generator=g)
        seq = torch.tensor([0, 1, 9, 4, 12, 5])[perm]                   # the same lengths in another order: the same total
        bags = torch.tensor([2, 0, 1, 1, 3, 0, 4, 4, 0, 1, 2, 2]).view(F, B)[:, perm].reshape(-1)
        big = torch.randint(0, 9, (20000,), generator=g)                # a look-back scan: its clearing launch is captured too
        return dict(seq=seq, values=torch.randn(31, D, generator=g).bfloat16(), bags=bags,
                    ids=torch.randint(0, 10 ** 6, (20,), generator=g), weights=torch.randn(20, generator=g),
                    indices=torch.randperm(B, generator=g), big=big)

    def run(c):
        off = ops.asynchronous_complete_cumsum(c["seq"])
        dense = ops.jagged_to_padded_dense(c["values"], [off], [N], 0.25)
        jag = ops.dense_to_jagged(dense, [off], 31)[0]
        bag_off = ops.asynchronous_complete_cumsum(c["bags"])
        sel = ops.keyed_jagged_index_select_dim1(c["ids"], c["bags"], bag_off, c["indices"], B, c["weights"], 20)
        return [off, dense, jag, ops.asynchronous_exclusive_cumsum(c["big"])] + list(sel)

    def twin(c):
        off = T.cumsum(c["seq"], "complete")
        dense = T.jagged_to_padded_dense(c["values"], off, N, 0.25)
        sel = T.keyed_jagged_index_select_dim1(c["ids"], c["bags"], T.cumsum(c["bags"], "complete"), c["indices"], B, c["weights"])
        return [off, dense, T.dense_to_jagged(dense, off, 31), T.cumsum(c["big"], "exclusive")] + sel

    first = contents(1)
    static = {k: v.cuda() for k, v in first.items()}
    run(static)   # (loads the library outside the capture)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(graph, stream=side):
        captured = run(static)
    for c in (contents(2), contents(3)):
        for k, v in c.items():
            static[k].copy_(v)
        for t in captured:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        want = twin(c)
        names = ["offsets", "dense", "jagged", "look-back scan", "selected values", "selected lengths", "selected weights"]
        assert len(want) == len(captured) == len(names)
        for name, a, b in zip(names, captured, want):
            assert _same(a, b), name
