"""GPU checks of the HSTU positional encoder (csrc/position_ops.hip behind hstu_position) and of split_2D_jagged, against the
float64 twin of tests/position_twin.py.  The shapes are the smallest that reach every branch: six sequences of 0, 1, 7, 67, 130
and 40 rows (empty, shorter than a wave's run, longer than a 64-row chunk and than the table), a table of K = 48 rows, and
D = 8, 72 and 256 (72: no power of two and no multiple of 64).

Bounds, with u the unit roundoff of the dtype written (2^-8 bf16, 2^-11 fp16, 2^-24 fp32):
* forward of the position add: |out - ref| <= u |ref| + 2^-22 (|jagged scale| + |dense|): one rounding after at most two fp32
  operations on O(1) inputs.
* a table gradient of M terms: |err| <= (M + 1) 2^-24 sum|terms| + u |ref|: an fp32 sum of M terms in any order, then one rounding;
  M and sum|terms| come per element from the twin's index map.
* the timestamp forward is specified to the bit and compared bit for bit."""
import pytest
import torch

import position_twin as T

pytestmark = pytest.mark.gpu

DEV = "cuda"
LENGTHS = (0, 1, 7, 67, 130, 40)
K = 48
DIMS = (8, 72, 256)
DTYPES = (torch.bfloat16, torch.float16, torch.float32)
# mixed: one sequence (the last) is all targets; heavy: 217 of the 245 rows are targets
TARGETS = {"none": None, "zeros": (0, 0, 0, 0, 0, 0), "mixed": (0, 1, 3, 10, 20, 40), "heavy": (0, 1, 6, 60, 120, 30)}
IND_OFFSETS = (0, 3, 0, 100, 5, 2)   # 100 pushes the whole 67-row sequence past its high index


def _P():
    import hstu_position as P

    return P


def _offsets():
    return torch.tensor([0] + list(torch.tensor(LENGTHS).cumsum(0)), dtype=torch.int64, device=DEV)


def _lengths():
    return torch.tensor(LENGTHS, dtype=torch.int64, device=DEV)


def _high(targets):
    high = torch.tensor(LENGTHS, dtype=torch.int64)
    if TARGETS[targets] is not None:
        high = high - torch.tensor(TARGETS[targets])
    return high.to(DEV)


def _table_dtypes(dtype):
    return (torch.float32,) if dtype == torch.float32 else (torch.float32, dtype)


def _rand(rows, D, dtype, strided=False):
    """O(1) values; strided: a column slice of a wider tensor (row stride D + 8)"""
    if strided:
        return torch.randn(rows, D + 8, device=DEV).to(dtype)[:, 8:]
    return torch.randn(rows, D, device=DEV).to(dtype)


def _assert_table_grad(got, d_out, idx, rows, name):
    total, mags, count = T.rows_sum(d_out, idx, rows)
    err = (got.detach().cpu().double() - total).abs()
    bound = (count[:, None] + 1) * 2.0 ** -24 * mags + T.unit_roundoff(got.dtype) * total.abs()
    worst = float((err / bound.clamp(min=1e-300)).max())
    print(f"{name}: worst |err| / bound = {worst:.3f}")
    assert bool((err <= bound).all()), f"{name}: worst |err| / bound = {worst}"
    empty = count == 0
    assert bool((got.detach().cpu()[empty] == 0).all()), f"{name}: a row nothing maps to is not zero"


# ---- (a) add_position_embeddings ----
@pytest.mark.parametrize("with_ind", [False, True])
@pytest.mark.parametrize("targets", ["none", "zeros", "mixed"])
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_add_position_embeddings_forward(dtype, D, targets, with_ind):
    P = _P()
    off, high = _offsets(), _high(targets)
    ind = torch.tensor(IND_OFFSETS, dtype=torch.int64, device=DEV) if with_ind else None
    for table_dtype in _table_dtypes(dtype):
        for strided in (False, True):
            jag, dense = _rand(sum(LENGTHS), D, dtype, strided), _rand(K, D, table_dtype, strided)
            scale = 1.0 if strided else D ** 0.5
            out = P.add_position_embeddings(jag, off, high, max(LENGTHS), dense, scale, ind)
            assert out.dtype == dtype and out.shape == jag.shape and out.is_contiguous()
            ref, mag = T.add_position_embeddings(jag, off, high, dense, scale, ind)
            err = (out.cpu().double() - ref).abs()
            bound = T.unit_roundoff(dtype) * ref.abs() + 2.0 ** -22 * mag
            assert bool((err <= bound).all()), f"worst |err| / bound = {float((err / bound.clamp(min=1e-300)).max())}"


def test_add_position_embeddings_converts_int32_arguments():
    P = _P()
    off, high = _offsets(), _high("mixed")
    jag, dense = _rand(sum(LENGTHS), 72, torch.bfloat16), _rand(K, 72, torch.float32)
    a = P.add_position_embeddings(jag, off, high, 130, dense, 2.0)
    b = P.triton_add_position_embeddings(jag, off.to(torch.int32), high.to(torch.int32), 130, dense, 2.0)
    assert torch.equal(a, b)


@pytest.mark.parametrize("scale", [1.0, 3.0])
@pytest.mark.parametrize("targets", ["none", "zeros", "mixed"])
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_add_position_embeddings_backward(dtype, D, targets, scale):
    P = _P()
    off, high = _offsets(), _high(targets)
    idx = T.position_index(off, high, K)
    for table_dtype in _table_dtypes(dtype):
        jag = _rand(sum(LENGTHS), D, dtype).requires_grad_(True)
        dense = _rand(K, D, table_dtype).requires_grad_(True)
        d_out = _rand(sum(LENGTHS), D, dtype, strided=(scale != 1.0))
        grads = []
        for _ in range(2):
            out = P.add_position_embeddings(jag, off, high, max(LENGTHS), dense, scale)
            grads.append(torch.autograd.grad(out, (jag, dense), d_out))
        (d_jag, d_dense), (d_jag2, d_dense2) = grads
        assert d_dense.dtype == table_dtype and d_dense.shape == (K, D) and d_jag.dtype == dtype
        assert torch.equal(d_dense, d_dense2) and torch.equal(d_jag, d_jag2)   # bitwise reproducible
        if scale == 1.0:
            assert d_jag.data_ptr() == d_out.data_ptr()
        else:
            want = (d_out.float() * scale).to(dtype).cpu().double()
            assert bool(((d_jag.cpu().double() - want).abs() <= T.ulp(want, dtype)).all())
        _assert_table_grad(d_dense, d_out, idx, K, f"d_dense {dtype} {table_dtype} D={D} {targets}")


def test_add_position_embeddings_backward_with_ind_offsets_raises():
    P = _P()
    jag = _rand(sum(LENGTHS), 8, torch.bfloat16).requires_grad_(True)
    dense = _rand(K, 8, torch.float32).requires_grad_(True)
    ind = torch.tensor(IND_OFFSETS, dtype=torch.int64, device=DEV)
    out = P.add_position_embeddings(jag, _offsets(), _high("none"), 130, dense, 2.0, ind)
    with pytest.raises(AssertionError, match="No backward support for position encoder with incremental input"):
        out.sum().backward()


# ---- (c) add_timestamp_positional_embeddings ----
TS_CONFIGS = [  # (targets, interleave, max_contextual_seq_len, fn)
    ("none", False, 0, "sqrt"), ("zeros", False, 2, "sqrt"), ("mixed", False, 0, "sqrt"), ("mixed", True, 2, "sqrt"),
    ("mixed", False, 2, "log"), ("none", False, 0, "log"),
]


def _ts_case(targets, interleave, mcsl, fn, Np, recent=None, seed=11):
    off = _offsets()
    stamps = T.make_timestamps(off, fn, seed, recent)
    nt = None if TARGETS[targets] is None else torch.tensor(TARGETS[targets], dtype=torch.int64)
    p = T.timestamp_position_index(off, torch.tensor(LENGTHS), nt, interleave, mcsl, Np)
    t = T.time_bucket(T.time_deltas(off, stamps), fn)
    return off, stamps.to(DEV), (None if nt is None else nt.to(DEV)), p, t


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_add_timestamp_positional_embeddings_forward(dtype, D):
    import mi355_native as N

    P = _P()
    rows, Np = sum(LENGTHS), K
    for table_dtype in _table_dtypes(dtype):
        for strided, (targets, interleave, mcsl, fn) in enumerate(TS_CONFIGS):
            off, stamps, nt, p, t = _ts_case(targets, interleave, mcsl, fn, Np)
            seq = _rand(rows, D, dtype, strided % 2 == 1)
            pos, ts = _rand(Np, D, table_dtype), _rand(P.NUM_TIME_BUCKETS + 1, D, table_dtype, strided % 2 == 1)
            out = P.add_timestamp_positional_embeddings(seq, off, pos, ts, stamps, 130, mcsl, _lengths(), nt, interleave, fn)
            want = seq + (pos[p.to(DEV)] + ts[t.to(DEV)]).to(dtype)
            assert torch.equal(out, want), f"{table_dtype} {targets} interleave={interleave} mcsl={mcsl} {fn}"
            # the index maps the kernel writes for the training call, every row of them
            pos_inds = torch.full((rows,), -1, dtype=torch.int32, device=DEV)
            ts_inds = torch.full((rows,), -1, dtype=torch.int32, device=DEV)
            seq_c, out2 = seq.contiguous(), torch.empty(rows, D, dtype=dtype, device=DEV)
            N.check(N.lib().mi355_hstu_add_timestamp_position_embeddings(
                N.ptr(seq_c), D, rows, D, N.dt(seq_c), N.ptr(off), N.ptr(_lengths()), len(LENGTHS), N.ptr(pos), D, Np,
                N.ptr(ts), ts.stride(0), ts.size(0), N.dt(pos), N.ptr(stamps), N.ptr(nt), int(interleave), mcsl,
                {"sqrt": 0, "log": 1}[fn], 2048, 60.0, 1.0, 0, N.ptr(out2), D, N.ptr(pos_inds), N.ptr(ts_inds), N.stream()))
            assert torch.equal(pos_inds.cpu().long(), p) and torch.equal(ts_inds.cpu().long(), t)
            assert torch.equal(out2, want)


@pytest.mark.parametrize("case", ["plain", "bucket0", "targets"])
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_add_timestamp_positional_embeddings_backward(dtype, D, case):
    P = _P()
    rows, Np = sum(LENGTHS), K
    # bucket0: 120 of the 130 rows of one sequence in timestamp bucket 0; targets: more than half of all rows are targets
    targets, recent = {"plain": ("zeros", None), "bucket0": ("none", (4, 120)), "targets": ("heavy", None)}[case]
    off, stamps, nt, p, t = _ts_case(targets, False, 0, "sqrt", Np, recent)
    if case == "bucket0":
        assert int((t[75:205] == 0).sum()) >= 120
    if case == "targets":
        assert int((p == 0).sum()) > rows // 2
    for table_dtype in _table_dtypes(dtype):
        seq = _rand(rows, D, dtype).requires_grad_(True)
        pos = _rand(Np, D, table_dtype).requires_grad_(True)
        ts = _rand(P.NUM_TIME_BUCKETS + 1, D, table_dtype).requires_grad_(True)
        d_out = _rand(rows, D, dtype, strided=(case == "plain"))
        grads = []
        for _ in range(2):
            out = P.add_timestamp_positional_embeddings(seq, off, pos, ts, stamps, 130, 0, _lengths(), nt, False, "sqrt")
            grads.append(torch.autograd.grad(out, (seq, pos, ts), d_out))
        (d_seq, d_pos, d_ts), (_, d_pos2, d_ts2) = grads
        assert d_seq.data_ptr() == d_out.data_ptr()
        assert d_pos.dtype == table_dtype and d_pos.shape == pos.shape and d_ts.shape == ts.shape
        assert torch.equal(d_pos, d_pos2) and torch.equal(d_ts, d_ts2)   # bitwise reproducible
        _assert_table_grad(d_pos, d_out, p, Np, f"d_pos {case} {dtype} {table_dtype} D={D}")
        _assert_table_grad(d_ts, d_out, t, ts.size(0), f"d_ts {case} {dtype} {table_dtype} D={D}")


# ---- paths the six-sequence shapes do not reach ----
def test_backward_of_rows_wider_than_one_wave():
    """D = 520: 65 pieces of 8 elements per row, so every reducing wave pair covers a row in two column slabs, the second with
    one active lane"""
    P = _P()
    D, rows, Np = 520, sum(LENGTHS), K
    off, high = _offsets(), _high("mixed")
    jag = _rand(rows, D, torch.bfloat16).requires_grad_(True)
    dense = _rand(K, D, torch.float32).requires_grad_(True)
    d_out = _rand(rows, D, torch.bfloat16)
    out = P.add_position_embeddings(jag, off, high, 130, dense, 1.0)
    (d_dense,) = torch.autograd.grad(out, dense, d_out)
    _assert_table_grad(d_dense, d_out, T.position_index(off, high, K), K, "d_dense D=520")
    off, stamps, nt, p, t = _ts_case("mixed", False, 0, "sqrt", Np)
    pos, ts = _rand(Np, D, torch.float32).requires_grad_(True), _rand(2049, D, torch.float32).requires_grad_(True)
    out = P.add_timestamp_positional_embeddings(jag, off, pos, ts, stamps, 130, 0, _lengths(), nt, False, "sqrt")
    assert torch.equal(out, jag + (pos[p.to(DEV)] + ts[t.to(DEV)]).to(torch.bfloat16))
    d_pos, d_ts = torch.autograd.grad(out, (pos, ts), d_out)
    _assert_table_grad(d_pos, d_out, p, Np, "d_pos D=520")
    _assert_table_grad(d_ts, d_out, t, 2049, "d_ts D=520")


def test_index_rows_sum_past_the_chunk_threshold():
    """from 2^18 list entries on the sorted list is cut into chunks of 64 entries instead of 32: one more than that many rows,
    three quarters of them on one key, the last chunk partial"""
    import mi355_native as N

    count, D, keys_n = (1 << 18) + 77, 8, K
    g = torch.Generator().manual_seed(4)
    inds = torch.randint(0, keys_n, (count,), generator=g, dtype=torch.int32)
    inds[torch.rand(count, generator=g) < 0.75] = 5
    d_out = _rand(count, D, torch.bfloat16)
    keys, rows_of = torch.sort(inds.to(DEV), stable=True)
    lib = N.lib()
    nbytes = lib.mi355_hstu_index_rows_sum_workspace_bytes(count, keys_n, D)
    assert nbytes == (4097 + 1 + keys_n) * D * 4   # 4098 chunks of 64 entries
    got = []
    for _ in range(2):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        d_table = torch.empty(keys_n, D, dtype=torch.float32, device=DEV)
        N.check(lib.mi355_hstu_index_rows_sum(N.ptr(d_out), D, count, D, N.dt(d_out), N.ptr(keys), N.ptr(rows_of), count,
                                              N.ptr(d_table), D, keys_n, N.dt(d_table), N.ptr(ws), nbytes, N.stream()))
        got.append(d_table)
    assert torch.equal(got[0], got[1])
    _assert_table_grad(got[0], d_out, inds.long(), keys_n, "d_table past the chunk threshold")


# ---- the module ----
def _encoder(use_time, is_inference, D=72):
    P = _P()
    torch.manual_seed(5)
    return P.HSTUPositionalEncoder(num_position_buckets=K, num_time_buckets=2048, embedding_dim=D,
                                   training_dtype=torch.bfloat16, is_inference=is_inference, use_time_encoding=use_time,
                                   static_max_seq_len=256).to(DEV)


def test_encoder_time_encoding_branch():
    enc, D = _encoder(True, False), 72
    off, stamps, nt, p, t = _ts_case("mixed", False, 0, "sqrt", K)
    seq = _rand(sum(LENGTHS), D, torch.bfloat16)
    out = enc(130, _lengths(), off, seq, nt, stamps)
    pos, ts = enc._position_embeddings_weight, enc._timestamp_embeddings_weight
    want = seq * D ** 0.5 + (pos[p.to(DEV)] + ts[t.to(DEV)]).to(torch.bfloat16)
    assert torch.equal(out, want)
    out.float().sum().backward()
    assert pos.grad is not None and ts.grad is not None and pos.grad.dtype == torch.float32


@pytest.mark.parametrize("incremental", [False, True])
def test_encoder_position_branches(incremental):
    D = 72
    enc = _encoder(False, incremental, D)
    off = _offsets()
    nt = torch.tensor(TARGETS["mixed"], dtype=torch.int64, device=DEV)
    start = torch.tensor(IND_OFFSETS, dtype=torch.int64, device=DEV) if incremental else None
    seq = _rand(sum(LENGTHS), D, torch.bfloat16)
    with torch.no_grad():
        out = enc(130, _lengths(), off, seq, nt, None, start)
    # the twin composed the same way: high = min(length (+ start) - targets, K - 1), rows shifted by start
    high = (_lengths() + (start if incremental else 0) - nt).clamp(max=K - 1)
    ref, mag = T.add_position_embeddings(seq, off, high, enc._position_embeddings_weight, D ** 0.5, start)
    err = (out.cpu().double() - ref).abs()
    assert bool((err <= T.unit_roundoff(torch.bfloat16) * ref.abs() + 2.0 ** -22 * mag).all())


def test_encoder_inference_branch_in_a_graph():
    D = 72
    enc = _encoder(False, True, D)
    off, lengths = _offsets(), _lengths()
    nt = torch.tensor(TARGETS["mixed"], dtype=torch.int64, device=DEV)
    start = torch.tensor(IND_OFFSETS, dtype=torch.int64, device=DEV)
    seq = _rand(sum(LENGTHS), D, torch.bfloat16)
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            enc(130, lengths, off, seq, nt, None, start)   # (loads the library, warms the allocator)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = enc(130, lengths, off, seq, nt, None, start)
        for step in range(2):
            seq.copy_(_rand(sum(LENGTHS), D, torch.bfloat16))
            start.copy_(torch.tensor(IND_OFFSETS, device=DEV).roll(step + 1))
            graph.replay()
            assert torch.equal(out, enc(130, lengths, off, seq, nt, None, start)), f"replay {step}"


# ---- split_2D_jagged ----
def _split_case(dtype, D, kind):
    la = torch.tensor([3, 0, 70, 5, 1, 9])
    lb = torch.tensor([2, 4, 0, 66, 1, 7])
    dense = 5
    if kind == "dense_a":
        la = torch.full_like(la, dense)
    if kind == "dense_b":
        lb = torch.full_like(lb, dense)
    oa = torch.cat([torch.zeros(1, dtype=torch.int64), la.cumsum(0)]).to(DEV)
    ob = torch.cat([torch.zeros(1, dtype=torch.int64), lb.cumsum(0)]).to(DEV)
    values = _rand(int(la.sum() + lb.sum()), D, dtype).requires_grad_(True)
    return values, oa, ob, dense


@pytest.mark.parametrize("kind", ["jagged", "dense_a", "dense_b"])
@pytest.mark.parametrize("D", [8, 72])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_split_2D_jagged(dtype, D, kind):
    import hstu_cuda_ops as H

    values, oa, ob, dense = _split_case(dtype, D, kind)
    ia, ib = T.split_rows(oa, ob)
    a, b = H.split_2D_jagged(values, 200, offsets_a=None if kind == "dense_a" else oa,
                             offsets_b=None if kind == "dense_b" else ob, dense_size=dense if kind != "jagged" else 0)
    want_a, want_b = values.detach()[ia.to(DEV)], values.detach()[ib.to(DEV)]
    if kind == "dense_a":
        assert a.shape == (6, dense, D)
    if kind == "dense_b":
        assert b.shape == (6, dense, D)
    assert torch.equal(a.reshape(-1, D), want_a) and torch.equal(b.reshape(-1, D), want_b)
    # the gradient is the concat of the two incoming gradients, sample by sample
    ga, gb = torch.randn_like(a), torch.randn_like(b)
    (g,) = torch.autograd.grad((a, b), values, (ga, gb))
    want = torch.cat([torch.cat([ga.reshape(-1, D)[oa[i]:oa[i + 1]], gb.reshape(-1, D)[ob[i]:ob[i + 1]]])
                      for i in range(6)])
    assert torch.equal(g, want)
    if kind == "jagged":   # the row counts handed in spare the host read and change nothing
        a2, b2 = H.triton_split_2D_jagged(values, 200, offsets_a=oa, offsets_b=ob, seq_len_a=oa[-1].cpu(),
                                          seq_len_b=int(ob[-1]))
        assert torch.equal(a2, a) and torch.equal(b2, b)
        with pytest.raises(NotImplementedError, match="n_prefix_to_right"):
            H.split_2D_jagged(values, 200, offsets_a=oa, offsets_b=ob, n_prefix_to_right=1)
