"""GPU checks of `hstu_cuda_ops` (csrc/jagged_ops.hip behind the C ABI).  Every comparison is bit-exact: the kernels copy rows.
The oracle is a handful of torch statements: per sample, torch.cat of the tensors' slices."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
DIMS = (1, 3, 4, 8, 136, 1032)   # bf16: 2-, 2-, 8-, 16-byte pieces, a 16-byte multiple that is no power of two, a row > 1 KiB
LONG = 300                       # rows of the one long sample: more than the 64 rows a wave takes at most


def _H():
    import hstu_cuda_ops as H

    return H


def _lengths(n, B, seed):
    """[n, B] lengths in 0..9; tensor 1 is empty in every sample, sample 1 (where there is one) in every tensor, and one sample
    of tensor 0 holds LONG rows next to empty ones"""
    L = np.random.default_rng(seed).integers(0, 10, size=(n, B))
    L[1, :] = 0
    if B >= 3:
        L[:, 1] = 0
        L[:, 3] = 0
        L[0, 2] = LONG
    else:
        L[0, 0] = LONG
    return L


def _offsets(L):
    return [torch.tensor(np.concatenate([[0], np.cumsum(row)]), dtype=torch.int64, device=DEV) for row in L]


def _values(L, D, dtype, requires_grad=False):
    return [torch.randn(int(row.sum()), D, device=DEV).to(dtype).requires_grad_(requires_grad) for row in L]


def _oracle_concat(values, L):
    n, B = L.shape
    off = np.concatenate([np.zeros((n, 1), dtype=np.int64), np.cumsum(L, 1)], 1)
    return torch.cat([values[t][off[t, b]:off[t, b + 1]] for b in range(B) for t in range(n)], 0)


def _oracle_split(g, L):
    """per tensor, the slices of the merged gradient that are its rows"""
    n, B = L.shape
    out = [[] for _ in range(n)]
    pos = 0
    for b in range(B):
        for t in range(n):
            out[t].append(g[pos:pos + L[t, b]])
            pos += L[t, b]
    return [torch.cat(p, 0) for p in out]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("n", [2, 3, 128])
def test_concat_forward_backward_match_the_oracle(n, B, dtype):
    H = _H()
    L = _lengths(n, B, seed=n * 10 + B)
    offsets = _offsets(L)
    for D in DIMS:
        values = _values(L, D, dtype, requires_grad=True)
        out, lengths = H.jagged_2D_tensor_concat(values, offsets, [int(r.max()) for r in L])
        assert out.shape == (int(L.sum()), D) and out.dtype == dtype
        assert torch.equal(out, _oracle_concat([v.detach() for v in values], L)), f"forward D={D}"
        assert lengths.dtype == torch.int64 and lengths.tolist() == L.sum(0).tolist() and not lengths.requires_grad
        g = torch.randn(out.shape, device=DEV).to(dtype)
        out.backward(g)
        for t, want in enumerate(_oracle_split(g, L)):
            assert values[t].grad.shape == values[t].shape
            assert torch.equal(values[t].grad, want), f"backward D={D} tensor {t}"


def test_base_pointers_aligned_to_8_bytes_only():
    """D = 8 bf16 rows are 16 bytes, but a tensor that starts 4 elements into its storage is 8-byte aligned: forward with such
    a values tensor, backward with such a merged gradient"""
    H = _H()
    L = _lengths(3, 5, seed=7)
    offsets = _offsets(L)
    D = 8
    values = []
    for row in L:
        rows = int(row.sum())
        v = torch.randn(rows * D + 4, device=DEV).bfloat16()[4:].view(rows, D)
        assert rows == 0 or v.data_ptr() % 16 == 8
        values.append(v.requires_grad_(True))
    out, _ = H.jagged_2D_tensor_concat(values, offsets, [LONG] * 3)
    assert torch.equal(out, _oracle_concat([v.detach() for v in values], L))
    g = torch.randn(out.numel() + 4, device=DEV).bfloat16()[4:].view(out.shape)
    assert g.data_ptr() % 16 == 8 and g.is_contiguous()
    out.backward(g)
    for t, want in enumerate(_oracle_split(g, L)):
        assert torch.equal(values[t].grad, want)


def test_row_strided_input():
    H = _H()
    L = _lengths(2, 5, seed=8)
    L[1, :] = [2, 0, 5, 0, 1]
    offsets = _offsets(L)
    D = 8
    wide = [torch.randn(int(row.sum()), D + 5, device=DEV).bfloat16() for row in L]
    values = [w[:, :D] for w in wide]
    assert not values[0].is_contiguous() and values[0].stride(-1) == 1
    out, _ = H.jagged_2D_tensor_concat(values, offsets, [LONG, 5])
    assert torch.equal(out, _oracle_concat(values, L))


def test_all_empty_returns_zero_rows_and_zero_row_gradients():
    H = _H()
    offsets = [torch.zeros(4, dtype=torch.int64, device=DEV) for _ in range(2)]
    values = [torch.zeros(0, 16, device=DEV, dtype=torch.bfloat16, requires_grad=True) for _ in range(2)]
    out, lengths = H.jagged_2D_tensor_concat(values, offsets, [0, 0])
    assert out.shape == (0, 16) and lengths.tolist() == [0, 0, 0]
    out.backward(torch.zeros_like(out))
    assert all(v.grad is not None and v.grad.shape == (0, 16) for v in values)


def test_single_tensor_passes_through():
    H = _H()
    L = np.array([[3, 0, 4]])
    v = _values(L, 8, torch.float32, requires_grad=True)[0]
    out, lengths = H.jagged_2D_tensor_concat([v], _offsets(L), [4])
    assert torch.equal(out, v) and lengths.tolist() == [3, 0, 4]
    g = torch.randn_like(out)
    out.backward(g)
    assert torch.equal(v.grad, g)


def test_130_tensors_are_grouped_128_plus_2():
    H = _H()
    n, B, D = 130, 2, 4
    L = np.random.default_rng(130).integers(0, 3, size=(n, B))
    L[128:, :] = [[2, 1], [1, 3]]   # the two tensors of the second group are not empty
    values = _values(L, D, torch.bfloat16, requires_grad=True)
    out, lengths = H.jagged_2D_tensor_concat(values, _offsets(L), [int(r.max()) for r in L])
    assert torch.equal(out, _oracle_concat([v.detach() for v in values], L))
    assert lengths.tolist() == L.sum(0).tolist()
    g = torch.randn(out.shape, device=DEV).bfloat16()
    out.backward(g)
    for t, want in enumerate(_oracle_split(g, L)):
        assert torch.equal(values[t].grad, want)


@pytest.mark.parametrize("seqlen_per_block", [8, 1])
def test_raw_ops_in_the_order_of_the_reference_wrapper(seqlen_per_block):
    H = _H()
    ops = torch.ops.hstu_cuda_ops
    n, B, D = 3, 5, 136
    L = _lengths(n, B, seed=9)
    L[0, 2] = 21
    max_seqlen = int(L.max())
    assert max_seqlen == 21
    offsets = _offsets(L)
    values = _values(L, D, torch.bfloat16)
    direct, _ = H.jagged_2D_tensor_concat(values, offsets, [max_seqlen] * n)

    nb = -(-max_seqlen // seqlen_per_block)
    total_blocks = B * n * nb
    workloads = torch.full((total_blocks,), -7, dtype=torch.int64, device=DEV)
    ops.compute_block_workloads(offsets, seqlen_per_block, max_seqlen, workloads)
    idx = np.arange(nb)[None, None, :] * seqlen_per_block
    closed = np.clip(np.minimum(L.T[:, :, None] - idx, seqlen_per_block), 0, None)   # [B, n, nb]
    assert np.array_equal(workloads.cpu().numpy(), closed.reshape(-1))
    workload_offset = torch.cat([workloads.new_zeros(1), torch.cumsum(workloads, 0)])

    merged_offsets = torch.stack(offsets).sum(0)
    kept = merged_offsets.clone()
    blocks, threads = min(2048, total_blocks), 256
    merged = torch.empty_like(direct)
    ops.concat_2D_jagged_tensors_forward(values, offsets, seqlen_per_block, max_seqlen, total_blocks, blocks, threads,
                                         workload_offset, merged, merged_offsets)
    assert torch.equal(merged, direct) and torch.equal(merged_offsets, kept)

    merged2 = torch.empty_like(direct)
    ops.concat_2D_jagged_tensors_fwd_exportable(values, offsets, seqlen_per_block, max_seqlen,
                                                torch.tensor([total_blocks], dtype=torch.int32),
                                                torch.tensor([blocks], dtype=torch.int32), threads, workload_offset, merged2,
                                                merged_offsets)
    assert torch.equal(merged2, direct)

    g = torch.randn(direct.shape, device=DEV).bfloat16()
    grads = [torch.empty_like(v) for v in values]
    ops.concat_2D_jagged_tensors_backward(g, torch.zeros(B, device=DEV), seqlen_per_block, max_seqlen, total_blocks, blocks,
                                          threads, workload_offset, grads, offsets, merged_offsets)
    for got, want in zip(grads, _oracle_split(g, L)):
        assert torch.equal(got, want)


def test_forward_and_backward_replay_from_a_graph():
    _H()
    ops = torch.ops.hstu_cuda_ops
    n, B, D = 3, 5, 136
    L = _lengths(n, B, seed=10)
    offsets = _offsets(L)
    values = _values(L, D, torch.bfloat16)
    merged_offsets = torch.stack(offsets).sum(0)
    merged = torch.empty(int(L.sum()), D, device=DEV, dtype=torch.bfloat16)
    g = torch.randn(merged.shape, device=DEV).bfloat16()
    grads = [torch.empty_like(v) for v in values]
    none = torch.zeros(1, dtype=torch.int64, device=DEV)

    def step():
        ops.concat_2D_jagged_tensors_forward(values, offsets, 8, LONG, 1, 1, 256, none, merged, merged_offsets)
        ops.concat_2D_jagged_tensors_backward(g, none, 8, LONG, 1, 1, 256, none, grads, offsets, merged_offsets)

    step()   # loads the library outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for v in values:
        v.copy_(torch.randn(v.shape, device=DEV).bfloat16())
    g.copy_(torch.randn(g.shape, device=DEV).bfloat16())
    merged.zero_()
    for gr in grads:
        gr.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(merged, _oracle_concat(values, L))
    for got, want in zip(grads, _oracle_split(g, L)):
        assert torch.equal(got, want)


# (h, e, C) per sample: history items, extra leading action, candidates
PRE_SAMPLES = ((0, 0, 2), (3, 0, 0), (2, 1, 1), (0, 1, 0))


def _preprocess_oracle(item, action, samples):
    rows, i0, a0 = [], 0, 0
    for h, e, C in samples:
        I, A = h + C, h + C + e
        for r in range(2 * h + e + C):
            if r < e:
                rows.append(action[a0])
                continue
            rp = r - e
            if rp < 2 * h:
                rows.append(item[i0 + rp // 2] if rp % 2 == 0 else action[a0 + rp // 2 + e])
            else:
                rows.append(item[i0 + h + rp - 2 * h])
        i0, a0 = i0 + I, a0 + A
    return torch.stack(rows)


@pytest.mark.parametrize("len_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("D", [4, 128])
def test_inference_preprocess(D, dtype, len_dtype):
    _H()
    il = [h + C for h, e, C in PRE_SAMPLES]
    al = [h + C + e for h, e, C in PRE_SAMPLES]
    nc = [C for h, e, C in PRE_SAMPLES]
    ol = [2 * h + e + C for h, e, C in PRE_SAMPLES]
    item = torch.randn(sum(il), D, device=DEV).to(dtype)
    action = torch.randn(sum(al), D, device=DEV).to(dtype)
    t = lambda x: torch.tensor(x, dtype=len_dtype, device=DEV)   # noqa: E731
    values, lengths, offsets, cand = torch.ops.hstu_cuda_ops.hstu_inference_preprocess(item, t(il), action, t(al), t(nc))
    assert values.dtype == dtype and torch.equal(values, _preprocess_oracle(item, action, PRE_SAMPLES))
    assert lengths.dtype == torch.int64 and lengths.tolist() == ol
    assert offsets.dtype == torch.int64 and offsets.tolist() == np.concatenate([[0], np.cumsum(ol)]).tolist()
    assert cand.dtype == torch.int32 and cand.tolist() == np.concatenate([[0], np.cumsum(nc)]).tolist()


@pytest.mark.parametrize("il,al,nc,word", [
    ([2, 3], [2, 3], [3, 0], "item history lengths"),        # C > I
    ([2, 3], [2, 2], [0, 0], "each action length"),          # A < I
    ([2, 3], [4, 3], [0, 0], "each action length"),          # A = I + 2
])
def test_inference_preprocess_rejects_invalid_lengths(il, al, nc, word):
    _H()
    item = torch.zeros(sum(il), 4, device=DEV)
    action = torch.zeros(sum(al), 4, device=DEV)
    t = lambda x: torch.tensor(x, dtype=torch.int64, device=DEV)   # noqa: E731
    with pytest.raises(RuntimeError, match=word):
        torch.ops.hstu_cuda_ops.hstu_inference_preprocess(item, t(il), action, t(al), t(nc))


def test_kjt_helpers_on_cuda_tensors():
    _H()
    ops = torch.ops.hstu_cuda_ops
    lengths = torch.tensor([2, 0, 1, 3, 1, 0], dtype=torch.int32, device=DEV)
    values = torch.arange(21.0, device=DEV).view(7, 3)
    for lens in (lengths, lengths.cpu()):   # lengths_1d may sit on either device
        out = ops.split_by_lengths(values, lens, 3)
        assert all(torch.equal(a, b) for a, b in zip(out, torch.split(values, [2, 4, 1], 0)))
    assert torch.equal(ops.lengths_reduce_dim1(lengths, 3), lengths.view(3, 2).sum(1))
    parts = ops.lengths_splits(lengths, 2)
    assert torch.equal(parts[0], lengths[:3]) and torch.equal(parts[1], lengths[3:])

    batch = 2
    jl = torch.tensor([1, 2, 0, 3, 2, 2, 1, 0], device=DEV)
    jo = torch.cat([jl.new_zeros(1), torch.cumsum(jl, 0)])
    feats = torch.arange(int(jl.sum()), device=DEV) * 10
    joc = jo.tolist()
    per_feature = [feats[joc[f * batch]:joc[(f + 1) * batch]] for f in range(4)]
    per_length = [jl[f * batch:(f + 1) * batch] for f in range(4)]
    out = ops.permute_and_split(feats, jl, jo, 2, 2, [2, 0, 3, 1])
    assert torch.equal(out[0], torch.cat([per_feature[2], per_feature[0]]))
    assert torch.equal(out[1], torch.cat([per_feature[3], per_feature[1]]))
    assert torch.equal(out[2], torch.cat([per_length[2], per_length[0]]))
    assert torch.equal(out[3], torch.cat([per_length[3], per_length[1]]))

    # sample 0: 5 cached tokens against 2 context rows: 3 spill, item loses 2 and action 1
    sl = torch.tensor([2, 1, 0, 4, 3, 2, 4, 3, 2], dtype=torch.int32, device=DEV)
    so = torch.cat([torch.zeros(1, dtype=torch.int64, device=DEV), torch.cumsum(sl.long(), 0)])
    sv = torch.arange(int(sl.sum()), device=DEV) + 100
    got_v, got_l = ops.strip_cached_tokens(sv, sl, so, torch.tensor([5, 0, 1], device=DEV), [0, 1, 2])
    assert got_l.dtype == torch.int32 and got_l.tolist() == [0, 1, 0, 2, 3, 1, 3, 3, 2]
    starts, strip = so.tolist(), [2, 0, 0, 2, 0, 1, 1, 0, 0]
    want = torch.cat([sv[starts[i] + strip[i]:starts[i + 1]] for i in range(9)])
    assert torch.equal(got_v, want)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        ops.split_by_lengths(values.cpu(), lengths, 3)   # a CUDA lengths tensor dispatches to the CUDA implementation
