"""GPU checks of the KV cache GPU tier: the page mover of csrc/kvcache_ops.hip (both directions, every kind of table, the bounds
guard, offsets past 2^32 elements), the append-metadata kernel, and DeviceKVCache end to end -- offload, eviction, onboard and
append of one user's history, the metadata of `allocate` feeding append_kvcache and the paged attention as it stands, and a
graph capture of `offload_pages`.  16-bit payloads are random BIT patterns (NaNs included) compared as int16."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
H = 2


def _bits(shape, dtype):
    return torch.randint(-32768, 32768, tuple(shape), dtype=torch.int16, device=DEV).view(dtype)


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def _ids(values):
    return torch.tensor(values, dtype=torch.int32, device=DEV)


def _kv(L, P, ps, D, dtype, chunk=8):
    from recsys_kvcache_manager import DeviceKVCache

    kv = DeviceKVCache(L, H, D, ps, chunk, P, P, 4, 64, dtype, torch.cuda.current_device())
    kv.gpu_kvcache_tensor.copy_(_bits(kv.gpu_kvcache_tensor.shape, dtype))
    return kv


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D", [32, 64])
@pytest.mark.parametrize("ps", [4, 32])
@pytest.mark.parametrize("L", [1, 3])
def test_mover_gathers_and_scatters_every_page_list(L, ps, D, dtype):
    P = 12
    kv = _kv(L, P, ps, D, dtype)
    cache = kv.gpu_kvcache_tensor
    shape = tuple(cache.shape[2:])
    rng = np.random.default_rng(L * 1000 + ps * 10 + D)
    lists = {"one": [7], "five": rng.permutation(P)[:5].tolist(), "all reversed": list(range(P))[::-1]}
    # n = 0: no launch, an empty staging tensor, nothing written
    before = cache.clone()
    assert kv.offload_pages(_ids([])).shape == (L, 0) + shape
    kv.onboard_pages(torch.empty((L, 0) + shape, dtype=dtype, device=DEV), _ids([]))
    assert _same(cache, before)
    for name, ids in lists.items():
        staging = kv.offload_pages(_ids(ids))
        assert staging.shape == (L, len(ids)) + shape, name
        assert _same(staging, cache[:, ids]), name
        # a CPU list as acquire_offload_pages returns it is uploaded
        assert _same(kv.offload_pages(torch.tensor(ids, dtype=torch.int32)), staging), name
        # scatter into a poisoned cache changes exactly the listed pages
        poison = _bits(cache.shape, dtype)
        want = poison.clone()
        want[:, ids] = staging
        cache.copy_(poison)
        kv.onboard_pages(staging, _ids(ids))
        assert _same(cache, want), name
        cache.copy_(before)
    # a repeated id in a gather
    rep = [3, 9, 3, 3, 0]
    assert _same(kv.offload_pages(_ids(rep)), cache[:, rep])
    # gather, then scatter to other ids: the pages travel
    src, dst = lists["five"], [(p + 5) % P for p in lists["five"]][::-1]
    staging = kv.offload_pages(_ids(src))
    want = cache.clone()
    want[:, dst] = cache[:, src]
    kv.onboard_pages(staging, _ids(dst))
    assert _same(cache, want)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("ps,D", [(4, 32), (32, 64), (4, 64)])
def test_mover_on_layer_views_padded_tables_and_layer_ranges(ps, D, dtype):
    import paged_kvcache_ops

    L, P = 3, 12
    kv = _kv(L, P, ps, D, dtype)
    cache = kv.gpu_kvcache_tensor
    shape = tuple(cache.shape[2:])
    elems = 2 * ps * H * D
    ids = [5, 0, 11, 2, 8]
    dev_ids = _ids(ids + [1, 1])     # (num_pages says how many of them count)
    # per-layer unbind tables through gather_kvcache / scatter_kvcache, the reference's single-layer op
    for l, table in enumerate(kv.get_cache_tables()):
        buf = _bits((6,) + shape, dtype)
        tail = buf[5].clone()
        paged_kvcache_ops.gather_kvcache(buf, table, dev_ids, 5, 0, 304)
        assert _same(buf[:5], cache[l, ids]) and _same(buf[5], tail)
        poison = _bits(table.shape, dtype)
        want = poison.clone()
        want[ids] = buf[:5]
        other = cache.clone()
        table.copy_(poison)
        other[l] = poison
        paged_kvcache_ops.scatter_kvcache(buf, table, dev_ids, 5, 0, 304)
        other[l] = want
        assert _same(cache, other)      # the other layers are untouched
    # kv_layout 1 (HND) is the same move: a page is one contiguous block either way
    hnd = cache[0].view(P, 2, H, ps, D)
    buf = torch.empty((5, 2, H, ps, D), dtype=dtype, device=DEV)
    paged_kvcache_ops.gather_kvcache(buf, hnd, dev_ids, 5, 1, 304)
    assert _same(buf, hnd[ids])
    # a table whose pages are 8 elements apart from each other, gathered into a padded staging buffer as well
    padded = _bits((L, P, elems + 8), dtype)
    table = padded.as_strided((L, P) + shape, (P * (elems + 8), elems + 8, ps * H * D, H * D, D, 1))
    stage_store = _bits((L, 5, elems + 8), dtype)
    stage_before = stage_store.clone()
    stage = stage_store.as_strided((L, 5) + shape, (5 * (elems + 8), elems + 8, ps * H * D, H * D, D, 1))
    from recsys_kvcache_manager import page_ops
    page_ops.move_pages(page_ops.GATHER, table, stage, dev_ids, 5)
    assert _same(stage_store[..., :elems], padded[:, ids, :elems])
    assert _same(stage_store[..., elems:], stage_before[..., elems:])          # the padding is not written
    padded_before = padded.clone()
    page_ops.move_pages(page_ops.SCATTER, table, stage, _ids([(p + 1) % P for p in ids]), 5)
    want = padded_before.clone()
    want[:, [(p + 1) % P for p in ids], :elems] = padded_before[:, ids, :elems]
    assert _same(padded, want)
    # one block walks every run with the grid stride, under either cache hint
    for nt in (0, 1):
        got = _bits((L, 5) + shape, dtype)
        page_ops.move_pages(page_ops.GATHER, cache, got, dev_ids, 5, grid_cap=1, nontemporal=nt)
        assert _same(got, cache[:, ids]), nt
        before = cache.clone()
        page_ops.move_pages(page_ops.SCATTER, cache, got, _ids(ids[::-1]), 5, grid_cap=1, nontemporal=nt)
        want = before.clone()
        want[:, ids[::-1]] = got
        assert _same(cache, want), nt
    # a range of layers
    staging = kv.offload_pages(_ids(ids), layers=(1, 3))
    assert staging.shape == (2, 5) + shape and _same(staging, cache[1:3, ids])
    before = cache.clone()
    kv.onboard_pages(staging, _ids(ids[::-1]), layers=range(0, 2))
    want = before.clone()
    want[0:2, ids[::-1]] = staging
    assert _same(cache, want)
    # a page interior that is not contiguous is refused by name
    with pytest.raises(ValueError, match="paged_kv_cache: the inside of a page must be contiguous"):
        paged_kvcache_ops.gather_kvcache(buf.view(5, 2, ps, H, D), cache[0].transpose(2, 3).contiguous().transpose(2, 3),
                                         dev_ids, 5, 0, 304)
    with pytest.raises(ValueError, match="gather_kv_gpu_buffer: the inside of a page must be contiguous"):
        paged_kvcache_ops.gather_kvcache(torch.empty((5, 2, ps, H, 2 * D), dtype=dtype, device=DEV)[..., :D], cache[0],
                                         dev_ids, 5, 0, 304)


@pytest.mark.parametrize("L", [1, 3])
def test_ids_outside_the_table_are_skipped(L):
    """The cache under test is the middle P pages of a larger allocation whose first and last page are poison: ids -1 and P
    point at memory this process owns, so the check needs no out-of-allocation access even if the guard were missing."""
    from recsys_kvcache_manager import page_ops

    P, ps, D, dtype = 12, 4, 32, torch.bfloat16
    big = _bits((L, P + 2, 2, ps, H, D), dtype)
    cache = big[:, 1:P + 1]
    ids = [4, -1, 0, P, P - 1]
    staging = _bits((L, len(ids), 2, ps, H, D), dtype)
    poison = staging.clone()
    page_ops.move_pages(page_ops.GATHER, cache, staging, _ids(ids), len(ids))
    for j, p in enumerate(ids):
        assert _same(staging[:, j], cache[:, p] if 0 <= p < P else poison[:, j]), (j, p)
    before = big.clone()
    fresh = _bits(staging.shape, dtype)
    page_ops.move_pages(page_ops.SCATTER, cache, fresh, _ids(ids), len(ids))
    want = before.clone()
    for j, p in enumerate(ids):
        if 0 <= p < P:
            want[:, 1 + p] = fresh[:, j]
    assert _same(big[:, 0], before[:, 0]) and _same(big[:, P + 1], before[:, P + 1])     # the guard pages
    assert _same(big, want)


def test_offsets_past_two_to_the_32_elements():
    """A cache of 5 x 26215 pages of 32768 elements is 98304 elements (3 pages) over 2^32: the last three pages of the top layer
    sit past the line.  A 32-bit page_id * stride_page or layer * stride_layer would land 2^32 elements lower."""
    from recsys_kvcache_manager import page_ops

    L, P, ps, Hh, D, dtype = 5, 26215, 32, 4, 128, torch.bfloat16
    elems = 2 * ps * Hh * D
    total = L * P * elems
    assert 0 < total - 2 ** 32 <= 3 * elems
    free, _ = torch.cuda.mem_get_info()
    if free < 4 * total * 2:
        reason = f"needs {4 * total * 2 / 2 ** 30:.0f} GiB free for an {total * 2 / 2 ** 30:.1f} GiB cache, {free / 2 ** 30:.0f} GiB are"
        print("SKIPPED:", reason)
        pytest.skip(reason)
    cache = torch.empty((L, P, 2, ps, Hh, D), dtype=dtype, device=DEV)
    ids = [P - 4, P - 3, P - 2, P - 1, 0]
    src = _bits((L, len(ids), 2, ps, Hh, D), dtype)
    for l in range(L):
        for j, p in enumerate(ids):
            cache[l, p].copy_(src[l, j])
    staging = _bits(src.shape, dtype)
    page_ops.move_pages(page_ops.GATHER, cache, staging, _ids(ids), len(ids))
    assert _same(staging, src)
    fresh = _bits(src.shape, dtype)
    page_ops.move_pages(page_ops.SCATTER, cache, fresh, _ids(ids), len(ids))
    for l in range(L):
        for j, p in enumerate(ids):
            assert _same(cache[l, p], fresh[l, j]), (l, p)
    del cache
    torch.cuda.empty_cache()


@pytest.mark.parametrize("new,total", [([0, 1, 300, 0, 7], [5, 1, 300, 9, 40]), ([4], [10]), ([0, 0, 3], [2, 0, 3])])
def test_append_metadata_kernel_matches_the_formula(new, total):
    from recsys_kvcache_manager import page_ops

    off = np.concatenate([[0], np.cumsum(new)]).astype(np.int32)
    nnz = int(off[-1])
    want_b = np.repeat(np.arange(len(new)), new)
    want_p = np.concatenate([total[b] - new[b] + np.arange(new[b]) for b in range(len(new))])
    out = torch.full((2 * nnz + 2,), -7, dtype=torch.int32, device=DEV)
    page_ops.batch_positions(torch.from_numpy(off).to(DEV), _ids(total), nnz, out[:nnz], out[nnz:2 * nnz])
    got = out.cpu().numpy()
    np.testing.assert_array_equal(got[:nnz], want_b)
    np.testing.assert_array_equal(got[nnz:2 * nnz], want_p)
    assert got[2 * nnz:].tolist() == [-7, -7]


def test_offload_evict_onboard_round_trip_of_one_user():
    """Scenario B of tests/test_kvcache_allocator_cpu.py with data: what user 20 gets back after its pages were offloaded, freed
    and overwritten by user 22 is what it put, bit for bit, on every layer."""
    from recsys_kvcache_manager import KVLookupResult

    L, D, ps, dtype = 2, 64, 4, torch.bfloat16
    kv = _kv(L, 8, ps, D, dtype)
    u20, u22 = torch.tensor([20]), torch.tensor([22])
    rows = [(_bits((15, H, D), dtype), _bits((15, H, D), dtype)) for _ in range(L)]
    meta = kv.allocate(u20, torch.tensor([13]), kv.lookup(u20))
    assert meta.kv_indices.tolist() == [0, 1, 2, 3] and meta.new_history_nnz == 13
    assert meta.position.tolist() == list(range(13)) and meta.batch_indices.tolist() == [0] * 13
    for l in range(L):
        kv.put(rows[l][0][:13], rows[l][1][:13], l, meta)
    users, starts, page_lists = kv.acquire_offload_pages(u20, torch.tensor([0], dtype=torch.int32))
    assert users.tolist() == [20] and starts.tolist() == [0] and page_lists[0].tolist() == [0, 1, 2]
    staging = kv.offload_pages(page_lists[0])
    kv.release_offload_pages(users, starts, torch.tensor([12], dtype=torch.int32), True)
    # user 22 fills the cache: pages 0 and 1 of user 20 are overwritten
    meta22 = kv.allocate(u22, torch.tensor([24]), kv.lookup(u22))
    assert meta22.kv_indices.tolist() == [4, 5, 6, 7, 0, 1]
    for l in range(L):
        kv.put(_bits((24, H, D), dtype), _bits((24, H, D), dtype), l, meta22)
    look = kv.lookup(u20)
    assert look.gpu_cached_start_indices.tolist() == [12] and look.gpu_cached_lengths.tolist() == [1]
    look.host_cached_lengths = torch.tensor([12], dtype=torch.int32)
    meta = kv.allocate(u20, torch.tensor([15]), look)
    assert meta.kv_indices.tolist() == [2, 4, 5, 3] and meta.kv_last_page_len.tolist() == [3]
    assert meta.new_history_offsets.tolist() == [0, 2] and meta.position.tolist() == [13, 14] and meta.max_seqlen == 15
    kv.onboard_pages(staging, meta.kv_indices[:3])
    for l in range(L):
        kv.put(rows[l][0][13:], rows[l][1][13:], l, meta)
        k, v = kv.get(meta.kv_indices, meta.kv_last_page_len[0], l)
        assert k.shape == (15, H, D) and _same(k, rows[l][0]) and _same(v, rows[l][1]), l
    assert kv.lookup(torch.tensor([20, 22])).gpu_cached_lengths.tolist() == [15, 0]


def test_allocate_metadata_feeds_append_and_paged_attention():
    """Scenario A, steps 1-3: the tensors `allocate` returns go to append_kvcache and to the paged attention as they are; the
    output equals the cache-less delta-q call on the same keys bit for bit (as tests/test_hstu_gpu.py asserts for hand-built
    page arrays)."""
    from hstu.hstu_attn_interface import append_kvcache, hstu_attn_varlen_func

    D, ps, dtype = 64, 4, torch.bfloat16
    kv = _kv(1, 6, ps, D, dtype)
    history = {}
    alpha, scaling = 1.0 / D ** 0.5, 50.0
    expected_pages = [[0, 1, 2, 3, 4], [5, 0], [2, 3, 4]]
    for step, (users, totals, cands) in enumerate([([10, 11], [6, 9], [2, 1]), ([12], [8], [3]), ([11], [12], [2])]):
        uids = torch.tensor(users)
        look = kv.lookup(uids)
        meta = kv.allocate(uids, torch.tensor(totals), look)
        assert meta.kv_indices.tolist() == expected_pages[step]
        new = [t - c for t, c in zip(totals, look.gpu_cached_lengths.tolist())]
        num_cand = torch.tensor(cands, dtype=torch.int32, device=DEV)
        cand_off = torch.cat([num_cand.new_zeros(1), num_cand.cumsum(0).int()])
        rows = sum(new) + sum(cands)
        q, k, v = (torch.empty(rows, H, D, device=DEV).uniform_(-1, 1).to(dtype) for _ in range(3))
        append_kvcache(k, v, meta.batch_indices, meta.position, cand_off, meta.new_history_nnz_cuda, 0, kv.get_cache_tables(0),
                       meta.kv_indices, meta.kv_indptr, meta.kv_last_page_len, 0)
        cuq, cuk = meta.new_history_offsets + cand_off, meta.total_history_offsets + cand_off
        out_paged = hstu_attn_varlen_func(q, k, v, cuq, cuk, None, None, max(n + c for n, c in zip(new, cands)),
                                          meta.max_seqlen + max(cands), scaling, None, num_cand, window_size=(-1, 0), alpha=alpha,
                                          kv_cache=kv.get_cache_tables(0), page_offsets=meta.kv_indptr, page_ids=meta.kv_indices,
                                          last_page_lens=meta.kv_last_page_len)
        # the same keys without a cache: each user's earlier history in front of this request's rows
        kf, vf, row = [], [], 0
        for u, n, c in zip(users, new, cands):
            old_k, old_v = history.get(u, (k[:0], v[:0]))
            kf += [old_k, k[row:row + n + c]]
            vf += [old_v, v[row:row + n + c]]
            history[u] = (torch.cat([old_k, k[row:row + n]]), torch.cat([old_v, v[row:row + n]]))
            row += n + c
        out_dense = hstu_attn_varlen_func(q, torch.cat(kf), torch.cat(vf), cuq, cuk, None, None,
                                          max(n + c for n, c in zip(new, cands)), meta.max_seqlen + max(cands), scaling, None,
                                          num_cand, window_size=(-1, 0), alpha=alpha)
        assert out_paged.abs().max() > 0 and torch.equal(out_paged, out_dense), step
    assert [history[u][0].shape[0] for u in (10, 11, 12)] == [6, 12, 8]


def test_offload_pages_replays_from_a_graph():
    L, P, ps, D, dtype = 2, 12, 4, 32, torch.bfloat16
    kv = _kv(L, P, ps, D, dtype)
    ids = _ids([9, 2, 5])
    out = torch.zeros((L, 3) + tuple(kv.gpu_kvcache_tensor.shape[2:]), dtype=dtype, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        kv.offload_pages(ids, out=out)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert kv.offload_pages(ids, out=out) is out
    kv.gpu_kvcache_tensor.copy_(_bits(kv.gpu_kvcache_tensor.shape, dtype))
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert _same(out, kv.gpu_kvcache_tensor[:, [9, 2, 5]])
    # the ids are read at replay time too
    ids.copy_(_ids([0, 11, 11]))
    graph.replay()
    torch.cuda.synchronize()
    assert _same(out, kv.gpu_kvcache_tensor[:, [0, 11, 11]])
