"""CPU checks of the KV cache GPU tier's host side (recsys_kvcache_manager): the page allocator against two traces worked by
hand from the reference's gpu_kvcache_manager_impl.cpp (:86-389, :436-563), its refusal when only locked users are left, the
offload bookkeeping, invariants along a random trace, the names shared with the reference (tests/golden/
kvcache_signatures.json), KVLookupResult.merge and the layout of the metadata buffer."""
import dataclasses
import inspect
import json
import os
import random

import pytest
import torch

from recsys_kvcache_manager import (DeviceKVCache, GPUKVCacheManager, KVCacheMetadata, KVCacheOffloadMode, KVIndexMeta,
                                    KVLookupResult, PageAllocator, copy_kvcache_metadata, get_kvcache_metadata_buffer)

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "kvcache_signatures.json")


def _fields(words, B):
    """the six fields of the 5 B + 4 metadata words"""
    assert len(words) == 5 * B + 4
    return {"indptr": words[0:B + 1], "last": words[B + 1:2 * B + 1], "totals": words[2 * B + 1:3 * B + 1],
            "total_offsets": words[3 * B + 1:4 * B + 2], "nnz": words[4 * B + 2], "new_offsets": words[4 * B + 3:5 * B + 4]}


def _positions(words, B):
    """the append positions by the formula: token i of sequence b sits at total[b] - new[b] + i"""
    f = _fields(words, B)
    out = []
    for b in range(B):
        new = f["new_offsets"][b + 1] - f["new_offsets"][b]
        out += [f["totals"][b] - new + i for i in range(new)]
    return out


def test_scenario_a_growth_and_lru_eviction():
    a = PageAllocator(4, 8, 6)
    pages, words = a.allocate([10, 11], [6, 9], [0, 0])
    assert pages == [0, 1, 2, 3, 4]
    assert len(words) == 14
    assert words[0:3] == [0, 2, 5] and words[3:5] == [2, 1] and words[5:7] == [6, 9]
    assert words[7:10] == [0, 6, 15] and words[10] == 15 and words[11:14] == [0, 6, 15]
    # 2. one free page left: user 10, at the front of the LRU, goes; its pages follow page 5 in the queue
    pages, words = a.allocate([12], [8])
    assert pages == [5, 0]
    assert a.lookup([10, 11, 12]) == ([0, 0, 0], [0, 9, 8])
    # 3. user 11 grows inside its last page
    pages, words = a.allocate([11], [12])
    f = _fields(words, 1)
    assert pages == [2, 3, 4] and f["last"] == [4] and f["new_offsets"] == [0, 3]
    assert _positions(words, 1) == [9, 10, 11]
    # 4. and into a new one
    pages, words = a.allocate([11], [14])
    assert pages == [2, 3, 4, 1] and _fields(words, 1)["last"] == [2]
    # 5. user 12 is now the least recently allocated, not 11
    pages, words = a.allocate([13], [5])
    assert pages == [5, 0]
    assert a.lookup([11, 12, 13]) == ([0, 0, 0], [14, 0, 5])


def test_scenario_b_offloaded_pages_go_before_users_and_come_back_first():
    a = PageAllocator(4, 8, 8)
    pages, _ = a.allocate([20], [13])
    assert pages == [0, 1, 2, 3]
    assert a.acquire_offload_pages([20], [0], False) == ([20], [0], [[0, 1, 2]])
    a.release_offload_pages([20], [0], [12], [1])
    assert a.total_offloaded_pages == 3
    # 3. the three offloaded pages of user 20 are freed, the user stays with its last page
    pages, _ = a.allocate([22], [24])
    assert pages == [4, 5, 6, 7, 0, 1]
    assert a.lookup([20]) == ([12], [1])
    assert a.pages_of(20) == [3] and a.total_offloaded_pages == 0
    # 4. user 20 returns: user 22 goes, three pages for what the host holds come first, then the kept page
    pages, words = a.allocate([20], [15], [12])
    f = _fields(words, 1)
    assert pages == [2, 4, 5, 3]
    assert f["last"] == [3] and f["new_offsets"] == [0, 2] and f["indptr"] == [0, 4]
    assert _positions(words, 1) == [13, 14]
    assert a.lookup([20, 22]) == ([0, 0], [15, 0])


def test_shortage_with_only_locked_users_raises_and_changes_nothing():
    a = PageAllocator(4, 8, 4)
    a.allocate([1], [8])
    a.allocate([2], [8])
    assert a.acquire_offload_pages([1, 2], [0, 0], False) == ([1, 2], [0, 0], [[0, 1], [2, 3]])
    before = (a.lookup([1, 2, 3]), a.free_pages(), a.users(), a.pages_of(1), a.pages_of(2))
    with pytest.raises(RuntimeError, match=r"needs 1 pages.* 0 can be freed"):
        a.allocate([3], [4])
    assert (a.lookup([1, 2, 3]), a.free_pages(), a.users(), a.pages_of(1), a.pages_of(2)) == before
    # the locks come back: user 1, the least recently allocated, can go now
    a.release_offload_pages([1, 2], [0, 0], [0, 0], [0, 0])
    pages, _ = a.allocate([3], [4])
    assert pages == [0] and a.lookup([1, 2, 3]) == ([0, 0, 0], [0, 8, 4])


def test_shortage_in_the_middle_of_a_batch_changes_nothing():
    a = PageAllocator(4, 8, 4)
    a.allocate([1], [8])
    before = (a.lookup([1, 2, 3]), a.free_pages(), a.users())
    # user 2 alone would fit after evicting user 1; users 2 and 3 together need 5 of the 4 pages
    with pytest.raises(RuntimeError, match=r"needs 5 pages.* 4 can be freed"):
        a.allocate([2, 3], [8, 12])
    assert (a.lookup([1, 2, 3]), a.free_pages(), a.users()) == before
    with pytest.raises(ValueError, match="shorter"):
        a.allocate([1], [7])
    assert (a.lookup([1, 2, 3]), a.free_pages(), a.users()) == before
    pages, _ = a.allocate([2, 3], [8, 8])
    assert pages == [2, 3, 0, 1]


def test_evict_all_restores_the_page_order():
    a = PageAllocator(4, 8, 6)
    a.allocate([1, 2], [5, 9])
    a.allocate([3], [8])
    a.acquire_offload_pages([2], [0], False)
    assert a.free_pages() != list(range(6))
    a.evict_all()
    assert a.free_pages() == list(range(6)) and a.users() == [] and a.total_offloaded_pages == 0
    assert a.lookup([1, 2, 3]) == ([0, 0, 0], [0, 0, 0])
    pages, _ = a.allocate([4], [24])    # (a lock left behind would make this raise)
    assert pages == [0, 1, 2, 3, 4, 5]


def test_evict_returns_the_pages_in_list_order():
    a = PageAllocator(4, 8, 6)
    a.allocate([1, 2], [8, 8])
    a.evict(1)
    a.evict(7)    # unknown: nothing happens
    assert a.free_pages() == [4, 5, 0, 1] and a.users() == [2]


def test_revoke_onboard_pages_frees_the_leading_pages_and_moves_the_start():
    a = PageAllocator(4, 8, 8)
    pages, words = a.allocate([5], [10], [8])      # the GPU holds nothing of user 5, the host 8 tokens: two onboard pages
    assert pages == [0, 1, 2] and _fields(words, 1)["new_offsets"] == [0, 2]
    a.revoke_onboard_pages([5], [0], [8])
    assert a.pages_of(5) == [2] and a.lookup([5]) == ([8], [2])
    assert a.free_pages() == [3, 4, 5, 6, 7, 0, 1]
    # the next allocate makes room for the host part again, in front
    pages, words = a.allocate([5], [11], [8])
    assert pages == [3, 4, 2] and _fields(words, 1)["new_offsets"] == [0, 1] and a.lookup([5]) == ([0], [11])
    # revoking everything a user has evicts it
    b = PageAllocator(4, 8, 4)
    b.allocate([6], [8], [8])
    b.revoke_onboard_pages([6], [0], [8])
    assert b.users() == [] and b.free_pages() == [2, 3, 0, 1]


def test_check_for_offload_two_users():
    """users 30 (9 tokens, pages 0-2) and 31 (13 tokens, pages 3-6), one free page, chunk 8, page 4, nothing offloaded:
    30 has 2 whole pages to offload, 31 has 3.  The scan of the other users stops once offloaded + pending + free pages exceed
    the buffer pages (gpu_kvcache_manager_impl.cpp:391-434)."""
    def make(buffer_pages):
        a = PageAllocator(4, 8, 8, buffer_pages, max_batch_size=2, max_sequence_length=32)
        a.allocate([30, 31], [9, 13])
        return a

    a = make(8)
    assert a.check_for_offload([31]) == [31, 30]       # 0 + 3 + 1 <= 8: user 30 is looked at and has a chunk
    assert a.check_for_offload([]) == [30, 31]         # LRU order
    assert make(3).check_for_offload([31]) == [31]     # 0 + 3 + 1 > 3: the scan stops before user 30
    assert make(3).check_for_offload([]) == [30, 31]   # 0 + 0 + 1 <= 3 admits 30 (2 pages), 0 + 2 + 1 <= 3 admits 31
    assert make(2).check_for_offload([]) == [30]       # 0 + 2 + 1 > 2: the scan stops before user 31
    assert a.acquire_offload_pages([30], [0], False) == ([30], [0], [[0, 1]])
    a.release_offload_pages([30], [0], [8], [1])
    assert a.total_offloaded_pages == 2
    assert a.check_for_offload([]) == [31]             # user 30 has 1 token past the host's 8: less than a chunk
    # always_offload: every page from position 0, whatever the host holds
    assert a.acquire_offload_pages([30, 99], [], True) == ([30, 99], [0, 0], [[0, 1, 2], []])
    a.release_offload_pages([30, 99], [0, 0], [0, 0], [0, 0])
    # max_offload_pages = 1 * 2 = 2: user 31's 3 pages do not fit behind user 30's 2
    small = PageAllocator(4, 8, 8, 8, max_batch_size=1, max_sequence_length=8)
    small.allocate([30, 31], [9, 13])
    assert small.check_for_offload([]) == [30]


def _check_invariants(a: PageAllocator, P: int, ps: int):
    free = a.free_pages()
    listed = [p for u in a.users() for p in a.pages_of(u)]
    assert len(set(free)) == len(free) and len(set(listed)) == len(listed), "a page is held twice"
    assert not set(free) & set(listed), "a page is free and listed"
    assert sorted(free + listed) == list(range(P)), "pages were lost or invented"
    starts, lengths = a.lookup(a.users())
    for u, s, n in zip(a.users(), starts, lengths):
        assert n > 0 and s % ps == 0
        assert len(a.pages_of(u)) == -(-n // ps), (u, s, n, a.pages_of(u))


def test_invariants_along_a_random_trace():
    P, ps = 12, 4
    rng = random.Random(20240611)
    a = PageAllocator(ps, 8, P, 6, max_batch_size=4, max_sequence_length=24)
    length, host, next_uid, pool, locked = {}, {}, 100, list(range(8)), []
    refused = allocated = 0
    for step in range(300):
        # offloads: users are locked at the end of a step (below) and released one or two steps later
        if locked and rng.random() < 0.6:
            users, offs, lists = locked.pop(0)
            done = [int(rng.random() < 0.8) for _ in users]
            a.release_offload_pages(users, offs, [len(l) * ps for l in lists], done)
            for u, o, l, d in zip(users, offs, lists, done):
                if d:
                    host[u] = o + len(l) * ps
            _check_invariants(a, P, ps)
        batch = rng.sample(pool, rng.randint(1, 4))
        for i, u in enumerate(batch):      # a user that has grown to 12 tokens is replaced by a new one
            if length.get(u, 0) >= 12:
                pool[pool.index(u)] = batch[i] = next_uid
                next_uid += 1
        totals = [length.get(u, 0) + rng.randint(0 if length.get(u, 0) else 1, 5) for u in batch]
        starts, lens = a.lookup(batch)
        # what the host tier holds: nothing, or what an offload left there (sometimes lost again)
        hosts = [0 if rng.random() < 0.1 else host.get(u, 0) for u in batch]
        # (a GPU part that starts past a lost host part is dropped by allocate; the sequence then counts as uncached)
        before = (a.lookup(pool), a.free_pages(), a.users())
        try:
            pages, words = a.allocate(batch, totals, hosts)
        except RuntimeError:
            refused += 1
            assert (a.lookup(pool), a.free_pages(), a.users()) == before
            continue
        allocated += 1
        f = _fields(words, len(batch))
        assert f["indptr"][-1] == len(pages) == sum(-(-t // ps) for t in totals)
        assert a.lookup(batch) == ([0] * len(batch), totals)
        for b, u in enumerate(batch):
            assert pages[f["indptr"][b]:f["indptr"][b + 1]] == a.pages_of(u)
            cached = 0 if (lens[b] > 0 and hosts[b] < starts[b]) else max(hosts[b], starts[b] + lens[b])
            assert f["new_offsets"][b + 1] - f["new_offsets"][b] == totals[b] - cached
            length[u] = totals[b]
        _check_invariants(a, P, ps)
        if rng.random() < 0.4:
            asked = a.check_for_offload(batch[:2])
            if asked:
                locked.append(a.acquire_offload_pages(asked, [host.get(u, 0) for u in asked], False))
                for u, l in zip(locked[-1][0], locked[-1][2]):
                    assert set(l) <= set(a.pages_of(u))
    assert allocated >= 100 and refused >= 10, (allocated, refused)   # (the trace walks both ways out of allocate)


def _sig(fn):
    return [(p.name, p.default is not inspect.Parameter.empty) for p in inspect.signature(fn).parameters.values()]


def test_names_are_the_reference_s():
    import paged_kvcache_ops

    golden = json.load(open(GOLDEN))
    assert len(golden["DeviceKVCache"]) == 12
    for name, want in golden["DeviceKVCache"].items():
        assert _sig(getattr(DeviceKVCache, name)) == [(p, d is not None) for p, d in want], name
    assert golden["DeviceKVCache_aliases"] == ["GPUKVCacheManager"] and GPUKVCacheManager is DeviceKVCache
    for cls in (KVCacheMetadata, KVLookupResult, KVIndexMeta):
        assert [f.name for f in dataclasses.fields(cls)] == golden[cls.__name__], cls.__name__
    for name, want in golden["kvcache_metadata_functions"].items():
        fn = {"get_kvcache_metadata_buffer": get_kvcache_metadata_buffer, "copy_kvcache_metadata": copy_kvcache_metadata}[name]
        assert _sig(fn) == [(p, d is not None) for p, d in want], name
    assert [p for p, _ in _sig(paged_kvcache_ops.gather_kvcache)] == golden["gather_kvcache"]
    assert len(_sig(paged_kvcache_ops.scatter_kvcache)) == len(golden["gather_kvcache"])
    assert [m.value for m in KVCacheOffloadMode] == ["lazy", "eager"]


def _i32(*v):
    return torch.tensor(v, dtype=torch.int32)


def test_lookup_merge_takes_the_three_branches():
    uids = torch.tensor([1, 2, 3, 4])
    gpu = KVLookupResult(user_ids=uids, gpu_cached_start_indices=_i32(0, 0, 8, 4), gpu_cached_lengths=_i32(0, 7, 5, 3))
    host = KVLookupResult(user_ids=uids, host_cached_start_indices=_i32(0, 0, 0, 0), host_cached_lengths=_i32(6, 0, 8, 12),
                          extra={"slots": 3})
    for m in (KVLookupResult.merge(gpu, host), KVLookupResult.merge(host, gpu)):
        # host only; GPU only; both, GPU end past the host part; both, host part past the GPU end
        assert m.cached_start_indices.tolist() == [0, 0, 0, 0]
        assert m.cached_lengths.tolist() == [6, 7, 13, 12]
        assert m.gpu_cached_lengths is gpu.gpu_cached_lengths and m.host_cached_lengths is host.host_cached_lengths
        assert m.extra == {"slots": 3} and m.user_ids is uids
    # GPU only keeps the GPU start
    g = KVLookupResult(user_ids=uids[:1], gpu_cached_start_indices=_i32(4), gpu_cached_lengths=_i32(3))
    h = KVLookupResult(user_ids=uids[:1], host_cached_start_indices=_i32(0), host_cached_lengths=_i32(0))
    m = KVLookupResult.merge(g, h)
    assert m.cached_start_indices.tolist() == [4] and m.cached_lengths.tolist() == [3]
    # a gap between the host part and the GPU part, two results of one tier, other users
    h.host_cached_lengths = _i32(2)
    with pytest.raises(ValueError, match="gap"):
        KVLookupResult.merge(g, h)
    with pytest.raises(ValueError):
        KVLookupResult.merge(g, g)
    with pytest.raises(ValueError):
        KVLookupResult.merge(gpu, h)


def test_metadata_views_alias_one_buffer():
    B, nnz, pages = 2, 15, 5
    m = get_kvcache_metadata_buffer(B, nnz, pages, device="cpu")
    buf = m.metadata_gpu_buffer
    assert buf.numel() == 5 * B + 4 + 2 * nnz and buf.dtype == torch.int32 and m.page_ids_gpu_buffer.numel() == pages
    assert m.kv_indices is m.page_ids_gpu_buffer and m.new_history_nnz == nnz
    buf.copy_(torch.arange(buf.numel(), dtype=torch.int32))
    views = {"kv_indptr": (0, 3), "kv_last_page_len": (3, 2), "total_history_lengths": (5, 2), "total_history_offsets": (7, 3),
             "new_history_nnz_cuda": (10, 1), "new_history_offsets": (11, 3), "batch_indices": (14, nnz), "position": (14 + nnz, nnz)}
    for name, (start, n) in views.items():
        v = getattr(m, name)
        assert v.tolist() == list(range(start, start + n)), name
        assert v.data_ptr() == buf.data_ptr() + 4 * start, name
    assert m.kv_seqlens.shape == (B,) and m.kv_seqlen_offsets.shape == (B + 1,)
    assert m.kv_seqlens.data_ptr() != m.total_history_lengths.data_ptr()
    # the allocator's words land in those views as they are
    _, words = PageAllocator(4, 8, 6).allocate([10, 11], [6, 9])
    buf[:14] = torch.tensor(words, dtype=torch.int32)
    assert m.kv_indptr.tolist() == [0, 2, 5] and m.kv_last_page_len.tolist() == [2, 1]
    assert m.new_history_offsets.tolist() == [0, 6, 15] and m.new_history_nnz_cuda.item() == 15
    # a given buffer is used, and refused when it is too small
    again = get_kvcache_metadata_buffer(B, nnz, pages, metadata_gpu_buffer=buf, device="cpu")
    assert again.metadata_gpu_buffer is buf and again.position.data_ptr() == m.position.data_ptr()
    with pytest.raises(ValueError, match="words"):
        get_kvcache_metadata_buffer(B, nnz + 1, pages, metadata_gpu_buffer=buf, device="cpu")


def test_copy_metadata_pads_lengths_with_zero_and_offsets_with_their_end():
    src = get_kvcache_metadata_buffer(1, 2, 2, device="cpu")
    dst = get_kvcache_metadata_buffer(3, 4, 4, device="cpu")
    src.metadata_gpu_buffer.copy_(torch.tensor([0, 2, 3, 7, 0, 7, 2, 0, 2, 0, 0, 5, 6], dtype=torch.int32))
    src.page_ids_gpu_buffer.copy_(_i32(4, 1))
    src.kv_seqlens.copy_(_i32(9))
    src.kv_seqlen_offsets.copy_(_i32(0, 9))
    dst.metadata_gpu_buffer.fill_(-1)
    dst.page_ids_gpu_buffer.fill_(-1)
    copy_kvcache_metadata(dst, src)
    assert dst.kv_indices.tolist() == [4, 1, 0, 0] and dst.kv_indptr.tolist() == [0, 2, 2, 2]
    assert dst.kv_last_page_len.tolist() == [3, 0, 0] and dst.new_history_offsets.tolist() == [0, 2, 2, 2]
    assert dst.total_history_offsets.tolist() == [0, 7, 7, 7] and dst.new_history_nnz_cuda.tolist() == [2]
    assert dst.batch_indices.tolist() == [0, 0, 0, 0] and dst.position.tolist() == [5, 6, 0, 0]
    assert dst.kv_seqlens.tolist() == [9, 0, 0] and dst.kv_seqlen_offsets.tolist() == [0, 9, 9, 9]
    assert dst.new_history_nnz == 2


def test_mover_arguments_are_checked_before_a_kernel_runs():
    import mi355_native as N
    import paged_kvcache_ops

    cache = torch.zeros(4, 2, 4, 2, 32, dtype=torch.bfloat16)
    ids = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(N.NativeError):
        paged_kvcache_ops.gather_kvcache(torch.zeros(2, 2, 4, 2, 32, dtype=torch.bfloat16), cache, ids, 2, 0, 1)
    with pytest.raises(ValueError, match="paged_kv_cache must have 5 dimensions"):
        paged_kvcache_ops.gather_kvcache(cache[:2], cache[0], ids, 2, 0, 1)
    with pytest.raises(ValueError, match="kv_layout"):
        paged_kvcache_ops.scatter_kvcache(cache[:2], cache, ids, 2, 2, 1)
    lib = N.lib()
    assert lib.mi355_kvcache_move_pages(0, None, None, None, 0, 4, 1, 512, 512, 0, 512, 0, 0, 0, None) == 0
    assert lib.mi355_kvcache_move_pages(0, None, None, None, 2, 4, 1, 512, 512, 0, 512, 0, 0, 0, None) == -1
    assert b"null" in lib.mi355_last_error()
    assert lib.mi355_kvcache_move_pages(0, None, None, None, 2, 4, 1, 512, 516, 0, 512, 0, 0, 0, None) == -1
    assert b"multiples of 8" in lib.mi355_last_error()
    assert lib.mi355_kvcache_move_pages(2, None, None, None, 2, 4, 1, 512, 512, 0, 512, 0, 0, 0, None) == -1
    assert lib.mi355_kvcache_batch_positions(None, None, 3, 0, None, None, None) == 0
    assert lib.mi355_kvcache_batch_positions(None, None, 3, 5, None, None, None) == -1
