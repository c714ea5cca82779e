"""The GPU tier of the KV cache manager: which pages of the paged cache a user's history lives in.

`PageAllocator` is the bookkeeping of the reference's GPUKVCacheManagerImpl (corelib/recsys_kvcache_manager/src/
gpu_kvcache_manager_impl.cpp) as pure host code: the FIFO queue of free pages, the LRU of users, per user the page list, the
cached start position, the cached length and the offloaded length, the offload locks.  It makes no torch device call.

`DeviceKVCache` (alias `GPUKVCacheManager`) is the reference's class of that name (recsys_kvcache_manager/
gpu_kvcache_manager.py): the cache tensor [L, P, 2, page_size, H, D], the allocator, the upload of a batch's metadata and the
append-metadata kernel, plus `offload_pages` / `onboard_pages` over the page mover of csrc/kvcache_ops.hip.

One deliberate difference: where the reference asserts, or as a last resort evicts a user whose pages are locked
for an offload in flight, `allocate` raises RuntimeError and leaves every user as it was."""
from collections import OrderedDict, deque
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch

import mi355_native as N

from . import page_ops
from .kvcache_metadata import KVCacheMetadata, get_kvcache_metadata_buffer, header_words
from .kvcache_utils import KVLookupResult


def _ceil_div(a: int, b: int) -> int:
    return -(-a // b)


class PageAllocator:
    def __init__(self, num_tokens_per_page: int, num_tokens_per_chunk: int, num_primary_cache_pages: int,
                 num_buffer_pages: int = 0, max_batch_size: int = 1, max_sequence_length: int = 0):
        if num_tokens_per_page <= 0 or num_primary_cache_pages < 0:
            raise ValueError("num_tokens_per_page must be positive and num_primary_cache_pages not negative")
        self.page_size = num_tokens_per_page
        self.chunk_size = num_tokens_per_chunk
        self.num_primary_cache_pages = num_primary_cache_pages
        self.num_buffer_pages = num_buffer_pages
        self.max_offload_pages = max_batch_size * _ceil_div(max_sequence_length, num_tokens_per_page)
        self.evict_all()

    # ---- state ------------------------------------------------------------------------------------------------------
    def evict_all(self) -> None:
        self._free = deque(range(self.num_primary_cache_pages))   # FIFO: pages are reused in the order they were freed
        self._lru: "OrderedDict[int, None]" = OrderedDict()        # front: least recently allocated user
        self._pages: Dict[int, List[int]] = {}
        self._start: Dict[int, int] = {}       # first cached position on the GPU (> 0 once leading pages were offloaded and freed)
        self._length: Dict[int, int] = {}      # cached tokens from _start on
        self._offloaded: Dict[int, int] = {}   # tokens from position 0 that a host tier holds
        self._locks: Dict[int, int] = {}       # offloads in flight per user
        self.total_offloaded_pages = 0

    def free_pages(self) -> List[int]:
        return list(self._free)

    def users(self) -> List[int]:
        """users in eviction order, least recently allocated first"""
        return list(self._lru)

    def pages_of(self, uid: int) -> List[int]:
        return list(self._pages.get(uid, ()))

    def _offloaded_pages(self, uid: int) -> int:
        """whole pages at the front of the user's list that a host tier holds as well"""
        return max(0, (self._offloaded.get(uid, 0) - self._start.get(uid, 0)) // self.page_size)

    def lookup(self, uids: Sequence[int]) -> Tuple[List[int], List[int]]:
        """(cached start positions, cached lengths); 0, 0 for a user the GPU tier does not hold"""
        return [self._start.get(u, 0) for u in uids], [self._length.get(u, 0) for u in uids]

    # ---- eviction ---------------------------------------------------------------------------------------------------
    def _forget(self, uid: int) -> None:
        self._lru.pop(uid, None)
        for d in (self._pages, self._start, self._length, self._offloaded):
            d.pop(uid, None)

    def evict(self, uid: int) -> None:
        if uid not in self._lru:
            return
        self._free.extend(self._pages.get(uid, ()))
        self.total_offloaded_pages -= self._offloaded_pages(uid)
        self._forget(uid)

    def _evict_offloaded(self, uid: int) -> None:
        """frees the leading pages a host tier holds; the user keeps the rest and starts later"""
        n = self._offloaded_pages(uid)
        if n == 0:
            return
        pages = self._pages[uid]
        self._free.extend(pages[:n])
        del pages[:n]
        self._start[uid] += n * self.page_size
        self._length[uid] -= n * self.page_size
        self.total_offloaded_pages -= n

    def _evictable(self, frozen) -> List[int]:
        return [u for u in self._lru if u not in self._locks and u not in frozen]

    # ---- allocation -------------------------------------------------------------------------------------------------
    def plan(self, uids: Sequence[int], total_lengths: Sequence[int], host_cached_lengths: Optional[Sequence[int]] = None):
        """What `allocate` of this batch would do, without doing it: (new tokens, pages of the batch, pages to take from the
        free queue).  Raises what `allocate` would raise."""
        B, ps = len(uids), self.page_size
        host = [0] * B if host_cached_lengths is None else list(host_cached_lengths)
        if len(total_lengths) != B or len(host) != B:
            raise ValueError("uids, total_lengths and host_cached_lengths must have one length")
        dropped, cached, reclaimed = set(), [], 0
        for uid, h in zip(uids, host):
            known = uid in self._length and uid not in dropped
            start, length = (self._start[uid], self._length[uid]) if known else (0, 0)
            if length > 0 and h < start:   # the host lost what the GPU part builds on: the GPU part is dropped
                dropped.add(uid)
                reclaimed += len(self._pages[uid])
                cached.append(0)
            else:
                cached.append(max(h, start + length))
        state, need, nnz, num_pages = {}, 0, 0, 0
        for uid, total, h, c in zip(uids, total_lengths, host, cached):
            if uid in state:
                start, length = state[uid]
            elif uid in self._length and uid not in dropped:
                start, length = self._start[uid], self._length[uid]
            else:
                start, length = 0, 0
            total_pages = _ceil_div(total, ps)
            onboard = _ceil_div(h, ps) if length == 0 else start // ps
            append = total_pages - onboard - _ceil_div(length, ps)
            if total < c or append < 0:
                raise ValueError(f"user {uid}: total history length {total} is shorter than the {c} cached tokens")
            need += onboard + append
            nnz += total - c
            num_pages += total_pages
            state[uid] = (0, total)
        available = len(self._free) + reclaimed
        if need > available:
            frozen = set(uids)
            available += sum(len(self._pages[u]) for u in self._evictable(frozen))
            if need > available:
                raise RuntimeError(
                    f"KV cache allocation needs {need} pages, but only {available} can be freed "
                    f"({len(self._free)} free; the users of the batch and {len(self._locks)} users locked for an offload in "
                    f"flight are kept)")
        return nnz, num_pages, need

    def _alloc_single(self, uid: int, total: int, host_length: int, frozen) -> List[int]:
        ps = self.page_size
        known = uid in self._lru
        self._lru.pop(uid, None)
        self._lru[uid] = None            # most recently used
        start, length = (self._start.get(uid, 0), self._length.get(uid, 0)) if known else (0, 0)
        # 1. pages for what comes back from the host: the whole host part of a user the GPU does not hold, else the
        #    leading pages that were offloaded and freed
        onboard = _ceil_div(host_length, ps) if length == 0 else start // ps
        # 2. pages for the new tokens
        current = _ceil_div(length, ps)
        total_pages = _ceil_div(total, ps)
        required = total_pages - current
        # 3. offloaded pages go first (the host still has them), whole users after
        for u in list(self._lru):
            if required <= len(self._free):
                break
            if u in self._locks or u in frozen:
                continue
            self._evict_offloaded(u)
            if self._length[u] == 0:
                self._forget(u)
        while required > len(self._free):   # (plan() has shown that enough users can go)
            self.evict(self._evictable(frozen)[0])
        mine = self._pages.get(uid, []) if known else []
        pages = [self._free.popleft() for _ in range(onboard)] + mine[:current]
        pages += [self._free.popleft() for _ in range(total_pages - len(pages))]
        self._pages[uid] = pages
        self._start[uid] = 0
        self._length[uid] = total
        return pages

    def allocate(self, uids: Sequence[int], total_lengths: Sequence[int],
                 host_cached_lengths: Optional[Sequence[int]] = None) -> Tuple[List[int], List[int]]:
        """Pages for a batch whose sequences have grown to total_lengths.  Returns (page ids of all sequences back to back,
        the 5 B + 4 metadata words in the layout of kvcache_metadata).  On RuntimeError / ValueError nothing has changed."""
        uids, total_lengths = list(uids), list(total_lengths)
        B, ps = len(uids), self.page_size
        host = [0] * B if host_cached_lengths is None else list(host_cached_lengths)
        self.plan(uids, total_lengths, host)
        cached = []
        for uid, h in zip(uids, host):
            start, length = self._start.get(uid, 0), self._length.get(uid, 0)
            if length > 0 and h < start:
                self.evict(uid)
                cached.append(0)
                continue
            cached.append(max(h, start + length))
            self._offloaded[uid] = h
        words = [0] * header_words(B)
        indptr, last, totals, total_off, new_off = 0, B + 1, 2 * B + 1, 3 * B + 1, 4 * B + 3
        frozen, page_ids = set(uids), []
        for i, (uid, total, h) in enumerate(zip(uids, total_lengths, host)):
            pages = self._alloc_single(uid, total, h, frozen)
            page_ids += pages
            words[indptr + i + 1] = words[indptr + i] + len(pages)
            words[last + i] = total % ps or ps
            words[totals + i] = total
            words[total_off + i + 1] = words[total_off + i] + total
            words[new_off + i + 1] = words[new_off + i] + total - cached[i]
        words[4 * B + 2] = words[new_off + B]
        return page_ids, words

    # ---- offload / onboard ------------------------------------------------------------------------------------------
    def revoke_onboard_pages(self, uids: Sequence[int], onboard_starts: Sequence[int], onboard_lengths: Sequence[int]) -> None:
        """an onboard that `allocate` made room for did not happen: its pages return to the free queue and the user starts later"""
        ps = self.page_size
        for uid, s, n in zip(uids, onboard_starts, onboard_lengths):
            if uid not in self._pages:
                continue
            first, end = s // ps, (s + n) // ps
            pages = self._pages[uid]
            self._free.extend(pages[first:end])
            count = len(pages[first:end])
            del pages[first:end]
            self._start[uid] += count * ps
            self._length[uid] -= count * ps
            if not pages:
                self.evict(uid)

    def _pending(self, uid: int) -> int:
        """cached tokens past what a host tier holds"""
        return self._start.get(uid, 0) + self._length.get(uid, 0) - self._offloaded.get(uid, 0)

    def check_for_offload(self, uids: Sequence[int] = ()) -> List[int]:
        """Users with at least a chunk of tokens to offload: those of `uids` first, then others in LRU order while the buffer
        pages allow and at most max_offload_pages pages."""
        chosen, seen, pages = [], set(), 0
        for uid in uids:
            if self._pending(uid) >= self.chunk_size:
                chosen.append(uid)
                seen.add(uid)
            pages += self._pending(uid) // self.page_size
        for uid in self._lru:
            if self.total_offloaded_pages + pages + len(self._free) > self.num_buffer_pages:
                break
            if uid in seen or self._offloaded.get(uid, 0) < self._start[uid]:
                continue
            if self._pending(uid) >= self.chunk_size:
                pages += self._pending(uid) // self.page_size
                if pages > self.max_offload_pages:
                    break
                chosen.append(uid)
                seen.add(uid)
        return chosen

    def acquire_offload_pages(self, uids: Sequence[int], offloaded_lengths: Sequence[int] = (),
                              always_offload: bool = False) -> Tuple[List[int], List[int], List[List[int]]]:
        """(users to offload, first position to offload per user, page ids per user) and a lock on each user asked about;
        `release_offload_pages` takes the locks back.  always_offload: every page of every user, from position 0."""
        if always_offload:
            lists = []
            for uid in uids:
                lists.append(self.pages_of(uid))
                if uid in self._pages:
                    self._locks[uid] = self._locks.get(uid, 0) + 1
            return list(uids), [0] * len(uids), lists
        out_uids, out_starts, out_pages = [], [], []
        for i, uid in enumerate(uids):
            if len(offloaded_lengths) == len(uids) and uid in self._pages:
                self._offloaded[uid] = int(offloaded_lengths[i])
            if self._pending(uid) >= self.chunk_size:
                off = self._offloaded.get(uid, 0)
                first = (off - self._start[uid]) // self.page_size
                out_uids.append(uid)
                out_starts.append(off)
                out_pages.append(self._pages[uid][first:first + self._pending(uid) // self.page_size])
            self._locks[uid] = self._locks.get(uid, 0) + 1
        return out_uids, out_starts, out_pages

    def release_offload_pages(self, uids: Sequence[int], offload_starts: Sequence[int], offload_lengths: Sequence[int],
                              offloaded: Sequence[int]) -> None:
        for i, uid in enumerate(uids):
            if uid not in self._locks:
                continue
            self._locks[uid] -= 1
            if self._locks[uid] <= 0:
                del self._locks[uid]
            if offloaded[i] and uid in self._pages:
                self.total_offloaded_pages -= self._offloaded_pages(uid)
                self._offloaded[uid] = int(offload_starts[i]) + int(offload_lengths[i])
                self.total_offloaded_pages += self._offloaded_pages(uid)


def _ints(t) -> List[int]:
    return [int(x) for x in (t.tolist() if isinstance(t, torch.Tensor) else t)]


def _i32(values) -> torch.Tensor:
    return torch.tensor(values, dtype=torch.int32)


class _Staging:
    """one pinned upload buffer and the event that says its last copy ran"""

    def __init__(self):
        self.buf = torch.empty(0, dtype=torch.int32).pin_memory()
        self.event: Optional[torch.cuda.Event] = None

    def take(self, words: int) -> torch.Tensor:
        if self.event is not None:
            self.event.synchronize()
        if self.buf.numel() < words:
            self.buf = torch.empty(max(words, 2 * self.buf.numel()), dtype=torch.int32).pin_memory()
        return self.buf


class DeviceKVCache:
    def __init__(self, num_layers: int, num_heads: int, head_dim: int, num_tokens_per_page: int, num_tokens_per_chunk: int,
                 num_primary_cache_pages: int, num_buffer_pages: int, max_batch_size: int, max_sequence_length: int,
                 dtype: torch.dtype, device_idx: int):
        self.num_layers = num_layers
        self.num_heads = num_heads
        self.head_dim = head_dim
        self.page_size = num_tokens_per_page
        self.chunk_size = num_tokens_per_chunk
        self.num_primary_cache_pages = num_primary_cache_pages
        self.num_buffer_pages = num_buffer_pages
        self.max_batch_size = max_batch_size
        self.max_sequence_length = max_sequence_length
        self.dtype = dtype
        self.device_idx = device_idx
        if dtype not in (torch.bfloat16, torch.float16):
            raise ValueError(f"the KV cache holds bf16 or fp16, got {dtype}")
        self.gpu_kvcache_tensor: torch.Tensor = torch.empty(
            [num_layers, num_primary_cache_pages, 2, self.page_size, num_heads, head_dim], dtype=dtype, device=device_idx)
        self.gpu_kvcache_tables = list(self.gpu_kvcache_tensor.unbind(dim=0))
        self.allocator = PageAllocator(num_tokens_per_page, num_tokens_per_chunk, num_primary_cache_pages, num_buffer_pages,
                                       max_batch_size, max_sequence_length)
        self.num_sms = torch.cuda.get_device_properties(device_idx).multi_processor_count
        # two pinned upload buffers, used in turn; each waits for the event behind its own last copy before it is overwritten
        self._staging = [_Staging(), _Staging()]
        self._turn = 0

    def get_cache_tables(self, layer_idx: int = -1) -> Union[torch.Tensor, List[torch.Tensor]]:
        if layer_idx == -1:
            return self.gpu_kvcache_tables
        return self.gpu_kvcache_tables[layer_idx]

    def lookup(self, uids: torch.Tensor) -> KVLookupResult:
        starts, lengths = self.allocator.lookup(_ints(uids))
        return KVLookupResult(user_ids=uids, gpu_cached_start_indices=_i32(starts), gpu_cached_lengths=_i32(lengths))

    def allocate(self, uids: torch.Tensor, seq_hist_lengths: torch.Tensor, lookup_results: KVLookupResult,
                 output_kvcache_metadata: Optional[KVCacheMetadata] = None) -> KVCacheMetadata:
        """Pages for the batch and its metadata on the device, in stream order on the current stream (no host wait behind
        it).  lookup_results.host_cached_lengths None: no host tier, zeros.  lookup_results.cached_lengths is not needed:
        the allocator knows what the GPU holds."""
        ids, totals = _ints(uids), _ints(seq_hist_lengths)
        B = len(ids)
        host = None if lookup_results is None or lookup_results.host_cached_lengths is None \
            else _ints(lookup_results.host_cached_lengths)
        meta = output_kvcache_metadata
        if meta is not None:   # the caller's buffers must hold the batch: checked before anything changes
            nnz, num_pages, _ = self.allocator.plan(ids, totals, host)
            if meta.kv_indptr.numel() != B + 1:
                raise ValueError(f"output_kvcache_metadata was laid out for a batch of {meta.kv_indptr.numel() - 1}, not {B}")
            if meta.page_ids_gpu_buffer.numel() < num_pages or min(meta.batch_indices.numel(), meta.position.numel()) < nnz:
                raise ValueError(f"output_kvcache_metadata is too small for {num_pages} pages and {nnz} new tokens")
        page_ids, words = self.allocator.allocate(ids, totals, host)
        nnz = words[4 * B + 2]
        if meta is None:
            meta = get_kvcache_metadata_buffer(B, nnz, len(page_ids), device=self.device_idx)
            meta.kv_cache_table = self.gpu_kvcache_tables
        meta.max_seqlen = max(totals) if totals else 0
        meta.new_history_nnz = nnz
        staging = self._staging[self._turn]
        self._turn ^= 1
        pinned = staging.take(len(words) + len(page_ids))
        pinned[:len(words)] = _i32(words)
        pinned[len(words):len(words) + len(page_ids)] = _i32(page_ids)
        with torch.cuda.device(self.device_idx):
            meta.metadata_gpu_buffer[:len(words)].copy_(pinned[:len(words)], non_blocking=True)
            meta.page_ids_gpu_buffer[:len(page_ids)].copy_(pinned[len(words):len(words) + len(page_ids)], non_blocking=True)
            staging.event = torch.cuda.Event()
            staging.event.record()
            page_ops.batch_positions(meta.new_history_offsets, meta.total_history_lengths, nnz, meta.batch_indices, meta.position)
        return meta

    def evict(self, uids: torch.Tensor) -> None:
        for uid in _ints(uids):
            self.allocator.evict(uid)

    def evict_all(self) -> None:
        self.allocator.evict_all()

    def put(self, k, v, layer_idx, kvcache_metadata: KVCacheMetadata, append_offsets: Optional[torch.Tensor] = None) -> None:
        """appends the batch's new tokens k, v [nnz, H, D] to layer layer_idx (paged_kvcache_ops.append_kvcache)"""
        from hstu.hstu_attn_interface import append_kvcache

        if k.shape != v.shape:
            raise ValueError(f"key and value shapes differ: {tuple(k.shape)} and {tuple(v.shape)}")
        if k.dim() != 3 or tuple(k.shape[-2:]) != (self.num_heads, self.head_dim):
            raise ValueError(f"k and v must be [tokens, {self.num_heads}, {self.head_dim}] of one layer, got {tuple(k.shape)}")
        m = kvcache_metadata
        if append_offsets is None:
            append_offsets = torch.zeros((m.kv_indptr.numel() - 1,), dtype=torch.int32, device=k.device)
        self.gpu_kvcache_tables[layer_idx] = append_kvcache(
            k, v, m.batch_indices, m.position, append_offsets, m.new_history_nnz_cuda, 0, self.gpu_kvcache_tables[layer_idx],
            m.kv_indices, m.kv_indptr, m.kv_last_page_len, 0)

    def get(self, page_ids, last_page_lens, layer_idx) -> Tuple[torch.Tensor, torch.Tensor]:
        """the keys and values [tokens, H, D] of one sequence, read back from its pages (a debugging aid)"""
        table = self.gpu_kvcache_tables[layer_idx]
        ids = torch.as_tensor(page_ids, device=table.device).long()
        rows = ids.numel() * self.page_size - (self.page_size - int(last_page_lens)) if ids.numel() else 0
        k = table[ids, 0].reshape(-1, self.num_heads, self.head_dim)[:rows].clone()
        v = table[ids, 1].reshape(-1, self.num_heads, self.head_dim)[:rows].clone()
        return k, v

    def revoke_onboard_pages(self, user_ids, onboard_page_starts, num_onboard_pages):
        self.allocator.revoke_onboard_pages(_ints(user_ids), _ints(onboard_page_starts), _ints(num_onboard_pages))

    def check_for_offload(self, uids: Optional[torch.Tensor] = None) -> torch.Tensor:
        return torch.tensor(self.allocator.check_for_offload(() if uids is None else _ints(uids)), dtype=torch.int64)

    def acquire_offload_pages(self, uids: torch.Tensor, offloaded_lengths: torch.Tensor,
                              always_offload: bool = False) -> Tuple[torch.Tensor, torch.Tensor, List[torch.Tensor]]:
        users, starts, pages = self.allocator.acquire_offload_pages(_ints(uids), _ints(offloaded_lengths), always_offload)
        return torch.tensor(users, dtype=torch.int64), _i32(starts), [_i32(p) for p in pages]

    def release_offload_pages(self, uids: torch.Tensor, offload_start_indices: torch.Tensor, offload_lengths: torch.Tensor,
                              offloaded: bool) -> None:
        n = len(_ints(uids))
        flags = [int(offloaded)] * n if isinstance(offloaded, (bool, int)) else _ints(offloaded)
        self.allocator.release_offload_pages(_ints(uids), _ints(offload_start_indices), _ints(offload_lengths), flags)

    # ---- page movement (the reference keeps these two in its host manager) ------------------------------------------
    def _layer_range(self, layers) -> Tuple[int, int]:
        if layers is None:
            return 0, self.num_layers
        if isinstance(layers, (range, slice)):
            lo, hi, step = layers.indices(self.num_layers) if isinstance(layers, slice) else (layers.start, layers.stop, layers.step)
        else:
            (lo, hi), step = layers, 1
        if step != 1 or not 0 <= lo <= hi <= self.num_layers:
            raise ValueError(f"layers must be a contiguous range inside [0, {self.num_layers}), got {layers}")
        return lo, hi

    def _device_ids(self, page_ids) -> torch.Tensor:
        ids = torch.as_tensor(page_ids)
        if ids.dim() != 1 or ids.dtype.is_floating_point:
            raise ValueError("page_ids must be a 1-D tensor of integers")
        if not ids.is_cuda:
            ids = ids.to(torch.int32).to(self.gpu_kvcache_tensor.device)
        return ids.to(torch.int32).contiguous()

    def offload_pages(self, page_ids, out: Optional[torch.Tensor] = None, layers=None) -> torch.Tensor:
        """staging [layers, n, 2, page_size, H, D]: slot j of every layer of the range is a copy of page page_ids[j].  page_ids:
        a device int32 tensor, or a CPU tensor as acquire_offload_pages returns (uploaded here).  With `out` and device ids
        the call allocates nothing and captures into a graph."""
        lo, hi = self._layer_range(layers)
        ids = self._device_ids(page_ids)
        n = ids.numel()
        if out is None:
            out = torch.empty((hi - lo, n) + tuple(self.gpu_kvcache_tensor.shape[2:]), dtype=self.dtype,
                              device=self.gpu_kvcache_tensor.device)
        page_ops.move_pages(page_ops.GATHER, self.gpu_kvcache_tensor[lo:hi], out, ids, n)
        return out

    def onboard_pages(self, staging: torch.Tensor, page_ids, layers=None) -> None:
        """the inverse of offload_pages: page page_ids[j] of every layer of the range becomes staging slot j"""
        lo, hi = self._layer_range(layers)
        ids = self._device_ids(page_ids)
        page_ops.move_pages(page_ops.SCATTER, self.gpu_kvcache_tensor[lo:hi], staging, ids, ids.numel())


GPUKVCacheManager = DeviceKVCache
