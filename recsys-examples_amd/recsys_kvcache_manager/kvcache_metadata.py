"""The metadata of one batch of the paged KV cache (the reference's recsys_kvcache_manager/kvcache_metadata.py): the page ids
in one int32 buffer, everything else as views of a second one.

Layout of `metadata_gpu_buffer` for a batch of B sequences and nnz new tokens (int32 words; gpu_kvcache_manager_impl.cpp:307-312
and 373-377), 5 B + 4 header words followed by the per-token outputs of the append-metadata kernel:

    0           kv_indptr              [B + 1]   page offsets into kv_indices
    B + 1       kv_last_page_len       [B]
    2 B + 1     total_history_lengths  [B]
    3 B + 1     total_history_offsets  [B + 1]
    4 B + 2     new_history_nnz_cuda   [1]
    4 B + 3     new_history_offsets    [B + 1]
    5 B + 4     batch_indices          [nnz]
    5 B + 4 + nnz   position           [nnz]
"""
from dataclasses import dataclass
from typing import List, Optional

import torch


def header_words(batch_size: int) -> int:
    return 5 * batch_size + 4


@dataclass
class KVCacheMetadata:
    page_ids_gpu_buffer: torch.Tensor
    metadata_gpu_buffer: torch.Tensor

    # paged cache
    kv_indices: torch.Tensor = None              # [pages]
    kv_indptr: torch.Tensor = None               # [B + 1]
    kv_last_page_len: torch.Tensor = None        # [B]
    total_history_lengths: torch.Tensor = None   # [B]
    total_history_offsets: torch.Tensor = None   # [B + 1]
    new_history_offsets: torch.Tensor = None     # [B + 1]

    # append
    batch_indices: torch.Tensor = None           # [nnz]
    position: torch.Tensor = None                # [nnz]
    new_history_nnz: int = 0
    new_history_nnz_cuda: torch.Tensor = None    # [1]

    # key lengths of the attention call (filled by the caller: history + candidates)
    kv_seqlens: Optional[torch.Tensor] = None         # [B]
    kv_seqlen_offsets: Optional[torch.Tensor] = None  # [B + 1]

    kv_cache_table: Optional[List[torch.Tensor]] = None

    kv_onload_handle: Optional[object] = None

    max_seqlen: Optional[int] = 0

    onboard_slot_mappings: Optional[List[torch.Tensor]] = None
    onboard_task_ids: Optional[torch.Tensor] = None


def get_kvcache_metadata_buffer(batch_size: int, num_new_tokens: int, num_pages: int,
                                page_ids_gpu_buffer: Optional[torch.Tensor] = None,
                                metadata_gpu_buffer: Optional[torch.Tensor] = None, device: Optional[int] = None):
    """A KVCacheMetadata whose tensor fields are views of the two buffers (allocated here unless given)."""
    if device is None:
        device = torch.cuda.current_device()
    if page_ids_gpu_buffer is None:
        page_ids_gpu_buffer = torch.empty((num_pages,), dtype=torch.int32, device=device)
    words = header_words(batch_size) + 2 * num_new_tokens
    if metadata_gpu_buffer is None:
        metadata_gpu_buffer = torch.empty((words,), dtype=torch.int32, device=device)
    elif metadata_gpu_buffer.numel() < words:
        raise ValueError(f"metadata_gpu_buffer holds {metadata_gpu_buffer.numel()} words, {words} are needed")
    B, buf = batch_size, metadata_gpu_buffer
    total_history_lengths = buf.narrow(0, 2 * B + 1, B)
    total_history_offsets = buf.narrow(0, 3 * B + 1, B + 1)
    return KVCacheMetadata(
        page_ids_gpu_buffer=page_ids_gpu_buffer,
        metadata_gpu_buffer=buf,
        kv_indices=page_ids_gpu_buffer,
        kv_indptr=buf.narrow(0, 0, B + 1),
        kv_last_page_len=buf.narrow(0, B + 1, B),
        total_history_lengths=total_history_lengths,
        total_history_offsets=total_history_offsets,
        new_history_offsets=buf.narrow(0, 4 * B + 3, B + 1),
        batch_indices=buf.narrow(0, 5 * B + 4, num_new_tokens),
        position=buf.narrow(0, 5 * B + 4 + num_new_tokens, num_new_tokens),
        new_history_nnz=num_new_tokens,
        new_history_nnz_cuda=buf.narrow(0, 4 * B + 2, 1),
        kv_seqlens=torch.empty_like(total_history_lengths),
        kv_seqlen_offsets=torch.empty_like(total_history_offsets),
    )


def _copy_padded(dst: torch.Tensor, src: torch.Tensor, repeat_last: bool) -> None:
    n = src.shape[0]
    dst[:n].copy_(src, non_blocking=True)
    if dst.shape[0] > n:
        dst[n:] = src[-1] if repeat_last else 0


def copy_kvcache_metadata(dst_metadata: KVCacheMetadata, src_metadata: KVCacheMetadata):
    """Copies a batch's metadata into the (larger, static) buffers of a captured graph: lengths and indices are padded with
    zeros, offsets with their last entry, so that the padding sequences are empty."""
    for name, is_offsets in (("kv_indices", False), ("kv_indptr", True), ("kv_last_page_len", False), ("batch_indices", False),
                             ("position", False), ("new_history_nnz_cuda", False), ("total_history_offsets", True),
                             ("new_history_offsets", True), ("kv_seqlens", False), ("kv_seqlen_offsets", True)):
        _copy_padded(getattr(dst_metadata, name), getattr(src_metadata, name), is_offsets)
    dst_metadata.new_history_nnz = src_metadata.new_history_nnz
    dst_metadata.kv_onload_handle = src_metadata.kv_onload_handle
