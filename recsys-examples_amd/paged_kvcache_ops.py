"""`paged_kvcache_ops` of the reference (examples/commons/ops/cuda_ops/csrc/paged_kvcache_ops_cuda.cpp:325-337) on
MI355X: importing this module registers `torch.ops.paged_kvcache_ops.append_kvcache` with the reference's schema, so
`examples/hstu/modules/paged_hstu_infer_layer.py:350-364` calls it unchanged.  `gather_kvcache` (cache off-load,
paged_kvcache_ops_cuda.cpp:229-234, a plain function as in the reference's pybind module) and its mirror image
`scatter_kvcache` (on-load) run the page mover of csrc/kvcache_ops.hip on one layer's table; the manager that decides which
pages move is recsys_kvcache_manager.DeviceKVCache."""
import torch

from hstu.hstu_attn_interface import append_kvcache  # noqa: F401
from recsys_kvcache_manager import page_ops as _page_ops

_lib = torch.library.Library("paged_kvcache_ops", "FRAGMENT")
_lib.define("append_kvcache(Tensor append_key, Tensor append_value, Tensor batch_indices, Tensor positions, "
            "Tensor seqlen_offsets, Tensor nnz_cuda, int max_nnz, Tensor(a!) kv_cache_table, Tensor kv_indices, "
            "Tensor kv_indptr, Tensor kv_last_page_len, int kv_layout) -> Tensor(a!)")


def _impl(append_key, append_value, batch_indices, positions, seqlen_offsets, nnz_cuda, max_nnz, kv_cache_table,
          kv_indices, kv_indptr, kv_last_page_len, kv_layout):
    return append_kvcache(append_key, append_value, batch_indices, positions, seqlen_offsets, nnz_cuda, max_nnz,
                          kv_cache_table, kv_indices, kv_indptr, kv_last_page_len, kv_layout)


_lib.impl("append_kvcache", _impl, "CUDA")


def _single_layer(direction, buffer, buffer_name, paged_kv_cache, page_ids, num_pages, kv_layout):
    if kv_layout not in (0, 1):
        raise ValueError(f"kv_layout must be 0 (NHD) or 1 (HND), got {kv_layout}")
    for t, name in ((paged_kv_cache, "paged_kv_cache"), (buffer, buffer_name)):
        if t.dim() != 5:
            raise ValueError(f"{name} must have 5 dimensions (num_pages, 2, page_size, num_head, head_dim), got {t.dim()}")
    _page_ops.move_pages(direction, paged_kv_cache, buffer, page_ids, num_pages, names=("paged_kv_cache", buffer_name))


def gather_kvcache(gather_kv_gpu_buffer, paged_kv_cache, page_ids_to_offload, num_pages, kv_layout, num_sms):
    """gather_kv_gpu_buffer[j] = paged_kv_cache[page_ids_to_offload[j]] for j < num_pages, bit-exact, on the current stream.
    Both tensors are one layer's [pages, 2, page_size, H, D] (kv_layout 0) or [pages, 2, H, page_size, D] (kv_layout 1) with a
    contiguous page interior; the page strides are free.  Ids outside the table are skipped.  num_sms is accepted and ignored:
    the launch is sized from the bytes to move."""
    _single_layer(_page_ops.GATHER, gather_kv_gpu_buffer, "gather_kv_gpu_buffer", paged_kv_cache, page_ids_to_offload, num_pages,
                  kv_layout)


def scatter_kvcache(scatter_kv_gpu_buffer, paged_kv_cache, page_ids_to_onboard, num_pages, kv_layout, num_sms):
    """paged_kv_cache[page_ids_to_onboard[j]] = scatter_kv_gpu_buffer[j] for j < num_pages: the inverse of gather_kvcache.
    An id listed twice is written twice, which copy stays is undefined."""
    _single_layer(_page_ops.SCATTER, scatter_kv_gpu_buffer, "scatter_kv_gpu_buffer", paged_kv_cache, page_ids_to_onboard, num_pages,
                  kv_layout)
