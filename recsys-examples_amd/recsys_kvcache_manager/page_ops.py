"""Thin launchers of csrc/kvcache_ops.hip: the page mover and the append-metadata kernel.  Argument checks happen here, on
shapes and strides only -- nothing is read from the device, nothing is allocated, so both calls capture into a graph."""
import torch

import mi355_native as N

GATHER, SCATTER = 0, 1


def _page_layout(t: torch.Tensor, name: str):
    """(layers, pages, page elements, layer stride, page stride) of a [L, P, 2, page_size, H, D] or [P, 2, page_size, H, D]
    table whose page interior is contiguous"""
    if t.dim() not in (5, 6):
        raise ValueError(f"{name} must be [pages, 2, page_size, heads, head_dim] with an optional leading layer dimension, "
                         f"got {t.dim()} dimensions")
    if t.size(-4) != 2:
        raise ValueError(f"{name}: dimension {t.dim() - 4} must hold the K and the V half, got {t.size(-4)}")
    inner, want = 1, []
    for size in reversed(t.shape[-4:]):
        want.append(inner)
        inner *= size
    for d, (size, stride, w) in enumerate(zip(reversed(t.shape[-4:]), reversed(t.stride()[-4:]), want)):
        if size > 1 and stride != w:
            raise ValueError(f"{name}: the inside of a page must be contiguous (dimension {t.dim() - 1 - d} has stride {stride}, "
                             f"expected {w})")
    layers = t.size(0) if t.dim() == 6 else 1
    pages = t.size(-5)
    layer_stride = t.stride(0) if t.dim() == 6 and layers > 1 else 0
    page_stride = t.stride(-5) if pages > 1 else 0
    return layers, pages, inner, layer_stride, page_stride


def move_pages(direction: int, cache: torch.Tensor, staging: torch.Tensor, page_ids: torch.Tensor, num_pages: int,
               grid_cap: int = 0, nontemporal: int = -1, names=("cache", "staging")) -> None:
    """direction GATHER: staging[..., j, :] = cache[..., page_ids[j], :] for j < num_pages; SCATTER: the inverse.  Ids outside
    [0, pages of cache) are skipped.  grid_cap / nontemporal: measurement knobs of tools/bench_kvcache_pages.py (0 / -1: the
    library's measured defaults).  names: what
    the caller calls the two tensors, for the error messages."""
    num_pages = int(num_pages)
    if not (cache.is_cuda and staging.is_cuda and page_ids.is_cuda):
        raise N.NativeError("the page mover expects GPU tensors (no CPU fallback exists)")
    if cache.device != staging.device or cache.device != page_ids.device:
        raise ValueError("cache, staging and page_ids must be on one device")
    if cache.dtype != staging.dtype or cache.element_size() != 2:
        raise ValueError(f"cache and staging must share one 16-bit dtype, got {cache.dtype} and {staging.dtype}")
    if page_ids.dtype != torch.int32 or page_ids.dim() != 1 or (page_ids.numel() > 1 and page_ids.stride(0) != 1):
        raise ValueError("page_ids must be a contiguous 1-D int32 tensor")
    if cache.dim() != staging.dim():
        raise ValueError(f"cache has {cache.dim()} dimensions and staging {staging.dim()}")
    L, P, elems, c_layer, c_page = _page_layout(cache, names[0])
    Ls, n, _, s_layer, s_page = _page_layout(staging, names[1])
    if L != Ls or cache.shape[-4:] != staging.shape[-4:]:
        raise ValueError(f"cache is {tuple(cache.shape)} and staging {tuple(staging.shape)}: layers or page shapes differ")
    if not 0 <= num_pages <= min(n, page_ids.numel()):
        raise ValueError(f"num_pages = {num_pages}, but staging holds {n} pages and page_ids {page_ids.numel()} ids")
    if num_pages == 0 or L == 0:
        return
    N.check(N.lib().mi355_kvcache_move_pages(direction, N.ptr(cache), N.ptr(staging), N.ptr(page_ids), num_pages, P, L, elems,
                                             c_page, c_layer, s_page, s_layer, int(grid_cap), int(nontemporal),
                                             N.stream()), "mi355_kvcache_move_pages")


def batch_positions(new_history_offsets: torch.Tensor, total_history_lengths: torch.Tensor, nnz: int,
                    batch_indices: torch.Tensor, positions: torch.Tensor) -> None:
    """batch_indices[i], positions[i] of new token i < nnz (include/recsys_amd.h, mi355_kvcache_batch_positions)"""
    ts = (new_history_offsets, total_history_lengths, batch_indices, positions)
    if not all(t.is_cuda for t in ts):
        raise N.NativeError("batch_positions expects GPU tensors (no CPU fallback exists)")
    if any(t.dtype != torch.int32 or t.dim() != 1 or (t.numel() > 1 and t.stride(0) != 1) for t in ts):
        raise ValueError("batch_positions takes contiguous 1-D int32 tensors")
    B = total_history_lengths.numel()
    if new_history_offsets.numel() != B + 1:
        raise ValueError(f"new_history_offsets holds {new_history_offsets.numel()} entries for a batch of {B}")
    if not 0 <= nnz <= min(batch_indices.numel(), positions.numel()):
        raise ValueError(f"nnz = {nnz}, but the outputs hold {batch_indices.numel()} and {positions.numel()} entries")
    N.check(N.lib().mi355_kvcache_batch_positions(N.ptr(new_history_offsets), N.ptr(total_history_lengths), B, int(nnz),
                                                  N.ptr(batch_indices), N.ptr(positions), N.stream()),
            "mi355_kvcache_batch_positions")
