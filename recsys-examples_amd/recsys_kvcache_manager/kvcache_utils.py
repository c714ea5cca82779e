"""Plain records of the KV cache manager (the reference's recsys_kvcache_manager/kvcache_utils.py): what a lookup found, per
user, on the GPU tier and on a host tier."""
from dataclasses import dataclass, field
from enum import Enum
from typing import Any, Dict, Optional

import torch


class KVCacheOffloadMode(Enum):
    LAZY = "lazy"
    EAGER = "eager"


@dataclass
class KVLookupResult:
    """Per user of `user_ids`: where its cached history starts and how long it is, on the GPU (`gpu_*`), on the host (`host_*`)
    and merged (`cached_*`).  A tier that was not asked leaves its two fields None."""
    user_ids: torch.Tensor
    cached_start_indices: Optional[torch.Tensor] = None
    cached_lengths: Optional[torch.Tensor] = None
    gpu_cached_start_indices: Optional[torch.Tensor] = None
    gpu_cached_lengths: Optional[torch.Tensor] = None
    host_cached_start_indices: Optional[torch.Tensor] = None
    host_cached_lengths: Optional[torch.Tensor] = None
    token_ids: Optional[torch.Tensor] = None
    token_mask: Optional[torch.Tensor] = None
    extra: Dict[str, Any] = field(default_factory=dict)

    def _has(self, tier: str) -> bool:
        return getattr(self, tier + "_cached_start_indices") is not None and getattr(self, tier + "_cached_lengths") is not None

    @classmethod
    def merge(cls, lookup_res1, lookup_res2):
        """One result from a GPU lookup and a host lookup of the same users, given in either order.  Per user: nothing on the
        host -> the GPU entry as it is; nothing on the GPU -> the host entry; both -> start 0 and the longer of the host
        length and the GPU end (the host tier caches from the beginning, and the GPU part must start inside it)."""
        if not torch.equal(lookup_res1.user_ids, lookup_res2.user_ids):
            raise ValueError("merge: the two lookups are of different users")
        gpu, host = (lookup_res2, lookup_res1) if lookup_res1._has("host") else (lookup_res1, lookup_res2)
        if not gpu._has("gpu") or not host._has("host"):
            raise ValueError("merge needs one GPU lookup result and one host lookup result")
        if gpu.extra:
            raise ValueError("a GPU lookup result carries no extra fields")
        starts = torch.empty_like(gpu.gpu_cached_start_indices)
        lengths = torch.empty_like(gpu.gpu_cached_lengths)
        g_start, g_len = gpu.gpu_cached_start_indices.tolist(), gpu.gpu_cached_lengths.tolist()
        h_start, h_len = host.host_cached_start_indices.tolist(), host.host_cached_lengths.tolist()
        for i in range(len(g_len)):
            if h_len[i] == 0:
                start, length = g_start[i], g_len[i]
            else:
                if h_start[i] != 0:
                    raise ValueError(f"user {i}: the host tier must cache from the beginning of the sequence")
                if g_len[i] == 0:
                    start, length = 0, h_len[i]
                else:
                    if not 0 <= g_start[i] <= h_len[i]:
                        raise ValueError(f"user {i}: gap between the host part (length {h_len[i]}) and the GPU part "
                                         f"(start {g_start[i]})")
                    start, length = 0, max(h_len[i], g_start[i] + g_len[i])
            starts[i] = start
            lengths[i] = length
        return cls(user_ids=gpu.user_ids, cached_start_indices=starts, cached_lengths=lengths,
                   gpu_cached_start_indices=gpu.gpu_cached_start_indices, gpu_cached_lengths=gpu.gpu_cached_lengths,
                   host_cached_start_indices=host.host_cached_start_indices, host_cached_lengths=host.host_cached_lengths,
                   extra=host.extra or {})


@dataclass
class KVIndexMeta:
    user_ids: torch.Tensor
    seq_lengths: torch.Tensor
