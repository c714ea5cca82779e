"""The GPU tier of the reference's `recsys_kvcache_manager` (corelib/recsys_kvcache_manager) on MI355X: `DeviceKVCache`, the
page allocator behind it, the batch metadata and the lookup records.  Host storage, FlexKV, the asynchronous onboard / offload
task layer and the `kvcache_manager_ops` torch bindings are out of scope."""
from .gpu_kvcache_manager import DeviceKVCache, GPUKVCacheManager, PageAllocator
from .kvcache_metadata import KVCacheMetadata, copy_kvcache_metadata, get_kvcache_metadata_buffer
from .kvcache_utils import KVCacheOffloadMode, KVIndexMeta, KVLookupResult

__all__ = ["DeviceKVCache", "GPUKVCacheManager", "PageAllocator", "KVCacheMetadata", "get_kvcache_metadata_buffer",
           "copy_kvcache_metadata", "KVLookupResult", "KVIndexMeta", "KVCacheOffloadMode"]
