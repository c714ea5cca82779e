// KV cache GPU tier: the page mover (cache pages <-> a staging buffer, both directions, any range of layers in one launch) and
// the append metadata of a batch (batch index and cache position of every new-history token).
//
// Replaces (reference): GatherPagedKVCacheKernel / GatherPagedKVCacheAllLayersKernel
// (examples/commons/ops/cuda_ops/csrc/paged_kvcache_ops_kernel.cu:237-429), the gather / scatter kernels of
// corelib/recsys_kvcache_manager/src/gather_scatter_kernels.cu, and GetPagedBatchIndicesPositionsKernel
// (paged_kvcache_ops_kernel.cu:451-492).  Written for wave64 from the semantics.
//
// Page mover.  The cache is [L, P, 2, page_size, H, D]: a page (K half + V half) is 2 * page_size * H * D contiguous elements
// in the NHD and in the HND layout alike, so the mover never looks inside a page -- staging slot j of layer l is a bit-exact
// copy of page page_ids[j] of layer l.  The strides between pages and between layers are arguments, for the cache and for the
// staging buffer separately (a per-layer view, a padded table, a sliced table).
//   * The unit of work is a 16-byte chunk; a RUN is kRunChunks = 256 consecutive chunks of one page (4 KiB), one wave per run:
//     lane i of step u takes chunk 64 u + i, the four steps' loads are issued before their stores.  The page id is read once per
//     run, from a wave-uniform index (a scalar load), not once per lane per chunk.
//   * Load follows bytes: runs = layers x pages x ceil(page_chunks / 256), handed to the waves of a capped grid with a grid
//     stride.  Nothing is read back from the device and nothing is allocated: the launch is sized from num_pages on the host.
//   * Every offset is 64 bits wide (the reference multiplies int32 page_id by uint32 stride_page, which wraps once a cache
//     passes 2^32 elements).
//   * A slot whose id is outside [0, num_cache_pages) is skipped whole: no read, no write.
// Duplicate ids are fine in a gather; in a scatter which copy of a page wins is undefined.
#include "common.h"
#include "../../include/recsys_amd.h"

namespace mi355 {

typedef unsigned int kv_u32x4 __attribute__((ext_vector_type(4)));

constexpr int kRunSteps = 4;                       // 16-byte loads a lane has in flight
constexpr int kRunChunks = kRunSteps * kWave;      // chunks per run (4 KiB)
// Grid cap of the mover in 256-thread blocks.  Measured (profiles/kvcache_pages_bench.txt, 512 MiB of 64 KiB pages = 32768
// blocks of four runs): the time falls from a cap of 2048 to no stride at all (gather 192 -> 179 us, scatter 212 -> 206) and
// is flat beyond; a 16 MiB move does not care.  Larger moves than that stride.
constexpr int64_t kMoveGridCap = 32768;
// Cache hint per direction {gather, scatter}: 1 = nontemporal loads and stores (same record).  The gather reads pages nobody
// reads again soon: 205 -> 179 us.  The scatter gains 3 % (206 -> 200) and writes pages the attention reads next: it stays plain.
constexpr int kMoveNontemporal[2] = {1, 0};

struct PageMoveArgs {
  kv_u32x4* cache;            // first layer of the range
  kv_u32x4* staging;
  const int32_t* page_ids;    // [num_pages]
  int64_t cache_page, cache_layer, staging_page, staging_layer;   // strides in 16-byte chunks
  uint32_t num_pages, num_cache_pages, page_chunks, runs_per_page, total_runs;
};

// DIR 0: cache -> staging (gather, offload); 1: staging -> cache (scatter, onboard).  NT: nontemporal loads and stores.
template <int DIR, bool NT>
__global__ void __launch_bounds__(256) kv_page_move_kernel(PageMoveArgs a) {
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint32_t wave = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) / kWave);
  const uint32_t nwaves = gridDim.x * (blockDim.x / kWave);
  for (uint32_t r = wave; r < a.total_runs; r += nwaves) {
    const uint32_t k = r % a.runs_per_page, t = r / a.runs_per_page;
    const uint32_t j = t % a.num_pages, l = t / a.num_pages;
    const int32_t page = a.page_ids[j];
    if ((uint32_t)page >= a.num_cache_pages) continue;   // (negative ids wrap above the bound)
    kv_u32x4* c = a.cache + (int64_t)l * a.cache_layer + (int64_t)page * a.cache_page;
    kv_u32x4* s = a.staging + (int64_t)l * a.staging_layer + (int64_t)j * a.staging_page;
    const kv_u32x4* src = DIR == 0 ? c : s;
    kv_u32x4* dst = DIR == 0 ? s : c;
    const uint32_t base = k * kRunChunks + lane;
    kv_u32x4 v[kRunSteps];
    if (k * kRunChunks + kRunChunks <= a.page_chunks) {   // a whole run: no lane is idle
#pragma unroll
      for (int u = 0; u < kRunSteps; ++u)
        v[u] = NT ? __builtin_nontemporal_load(src + base + u * kWave) : src[base + u * kWave];
#pragma unroll
      for (int u = 0; u < kRunSteps; ++u) {
        if (NT) __builtin_nontemporal_store(v[u], dst + base + u * kWave);
        else dst[base + u * kWave] = v[u];
      }
    } else {                                              // the tail of a page that is no multiple of 4 KiB
#pragma unroll
      for (int u = 0; u < kRunSteps; ++u)
        if (base + u * kWave < a.page_chunks) v[u] = src[base + u * kWave];
#pragma unroll
      for (int u = 0; u < kRunSteps; ++u)
        if (base + u * kWave < a.page_chunks) dst[base + u * kWave] = v[u];
    }
  }
}

// Token i of the new history: its sequence b is the last one with offsets[b] <= i (empty sequences in front of it share that
// offset and lose the search), its position total[b] - (offsets[b + 1] - offsets[b]) + (i - offsets[b]).  One thread per
// token: a batch of one long and many empty sequences costs what its tokens cost.
__global__ void __launch_bounds__(256)
kv_batch_positions_kernel(const int32_t* __restrict__ offsets, const int32_t* __restrict__ total, int B, int64_t nnz,
                          int32_t* __restrict__ batch_indices, int32_t* __restrict__ positions) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nnz; i += (int64_t)gridDim.x * blockDim.x) {
    int lo = 0, hi = B;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if ((int64_t)offsets[mid] <= i) lo = mid; else hi = mid;
    }
    const int32_t start = offsets[lo];
    batch_indices[i] = lo;
    positions[i] = total[lo] - (offsets[lo + 1] - start) + ((int32_t)i - start);
  }
}

}  // namespace mi355

using namespace mi355;

int mi355_kvcache_move_pages(int direction, void* cache, void* staging, const int32_t* page_ids, int64_t num_pages,
                             int64_t num_cache_pages, int64_t num_layers, int64_t page_elems, int64_t cache_page_stride,
                             int64_t cache_layer_stride, int64_t staging_page_stride, int64_t staging_layer_stride,
                             int64_t grid_cap, int nontemporal, hipStream_t stream) {
  MI355_CHECK_ARG(direction == 0 || direction == 1, "direction must be 0 (gather) or 1 (scatter)");
  MI355_CHECK_ARG(num_pages >= 0 && num_layers >= 0 && num_cache_pages >= 0, "negative page or layer count");
  MI355_CHECK_ARG(page_elems > 0 && page_elems % 8 == 0, "a page must hold a positive multiple of 8 elements");
  MI355_CHECK_ARG(cache_page_stride % 8 == 0 && cache_layer_stride % 8 == 0 && staging_page_stride % 8 == 0 &&
                      staging_layer_stride % 8 == 0, "page and layer strides must be multiples of 8 elements");
  MI355_CHECK_ARG(cache_page_stride >= 0 && cache_layer_stride >= 0 && staging_page_stride >= 0 && staging_layer_stride >= 0,
                  "page and layer strides must not be negative");
  if (num_pages == 0 || num_layers == 0) return MI355_OK;
  MI355_CHECK_ARG(cache && staging && page_ids, "null pointer");
  MI355_CHECK_ARG(((uintptr_t)cache | (uintptr_t)staging) % 16 == 0, "cache and staging must be 16-byte aligned");
  MI355_CHECK_ARG(num_cache_pages <= INT32_MAX && num_pages <= INT32_MAX, "page counts must fit 31 bits");
  const int64_t page_chunks = page_elems / 8;
  const int64_t rpp = ceil_div(page_chunks, (int64_t)kRunChunks);
  MI355_CHECK_ARG(page_chunks <= INT32_MAX && num_layers * num_pages <= INT32_MAX / rpp, "move too large for one launch");
  PageMoveArgs a;
  a.cache = (kv_u32x4*)cache; a.staging = (kv_u32x4*)staging; a.page_ids = page_ids;
  a.cache_page = cache_page_stride / 8; a.cache_layer = cache_layer_stride / 8;
  a.staging_page = staging_page_stride / 8; a.staging_layer = staging_layer_stride / 8;
  a.num_pages = (uint32_t)num_pages; a.num_cache_pages = (uint32_t)num_cache_pages; a.page_chunks = (uint32_t)page_chunks;
  a.runs_per_page = (uint32_t)rpp; a.total_runs = (uint32_t)(num_layers * num_pages * rpp);
  const dim3 grid(grid_for(a.total_runs, 256 / kWave, grid_cap > 0 ? grid_cap : kMoveGridCap)), block(256);
  if (nontemporal < 0) nontemporal = kMoveNontemporal[direction];
  if (direction == 0) {
    if (nontemporal) hipLaunchKernelGGL((kv_page_move_kernel<0, true>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((kv_page_move_kernel<0, false>), grid, block, 0, stream, a);
  } else {
    if (nontemporal) hipLaunchKernelGGL((kv_page_move_kernel<1, true>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((kv_page_move_kernel<1, false>), grid, block, 0, stream, a);
  }
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

int mi355_kvcache_batch_positions(const int32_t* new_history_offsets, const int32_t* total_history_lengths, int64_t batch,
                                  int64_t nnz, int32_t* batch_indices, int32_t* positions, hipStream_t stream) {
  MI355_CHECK_ARG(batch >= 0 && batch <= INT32_MAX && nnz >= 0 && nnz <= INT32_MAX, "batch and nnz must fit 31 bits");
  if (nnz == 0) return MI355_OK;
  MI355_CHECK_ARG(batch > 0, "new tokens without a sequence");
  MI355_CHECK_ARG(new_history_offsets && total_history_lengths && batch_indices && positions, "null pointer");
  hipLaunchKernelGGL(kv_batch_positions_kernel, dim3(grid_for(nnz, 256)), dim3(256), 0, stream, new_history_offsets,
                     total_history_lengths, (int)batch, nnz, batch_indices, positions);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}
