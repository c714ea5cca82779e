// Inference forward of a frozen embedding collection in ONE launch, and the general form of the table-id expansion.
//
// Replaces (reference): the forward of InferenceEmbeddingCollection (corelib/dynamicemb/dynamicemb/exportable_tables.py:501-564)
// -- INFERENCE_EMB::expand_table_ids (src/table_operation/expand_table_ids_torch_binding.cu:17-85), INFERENCE_EMB::table_lookup
// (lookup_torch_binding.cu, table_lookup_kernel kernels.cuh:81-187), an index_select + add, and the NVEmbedding / NVEmbeddingBag
// gather -- four to five launches with three [N] int64 temporaries between them.
//
// Here a lane resolves its key end to end: table id (binary search of the table boundaries, staged in LDS), slot (the
// one-lane probe of the eval forward, gather_dev.h: eval_probe_key -- digest vector, key word; scores are never touched, which is
// ScorePolicy.CONST), row address in the dense weight.  The 8-lane group_probe of table_dev.h was not tried here: the choice
// follows the eval forward's and is not backed by a measurement of its own.  An unknown key costs its lane the whole bucket
// (C / 16 digest vectors plus the key words of matching digests), and the wave waits for it.  The rows then move through the gather machinery of the training
// side: wave_copy_rows for sequence output, gather_pooled_eval for bags (gather_dev.h).  The kernel only reads its inputs.
//
// Weight layout (exportable_tables.py:281-292): table t owns the rows [table_offsets[t] - 1, table_offsets[t + 1] - 1); the
// first of them is the table's all-zero row, so slot -1 (unknown key) + table_offsets[t] lands on it.  A slot at or beyond the
// table's row count -- a table arena that was not loaded through the collection -- and, in identity mode, a key outside
// [0, rows) go to the zero row as well: nothing is read outside the table's rows.
#include <type_traits>
#include "common.h"
#include "gather_dev.h"
#include "../../include/recsys_amd.h"

namespace mi355 {

struct InfArgs {
  const uint64_t* keys;
  const int64_t* offsets;           // CSR offsets of the feature slots
  const int64_t* feature_offsets;   // [T + 1] feature -> table boundaries (nullptr: identity)
  const int64_t* tbo;               // [T + 1] bucket ranges of the tables (hash mode)
  const int64_t* table_offsets;     // [T + 1] first row of every table in the weight
  const void* weight;
  const float* psw;                 // per-sample weights (pooled, may be nullptr)
  void* out;
  int64_t n, lbs, offsets_numel;
  int T, D, row_bytes;
};

struct InfTabs {
  EvalTabs e;                   // seg = first key of every table, tptr = address of the table's first row
  int64_t rows[kEvalMaxT];      // rows of the table (without its zero row)
};

// called by the whole block; ends with a barrier
__device__ __forceinline__ void inf_tabs_load(InfTabs& L, const InfArgs& a, bool hash) {
  for (int t = threadIdx.x; t <= a.T; t += blockDim.x) {
    const int64_t f = a.feature_offsets ? a.feature_offsets[t] : t;
    const int64_t at = f * a.lbs;
    L.e.seg[t] = a.offsets[at < 0 ? 0 : (at < a.offsets_numel ? at : a.offsets_numel - 1)];   // (never outside the array, whatever feature_offsets holds)
    L.e.tbo[t] = hash ? a.tbo[t] : 0;
    if (t < a.T) {
      const uint64_t nb = hash ? (uint64_t)(a.tbo[t + 1] - a.tbo[t]) : 0ull;
      L.e.magic[t] = nb ? ~0ull / nb : 0ull;
      L.e.tptr[t] = (int64_t)(uintptr_t)a.weight + a.table_offsets[t] * a.row_bytes;
      L.e.rowb[t] = a.row_bytes;
      L.rows[t] = a.table_offsets[t + 1] - a.table_offsets[t] - 1;
    }
  }
  __syncthreads();
}

// key at position j -> address of its row in the weight (never 0 for a key that exists: unknown keys have the zero row)
template <bool kHash, bool kW>
struct InfHook {
  static constexpr bool kRow = true, kWeights = kW;
  const InfTabs* L;
  ProbeRefs pr;
  const float* psw;
  int C, cshift;
  __device__ __forceinline__ uintptr_t row(int64_t j, uint64_t key, bool have) const {
    const int t = eval_tab_index(L->e, pr.T, j);
    const EvalTab e = eval_tab_at(L->e, t);
    const uintptr_t end = (uintptr_t)(e.tp0 + L->rows[t] * e.rowb);
    uintptr_t rp;
    if constexpr (kHash) rp = eval_probe_key(pr, e, key, have, C, cshift);
    else rp = key < (uint64_t)L->rows[t] ? (uintptr_t)(e.tp0 + (int64_t)key * e.rowb) : 0;
    if (!have) return 0;
    return (rp != 0 && rp < end) ? rp : (uintptr_t)(e.tp0 - e.rowb);
  }
  __device__ __forceinline__ float weight(int64_t j) const { return psw[j]; }
};

template <bool kHash, bool kW>
__device__ __forceinline__ InfHook<kHash, kW> inf_hook(const InfTabs& tabs, const InfArgs& a, Table t) {
  InfHook<kHash, kW> h;
  h.L = &tabs; h.psw = a.psw;
  h.pr.keys = a.keys; h.pr.t = t; h.pr.T = a.T; h.pr.find_policy = kConst;
  h.C = (int)t.C; h.cshift = __builtin_ctz((unsigned)h.C);
  return h;
}

// Sequence output: a wave owns 64 consecutive keys, lane l resolves key i0 + l (64 independent chains), then the wave copies
// the 64 rows.  kFast: 16-byte aligned rows, moved as 32-bit words whatever the dtype is (a bit-exact copy), 4 LPR words per
// pass of wave_copy_rows.  Otherwise the rows are copied element by element (EB bytes each), one row after the other with
// min(D, 64) lanes busy: a fallback for odd D that is correct and not tuned.
template <bool kHash, bool kFast, int EB>
__global__ void __launch_bounds__(256) inference_rows_kernel(InfArgs a, Table t, int lpr_log2) {
  __shared__ InfTabs tabs;
  inf_tabs_load(tabs, a, kHash);
  const InfHook<kHash, false> hook = inf_hook<kHash, false>(tabs, a, t);
  const int64_t i0 = ((int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 64;
  if (i0 >= a.n) return;
  const int64_t j = i0 + lane_id();
  const int64_t jc = j < a.n ? j : a.n - 1;
  const uintptr_t rp = hook.row(jc, a.keys[jc], j < a.n);
  if constexpr (kFast) {
    const int words = a.row_bytes >> 2;
    for (int w0 = 0; w0 < words; w0 += 4 << lpr_log2)
      wave_copy_rows<kF32, kF32>(rp ? rp + (uintptr_t)w0 * 4 : 0, i0, a.n, words - w0, (float*)a.out + w0, words, lpr_log2);
  } else {
    using E = typename std::conditional<EB == 4, uint32_t, uint16_t>::type;
    const int rlo = (int)(rp & 0xffffffffu), rhi = (int)(rp >> 32);
    const int64_t left = a.n - i0;
    const int nr = (int)(left < 64 ? left : 64);
    for (int r = 0; r < nr; ++r) {
      const uintptr_t ad = (uintptr_t)(unsigned)__shfl(rlo, r, 64) | ((uintptr_t)(unsigned)__shfl(rhi, r, 64) << 32);
      const E* src = (const E*)ad;
      E* dst = (E*)a.out + (i0 + r) * a.D;
      for (int e = lane_id(); e < a.D; e += 64) dst[e] = src[e];
    }
  }
}

// Pooled output, rows of one column group (D <= 256, 16-byte aligned): the lane-group form of the eval forward with this
// file's row resolution and, optionally, per-sample weights
template <int DT, bool kHash, bool kW>
__global__ void __launch_bounds__(256) inference_pooled_kernel(PoolArgs g, InfArgs a, Table t, int lpr_log2) {
  __shared__ InfTabs tabs;
  inf_tabs_load(tabs, a, kHash);
  const InfHook<kHash, kW> hook = inf_hook<kHash, kW>(tabs, a, t);
  const int64_t sg = ((int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * (64 >> lpr_log2) + (lane_id() >> lpr_log2);
  gather_pooled_eval<DT, DT, 4, 4, true, InfHook<kHash, kW>>(g, hook.pr, lpr_log2, sg, &tabs.e, hook);
}

// Pooled output, every other row shape: a wave per bag, 64 keys resolved at a time, 64 columns per pass; fp32 accumulation
// in key order, one rounding at the store.  A fallback that is correct and not tuned: every 64-column pass resolves the bag's
// keys again (table search and probe), so D = 264 probes each key five times.
template <int DT, bool kHash>
__global__ void __launch_bounds__(256) inference_pooled_any_kernel(PoolArgs g, InfArgs a, Table t) {
  __shared__ InfTabs tabs;
  inf_tabs_load(tabs, a, kHash);
  const InfHook<kHash, false> hook = inf_hook<kHash, false>(tabs, a, t);
  const int64_t bag = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (bag >= g.FB) return;
  int64_t lo = g.offsets[bag], hi = g.offsets[bag + 1];
  lo = lo < 0 ? 0 : lo;
  hi = hi < a.n ? hi : a.n;
  const int lane = lane_id();
  for (int e0 = 0; e0 < a.D; e0 += 64) {
    const int e = e0 + lane;
    float acc = 0.f;
    for (int64_t r = lo; r < hi; r += 64) {
      const int64_t j = r + lane;
      const int64_t jc = j < hi ? j : hi - 1;
      const uintptr_t rp = hook.row(jc, a.keys[jc], j < hi);
      const float w = (a.psw && j < hi) ? a.psw[jc] : 1.f;
      const int rlo = (int)(rp & 0xffffffffu), rhi = (int)(rp >> 32);
      const int nr = (int)(hi - r < 64 ? hi - r : 64);
      for (int q = 0; q < nr; ++q) {
        const uintptr_t ad = (uintptr_t)(unsigned)__shfl(rlo, q, 64) | ((uintptr_t)(unsigned)__shfl(rhi, q, 64) << 32);
        const float wq = __shfl(w, q, 64);
        if (e < a.D) acc = fmaf(wq, ld1<DT>((const void*)ad, e), acc);
      }
    }
    if (g.combiner == 1 && hi > lo) acc /= (float)(hi - lo);
    if (e < a.D) st1<DT>(g.dst, bag * a.D + e, acc);
  }
}

// table id of position i: the largest t in [0, T] with offsets[fo[t] * lbs] <= i (fo == nullptr: identity)
__global__ void __launch_bounds__(256)
inference_expand_table_ids_kernel(const int64_t* __restrict__ offsets, const int64_t* __restrict__ fo, int T, int64_t lbs, int64_t n,
                                  int64_t* __restrict__ table_ids) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int lo = 0, hi = T;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      const int64_t f = fo ? fo[mid] : mid;
      if (offsets[f * lbs] <= i) lo = mid; else hi = mid - 1;
    }
    table_ids[i] = lo;
  }
}

}  // namespace mi355

using namespace mi355;

extern "C" {

int mi355_inference_expand_table_ids(const int64_t* offsets, int64_t offsets_numel, const int64_t* table_offsets_in_feature,
                                     int64_t num_tables, int64_t local_batch_size, int64_t n, int64_t* table_ids,
                                     hipStream_t stream) {
  MI355_CHECK_ARG(n >= 0, "mi355_inference_expand_table_ids: n < 0");
  if (n == 0) return MI355_OK;
  MI355_CHECK_ARG(local_batch_size > 0, "mi355_inference_expand_table_ids: local_batch_size must be > 0");
  MI355_CHECK_ARG(offsets && offsets_numel >= 1 && table_ids, "mi355_inference_expand_table_ids: null offsets / table_ids");
  if (!table_offsets_in_feature) num_tables = (offsets_numel - 1) / local_batch_size;
  MI355_CHECK_ARG(num_tables >= 0 && num_tables < (1ll << 30), "mi355_inference_expand_table_ids: num_tables out of range");
  // (identity form: the highest entry read is offsets[num_tables * local_batch_size], inside the array by construction)
  hipLaunchKernelGGL(inference_expand_table_ids_kernel, dim3(grid_for(n, 256)), dim3(256), 0, stream, offsets,
                     table_offsets_in_feature, (int)num_tables, local_batch_size, n, table_ids);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

int mi355_inference_emb_forward(const void* keys, int64_t n, const int64_t* offsets, int64_t offsets_numel,
                                const int64_t* feature_offsets, int64_t num_tables, int64_t local_batch_size,
                                const void* table_storage, const int64_t* table_bucket_offsets, int64_t bucket_capacity,
                                const int64_t* table_offsets, const void* weight, int64_t dim,
                                int weight_dtype, const int64_t* pooling_offsets, int64_t num_bags,
                                const float* per_sample_weights, int pooling_mode, int use_dynamic_hash, void* out,
                                hipStream_t stream) {
  MI355_CHECK_ARG(pooling_mode == -1 || pooling_mode == 1 || pooling_mode == 2,
                  "mi355_inference_emb_forward: pooling_mode must be -1 (none), 1 (sum) or 2 (mean)");
  MI355_CHECK_ARG(weight_dtype == kF32 || weight_dtype == kF16, "mi355_inference_emb_forward: weight dtype must be fp32 or fp16");
  MI355_CHECK_ARG(n >= 0 && dim >= 1 && dim < (1ll << 24), "mi355_inference_emb_forward: n / dim out of range");
  MI355_CHECK_ARG(num_tables >= 1 && num_tables <= kEvalMaxT, "mi355_inference_emb_forward: 1 .. 128 tables");
  MI355_CHECK_ARG(local_batch_size > 0, "mi355_inference_emb_forward: local_batch_size must be > 0");
  MI355_CHECK_ARG(offsets && offsets_numel >= 1 && table_offsets && weight, "mi355_inference_emb_forward: null offsets / table_offsets / weight");
  if (!feature_offsets)
    MI355_CHECK_ARG(offsets_numel > num_tables * local_batch_size, "mi355_inference_emb_forward: offsets shorter than num_tables * local_batch_size + 1");
  if (use_dynamic_hash) {
    MI355_CHECK_ARG(table_storage && table_bucket_offsets, "mi355_inference_emb_forward: null table arena");
    MI355_CHECK_ARG(bucket_capacity >= 16 && bucket_capacity <= (1 << 20) && (bucket_capacity & (bucket_capacity - 1)) == 0,
                    "mi355_inference_emb_forward: bucket_capacity must be a power of two >= 16");
  }
  const bool pooled = pooling_mode != -1;
  if (pooled) {
    MI355_CHECK_ARG(pooling_offsets && num_bags >= 0 && num_bags < (1ll << 31), "mi355_inference_emb_forward: pooling needs pooling_offsets");
    MI355_CHECK_ARG(!(pooling_mode == 2 && per_sample_weights), "mi355_inference_emb_forward: per_sample_weights with mean pooling is not supported");
  }
  const int64_t out_rows = pooled ? num_bags : n;
  if (out_rows == 0) return MI355_OK;
  MI355_CHECK_ARG(keys || n == 0, "mi355_inference_emb_forward: null keys");
  MI355_CHECK_ARG(out, "mi355_inference_emb_forward: null output");
  const int EB = (int)dtype_bytes(weight_dtype);
  if (n == 0) {   // bags without keys
    if (hipMemsetAsync(out, 0, (size_t)(out_rows * dim * EB), stream) != hipSuccess) { mi355_set_error("hipMemsetAsync failed"); return MI355_ELAUNCH; }
    return MI355_OK;
  }
  InfArgs a;
  a.keys = (const uint64_t*)keys; a.offsets = offsets; a.feature_offsets = feature_offsets; a.tbo = table_bucket_offsets;
  a.table_offsets = table_offsets; a.weight = weight; a.psw = per_sample_weights; a.out = out; a.n = n; a.lbs = local_batch_size; a.offsets_numel = offsets_numel;
  a.T = (int)num_tables; a.D = (int)dim; a.row_bytes = (int)dim * EB;
  const Table t = make_table(const_cast<void*>(table_storage), use_dynamic_hash ? bucket_capacity : 16, 1);
  const bool aligned = a.row_bytes % 16 == 0 && ((uintptr_t)weight & 15) == 0 && ((uintptr_t)out & 15) == 0;
  const bool hash = use_dynamic_hash != 0;
  if (!pooled) {
    const int words = a.row_bytes >> 2;
    int le = 3;
    while ((4 << le) < words && le < 6) ++le;
    const dim3 grid((unsigned)ceil_div(n, 256));
    MI355_CHECK_ARG(ceil_div(n, 256) < (1ll << 31), "mi355_inference_emb_forward: too many keys");
#define LAUNCH_ROWS(H, F, E) hipLaunchKernelGGL((inference_rows_kernel<H, F, E>), grid, dim3(256), 0, stream, a, t, le)
    if (aligned) { if (hash) LAUNCH_ROWS(true, true, 4); else LAUNCH_ROWS(false, true, 4); }
    else if (EB == 4) { if (hash) LAUNCH_ROWS(true, false, 4); else LAUNCH_ROWS(false, false, 4); }
    else { if (hash) LAUNCH_ROWS(true, false, 2); else LAUNCH_ROWS(false, false, 2); }
#undef LAUNCH_ROWS
  } else {
    PoolArgs g;
    g.src = nullptr; g.src_stride = 0; g.row_addr = nullptr; g.rev = nullptr; g.offsets = pooling_offsets; g.D_offsets = nullptr;
    g.dst = out; g.FB = num_bags; g.n = n; g.B = (int)num_bags; g.D = (int)dim; g.total_D = (int)dim; g.combiner = pooling_mode == 2 ? 1 : 0;
    int le = 3;
    while ((4 << le) < dim && le < 6) ++le;
    if (aligned && dim <= (4 << le)) {
      const dim3 grid((unsigned)grid_for(num_bags, 4 * (64 >> le) * 4, 1 << 20));
#define LAUNCH_POOL(DT, H, W) hipLaunchKernelGGL((inference_pooled_kernel<DT, H, W>), grid, dim3(256), 0, stream, g, a, t, le)
#define LAUNCH_POOL_DT(DT)                                                                                     \
  do {                                                                                                         \
    if (hash) { if (a.psw) LAUNCH_POOL(DT, true, true); else LAUNCH_POOL(DT, true, false); }                   \
    else { if (a.psw) LAUNCH_POOL(DT, false, true); else LAUNCH_POOL(DT, false, false); }                      \
  } while (0)
      if (weight_dtype == kF32) LAUNCH_POOL_DT(kF32); else LAUNCH_POOL_DT(kF16);
#undef LAUNCH_POOL_DT
#undef LAUNCH_POOL
    } else {
      const dim3 grid((unsigned)ceil_div(num_bags, 4));
#define LAUNCH_ANY(DT) do { if (hash) hipLaunchKernelGGL((inference_pooled_any_kernel<DT, true>), grid, dim3(256), 0, stream, g, a, t); \
                            else hipLaunchKernelGGL((inference_pooled_any_kernel<DT, false>), grid, dim3(256), 0, stream, g, a, t); } while (0)
      if (weight_dtype == kF32) LAUNCH_ANY(kF32); else LAUNCH_ANY(kF16);
#undef LAUNCH_ANY
    }
  }
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

}  // extern "C"
