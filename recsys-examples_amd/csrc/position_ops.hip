// HSTU positional encoder: position / timestamp embedding adds over a jagged [N, D] tensor, forward and backward.
//
// Replaces (reference, examples/hstu/ops/triton_ops/triton_position.py): _add_position_embeddings_kernel (:80-137) and its
// backward (:141-211), _add_timestamp_position_embeddings_kernel (:309-404) and the sort-and-atomics backward
// _add_embeddings_bwd_kernel (:434-482).  Written for wave64 from the arithmetic; the reference is Triton.
//
// Forward (both ops): the row run of jagged_dev.h with arithmetic in the copy.  Their own:
//   resolve: lane l's row -> its sequence (binary search of the offsets), the table row index (or the two of the timestamp
//            form), the addresses of its input row, its output row and its table rows.
//   stream:  wave_add_run, the load and store steps of jagged_dev.h's piece loop: a piece is V elements (Vec<>, vec_dev.h), up to
//            three loads a step, the add and its one rounding in the store step.
// V is the widest of 8 / 4 / 2 / 1 elements that divides D and that every base pointer and row stride of the call allows.
//
// Backward: a table-row gradient is a sum of d_out rows, bitwise reproducible, so no float atomics.  Two passes:
//   partials: the rows are cut into chunks of 64 consecutive rows of d_out (position form), or of 64 / 32 consecutive entries of
//             the SORTED index list (mi355_hstu_index_rows_sum; 32 while the call would be short of waves), one wave per chunk
//             (index form: per chunk and 64 pieces of columns).  Inside a chunk the rows that share a destination are one
//             contiguous range; the wave sums each range in row order and stores it as one fp32 partial row.  Along the chunk
//             sequence the pairs (chunk j, owner o) -- o the sequence b or the key k -- form a staircase, monotone in both, so
//             j + o is a unique slot: the workspace is (chunks + owners) fp32 rows and needs no index build and no memset.
//   sum:      one wave per (table row k, 64 pieces of columns): adds, in a fixed order, the rows that map to k one to one
//             (position form: row s_b + k of every sequence with k below its tail) and the partial rows of k in chunk order,
//             rounds once and writes the row -- every row, a row nothing maps to as zeros.
// A tail (or a bucket) of T rows is therefore split over T / 64 + 1 waves of the first pass; the second pass adds its
// T / 64 + 1 partial rows, eight loads in flight.  No lane ever loops over the T rows.
// Nothing outside a buffer is touched whatever the offsets / indices hold: table rows are clamped, rows outside [0, N) and keys
// outside [0, K) are skipped.
#include "common.h"
#include "jagged_dev.h"
#include "vec_dev.h"
#include "../../include/recsys_amd.h"

namespace mi355 {

__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : v > hi ? hi : v; }

struct PosArgs {                 // mi355_hstu_add_position_embeddings and the scaling of its backward
  uintptr_t in, out, dense;      // dense 0: out = in * scale
  int64_t in_stride, out_stride, dense_stride;   // bytes
  const int64_t* offsets;        // [B + 1]
  const int64_t* high;           // [B]
  const int64_t* ind_off;        // [B] or null
  int64_t N, B, K;
  float scale;
  RunPlan plan;                  // pieces of V elements
};

struct TsArgs {                  // mi355_hstu_add_timestamp_position_embeddings
  uintptr_t in, out, pos, ts;
  int64_t in_stride, out_stride, pos_stride, ts_stride;   // bytes
  const int64_t* offsets;        // [B + 1]
  const int64_t* lengths;        // [B]
  const int64_t* num_targets;    // [B] or null
  const int64_t* timestamps;     // [N]
  int32_t* pos_inds;             // [N] or null
  int32_t* ts_inds;              // [N] or null
  int64_t N, B, Np, Nt, mcsl, ntb, time_delta;
  float incr, tscale;
  int interleave, fn;
  RunPlan plan;
};

struct PosBwdArgs {              // the two passes of mi355_hstu_add_position_embeddings_bwd
  uintptr_t in, out, partial;    // d_out, d_dense, workspace
  int64_t in_stride, out_stride; // bytes
  const int64_t* offsets;
  const int64_t* high;
  int64_t N, B, K, D;
  uint32_t vpr, nslab;           // pieces per row, ceil(vpr / 64)
};

struct IdxArgs {                 // the two passes of mi355_hstu_index_rows_sum
  uintptr_t in, out, partial;
  int64_t in_stride, out_stride;
  const int32_t* keys;           // [count] ascending
  const int64_t* rows;           // [count]
  int64_t N, count, K, D;
  uint32_t vpr, nslab;
  int chunk_log2;                // entries per chunk: 64, or 32 while the call is short of waves
};

// The wave streams `nrows` rows of `vpr` pieces: lane l holds the addresses of row l (src or dst 0: skip the row; t0 0: no
// table row).  TS: out = in + round(t0 + t1), else out = in * scale + t0 (one rounding).
template <int DT, int TDT, int V, bool TS>
__device__ __forceinline__ void wave_add_run(uintptr_t src, uintptr_t dst, uintptr_t t0, uintptr_t t1, int nrows, uint32_t vpr,
                                             int vpr_shift, float scale) {
  constexpr int UN = 2;
  constexpr uintptr_t SB = Vec<DT, V>::BYTES, TB = Vec<TDT, V>::BYTES;
  const uintptr_t zero = (uintptr_t)g_zero_piece;
  float x[UN][V], p[UN][V], q[UN][V];
  uintptr_t d[UN];
  wave_run_pieces<UN>(
      nrows, vpr, vpr_shift,
      [&](int u, bool in, int row, uint32_t piece) {
        const uintptr_t col = (uintptr_t)piece;
        const uintptr_t s = shfl_addr(src, row), dd = shfl_addr(dst, row), a0 = shfl_addr(t0, row);
        const bool ok = in && s != 0 && dd != 0;
        Vec<DT, V>::ld(ok ? s + col * SB : zero, x[u]);
        Vec<TDT, V>::ld(ok && a0 != 0 ? a0 + col * TB : zero, p[u]);
        if constexpr (TS) {
          const uintptr_t a1 = shfl_addr(t1, row);
          Vec<TDT, V>::ld(ok && a1 != 0 ? a1 + col * TB : zero, q[u]);
        }
        d[u] = ok ? dd + col * SB : 0;
      },
      [&](int u) {
        if (d[u]) {
          float o[V];
#pragma unroll
          for (int e = 0; e < V; ++e) {
            if constexpr (TS) o[e] = x[u][e] + Elem<DT>::rnd(p[u][e] + q[u][e]);
            else o[e] = __fmaf_rn(x[u][e], scale, p[u][e]);
          }
          Vec<DT, V>::st(d[u], o);
        }
      });
}

template <int DT, int TDT, int V>
__global__ __launch_bounds__(256) void hstu_pos_add_kernel(const PosArgs a) {
  RowRun run;
  if (!row_run(a.N, a.plan.rpw_log2, run)) return;   // (wave-uniform)
  const bool have = run.have;
  const int64_t m = run.m;
  const int64_t b = sample_of(a.offsets, a.B, m);
  const int64_t s = a.offsets[b], e = a.offsets[b + 1];
  const bool ok = have && m >= s && m < e;
  const int64_t i = m - s + (a.ind_off ? a.ind_off[b] : 0);
  const int64_t h = a.high[b];
  const int64_t idx = clamp64(i >= h ? h : i, 0, a.K - 1);
  const uintptr_t src = ok ? a.in + (uintptr_t)m * a.in_stride : 0;
  const uintptr_t dst = ok ? a.out + (uintptr_t)m * a.out_stride : 0;
  const uintptr_t tab = ok && a.dense ? a.dense + (uintptr_t)idx * a.dense_stride : 0;
  wave_add_run<DT, TDT, V, false>(src, dst, tab, 0, run.nrows, a.plan.vpr, a.plan.vpr_shift, a.scale);
}

template <int DT, int TDT, int V>
__global__ __launch_bounds__(256) void hstu_ts_pos_add_kernel(const TsArgs a) {
  RowRun run;
  if (!row_run(a.N, a.plan.rpw_log2, run)) return;   // (wave-uniform)
  const bool have = run.have;
  const int64_t m = run.m;
  const int64_t b = sample_of(a.offsets, a.B, m);
  const int64_t s = a.offsets[b], e = a.offsets[b + 1];
  const bool ok = have && m >= s && m < e && e <= a.N;
  const int64_t n = m - s;
  // position index
  const int64_t nt = a.num_targets ? a.num_targets[b] : 0;
  const int64_t high = a.lengths[b] - (a.interleave ? 2 * nt : nt);
  int64_t p = high - (n < high ? n : high) + a.mcsl;
  p = p < a.Np - 1 ? p : a.Np - 1;
  if (n < a.mcsl) p = n;
  p = clamp64(p, 0, a.Np - 1);
  // timestamp bucket
  const int64_t tq = a.timestamps[ok ? e - 1 : m], tm = a.timestamps[m];
  float dt = (float)(tq - tm + a.time_delta);
  dt = fmaxf(dt, 1e-6f) / a.incr;
  float x = (a.fn == 0 ? sqrtf(dt) : logf(dt)) * a.tscale;
  x = fminf(fmaxf(x, 0.f), 2147483520.f);   // (NaN -> 0; the largest fp32 below 2^31)
  int64_t t = (int64_t)(int32_t)x;
  t = t < a.ntb ? t : a.ntb;
  t = clamp64(t, 0, a.Nt - 1);
  if (ok) {
    if (a.pos_inds) a.pos_inds[m] = (int32_t)p;
    if (a.ts_inds) a.ts_inds[m] = (int32_t)t;
  }
  const uintptr_t src = ok ? a.in + (uintptr_t)m * a.in_stride : 0;
  const uintptr_t dst = ok ? a.out + (uintptr_t)m * a.out_stride : 0;
  const uintptr_t t0 = ok ? a.pos + (uintptr_t)p * a.pos_stride : 0;
  const uintptr_t t1 = ok ? a.ts + (uintptr_t)t * a.ts_stride : 0;
  wave_add_run<DT, TDT, V, true>(src, dst, t0, t1, run.nrows, a.plan.vpr, a.plan.vpr_shift, 1.f);
}

// acc += rows [r0, r1) of the wave's chunk, piece c, in row order: lane r holds the address of row r (0: adds nothing)
template <int DT, int V>
__device__ __forceinline__ void wave_sum_rows(uintptr_t addr, int r0, int r1, uint32_t c, bool active, float (&acc)[V]) {
  constexpr int UN = 4;
  const uintptr_t zero = (uintptr_t)g_zero_piece;
  for (int r = r0; r < r1; r += UN) {
    float x[UN][V];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int rr = r + u;
      const uintptr_t ra = shfl_addr(addr, rr < 64 ? rr : 63);
      Vec<DT, V>::ld(rr < r1 && active && ra != 0 ? ra + (uintptr_t)c * Vec<DT, V>::BYTES : zero, x[u]);
    }
#pragma unroll
    for (int u = 0; u < UN; ++u)
#pragma unroll
      for (int e = 0; e < V; ++e) acc[e] += x[u][e];
  }
}

// acc += partial rows [j0 + o, j1 + o] of the workspace, piece c, in chunk order
template <int V>
__device__ __forceinline__ void wave_sum_partials(uintptr_t partial, int64_t D, int64_t j0, int64_t j1, int64_t o, uint32_t c,
                                                  bool active, float (&acc)[V]) {
  constexpr int UN = 8;
  const uintptr_t zero = (uintptr_t)g_zero_piece;
  for (int64_t j = j0; j <= j1; j += UN) {
    float x[UN][V];
#pragma unroll
    for (int u = 0; u < UN; ++u)
      Vec<kF32, V>::ld(j + u <= j1 && active ? partial + ((uintptr_t)(j + u + o) * D + (uintptr_t)c * V) * 4 : zero, x[u]);
#pragma unroll
    for (int u = 0; u < UN; ++u)
#pragma unroll
      for (int e = 0; e < V; ++e) acc[e] += x[u][e];
  }
}

// Rows n >= t_b = clamp(high_b, 0, K - 1) of sequence b all fall on table row t_b: the part of every such tail inside this
// wave's chunk j goes to partial row j + b.
template <int DT, int V>
__global__ __launch_bounds__(256) void hstu_pos_tail_partials_kernel(const PosBwdArgs a) {
  const int lane = lane_id();
  const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t m0 = j << 6;
  if (m0 >= a.N) return;
  const int64_t left = a.N - m0;
  const int nrows = left < 64 ? (int)left : 64;
  const bool have = lane < nrows;
  const int64_t m = m0 + (have ? lane : 0);
  const int64_t b = sample_of(a.offsets, a.B, m);
  const int64_t s = a.offsets[b], e = a.offsets[b + 1];
  const bool ok = have && m >= s && m < e;
  const bool tail = ok && m - s >= clamp64(a.high[b], 0, a.K - 1);
  const uintptr_t addr = a.in + (uintptr_t)m * a.in_stride;
  const int bi = (int)b;
  unsigned long long remaining = __ballot(ok);
  while (remaining) {   // (wave-uniform: one turn per sequence of the chunk)
    const int bc = __shfl(bi, __builtin_ctzll(remaining), 64);
    remaining &= ~__ballot(ok && bi == bc);
    const unsigned long long tm = __ballot(tail && bi == bc);
    if (!tm) continue;
    const int r0 = __builtin_ctzll(tm), r1 = 64 - __builtin_clzll(tm);
    for (uint32_t sl = 0; sl < a.nslab; ++sl) {
      const uint32_t c = sl * 64 + lane;
      const bool active = c < a.vpr;
      float acc[V] = {};
      wave_sum_rows<DT, V>(addr, r0, r1, c, active, acc);
      if (active) Vec<kF32, V>::st(a.partial + ((uintptr_t)(j + bc) * a.D + (uintptr_t)c * V) * 4, acc);
    }
  }
}

template <int DT, int TDT, int V>
__global__ __launch_bounds__(256) void hstu_pos_dense_grad_kernel(const PosBwdArgs a) {
  constexpr int UN = 4;
  const int lane = lane_id();
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= a.K * a.nslab) return;
  const int64_t k = w / a.nslab;
  const uint32_t c = (uint32_t)(w - k * a.nslab) * 64 + lane;
  const bool active = c < a.vpr;
  const uintptr_t zero = (uintptr_t)g_zero_piece;
  float acc[V] = {};
  // 64 sequences at a time, lane l resolving sequence b0 + l; then only the sequences that contribute are visited, in order
  for (int64_t b0 = 0; b0 < a.B; b0 += 64) {
    const bool in = b0 + lane < a.B;
    const int64_t b = in ? b0 + lane : 0;
    const int64_t s = a.offsets[b], e = a.offsets[b + 1];
    const int64_t t = clamp64(a.high[b], 0, a.K - 1);
    const bool fine = in && s >= 0 && e <= a.N;
    // rows below a sequence's tail map one to one: row s_b + k of every sequence that has it
    const uintptr_t row = fine && k < t && k < e - s ? a.in + (uintptr_t)(s + k) * a.in_stride : 0;
    unsigned long long hits = __ballot(row != 0);
    while (hits) {   // (wave-uniform)
      float x[UN][V];
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        const bool use = hits != 0;
        const uintptr_t ra = shfl_addr(row, use ? __builtin_ctzll(hits) : 0);
        hits &= hits - 1;
        Vec<DT, V>::ld(use && active ? ra + (uintptr_t)c * Vec<DT, V>::BYTES : zero, x[u]);
      }
#pragma unroll
      for (int u = 0; u < UN; ++u)
#pragma unroll
        for (int i = 0; i < V; ++i) acc[i] += x[u][i];
    }
    // the tails that fall on k, their partial rows in chunk order
    unsigned long long tails = __ballot(fine && t == k && e - s > t);
    while (tails) {
      const int r = __builtin_ctzll(tails);
      tails &= tails - 1;
      const int64_t first = (int64_t)shfl_addr((uintptr_t)(s + t), r), end = (int64_t)shfl_addr((uintptr_t)e, r);
      wave_sum_partials<V>(a.partial, a.D, first >> 6, (end - 1) >> 6, b0 + r, c, active, acc);
    }
  }
  if (active) Vec<TDT, V>::st(a.out + (uintptr_t)k * a.out_stride + (uintptr_t)c * Vec<TDT, V>::BYTES, acc);
}

// Chunk j of the sorted list: each run of equal keys k inside it is summed in list order into partial row j + k.  One wave per
// (chunk, 64 pieces of columns).
template <int DT, int V>
__global__ __launch_bounds__(256) void hstu_index_partials_kernel(const IdxArgs a) {
  const int lane = lane_id();
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t j = w / a.nslab;
  const int64_t p0 = j << a.chunk_log2;
  if (p0 >= a.count) return;
  const uint32_t c = (uint32_t)(w - j * a.nslab) * 64 + lane;
  const bool active = c < a.vpr;
  const int64_t left = a.count - p0;
  const int cnt = left < (1 << a.chunk_log2) ? (int)left : (1 << a.chunk_log2);
  const bool have = lane < cnt;
  const int64_t p = p0 + (have ? lane : 0);
  const int key = a.keys[p];
  const int64_t row = a.rows[p];
  const bool ok = have && row >= 0 && row < a.N;
  const uintptr_t addr = ok ? a.in + (uintptr_t)row * a.in_stride : 0;
  const int prev = __shfl_up(key, 1, 64);
  unsigned long long heads = __ballot(have && (lane == 0 || key != prev));
  while (heads) {   // (wave-uniform: one turn per run)
    const int r0 = __builtin_ctzll(heads);
    heads &= heads - 1;
    const int r1 = heads ? __builtin_ctzll(heads) : cnt;
    const int k = __shfl(key, r0, 64);
    if (k < 0 || k >= a.K) continue;
    float acc[V] = {};
    wave_sum_rows<DT, V>(addr, r0, r1, c, active, acc);
    if (active) Vec<kF32, V>::st(a.partial + ((uintptr_t)(j + k) * a.D + (uintptr_t)c * V) * 4, acc);
  }
}

// first i in [0, n] with keys[i] >= k (n if none), the 64 lanes probing 64 places of the range per step
__device__ __forceinline__ int64_t wave_lower_bound(const int32_t* keys, int64_t n, int64_t k) {
  const int lane = lane_id();
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t step = (hi - lo + 63) >> 6;
    const int64_t p = lo + lane * step;
    const bool less = p < hi && (int64_t)keys[p < hi ? p : lo] < k;
    const int cnt = __popcll(__ballot(less));
    if (cnt == 0) {
      hi = lo;
    } else {
      const int64_t nhi = lo + cnt * step;
      lo = lo + (cnt - 1) * step + 1;
      hi = nhi < hi ? nhi : hi;
    }
  }
  return lo;
}

template <int TDT, int V>
__global__ __launch_bounds__(256) void hstu_index_sum_kernel(const IdxArgs a) {
  const int lane = lane_id();
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= a.K * a.nslab) return;
  const int64_t k = w / a.nslab;
  const uint32_t c = (uint32_t)(w - k * a.nslab) * 64 + lane;
  const bool active = c < a.vpr;
  const int64_t lo = wave_lower_bound(a.keys, a.count, k), hi = wave_lower_bound(a.keys, a.count, k + 1);
  float acc[V] = {};
  if (hi > lo) wave_sum_partials<V>(a.partial, a.D, lo >> a.chunk_log2, (hi - 1) >> a.chunk_log2, k, c, active, acc);
  if (active) Vec<TDT, V>::st(a.out + (uintptr_t)k * a.out_stride + (uintptr_t)c * Vec<TDT, V>::BYTES, acc);
}

// most elements per access (8 / 4 / 2 / 1) that a buffer of `eb`-byte elements allows: base pointer and row stride
static inline int max_v(int v, const void* p, int64_t stride_bytes, int eb) {
  const uint64_t x = (uint64_t)(uintptr_t)p | (uint64_t)stride_bytes;
  while (v > 1 && (x % (uint64_t)(v * eb)) != 0) v >>= 1;
  return v;
}
static inline int max_v_of_d(int64_t D) { return D % 8 == 0 ? 8 : D % 4 == 0 ? 4 : D % 2 == 0 ? 2 : 1; }

// the reducing kernels give a lane one piece of a row: narrower pieces while a row would leave lanes of the wave idle
static inline int fill_lanes(int v, int64_t D) {
  while (v > 2 && D / v < 64) v >>= 1;
  return v;
}

}  // namespace mi355

using namespace mi355;

#define POS_SWITCH_V(v, ...)                                   \
  switch (v) {                                                 \
    case 8: { constexpr int V = 8; __VA_ARGS__; } break;       \
    case 4: { constexpr int V = 4; __VA_ARGS__; } break;       \
    case 2: { constexpr int V = 2; __VA_ARGS__; } break;       \
    default: { constexpr int V = 1; __VA_ARGS__; } break;      \
  }
#define POS_SWITCH_DT(dt, NAME, ...)                                    \
  switch (dt) {                                                         \
    case kF32: { constexpr int NAME = kF32; __VA_ARGS__; } break;       \
    case kBF16: { constexpr int NAME = kBF16; __VA_ARGS__; } break;     \
    default: { constexpr int NAME = kF16; __VA_ARGS__; } break;         \
  }
// the table is fp32 or has the dtype of the rows
#define POS_SWITCH_DT_TDT(dt, tdt, ...)                                                           \
  POS_SWITCH_DT(dt, DT, if ((tdt) == kF32) { constexpr int TDT = kF32; __VA_ARGS__; } else { constexpr int TDT = DT; __VA_ARGS__; })

#define POS_CHECK_COMMON(NAME, rows, D, dtype, tdtype, batch)                                                        \
  MI355_CHECK_ARG(D > 0 && D <= (int64_t)(1 << 22), NAME ": D must be in 1 .. 2^22");                                 \
  MI355_CHECK_ARG(elem_bytes(dtype) != 0, NAME ": unsupported dtype");                                               \
  MI355_CHECK_ARG(tdtype == kF32 || tdtype == dtype, NAME ": a table is fp32 or has the dtype of the rows");         \
  MI355_CHECK_ARG(rows >= 0 && rows < ((int64_t)1 << 36), NAME ": rows must be in 0 .. 2^36");                        \
  MI355_CHECK_ARG(batch >= 1 && batch < ((int64_t)1 << 31), NAME ": batch must be in 1 .. 2^31")

static inline bool aligned_to(const void* p, int64_t stride_elems, int eb) {
  return ((uintptr_t)p % eb) == 0 && stride_elems >= 0;
}

extern "C" int mi355_hstu_add_position_embeddings(const void* jagged, int64_t jagged_stride, int64_t rows, int64_t D, int dtype,
                                                  const int64_t* offsets, const int64_t* high_inds,
                                                  const int64_t* ind_offsets, int64_t batch, const void* dense,
                                                  int64_t dense_stride, int64_t K, int dense_dtype, float scale, void* out,
                                                  int64_t out_stride, hipStream_t stream) {
  POS_CHECK_COMMON("hstu_add_position_embeddings", rows, D, dtype, dense_dtype, batch);
  MI355_CHECK_ARG(offsets && high_inds, "hstu_add_position_embeddings: null offsets or high_inds");
  MI355_CHECK_ARG(dense && K >= 1, "hstu_add_position_embeddings: dense must hold at least one row");
  MI355_CHECK_ARG(jagged_stride >= D && out_stride >= D && dense_stride >= D,
                  "hstu_add_position_embeddings: a row stride is smaller than D");
  if (rows == 0) return MI355_OK;
  MI355_CHECK_ARG(jagged && out, "hstu_add_position_embeddings: null buffer with rows > 0");
  const int eb = elem_bytes(dtype), teb = elem_bytes(dense_dtype);
  MI355_CHECK_ARG(aligned_to(jagged, jagged_stride, eb) && aligned_to(out, out_stride, eb) && aligned_to(dense, dense_stride, teb),
                  "hstu_add_position_embeddings: a base pointer is not aligned to the element size");
  int v = max_v_of_d(D);
  v = max_v(v, jagged, jagged_stride * eb, eb);
  v = max_v(v, out, out_stride * eb, eb);
  v = max_v(v, dense, dense_stride * teb, teb);
  PosArgs a{};
  a.in = (uintptr_t)jagged; a.out = (uintptr_t)out; a.dense = (uintptr_t)dense;
  a.in_stride = jagged_stride * eb; a.out_stride = out_stride * eb; a.dense_stride = dense_stride * teb;
  a.offsets = offsets; a.high = high_inds; a.ind_off = ind_offsets;
  a.N = rows; a.B = batch; a.K = K; a.scale = scale;
  unsigned grid;
  if (const int rc = plan_run(rows, (uint64_t)D * eb, D / v, "hstu_add_position_embeddings", a.plan, grid)) return rc;
  POS_SWITCH_V(v, POS_SWITCH_DT_TDT(dtype, dense_dtype, hstu_pos_add_kernel<DT, TDT, V><<<dim3(grid), dim3(256), 0, stream>>>(a)));
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

extern "C" int64_t mi355_hstu_add_position_embeddings_bwd_workspace_bytes(int64_t rows, int64_t batch, int64_t D) {
  if (rows < 0 || batch < 0 || D <= 0) return 0;
  return (ceil_div(rows, 64) + batch) * D * 4;
}

extern "C" int mi355_hstu_add_position_embeddings_bwd(const void* d_out, int64_t d_out_stride, int64_t rows, int64_t D, int dtype,
                                                      const int64_t* offsets, const int64_t* high_inds, int64_t batch,
                                                      float scale, void* d_jagged, int64_t d_jagged_stride, void* d_dense,
                                                      int64_t d_dense_stride, int64_t K, int dense_dtype, void* workspace,
                                                      int64_t workspace_bytes, hipStream_t stream) {
  POS_CHECK_COMMON("hstu_add_position_embeddings_bwd", rows, D, dtype, dense_dtype, batch);
  MI355_CHECK_ARG(offsets && high_inds, "hstu_add_position_embeddings_bwd: null offsets or high_inds");
  MI355_CHECK_ARG(d_dense && K >= 1 && K < ((int64_t)1 << 31), "hstu_add_position_embeddings_bwd: d_dense must hold 1 .. 2^31 rows");
  MI355_CHECK_ARG(d_out_stride >= D && d_dense_stride >= D && (!d_jagged || d_jagged_stride >= D),
                  "hstu_add_position_embeddings_bwd: a row stride is smaller than D");
  MI355_CHECK_ARG(d_out || rows == 0, "hstu_add_position_embeddings_bwd: null d_out with rows > 0");
  MI355_CHECK_ARG(workspace && ((uintptr_t)workspace & 31) == 0 &&
                      workspace_bytes >= mi355_hstu_add_position_embeddings_bwd_workspace_bytes(rows, batch, D),
                  "hstu_add_position_embeddings_bwd: workspace is null, not 32-byte aligned or too small");
  const int eb = elem_bytes(dtype), teb = elem_bytes(dense_dtype);
  MI355_CHECK_ARG(aligned_to(d_out, d_out_stride, eb) && aligned_to(d_jagged, d_jagged_stride, eb) &&
                      aligned_to(d_dense, d_dense_stride, teb),
                  "hstu_add_position_embeddings_bwd: a base pointer is not aligned to the element size");
  if (d_jagged && rows > 0) {   // d_jagged = d_out * scale: the forward's kernel without a table
    int v = max_v_of_d(D);
    v = max_v(v, d_out, d_out_stride * eb, eb);
    v = max_v(v, d_jagged, d_jagged_stride * eb, eb);
    PosArgs s{};
    s.in = (uintptr_t)d_out; s.out = (uintptr_t)d_jagged; s.dense = 0;
    s.in_stride = d_out_stride * eb; s.out_stride = d_jagged_stride * eb; s.dense_stride = 0;
    s.offsets = offsets; s.high = high_inds; s.ind_off = nullptr;
    s.N = rows; s.B = batch; s.K = K; s.scale = scale;
    unsigned grid;
    if (const int rc = plan_run(rows, (uint64_t)D * eb, D / v, "hstu_add_position_embeddings_bwd", s.plan, grid)) return rc;
    POS_SWITCH_V(v, POS_SWITCH_DT(dtype, DT, hstu_pos_add_kernel<DT, DT, V><<<dim3(grid), dim3(256), 0, stream>>>(s)));
    MI355_LAUNCH_CHECK();
  }
  int v = max_v_of_d(D);
  v = max_v(v, d_out, d_out_stride * eb, eb);
  v = max_v(v, d_dense, d_dense_stride * teb, teb);
  v = fill_lanes(v, D);
  PosBwdArgs a{};
  a.in = (uintptr_t)d_out; a.out = (uintptr_t)d_dense; a.partial = (uintptr_t)workspace;
  a.in_stride = d_out_stride * eb; a.out_stride = d_dense_stride * teb;
  a.offsets = offsets; a.high = high_inds;
  a.N = rows; a.B = batch; a.K = K; a.D = D;
  a.vpr = (uint32_t)(D / v);
  a.nslab = (uint32_t)ceil_div(a.vpr, 64);
  if (rows > 0) {
    const unsigned grid = (unsigned)ceil_div(ceil_div(rows, 64), 4);
    POS_SWITCH_V(v, POS_SWITCH_DT(dtype, DT, hstu_pos_tail_partials_kernel<DT, V><<<dim3(grid), dim3(256), 0, stream>>>(a)));
    MI355_LAUNCH_CHECK();
  }
  const int64_t grid2 = ceil_div(K * a.nslab, 4);
  MI355_CHECK_ARG(grid2 < ((int64_t)1 << 31), "hstu_add_position_embeddings_bwd: K * D too large for one launch");
  POS_SWITCH_V(v, POS_SWITCH_DT_TDT(dtype, dense_dtype,
                                    hstu_pos_dense_grad_kernel<DT, TDT, V><<<dim3((unsigned)grid2), dim3(256), 0, stream>>>(a)));
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

extern "C" int mi355_hstu_add_timestamp_position_embeddings(
    const void* seq, int64_t seq_stride, int64_t rows, int64_t D, int dtype, const int64_t* offsets, const int64_t* lengths,
    int64_t batch, const void* pos_emb, int64_t pos_stride, int64_t Np, const void* ts_emb, int64_t ts_stride, int64_t Nt,
    int table_dtype, const int64_t* timestamps, const int64_t* num_targets, int interleave_targets,
    int64_t max_contextual_seq_len, int time_bucket_fn, int64_t num_time_buckets, float time_bucket_increments,
    float time_bucket_scale, int64_t time_delta, void* out, int64_t out_stride, int32_t* pos_inds, int32_t* ts_inds,
    hipStream_t stream) {
  POS_CHECK_COMMON("hstu_add_timestamp_position_embeddings", rows, D, dtype, table_dtype, batch);
  MI355_CHECK_ARG(offsets && lengths, "hstu_add_timestamp_position_embeddings: null offsets or lengths");
  MI355_CHECK_ARG(pos_emb && ts_emb && Np >= 1 && Nt >= 1 && Np < ((int64_t)1 << 31) && Nt < ((int64_t)1 << 31),
                  "hstu_add_timestamp_position_embeddings: each table must hold 1 .. 2^31 rows");
  MI355_CHECK_ARG(time_bucket_fn == 0 || time_bucket_fn == 1,
                  "hstu_add_timestamp_position_embeddings: time_bucket_fn must be 0 (sqrt) or 1 (log)");
  MI355_CHECK_ARG(num_time_buckets >= 0 && num_time_buckets < ((int64_t)1 << 31) && max_contextual_seq_len >= 0,
                  "hstu_add_timestamp_position_embeddings: num_time_buckets must be in 0 .. 2^31 and max_contextual_seq_len >= 0");
  MI355_CHECK_ARG(seq_stride >= D && out_stride >= D && pos_stride >= D && ts_stride >= D,
                  "hstu_add_timestamp_position_embeddings: a row stride is smaller than D");
  if (rows == 0) return MI355_OK;
  MI355_CHECK_ARG(seq && out && timestamps, "hstu_add_timestamp_position_embeddings: null buffer with rows > 0");
  const int eb = elem_bytes(dtype), teb = elem_bytes(table_dtype);
  MI355_CHECK_ARG(aligned_to(seq, seq_stride, eb) && aligned_to(out, out_stride, eb) && aligned_to(pos_emb, pos_stride, teb) &&
                      aligned_to(ts_emb, ts_stride, teb),
                  "hstu_add_timestamp_position_embeddings: a base pointer is not aligned to the element size");
  int v = max_v_of_d(D);
  v = max_v(v, seq, seq_stride * eb, eb);
  v = max_v(v, out, out_stride * eb, eb);
  v = max_v(v, pos_emb, pos_stride * teb, teb);
  v = max_v(v, ts_emb, ts_stride * teb, teb);
  TsArgs a{};
  a.in = (uintptr_t)seq; a.out = (uintptr_t)out; a.pos = (uintptr_t)pos_emb; a.ts = (uintptr_t)ts_emb;
  a.in_stride = seq_stride * eb; a.out_stride = out_stride * eb; a.pos_stride = pos_stride * teb; a.ts_stride = ts_stride * teb;
  a.offsets = offsets; a.lengths = lengths; a.num_targets = num_targets; a.timestamps = timestamps;
  a.pos_inds = pos_inds; a.ts_inds = ts_inds;
  a.N = rows; a.B = batch; a.Np = Np; a.Nt = Nt; a.mcsl = max_contextual_seq_len; a.ntb = num_time_buckets;
  a.time_delta = time_delta; a.incr = time_bucket_increments; a.tscale = time_bucket_scale;
  a.interleave = interleave_targets != 0; a.fn = time_bucket_fn;
  unsigned grid;
  if (const int rc = plan_run(rows, (uint64_t)D * eb, D / v, "hstu_add_timestamp_position_embeddings", a.plan, grid)) return rc;
  POS_SWITCH_V(v, POS_SWITCH_DT_TDT(dtype, table_dtype, hstu_ts_pos_add_kernel<DT, TDT, V><<<dim3(grid), dim3(256), 0, stream>>>(a)));
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

// entries per chunk of the sorted list: 64, or 32 while 64 would leave the chip short of waves
static inline int index_chunk_log2(int64_t count) { return ceil_div(count, 64) < 4096 ? 5 : 6; }

extern "C" int64_t mi355_hstu_index_rows_sum_workspace_bytes(int64_t count, int64_t K, int64_t D) {
  if (count < 0 || K < 0 || D <= 0) return 0;
  return (ceil_div(count, (int64_t)1 << index_chunk_log2(count)) + K) * D * 4;
}

extern "C" int mi355_hstu_index_rows_sum(const void* d_out, int64_t d_out_stride, int64_t rows, int64_t D, int dtype,
                                         const int32_t* sorted_keys, const int64_t* sorted_rows, int64_t count, void* d_table,
                                         int64_t table_stride, int64_t K, int table_dtype, void* workspace,
                                         int64_t workspace_bytes, hipStream_t stream) {
  POS_CHECK_COMMON("hstu_index_rows_sum", rows, D, dtype, table_dtype, (int64_t)1);
  MI355_CHECK_ARG(count >= 0 && count < ((int64_t)1 << 36), "hstu_index_rows_sum: count must be in 0 .. 2^36");
  MI355_CHECK_ARG(d_table && K >= 1 && K < ((int64_t)1 << 31) - 1, "hstu_index_rows_sum: d_table must hold 1 .. 2^31 - 2 rows");
  MI355_CHECK_ARG(d_out_stride >= D && table_stride >= D, "hstu_index_rows_sum: a row stride is smaller than D");
  MI355_CHECK_ARG((d_out && sorted_keys && sorted_rows) || count == 0, "hstu_index_rows_sum: null buffer with count > 0");
  MI355_CHECK_ARG(workspace && ((uintptr_t)workspace & 31) == 0 &&
                      workspace_bytes >= mi355_hstu_index_rows_sum_workspace_bytes(count, K, D),
                  "hstu_index_rows_sum: workspace is null, not 32-byte aligned or too small");
  const int eb = elem_bytes(dtype), teb = elem_bytes(table_dtype);
  MI355_CHECK_ARG(aligned_to(d_out, d_out_stride, eb) && aligned_to(d_table, table_stride, teb),
                  "hstu_index_rows_sum: a base pointer is not aligned to the element size");
  int v = max_v_of_d(D);
  v = max_v(v, d_out, d_out_stride * eb, eb);
  v = max_v(v, d_table, table_stride * teb, teb);
  v = fill_lanes(v, D);
  IdxArgs a{};
  a.in = (uintptr_t)d_out; a.out = (uintptr_t)d_table; a.partial = (uintptr_t)workspace;
  a.in_stride = d_out_stride * eb; a.out_stride = table_stride * teb;
  a.keys = sorted_keys; a.rows = sorted_rows;
  a.N = rows; a.count = count; a.K = K; a.D = D;
  a.vpr = (uint32_t)(D / v);
  a.nslab = (uint32_t)ceil_div(a.vpr, 64);
  a.chunk_log2 = index_chunk_log2(count);
  if (count > 0) {
    const unsigned grid = (unsigned)ceil_div(ceil_div(count, (int64_t)1 << a.chunk_log2) * a.nslab, 4);
    POS_SWITCH_V(v, POS_SWITCH_DT(dtype, DT, hstu_index_partials_kernel<DT, V><<<dim3(grid), dim3(256), 0, stream>>>(a)));
    MI355_LAUNCH_CHECK();
  }
  const int64_t grid2 = ceil_div(K * a.nslab, 4);
  MI355_CHECK_ARG(grid2 < ((int64_t)1 << 31), "hstu_index_rows_sum: K * D too large for one launch");
  POS_SWITCH_V(v, POS_SWITCH_DT(table_dtype, TDT, hstu_index_sum_kernel<TDT, V><<<dim3((unsigned)grid2), dim3(256), 0, stream>>>(a)));
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}
