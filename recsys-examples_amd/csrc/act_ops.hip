// HSTU activation kernels: SiLU forward, and SiLU backward fused with the bias gradient, over rows [rows, N].
//
// Replaces (reference, examples/hstu/ops/triton_ops): the SiLU epilogue of _addmm_optional_silu_fwd and triton_silu.py, and in
// triton_addmm_silu_bwd (triton_addmm.py:278-309) the pair aten.silu_backward + torch.sum(dz, 0), which reads dz from HBM again:
// four passes over a [rows, N] tensor there, three here.  Written for wave64 from the arithmetic.
//
// Values (all arithmetic fp32, every stored value rounded once):
//   s   = z / (1 + expf(-z))
//   sig = 1 / (1 + expf(-z));  dz = (g * sig) * (1 + z * (1 - sig));  dbias[c] = sum over rows of dz[., c] before its rounding
// expf(-z) may be +inf (z < -88.7): s and dz are then 0 with the sign the products give, never NaN for finite inputs.
//
// Layout of a call.  A thread owns one piece of V consecutive columns (V = 16 bytes' worth where N, every base pointer and every
// stride allow, else 1) and walks down rows; a wave owns 64 pieces, the four waves of a block own four consecutive rows of the same
// 64 pieces.  blockIdx.x is the column chunk, blockIdx.y the row group; the grid is resident: act_row_blocks(rows, N) row groups
// stride over the rows, four rows in flight per thread.  A thread keeps the fp32 column sums of its own rows in row order; a block folds its four waves in wave order through LDS into one workspace row, and hstu_silu_dbias_kernel sums the workspace rows
// of a column as 16 runs of consecutive blocks, each in block order, and the 16 runs in order.  No atomics.  The number of row
// groups is a function of (rows, N) alone, never of dtype or V, so dbias depends on (rows, N) and the values alone.
// In place (s == z, dz == g): a thread reads a piece before it writes the same piece, and no other thread touches it.
#include "common.h"
#include "vec_dev.h"
#include "../../include/recsys_amd.h"

namespace mi355 {

constexpr int kActRowsInFlight = 4;

struct ActArgs {
  uintptr_t g, z, o;                       // g: backward only; o: s or dz
  int64_t g_stride, z_stride, o_stride;    // bytes
  float* partial;                          // backward with dbias: [gridDim.y][N] fp32, else null
  int64_t rows, N;
};

__device__ __forceinline__ float act_sigmoid(float z) { return 1.f / (1.f + expf(-z)); }
__device__ __forceinline__ float act_silu(float z) { return z / (1.f + expf(-z)); }
__device__ __forceinline__ float act_silu_bwd(float g, float z) {
  const float sig = act_sigmoid(z);
  return __fmul_rn(__fmul_rn(g, sig), __fadd_rn(1.f, __fmul_rn(z, __fsub_rn(1.f, sig))));
}

template <int DT, int V, bool BWD>
__global__ __launch_bounds__(256) void hstu_silu_kernel(const ActArgs a) {
  constexpr uintptr_t EB = Vec<DT, V>::EB;
  constexpr int UN = kActRowsInFlight;
  __shared__ float s_fold[BWD ? 4 * 64 * V : 1];
  const int lane = lane_id(), wv = threadIdx.x >> 6;
  const int64_t c = ((int64_t)blockIdx.x * 64 + lane) * V;
  const bool active = c < a.N;
  const int64_t step = (int64_t)gridDim.y * 4;
  float acc[V];
#pragma unroll
  for (int e = 0; e < V; ++e) acc[e] = 0.f;
  if (active) {
    const uintptr_t co = (uintptr_t)c * EB;
    for (int64_t row = (int64_t)blockIdx.y * 4 + wv; row < a.rows; row += step * UN) {
      float z[UN][V], g[UN][V];
#pragma unroll
      for (int i = 0; i < UN; ++i) {
        const int64_t r = row + i * step;
        if (r < a.rows) {
          Vec<DT, V>::ld(a.z + (uintptr_t)r * a.z_stride + co, z[i]);
          if constexpr (BWD) Vec<DT, V>::ld(a.g + (uintptr_t)r * a.g_stride + co, g[i]);
        }
      }
#pragma unroll
      for (int i = 0; i < UN; ++i) {
        const int64_t r = row + i * step;
        if (r < a.rows) {
          float o[V];
#pragma unroll
          for (int e = 0; e < V; ++e) {
            if constexpr (BWD) {
              o[e] = act_silu_bwd(g[i][e], z[i][e]);
              acc[e] += o[e];
            } else {
              o[e] = act_silu(z[i][e]);
            }
          }
          Vec<DT, V>::st(a.o + (uintptr_t)r * a.o_stride + co, o);
        }
      }
    }
  }
  if constexpr (BWD) {
    if (a.partial == nullptr) return;
    // one workspace row per block: the four waves folded in wave order
#pragma unroll
    for (int e = 0; e < V; ++e) s_fold[wv * 64 * V + lane * V + e] = acc[e];
    __syncthreads();
    float* out = a.partial + (size_t)blockIdx.y * a.N;
    const int64_t c0 = (int64_t)blockIdx.x * 64 * V;
    for (int j = (int)threadIdx.x; j < 64 * V; j += 256) {
      if (c0 + j < a.N) out[c0 + j] = ((s_fold[j] + s_fold[64 * V + j]) + s_fold[2 * 64 * V + j]) + s_fold[3 * 64 * V + j];
    }
  }
}

// dbias of 64 columns: wave k of the 16 sums the partial rows [k chunk, (k + 1) chunk) in row order, then the 16 sums are added
// in wave order and rounded once (the pattern of hstu_norm_dwdb_kernel).  P 0 writes zeros.
template <int ODT>
__global__ __launch_bounds__(1024) void hstu_silu_dbias_kernel(const float* partial, int P, int64_t N, void* dbias) {
  constexpr int UN = 8;
  __shared__ float s[16][64];
  const int lane = lane_id(), wv = threadIdx.x >> 6;
  const int64_t c = (int64_t)blockIdx.x * 64 + lane;
  const bool active = c < N;
  const int chunk = (P + 15) / 16;
  const int r0 = wv * chunk, r1 = r0 + chunk < P ? r0 + chunk : P;
  float acc = 0.f;
  for (int r = r0; r < r1; r += UN) {
    float v[UN];
#pragma unroll
    for (int i = 0; i < UN; ++i) v[i] = active && r + i < r1 ? partial[(size_t)(r + i) * N + c] : 0.f;
#pragma unroll
    for (int i = 0; i < UN; ++i) acc += v[i];
  }
  s[wv][lane] = acc;
  __syncthreads();
  if (wv == 0 && active) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += s[k][lane];
    st1<ODT>(dbias, c, t);
  }
}

// row groups of the resident grid, also the number of workspace rows: about 2048 blocks in all when a chunk is 512 columns
// (16-byte pieces of a 16-bit dtype), at least 64 and at most 2048 row groups, never more than the rows need
static inline int act_row_blocks(int64_t rows, int64_t N) {
  int64_t cap = 2048 / ceil_div(N < 1 ? 1 : N, 512);
  cap = cap < 64 ? 64 : cap;
  const int64_t g = ceil_div(rows, 4);
  return (int)(g < 1 ? 1 : g > cap ? cap : g);
}

struct ActVec {
  int v;
  void need(const void* p, int64_t stride_bytes) {
    if ((((uint64_t)(uintptr_t)p | (uint64_t)stride_bytes) % 16) != 0) v = 1;
  }
};

}  // namespace mi355

using namespace mi355;

template <int DT, int V, bool BWD>
static void act_go(const ActArgs& a, int gy, hipStream_t stream) {
  const dim3 grid((unsigned)ceil_div(a.N, (int64_t)64 * V), (unsigned)gy);
  hstu_silu_kernel<DT, V, BWD><<<grid, dim3(256), 0, stream>>>(a);
}
// v: 16 bytes of the row dtype, or 1
template <bool BWD>
static void act_launch(int dtype, int v, const ActArgs& a, int gy, hipStream_t stream) {
  if (dtype == kF32) {
    if (v != 1) act_go<kF32, 4, BWD>(a, gy, stream);
    else act_go<kF32, 1, BWD>(a, gy, stream);
  } else if (dtype == kBF16) {
    if (v != 1) act_go<kBF16, 8, BWD>(a, gy, stream);
    else act_go<kBF16, 1, BWD>(a, gy, stream);
  } else {
    if (v != 1) act_go<kF16, 8, BWD>(a, gy, stream);
    else act_go<kF16, 1, BWD>(a, gy, stream);
  }
}

#define ACT_CHECK_COMMON(NAME, rows, N, dtype)                                                                        \
  MI355_CHECK_ARG(elem_bytes(dtype) != 0, NAME ": unsupported dtype");                                                \
  MI355_CHECK_ARG(rows >= 0 && rows < ((int64_t)1 << 31) && N >= 0 && N < ((int64_t)1 << 31),                         \
                  NAME ": rows and N must be in 0 .. 2^31")

// the stride of a call with one row is never used
static inline bool act_stride_ok(int64_t rows, int64_t N, int64_t stride) { return rows <= 1 || stride >= N; }
static inline bool act_aligned(const void* p, int eb) { return ((uintptr_t)p % eb) == 0; }

extern "C" int mi355_hstu_silu_fwd(const void* z, int64_t z_stride, int64_t rows, int64_t N, int dtype, void* s, int64_t s_stride,
                                   hipStream_t stream) {
  ACT_CHECK_COMMON("hstu_silu_fwd", rows, N, dtype);
  MI355_CHECK_ARG(act_stride_ok(rows, N, z_stride) && act_stride_ok(rows, N, s_stride),
                  "hstu_silu_fwd: a row stride is not positive or smaller than N");
  if (rows == 0 || N == 0) return MI355_OK;
  MI355_CHECK_ARG(z && s, "hstu_silu_fwd: null buffer with rows > 0");
  const int eb = elem_bytes(dtype);
  MI355_CHECK_ARG(act_aligned(z, eb) && act_aligned(s, eb), "hstu_silu_fwd: a base pointer is not aligned to the element size");
  if (rows == 1) z_stride = s_stride = N;
  ActVec av{N % (16 / eb) == 0 ? 16 / eb : 1};
  av.need(z, z_stride * eb); av.need(s, s_stride * eb);
  ActArgs a{};
  a.z = (uintptr_t)z; a.o = (uintptr_t)s; a.z_stride = z_stride * eb; a.o_stride = s_stride * eb; a.rows = rows; a.N = N;
  act_launch<false>(dtype, av.v, a, act_row_blocks(rows, N), stream);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

extern "C" int64_t mi355_hstu_silu_bwd_workspace_bytes(int64_t rows, int64_t N) {
  if (rows < 0 || N < 0 || N >= ((int64_t)1 << 31)) return 0;
  const int64_t b = (int64_t)act_row_blocks(rows, N) * N * 4;
  return b < 16 ? 16 : b;
}

extern "C" int mi355_hstu_silu_bwd(const void* g, int64_t g_stride, const void* z, int64_t z_stride, int64_t rows, int64_t N,
                                   int dtype, void* dz, int64_t dz_stride, void* dbias, int dbias_dtype, void* workspace,
                                   int64_t workspace_bytes, hipStream_t stream) {
  ACT_CHECK_COMMON("hstu_silu_bwd", rows, N, dtype);
  MI355_CHECK_ARG(act_stride_ok(rows, N, g_stride) && act_stride_ok(rows, N, z_stride) && act_stride_ok(rows, N, dz_stride),
                  "hstu_silu_bwd: a row stride is not positive or smaller than N");
  const bool sum = dbias != nullptr;
  MI355_CHECK_ARG(!sum || dbias_dtype == kF32 || dbias_dtype == dtype, "hstu_silu_bwd: dbias is fp32 or has the dtype of the rows");
  MI355_CHECK_ARG(!sum || (workspace && ((uintptr_t)workspace & 15) == 0 &&
                           workspace_bytes >= mi355_hstu_silu_bwd_workspace_bytes(rows, N)),
                  "hstu_silu_bwd: workspace is null, not 16-byte aligned or too small");
  if (N == 0) return MI355_OK;
  const bool run = rows > 0;
  MI355_CHECK_ARG(!run || (g && z && dz), "hstu_silu_bwd: null buffer with rows > 0");
  const int eb = elem_bytes(dtype);
  MI355_CHECK_ARG(act_aligned(g, eb) && act_aligned(z, eb) && act_aligned(dz, eb) && (!sum || act_aligned(dbias, elem_bytes(dbias_dtype))),
                  "hstu_silu_bwd: a base pointer is not aligned to the element size");
  if (rows <= 1) g_stride = z_stride = dz_stride = N;
  const int gy = act_row_blocks(rows, N);
  if (run) {
    ActVec av{N % (16 / eb) == 0 ? 16 / eb : 1};
    av.need(g, g_stride * eb); av.need(z, z_stride * eb); av.need(dz, dz_stride * eb);
    ActArgs a{};
    a.g = (uintptr_t)g; a.z = (uintptr_t)z; a.o = (uintptr_t)dz;
    a.g_stride = g_stride * eb; a.z_stride = z_stride * eb; a.o_stride = dz_stride * eb;
    a.partial = sum ? (float*)workspace : nullptr; a.rows = rows; a.N = N;
    act_launch<true>(dtype, av.v, a, gy, stream);
    MI355_LAUNCH_CHECK();
  }
  if (sum) {
    const dim3 grid((unsigned)ceil_div(N, 64));
    const float* partial = (const float*)workspace;
    const int P = run ? gy : 0;
    if (dbias_dtype == kF32) hstu_silu_dbias_kernel<kF32><<<grid, dim3(1024), 0, stream>>>(partial, P, N, dbias);
    else if (dbias_dtype == kBF16) hstu_silu_dbias_kernel<kBF16><<<grid, dim3(1024), 0, stream>>>(partial, P, N, dbias);
    else hstu_silu_dbias_kernel<kF16><<<grid, dim3(1024), 0, stream>>>(partial, P, N, dbias);
    MI355_LAUNCH_CHECK();
  }
  return MI355_OK;
}
