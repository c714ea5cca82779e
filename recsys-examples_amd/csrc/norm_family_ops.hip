// HSTU swish layer norm and RMS norm over rows [N, D], forward and backward.
//
// Replaces (reference, examples/hstu/ops/triton_ops/triton_layer_norm.py): SwishLayerNormFunction (:763-877, the IS_SWISH
// branches of _weighted_layer_norm_fwd and _weighted_layer_norm_bwd_dx, :229-253) and RMSNormFunction with
// _weighted_rms_norm_fwd / _weighted_rms_norm_bwd_dx / _rms_norm_bwd_dwdb (:537-760).  Written for wave64 from the arithmetic.
//
// Values (all arithmetic fp32, every stored value rounded once):
//   swish:  mean, rstd, xh, ln = fmaf(xh, w, b) as in norm_ops.hip;  s = 1 / (1 + expf(-ln)) (act_ops.hip's sigmoid);  y = s * x
//           backward: q = ((dy * x) * s) * (1 - s);  g = w * q;  c1 = sum(xh * g) / D;  c2 = sum(g) / D;
//           dx = (g - (xh * c1 + c2)) * rstd + dy * s;  dw = sum over rows of q * xh;  db = sum over rows of q
//   rms:    rstd = 1 / sqrtf(sum(x^2) / D + eps);  xh = x * rstd;  y = xh * w
//           backward: g = w * dy;  c1 = sum(xh * g) / D;  dx = (g - xh * c1) * rstd;  dw = sum over rows of dy * xh
//
// Layout of a call: that of norm_ops.hip.  A thread keeps CAP elements of a row in registers as pieces of V elements (16 bytes'
// worth where D, every base pointer and every stride allow, else 1); D <= 2048: a wave owns a row, four waves a block;
// D > 2048: a workgroup owns a row and sums go through LDS.  Resident grids stride over the rows with w and b in registers.
// The backward keeps fp32 dw / db partials per thread, writes one workspace row per block and hstu_norm_dwdb_kernel
// (norm_dev.h) folds them in a fixed order.  No atomics: the result depends on (N, D) alone.
#include "norm_dev.h"
#include "../../include/recsys_amd.h"

namespace mi355 {

struct FamArgs {
  uintptr_t x, y, w, b, dy, dx;
  int64_t x_stride, y_stride, dy_stride, dx_stride;   // bytes
  float* mean;
  float* rstd;
  float* partial;      // backward: [2][gridDim.x][D] fp32 (rms: [1][gridDim.x][D])
  int64_t N;
  int D;
  float eps;
  int w_f32;
};

__device__ __forceinline__ float fam_sigmoid(float z) { return 1.f / (1.f + expf(-z)); }

template <int DT, int V, int CAP, bool BLOCK, bool RMS>
__global__ __launch_bounds__(256) void hstu_normfam_fwd_kernel(const FamArgs a) {
  constexpr int NP = CAP / V, T = BLOCK ? 256 : 64;
  constexpr uintptr_t EB = Vec<DT, V>::EB;
  __shared__ float s_red[16];
  const int tid = BLOCK ? (int)threadIdx.x : lane_id();
  const int64_t row0 = BLOCK ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t step = BLOCK ? (int64_t)gridDim.x : (int64_t)gridDim.x * 4;
  const float fD = (float)a.D;
  float w[NP][V], b[NP][V];
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    const int c = (tid + k * T) * V;
#pragma unroll
    for (int e = 0; e < V; ++e) { w[k][e] = 1.f; b[k][e] = 0.f; }
    if (c < a.D) {
      ld_param<DT, V>(a.w, c, a.w_f32, w[k]);
      if constexpr (!RMS) ld_param<DT, V>(a.b, c, a.w_f32, b[k]);
    }
  }
  int slot = 0;
  for (int64_t row = row0; row < a.N; row += step) {
    float x[NP][V];
    const uintptr_t xr = a.x + (uintptr_t)row * a.x_stride;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      const int c = (tid + k * T) * V;
#pragma unroll
      for (int e = 0; e < V; ++e) x[k][e] = 0.f;
      if (c < a.D) Vec<DT, V>::ld(xr + (uintptr_t)c * EB, x[k]);
    }
    float mean = 0.f, q[1] = {0.f};
    if constexpr (RMS) {
#pragma unroll
      for (int k = 0; k < NP; ++k)
#pragma unroll
        for (int e = 0; e < V; ++e) q[0] = __fmaf_rn(x[k][e], x[k][e], q[0]);   // (the padding holds zeros)
    } else {
      float s[1] = {0.f};
#pragma unroll
      for (int k = 0; k < NP; ++k)
#pragma unroll
        for (int e = 0; e < V; ++e) s[0] += x[k][e];
      row_sum<BLOCK, 1>(s, s_red, slot);
      slot ^= 1;
      mean = s[0] / fD;
#pragma unroll
      for (int k = 0; k < NP; ++k) {
        if ((tid + k * T) * V < a.D) {
#pragma unroll
          for (int e = 0; e < V; ++e) {
            const float d = x[k][e] - mean;
            q[0] = __fmaf_rn(d, d, q[0]);
          }
        }
      }
    }
    row_sum<BLOCK, 1>(q, s_red, slot);
    slot ^= 1;
    const float rstd = 1.f / sqrtf(q[0] / fD + a.eps);
    if (tid == 0) {
      if constexpr (!RMS) a.mean[row] = mean;
      a.rstd[row] = rstd;
    }
    const uintptr_t yr = a.y + (uintptr_t)row * a.y_stride;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      const int c = (tid + k * T) * V;
      if (c < a.D) {
        float o[V];
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const float xh = norm_xh(x[k][e], mean, rstd);
          if constexpr (RMS) o[e] = __fmul_rn(xh, w[k][e]);
          else o[e] = __fmul_rn(fam_sigmoid(norm_ln(xh, w[k][e], b[k][e])), x[k][e]);
        }
        Vec<DT, V>::st(yr + (uintptr_t)c * EB, o);
      }
    }
  }
}

template <int DT, int V, int CAP, bool BLOCK, bool RMS>
__global__ __launch_bounds__(256) void hstu_normfam_bwd_kernel(const FamArgs a) {
  constexpr int NP = CAP / V, T = BLOCK ? 256 : 64;
  constexpr uintptr_t EB = Vec<DT, V>::EB;
  __shared__ float s_red[16];
  __shared__ float s_fold[BLOCK ? 1 : 4 * kNormWaveMaxD];
  const int tid = BLOCK ? (int)threadIdx.x : lane_id();
  const int wv = threadIdx.x >> 6;
  const int64_t row0 = BLOCK ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * 4 + wv;
  const int64_t step = BLOCK ? (int64_t)gridDim.x : (int64_t)gridDim.x * 4;
  const float fD = (float)a.D;
  float w[NP][V], b[NP][V], dwp[NP][V], dbp[NP][V];
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    const int c = (tid + k * T) * V;
#pragma unroll
    for (int e = 0; e < V; ++e) { w[k][e] = 1.f; b[k][e] = 0.f; dwp[k][e] = 0.f; dbp[k][e] = 0.f; }
    if (c < a.D) {
      ld_param<DT, V>(a.w, c, a.w_f32, w[k]);
      if constexpr (!RMS) ld_param<DT, V>(a.b, c, a.w_f32, b[k]);
    }
  }
  int slot = 0;
  for (int64_t row = row0; row < a.N; row += step) {
    float x[NP][V], g[NP][V], ds[NP][V];   // ds: dy * s (swish)
    const uintptr_t xr = a.x + (uintptr_t)row * a.x_stride, dyr = a.dy + (uintptr_t)row * a.dy_stride;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      const int c = (tid + k * T) * V;
#pragma unroll
      for (int e = 0; e < V; ++e) { x[k][e] = 0.f; g[k][e] = 0.f; ds[k][e] = 0.f; }
      if (c < a.D) {
        Vec<DT, V>::ld(xr + (uintptr_t)c * EB, x[k]);
        Vec<DT, V>::ld(dyr + (uintptr_t)c * EB, g[k]);
      }
    }
    const float mean = RMS ? 0.f : a.mean[row], rstd = a.rstd[row];
    float sums[2] = {0.f, 0.f};   // sum(xh g), sum(g)
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      const int c = (tid + k * T) * V;
      if (c < a.D) {
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const float xh = norm_xh(x[k][e], mean, rstd);
          float gp = g[k][e];
          if constexpr (!RMS) {
            const float s = fam_sigmoid(norm_ln(xh, w[k][e], b[k][e]));
            ds[k][e] = __fmul_rn(gp, s);
            gp = __fmul_rn(__fmul_rn(__fmul_rn(gp, x[k][e]), s), 1.f - s);   // q, the gradient that reaches ln
            dbp[k][e] += gp;
          }
          dwp[k][e] = __fmaf_rn(gp, xh, dwp[k][e]);
          const float gg = w[k][e] * gp;
          g[k][e] = gg;
          sums[0] = __fmaf_rn(xh, gg, sums[0]);
          if constexpr (!RMS) sums[1] += gg;
        }
      }
    }
    if constexpr (RMS) {
      float s1[1] = {sums[0]};
      row_sum<BLOCK, 1>(s1, s_red, slot);
      sums[0] = s1[0];
    } else {
      row_sum<BLOCK, 2>(sums, s_red, slot);
    }
    slot ^= 1;
    const float c1 = sums[0] / fD, c2 = sums[1] / fD;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      const int c = (tid + k * T) * V;
      if (c < a.D) {
        float o[V];
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const float xh = norm_xh(x[k][e], mean, rstd);
          if constexpr (RMS) o[e] = (g[k][e] - __fmul_rn(xh, c1)) * rstd;
          else o[e] = (g[k][e] - __fmaf_rn(xh, c1, c2)) * rstd + ds[k][e];
        }
        Vec<DT, V>::st(a.dx + (uintptr_t)row * a.dx_stride + (uintptr_t)c * EB, o);
      }
    }
  }
  // one workspace row per block: a thread's own columns (BLOCK), or the four waves folded in wave order through LDS
  float* pw = a.partial + (size_t)blockIdx.x * a.D;
  float* pb = pw + (size_t)gridDim.x * a.D;
  if constexpr (BLOCK) {
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      const int c = (tid + k * T) * V;
      if (c < a.D) {
#pragma unroll
        for (int e = 0; e < V; ++e) {
          pw[c + e] = dwp[k][e];
          if constexpr (!RMS) pb[c + e] = dbp[k][e];
        }
      }
    }
  } else {
#pragma unroll
    for (int pass = 0; pass < (RMS ? 1 : 2); ++pass) {
#pragma unroll
      for (int k = 0; k < NP; ++k) {
        const int c = (tid + k * T) * V;
        if (c < a.D) {
#pragma unroll
          for (int e = 0; e < V; ++e) s_fold[wv * kNormWaveMaxD + c + e] = pass == 0 ? dwp[k][e] : dbp[k][e];
        }
      }
      __syncthreads();
      float* out = pass == 0 ? pw : pb;
      for (int c = (int)threadIdx.x; c < a.D; c += 256)
        out[c] = ((s_fold[c] + s_fold[kNormWaveMaxD + c]) + s_fold[2 * kNormWaveMaxD + c]) + s_fold[3 * kNormWaveMaxD + c];
      __syncthreads();
    }
  }
}

// blocks of the resident grids (those of norm_ops.hip); the backward's is also the number of workspace rows
static inline int fam_fwd_blocks(int64_t rows, int64_t D) {
  const int64_t g = D <= kNormWaveMaxD ? ceil_div(rows, 4) : rows;
  return (int)(g < 1 ? 1 : g > 2048 ? 2048 : g);
}
static inline int fam_bwd_blocks(int64_t rows, int64_t D) {
  const int64_t g = D <= kNormWaveMaxD ? ceil_div(rows, 4) : rows, cap = D <= kNormWaveMaxD ? 512 : 1024;
  return (int)(g < 1 ? 1 : g > cap ? cap : g);
}

}  // namespace mi355

using namespace mi355;

template <int DT, int V, int CAP, bool BLOCK, bool RMS, bool BWD>
static void fam_go(int grid, const FamArgs& a, hipStream_t stream) {
  if constexpr (BWD) hstu_normfam_bwd_kernel<DT, V, CAP, BLOCK, RMS><<<dim3(grid), dim3(256), 0, stream>>>(a);
  else hstu_normfam_fwd_kernel<DT, V, CAP, BLOCK, RMS><<<dim3(grid), dim3(256), 0, stream>>>(a);
}
// the elements a thread holds, by D; the element-wise path V = 1 always holds 32
template <int DT, int V, bool RMS, bool BWD>
static void fam_launch_cap(int grid, const FamArgs& a, hipStream_t stream) {
  const bool wave = a.D <= kNormWaveMaxD;
  if constexpr (V == 1) {
    if (wave) fam_go<DT, 1, 32, false, RMS, BWD>(grid, a, stream);
    else fam_go<DT, 1, 32, true, RMS, BWD>(grid, a, stream);
  } else {
    if (a.D <= 512) fam_go<DT, V, 8, false, RMS, BWD>(grid, a, stream);
    else if (a.D <= 1024) fam_go<DT, V, 16, false, RMS, BWD>(grid, a, stream);
    else if (wave) fam_go<DT, V, 32, false, RMS, BWD>(grid, a, stream);
    else if (a.D <= 4096) fam_go<DT, V, 16, true, RMS, BWD>(grid, a, stream);
    else fam_go<DT, V, 32, true, RMS, BWD>(grid, a, stream);
  }
}
template <bool RMS, bool BWD>
static void fam_launch(int dtype, int v, int grid, const FamArgs& a, hipStream_t stream) {
  if (dtype == kF32) {
    if (v != 1) fam_launch_cap<kF32, 4, RMS, BWD>(grid, a, stream);
    else fam_launch_cap<kF32, 1, RMS, BWD>(grid, a, stream);
  } else if (dtype == kBF16) {
    if (v != 1) fam_launch_cap<kBF16, 8, RMS, BWD>(grid, a, stream);
    else fam_launch_cap<kBF16, 1, RMS, BWD>(grid, a, stream);
  } else {
    if (v != 1) fam_launch_cap<kF16, 8, RMS, BWD>(grid, a, stream);
    else fam_launch_cap<kF16, 1, RMS, BWD>(grid, a, stream);
  }
}

#define FAM_CHECK_COMMON(NAME, rows, D, dtype, wdtype)                                                      \
  MI355_CHECK_ARG(D > 0 && D <= kNormMaxD, NAME ": D must be in 1 .. 8192");                                \
  MI355_CHECK_ARG(norm_ebytes(dtype) != 0, NAME ": unsupported dtype");                                     \
  MI355_CHECK_ARG(wdtype == kF32 || wdtype == dtype, NAME ": weights are fp32 or have the dtype of the rows"); \
  MI355_CHECK_ARG(rows >= 0 && rows < ((int64_t)1 << 31), NAME ": rows must be in 0 .. 2^31")

// dw (and db) from `blocks` workspace rows; blocks 0 writes zeros
static int fam_dwdb(const FamArgs& a, int blocks, int wdtype, void* dweight, void* dbias, hipStream_t stream) {
  const dim3 grid((unsigned)ceil_div(a.D, 64), dbias ? 2 : 1);
  if (wdtype == kF32) hstu_norm_dwdb_kernel<kF32><<<grid, dim3(1024), 0, stream>>>(a.partial, blocks, a.D, dweight, dbias);
  else if (wdtype == kBF16) hstu_norm_dwdb_kernel<kBF16><<<grid, dim3(1024), 0, stream>>>(a.partial, blocks, a.D, dweight, dbias);
  else hstu_norm_dwdb_kernel<kF16><<<grid, dim3(1024), 0, stream>>>(a.partial, blocks, a.D, dweight, dbias);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

template <bool RMS>
static int fam_fwd(const void* x, int64_t x_stride, int64_t rows, int64_t D, int dtype, const void* weight,
                   const void* bias, int weight_dtype, float eps, void* y, int64_t y_stride, float* mean, float* rstd,
                   hipStream_t stream) {
  const int eb = norm_ebytes(dtype);
  NormVec nv{D % (16 / eb) == 0 ? 16 / eb : 1};
  nv.need(x, x_stride * eb); nv.need(y, y_stride * eb); nv.need(weight, 0); nv.need(bias, 0);
  FamArgs a{};
  a.x = (uintptr_t)x; a.y = (uintptr_t)y; a.w = (uintptr_t)weight; a.b = (uintptr_t)bias;
  a.x_stride = x_stride * eb; a.y_stride = y_stride * eb;
  a.mean = mean; a.rstd = rstd; a.N = rows; a.D = (int)D; a.eps = eps; a.w_f32 = weight_dtype == kF32;
  fam_launch<RMS, false>(dtype, nv.v, fam_fwd_blocks(rows, D), a, stream);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

template <bool RMS>
static int fam_bwd(const void* dy, int64_t dy_stride, const void* x, int64_t x_stride, int64_t rows, int64_t D, int dtype,
                   const void* weight, const void* bias, int weight_dtype, const float* mean, const float* rstd, void* dx,
                   int64_t dx_stride, void* dweight, void* dbias, void* workspace, hipStream_t stream) {
  const int eb = norm_ebytes(dtype);
  NormVec nv{D % (16 / eb) == 0 ? 16 / eb : 1};
  nv.need(dy, dy_stride * eb); nv.need(x, x_stride * eb); nv.need(dx, dx_stride * eb); nv.need(weight, 0); nv.need(bias, 0);
  FamArgs a{};
  a.dy = (uintptr_t)dy; a.x = (uintptr_t)x; a.dx = (uintptr_t)dx; a.w = (uintptr_t)weight; a.b = (uintptr_t)bias;
  a.dy_stride = dy_stride * eb; a.x_stride = x_stride * eb; a.dx_stride = dx_stride * eb;
  a.mean = const_cast<float*>(mean); a.rstd = const_cast<float*>(rstd); a.partial = (float*)workspace;
  a.N = rows; a.D = (int)D; a.w_f32 = weight_dtype == kF32;
  const int grid = fam_bwd_blocks(rows, D);
  if (rows > 0) {
    fam_launch<RMS, true>(dtype, nv.v, grid, a, stream);
    MI355_LAUNCH_CHECK();
  }
  return fam_dwdb(a, rows > 0 ? grid : 0, weight_dtype, dweight, dbias, stream);
}

extern "C" int mi355_hstu_swish_layer_norm_fwd(const void* x, int64_t x_stride, int64_t rows, int64_t D, int dtype,
                                               const void* weight, const void* bias, int weight_dtype, float eps, void* y,
                                               int64_t y_stride, float* mean, float* rstd, hipStream_t stream) {
  FAM_CHECK_COMMON("hstu_swish_layer_norm_fwd", rows, D, dtype, weight_dtype);
  MI355_CHECK_ARG(x_stride >= D && y_stride >= D, "hstu_swish_layer_norm_fwd: a row stride is smaller than D");
  if (rows == 0) return MI355_OK;
  MI355_CHECK_ARG(x && y && weight && bias && mean && rstd, "hstu_swish_layer_norm_fwd: null buffer with rows > 0");
  const int eb = norm_ebytes(dtype), web = norm_ebytes(weight_dtype);
  MI355_CHECK_ARG(norm_aligned(x, eb) && norm_aligned(y, eb) && norm_aligned(weight, web) && norm_aligned(bias, web),
                  "hstu_swish_layer_norm_fwd: a base pointer is not aligned to the element size");
  return fam_fwd<false>(x, x_stride, rows, D, dtype, weight, bias, weight_dtype, eps, y, y_stride, mean, rstd, stream);
}

extern "C" int64_t mi355_hstu_swish_layer_norm_bwd_workspace_bytes(int64_t rows, int64_t D) {
  if (rows < 0 || D <= 0 || D > kNormMaxD) return 0;
  return (int64_t)2 * fam_bwd_blocks(rows, D) * D * 4;
}
extern "C" int64_t mi355_hstu_rms_norm_bwd_workspace_bytes(int64_t rows, int64_t D) {
  if (rows < 0 || D <= 0 || D > kNormMaxD) return 0;
  return (int64_t)fam_bwd_blocks(rows, D) * D * 4;
}

extern "C" int mi355_hstu_swish_layer_norm_bwd(const void* dy, int64_t dy_stride, const void* x, int64_t x_stride, int64_t rows,
                                               int64_t D, int dtype, const void* weight, const void* bias, int weight_dtype,
                                               const float* mean, const float* rstd, void* dx, int64_t dx_stride, void* dweight,
                                               void* dbias, void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  FAM_CHECK_COMMON("hstu_swish_layer_norm_bwd", rows, D, dtype, weight_dtype);
  MI355_CHECK_ARG(dy_stride >= D && x_stride >= D && dx_stride >= D, "hstu_swish_layer_norm_bwd: a row stride is smaller than D");
  MI355_CHECK_ARG(dweight && dbias && (rows == 0 || (dy && x && dx && weight && bias && mean && rstd)),
                  "hstu_swish_layer_norm_bwd: null buffer (dweight and dbias are needed for rows == 0 too)");
  MI355_CHECK_ARG(rows == 0 || (workspace && ((uintptr_t)workspace & 15) == 0 &&
                                workspace_bytes >= mi355_hstu_swish_layer_norm_bwd_workspace_bytes(rows, D)),
                  "hstu_swish_layer_norm_bwd: workspace is null, not 16-byte aligned or too small");
  const int eb = norm_ebytes(dtype), web = norm_ebytes(weight_dtype);
  MI355_CHECK_ARG(norm_aligned(dy, eb) && norm_aligned(x, eb) && norm_aligned(dx, eb) && norm_aligned(weight, web) &&
                      norm_aligned(bias, web) && norm_aligned(dweight, web) && norm_aligned(dbias, web),
                  "hstu_swish_layer_norm_bwd: a base pointer is not aligned to the element size");
  return fam_bwd<false>(dy, dy_stride, x, x_stride, rows, D, dtype, weight, bias, weight_dtype, mean, rstd, dx, dx_stride,
                        dweight, dbias, workspace, stream);
}

extern "C" int mi355_hstu_rms_norm_fwd(const void* x, int64_t x_stride, int64_t rows, int64_t D, int dtype, const void* weight,
                                       int weight_dtype, float eps, void* y, int64_t y_stride, float* rstd, hipStream_t stream) {
  FAM_CHECK_COMMON("hstu_rms_norm_fwd", rows, D, dtype, weight_dtype);
  MI355_CHECK_ARG(x_stride >= D && y_stride >= D, "hstu_rms_norm_fwd: a row stride is smaller than D");
  if (rows == 0) return MI355_OK;
  MI355_CHECK_ARG(x && y && weight && rstd, "hstu_rms_norm_fwd: null buffer with rows > 0");
  const int eb = norm_ebytes(dtype), web = norm_ebytes(weight_dtype);
  MI355_CHECK_ARG(norm_aligned(x, eb) && norm_aligned(y, eb) && norm_aligned(weight, web),
                  "hstu_rms_norm_fwd: a base pointer is not aligned to the element size");
  return fam_fwd<true>(x, x_stride, rows, D, dtype, weight, nullptr, weight_dtype, eps, y, y_stride, nullptr, rstd, stream);
}

extern "C" int mi355_hstu_rms_norm_bwd(const void* dy, int64_t dy_stride, const void* x, int64_t x_stride, int64_t rows, int64_t D,
                                       int dtype, const void* weight, int weight_dtype, const float* rstd, void* dx,
                                       int64_t dx_stride, void* dweight, void* workspace, int64_t workspace_bytes,
                                       hipStream_t stream) {
  FAM_CHECK_COMMON("hstu_rms_norm_bwd", rows, D, dtype, weight_dtype);
  MI355_CHECK_ARG(dy_stride >= D && x_stride >= D && dx_stride >= D, "hstu_rms_norm_bwd: a row stride is smaller than D");
  MI355_CHECK_ARG(dweight && (rows == 0 || (dy && x && dx && weight && rstd)),
                  "hstu_rms_norm_bwd: null buffer (dweight is needed for rows == 0 too)");
  MI355_CHECK_ARG(rows == 0 || (workspace && ((uintptr_t)workspace & 15) == 0 &&
                                workspace_bytes >= mi355_hstu_rms_norm_bwd_workspace_bytes(rows, D)),
                  "hstu_rms_norm_bwd: workspace is null, not 16-byte aligned or too small");
  const int eb = norm_ebytes(dtype), web = norm_ebytes(weight_dtype);
  MI355_CHECK_ARG(norm_aligned(dy, eb) && norm_aligned(x, eb) && norm_aligned(dx, eb) && norm_aligned(weight, web) &&
                      norm_aligned(dweight, web),
                  "hstu_rms_norm_bwd: a base pointer is not aligned to the element size");
  return fam_bwd<true>(dy, dy_stride, x, x_stride, rows, D, dtype, weight, nullptr, weight_dtype, nullptr, rstd, dx, dx_stride,
                       dweight, nullptr, workspace, stream);
}
