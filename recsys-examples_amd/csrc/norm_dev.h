// The row-kernel skeleton of the HSTU norms (norm_ops.hip, norm_family_ops.hip, group_norm_ops.hip).
//   leaves:    the DPP wave sum, the row sum through LDS, the Philox draw of the dropout masks, parameter loads;
//   skeleton:  RowPieces (which thread holds which piece of which rows), row_mean_rstd, mul_store_y (the mul-dropout forward's
//              stores, for a weight per element (layer norm) or per head (group norm));
//   kernels:   hstu_norm_fwd_kernel / hstu_norm_bwd_kernel for the four per-row kinds (norm_ops.hip instantiates layer norm and
//              LN-mul-dropout, norm_family_ops.hip swish and RMS) and hstu_norm_dwdb_kernel, which folds the dw / db partial rows;
//   host:      the grid size (norm_row_blocks, also the workspace row count), the dispatch ladder dtype -> V -> CAP / BLOCK
//              (norm_dispatch), norm_launch_dwdb, norm_set_dropout, NORM_CHECK_COMMON.
// The group norm's fast kernels keep bodies of their own (per-head statistics) on RowPieces and mul_store_y.
// The guarded loads, the mul-dropout backward head and the dw / db epilogue are written out in the kernels and NOT helpers: the
// backward leaves some product-sums to the compiler's contraction (db += gp, sum(g) += w gp, (..) * rstd + extra), and with those
// three behind function boundaries hipcc fused them differently in seven instantiations (last bits of dx and db moved) and
// took more registers or scratch in nine.  Written in this order every output bit and every kernel's resources are those of the
// kernels before they were merged.
//
// Layout of a call.  A thread keeps CAP elements of a row in registers, as pieces of V elements (V = 16 bytes' worth where
// D, every base pointer and every stride allow, else 1); piece i of the row belongs to thread i mod T.
//   D <= 2048: a wave owns a row (T = 64), CAP = 8 / 16 / 32 for D <= 512 / 1024 / 2048 (V = 1: always 32), four waves a block;
//   D >  2048: a workgroup owns a row (T = 256), CAP = 16 / 32 for D <= 4096 / 8192 (V = 1: always 32), sums through LDS.
// Both run a resident grid that strides over the rows with w and b held in registers.  The backward keeps fp32 dw / db partials
// per thread, folds a block's four waves in wave order through LDS and writes one workspace row per block; hstu_norm_dwdb_kernel
// then sums the rows of a column as 16 runs of consecutive blocks, each in block order, and the 16 runs in order.  No atomics.
#pragma once
#include "common.h"
#include "init_dev.h"
#include "vec_dev.h"

namespace mi355 {

constexpr int kNormMaxD = 8192;
constexpr int kNormWaveMaxD = 2048;

// sum over the 64 lanes, the same value in every lane (row_shr 1 / 2 / 4 / 8, row_bcast 15 / 31: wave_incl_scan of scan_dev.h)
#define NORM_DPP(v, ctrl, rows) \
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), ctrl, rows, 0xf, false))
__device__ __forceinline__ float wave_sum_f32(float v) {
  NORM_DPP(v, 0x111, 0xf);
  NORM_DPP(v, 0x112, 0xf);
  NORM_DPP(v, 0x114, 0xf);
  NORM_DPP(v, 0x118, 0xf);
  NORM_DPP(v, 0x142, 0xa);
  NORM_DPP(v, 0x143, 0xc);
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// sums of K values over the threads that share a row, the same in every thread; s_red [2][K][4], `slot` alternates
// between consecutive calls so that one barrier a call is enough
template <bool BLOCK, int K>
__device__ __forceinline__ void row_sum(float (&v)[K], float* s_red, int slot) {
#pragma unroll
  for (int i = 0; i < K; ++i) v[i] = wave_sum_f32(v[i]);
  if constexpr (BLOCK) {
    const int wv = threadIdx.x >> 6;
    float* s = s_red + slot * 8;
    if (lane_id() == 0) {
#pragma unroll
      for (int i = 0; i < K; ++i) s[4 * i + wv] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < K; ++i) v[i] = ((s[4 * i] + s[4 * i + 1]) + s[4 * i + 2]) + s[4 * i + 3];
  }
}

// the dropout of a call (the definition of the stream: norm_ops.hip)
struct NormDropout {
  float den;           // 1 - p
  uint32_t thr, seed_lo, seed_hi;
  int drop;
};

// the draw of one element; not inlined: the element-wise kernels hold 32 elements a thread, and 32 generators expanded in
// line and interleaved by the scheduler spill thousands of bytes a lane
static __device__ __noinline__ uint32_t philox_draw1(uint32_t rl, uint32_t rh, uint32_t c, uint32_t which, uint32_t k0, uint32_t k1) {
  const uint4 r = philox4x32(make_uint4(rl, rh, c >> 2, which), make_uint2(k0, k1));
  return (c & 3) == 0 ? r.x : (c & 3) == 1 ? r.y : (c & 3) == 2 ? r.z : r.w;
}

// the keep / scale of V elements from column c of `row` under mask `which`
template <int V>
__device__ __forceinline__ void drop_apply(const NormDropout& a, int64_t row, int c, uint32_t which, float (&v)[V]) {
  const uint2 key = make_uint2(a.seed_lo, a.seed_hi);
  const uint32_t rl = (uint32_t)row, rh = (uint32_t)((uint64_t)row >> 32);
  if constexpr (V == 1) {
    const uint32_t d = philox_draw1(rl, rh, (uint32_t)c, which, key.x, key.y);
    v[0] = d >= a.thr ? v[0] / a.den : 0.f;
  } else {
#pragma unroll
    for (int q = 0; q < V / 4; ++q) {
      const uint4 r = philox4x32(make_uint4(rl, rh, ((uint32_t)c >> 2) + q, which), key);
      v[4 * q + 0] = r.x >= a.thr ? v[4 * q + 0] / a.den : 0.f;
      v[4 * q + 1] = r.y >= a.thr ? v[4 * q + 1] / a.den : 0.f;
      v[4 * q + 2] = r.z >= a.thr ? v[4 * q + 2] / a.den : 0.f;
      v[4 * q + 3] = r.w >= a.thr ? v[4 * q + 3] / a.den : 0.f;
    }
  }
}

// V elements of weight / bias from column c: fp32 or the dtype of the rows
template <int DT, int V>
__device__ __forceinline__ void ld_param(uintptr_t p, int c, int f32, float (&f)[V]) {
  if (f32) Vec<kF32, V>::ld(p + (uintptr_t)c * 4, f);
  else Vec<DT, V>::ld(p + (uintptr_t)c * Vec<DT, V>::EB, f);
}

__device__ __forceinline__ float norm_xh(float x, float mean, float rstd) { return __fmul_rn(__fsub_rn(x, mean), rstd); }
__device__ __forceinline__ float norm_ln(float xh, float w, float b) { return __fmaf_rn(xh, w, b); }
__device__ __forceinline__ float norm_sigmoid(float z) { return 1.f / (1.f + expf(-z)); }

// ---- the skeleton ----
// Which pieces of which rows a thread holds: piece k of its NP is piece (tid + k T) of the row, column col(k); its rows are
// row0, row0 + step, ...
template <int V, int CAP, bool BLOCK>
struct RowPieces {
  static constexpr int NP = CAP / V, T = BLOCK ? 256 : 64;
  int tid, wv;
  int64_t row0, step;
  __device__ __forceinline__ RowPieces()
      : tid(BLOCK ? (int)threadIdx.x : lane_id()), wv(threadIdx.x >> 6),
        row0(BLOCK ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)),
        step(BLOCK ? (int64_t)gridDim.x : (int64_t)gridDim.x * 4) {}
  __device__ __forceinline__ int piece(int k) const { return tid + k * T; }
  __device__ __forceinline__ int col(int k) const { return (tid + k * T) * V; }
};

// mean (0: RMS) and rstd of the row held in x (zeros past D): the sum, / D, then the squared differences of the live columns
template <bool RMS, int V, int CAP, bool BLOCK>
__device__ __forceinline__ void row_mean_rstd(const RowPieces<V, CAP, BLOCK>& p, const float (&x)[CAP / V][V], int D, float eps,
                                              float* s_red, int& slot, float& mean, float& rstd) {
  constexpr int NP = CAP / V;
  const float fD = (float)D;
  float q[1] = {0.f};
  if constexpr (RMS) {
    mean = 0.f;
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
      if (p.col(k) < D) {
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
  rstd = 1.f / sqrtf(q[0] / fD + eps);
}

// ---- the mul-dropout piece code; w and b are V values (layer norm) or one (group norm: a piece lies in one head) ----
__device__ __forceinline__ float norm_par(float w, int) { return w; }
template <int V>
__device__ __forceinline__ float norm_par(const float (&w)[V], int e) { return w[e]; }

// The forward's stores of one piece (also the backward's compute_y): drop(ln * u), or the three parts.  A: the argument
// block, a NormDropout with y, y_stride, D and concat.
template <int DT, int V, class A, class W>
__device__ __forceinline__ void mul_store_y(const A& a, int64_t row, int c, const float (&x)[V], const float (&u)[V], const W& w,
                                            const W& b, float mean, float rstd) {
  constexpr uintptr_t EB = Vec<DT, V>::EB;
  const uintptr_t yr = a.y + (uintptr_t)row * a.y_stride + (uintptr_t)c * EB;
  float t[V];
#pragma unroll
  for (int e = 0; e < V; ++e) t[e] = __fmul_rn(norm_ln(norm_xh(x[e], mean, rstd), norm_par(w, e), norm_par(b, e)), u[e]);
  if (a.concat) {
    float p0[V], p1[V];
#pragma unroll
    for (int e = 0; e < V; ++e) { p0[e] = u[e]; p1[e] = x[e]; }
    if (a.drop) {
      drop_apply<V>(a, row, c, 0u, p0);
      drop_apply<V>(a, row, c, 1u, p1);
      drop_apply<V>(a, row, c, 2u, t);
    }
    Vec<DT, V>::st(yr, p0);
    Vec<DT, V>::st(yr + (uintptr_t)a.D * EB, p1);
    Vec<DT, V>::st(yr + (uintptr_t)a.D * 2 * EB, t);
    return;
  }
  if (a.drop) drop_apply<V>(a, row, c, 0u, t);
  Vec<DT, V>::st(yr, t);
}

// ---- the kernels of the four per-row norms ----
enum NormKind { kNormLayer, kNormLnMul, kNormSwish, kNormRms };

struct NormArgs : NormDropout {
  uintptr_t x, u, y, w, b, dy, dx, du, extra;         // extra: dx_accumulate (layer norm); y 0: not written
  int64_t x_stride, u_s0, u_s1, y_stride, dy_stride, dx_stride, du_s0, du_s1, extra_stride;   // bytes
  float* mean;
  float* rstd;
  float* partial;      // backward: [2][gridDim.x][D] fp32 (RMS: [1][gridDim.x][D])
  int64_t N;
  int D, UD;
  float eps;
  int w_f32, learnable, stats_given, concat;
};

// Swish and RMS always have their weight and always compute the statistics: learnable and stats_given are not read.
template <int DT, int V, int CAP, bool BLOCK, int KIND>
__global__ __launch_bounds__(256) void hstu_norm_fwd_kernel(const NormArgs a) {
  constexpr int NP = CAP / V;
  constexpr bool MUL = KIND == kNormLnMul, RMS = KIND == kNormRms, FAM = KIND == kNormSwish || RMS;
  constexpr uintptr_t EB = Vec<DT, V>::EB;
  __shared__ float s_red[16];
  const RowPieces<V, CAP, BLOCK> p;
  float w[NP][V], b[NP][V];
  uint32_t uo[NP];
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    const int c = p.col(k);
#pragma unroll
    for (int e = 0; e < V; ++e) { w[k][e] = 1.f; b[k][e] = 0.f; }
    uo[k] = 0;
    if (c < a.D) {
      if (FAM || a.learnable) {
        ld_param<DT, V>(a.w, c, a.w_f32, w[k]);
        if constexpr (!RMS) ld_param<DT, V>(a.b, c, a.w_f32, b[k]);
      }
      if constexpr (MUL) {
        const int h = c / a.UD;
        uo[k] = (uint32_t)((int64_t)h * a.u_s1 + (int64_t)(c - h * a.UD) * (int64_t)EB);
      }
    }
  }
  int slot = 0;
  for (int64_t row = p.row0; row < a.N; row += p.step) {
    float x[NP][V], u[NP][V];
    const uintptr_t xr = a.x + (uintptr_t)row * a.x_stride, ur = a.u + (uintptr_t)row * a.u_s0;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      const int c = p.col(k);
#pragma unroll
      for (int e = 0; e < V; ++e) { x[k][e] = 0.f; u[k][e] = 0.f; }
      if (c < a.D) {
        Vec<DT, V>::ld(xr + (uintptr_t)c * EB, x[k]);
        if constexpr (MUL) Vec<DT, V>::ld(ur + uo[k], u[k]);
      }
    }
    float mean, rstd;
    if (!FAM && a.stats_given) {
      mean = a.mean[row];
      rstd = a.rstd[row];
    } else {
      row_mean_rstd<RMS>(p, x, a.D, a.eps, s_red, slot, mean, rstd);
      if (p.tid == 0) {
        if constexpr (!RMS) a.mean[row] = mean;
        a.rstd[row] = rstd;
      }
    }
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      const int c = p.col(k);
      if (c < a.D) {
        if constexpr (MUL) {
          mul_store_y<DT, V>(a, row, c, x[k], u[k], w[k], b[k], mean, rstd);
        } else {
          float o[V];
#pragma unroll
          for (int e = 0; e < V; ++e) {
            const float xh = norm_xh(x[k][e], mean, rstd);
            if constexpr (RMS) o[e] = __fmul_rn(xh, w[k][e]);
            else if constexpr (FAM) o[e] = __fmul_rn(norm_sigmoid(norm_ln(xh, w[k][e], b[k][e])), x[k][e]);
            else o[e] = norm_ln(xh, w[k][e], b[k][e]);
          }
          Vec<DT, V>::st(a.y + (uintptr_t)row * a.y_stride + (uintptr_t)c * EB, o);
        }
      }
    }
  }
}

// gp, the gradient that reaches ln: dy (layer norm, RMS), dt u (LN-mul-dropout), ((dy x) s) (1 - s) (swish).  ex, what is
// added to dx: dx_accumulate, the x part of a concat_ux dy, dy s; RMS adds nothing and has neither db nor c2.
template <int DT, int V, int CAP, bool BLOCK, int KIND>
__global__ __launch_bounds__(256) void hstu_norm_bwd_kernel(const NormArgs a) {
  constexpr int NP = CAP / V, NS = KIND == kNormRms ? 1 : 2;
  constexpr bool MUL = KIND == kNormLnMul, SWISH = KIND == kNormSwish, RMS = KIND == kNormRms, FAM = SWISH || RMS;
  constexpr uintptr_t EB = Vec<DT, V>::EB;
  __shared__ float s_red[16];
  __shared__ float s_fold[BLOCK ? 1 : 4 * kNormWaveMaxD];
  const RowPieces<V, CAP, BLOCK> p;
  const float fD = (float)a.D;
  float w[NP][V], b[NP][V], dwp[NP][V], dbp[NP][V];
  uint32_t uo[NP], duo[NP];
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    const int c = p.col(k);
#pragma unroll
    for (int e = 0; e < V; ++e) { w[k][e] = 1.f; b[k][e] = 0.f; dwp[k][e] = 0.f; dbp[k][e] = 0.f; }
    uo[k] = duo[k] = 0;
    if (c < a.D) {
      if (FAM || a.learnable) {
        ld_param<DT, V>(a.w, c, a.w_f32, w[k]);
        if constexpr (MUL || SWISH) ld_param<DT, V>(a.b, c, a.w_f32, b[k]);
      }
      if constexpr (MUL) {
        const int h = c / a.UD;
        uo[k] = (uint32_t)((int64_t)h * a.u_s1 + (int64_t)(c - h * a.UD) * (int64_t)EB);
        duo[k] = (uint32_t)((int64_t)h * a.du_s1 + (int64_t)(c - h * a.UD) * (int64_t)EB);
      }
    }
  }
  const bool cat = MUL && a.concat;
  const bool have_extra = MUL ? cat : !FAM && a.extra != 0;
  int slot = 0;
  for (int64_t row = p.row0; row < a.N; row += p.step) {
    float x[NP][V], g[NP][V], u[NP][V], ex[NP][V];
    const uintptr_t xr = a.x + (uintptr_t)row * a.x_stride, ur = a.u + (uintptr_t)row * a.u_s0;
    const uintptr_t dyr = a.dy + (uintptr_t)row * a.dy_stride;
    const uintptr_t exr = MUL ? dyr + (uintptr_t)a.D * EB : a.extra + (uintptr_t)row * a.extra_stride;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      const int c = p.col(k);
#pragma unroll
      for (int e = 0; e < V; ++e) { x[k][e] = 0.f; g[k][e] = 0.f; u[k][e] = 0.f; ex[k][e] = 0.f; }
      if (c < a.D) {
        Vec<DT, V>::ld(xr + (uintptr_t)c * EB, x[k]);
        Vec<DT, V>::ld(dyr + (uintptr_t)(cat ? 2 * a.D + c : c) * EB, g[k]);
        if constexpr (MUL) Vec<DT, V>::ld(ur + uo[k], u[k]);
        if (have_extra) Vec<DT, V>::ld(exr + (uintptr_t)c * EB, ex[k]);
      }
    }
    const float mean = RMS ? 0.f : a.mean[row], rstd = a.rstd[row];
    float sums[NS] = {};   // sum(xh g), sum(g)
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      const int c = p.col(k);
      if (c < a.D) {
        if constexpr (MUL) {   // y again, the masks, du stored; g: dy_t in, gp = dt u out; ex: dy_x in, dropped out
          if (a.y) mul_store_y<DT, V>(a, row, c, x[k], u[k], w[k], b[k], mean, rstd);
          if (a.drop) {
            drop_apply<V>(a, row, c, cat ? 2u : 0u, g[k]);   // dt
            if (cat) drop_apply<V>(a, row, c, 1u, ex[k]);
          }
          float duv[V];
          if (cat) {
            Vec<DT, V>::ld(dyr + (uintptr_t)c * EB, duv);
            if (a.drop) drop_apply<V>(a, row, c, 0u, duv);
          } else {
#pragma unroll
            for (int e = 0; e < V; ++e) duv[e] = 0.f;
          }
#pragma unroll
          for (int e = 0; e < V; ++e) {
            const float ln = norm_ln(norm_xh(x[k][e], mean, rstd), w[k][e], b[k][e]);
            duv[e] = __fmaf_rn(g[k][e], ln, duv[e]);
            g[k][e] *= u[k][e];   // the gradient that reaches ln
          }
          Vec<DT, V>::st(a.du + (uintptr_t)row * a.du_s0 + duo[k], duv);
        }
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const float xh = norm_xh(x[k][e], mean, rstd);
          float gp = g[k][e];
          if constexpr (SWISH) {
            const float s = norm_sigmoid(norm_ln(xh, w[k][e], b[k][e]));
            ex[k][e] = __fmul_rn(gp, s);
            gp = __fmul_rn(__fmul_rn(__fmul_rn(gp, x[k][e]), s), 1.f - s);
            dbp[k][e] += gp;   // (here and not below: the place it had before the kinds were merged; fp16 CAP 8 wave rows 95 -> 93)
          }
          dwp[k][e] = __fmaf_rn(gp, xh, dwp[k][e]);
          if constexpr (!FAM) dbp[k][e] += gp;
          const float gg = w[k][e] * gp;
          g[k][e] = gg;
          sums[0] = __fmaf_rn(xh, gg, sums[0]);
          if constexpr (!RMS) sums[NS - 1] += gg;
        }
      }
    }
    row_sum<BLOCK, NS>(sums, s_red, slot);
    slot ^= 1;
    const float c1 = sums[0] / fD, c2 = sums[NS - 1] / fD;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      const int c = p.col(k);
      if (c < a.D) {
        float o[V];
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const float xh = norm_xh(x[k][e], mean, rstd);
          if constexpr (RMS) o[e] = (g[k][e] - __fmul_rn(xh, c1)) * rstd;
          else o[e] = (g[k][e] - __fmaf_rn(xh, c1, c2)) * rstd + ex[k][e];
        }
        Vec<DT, V>::st(a.dx + (uintptr_t)row * a.dx_stride + (uintptr_t)c * EB, o);
      }
    }
  }
  if (!FAM && !a.learnable) return;
  // one workspace row per block: a thread's own columns (BLOCK), or the four waves folded in wave order through LDS
  float* pw = a.partial + (size_t)blockIdx.x * a.D;
  float* pb = pw + (size_t)gridDim.x * a.D;
  if constexpr (BLOCK) {
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      const int c = p.col(k);
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
    for (int pass = 0; pass < NS; ++pass) {
#pragma unroll
      for (int k = 0; k < NP; ++k) {
        const int c = p.col(k);
        if (c < a.D) {
#pragma unroll
          for (int e = 0; e < V; ++e) s_fold[p.wv * kNormWaveMaxD + c + e] = pass == 0 ? dwp[k][e] : dbp[k][e];
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

// dw (blockIdx.y 0) and db (1) of 64 columns: wave k of the 16 sums the partial rows [k chunk, (k + 1) chunk) in row order,
// then the 16 sums are added in wave order and rounded once.  P 0 writes zeros.
template <int ODT>
__global__ __launch_bounds__(1024) void hstu_norm_dwdb_kernel(const float* partial, int P, int D, void* dw, void* db) {
  constexpr int UN = 8;
  __shared__ float s[16][64];
  const int lane = lane_id(), wv = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  const bool active = c < D;
  const float* src = partial + (size_t)blockIdx.y * P * D;
  const int chunk = (P + 15) / 16;
  const int r0 = wv * chunk, r1 = r0 + chunk < P ? r0 + chunk : P;
  float acc = 0.f;
  for (int r = r0; r < r1; r += UN) {
    float v[UN];
#pragma unroll
    for (int i = 0; i < UN; ++i) v[i] = active && r + i < r1 ? src[(size_t)(r + i) * D + c] : 0.f;
#pragma unroll
    for (int i = 0; i < UN; ++i) acc += v[i];
  }
  s[wv][lane] = acc;
  __syncthreads();
  if (wv == 0 && active) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += s[k][lane];
    st1<ODT>(blockIdx.y == 0 ? dw : db, c, t);
  }
}

// ---- host ----
// the elements of one access: 16 bytes' worth, or 1 as soon as a base pointer or a stride is not a multiple of 16 bytes
struct NormVec {
  int v;
  void need(const void* p, int64_t stride_bytes) {
    if ((((uint64_t)(uintptr_t)p | (uint64_t)stride_bytes) % 16) != 0) v = 1;
  }
};

static inline bool norm_aligned(const void* p, int eb) { return ((uintptr_t)p % eb) == 0; }

// blocks of the resident grid of a row kernel; the backward's is also the number of workspace rows that the
// *_workspace_bytes entry points promise
static inline int norm_row_blocks(int64_t rows, int64_t D, bool backward) {
  const bool wave = D <= kNormWaveMaxD;
  const int64_t g = wave ? ceil_div(rows, 4) : rows, cap = !backward ? 2048 : wave ? 512 : 1024;
  return (int)(g < 1 ? 1 : g > cap ? cap : g);
}

// The ladder: f(NormShape<DT, V, CAP, BLOCK>{}) for the dtype, v (16 bytes' worth of it, or 1) and D of a call.  CAP by D
// (header comment); the element-wise path V = 1 always holds 32 and exists only WITH_V1.
template <int DT_, int V_, int CAP_, bool BLOCK_>
struct NormShape {
  static constexpr int DT = DT_, V = V_, CAP = CAP_;
  static constexpr bool BLOCK = BLOCK_;
};
template <int DT, int V, bool WITH_V1, class F>
static void norm_dispatch_cap(int v, int D, F&& f) {
  const bool wave = D <= kNormWaveMaxD;
  if constexpr (WITH_V1) {
    if (v == 1) {
      if (wave) f(NormShape<DT, 1, 32, false>{});
      else f(NormShape<DT, 1, 32, true>{});
      return;
    }
  }
  if (D <= 512) f(NormShape<DT, V, 8, false>{});
  else if (D <= 1024) f(NormShape<DT, V, 16, false>{});
  else if (wave) f(NormShape<DT, V, 32, false>{});
  else if (D <= 4096) f(NormShape<DT, V, 16, true>{});
  else f(NormShape<DT, V, 32, true>{});
}
template <bool WITH_V1 = true, class F>
static void norm_dispatch(int dtype, int v, int D, F&& f) {
  if (dtype == kF32) norm_dispatch_cap<kF32, 4, WITH_V1>(v, D, f);
  else if (dtype == kBF16) norm_dispatch_cap<kBF16, 8, WITH_V1>(v, D, f);
  else norm_dispatch_cap<kF16, 8, WITH_V1>(v, D, f);
}

// hstu_norm_fwd_kernel / hstu_norm_bwd_kernel of one kind over `grid` blocks
template <int KIND, bool BWD>
static void norm_launch(int dtype, int v, int grid, const NormArgs& a, hipStream_t stream) {
  norm_dispatch(dtype, v, a.D, [&](auto s) {
    using S = decltype(s);
    if constexpr (BWD) hstu_norm_bwd_kernel<S::DT, S::V, S::CAP, S::BLOCK, KIND><<<dim3(grid), dim3(256), 0, stream>>>(a);
    else hstu_norm_fwd_kernel<S::DT, S::V, S::CAP, S::BLOCK, KIND><<<dim3(grid), dim3(256), 0, stream>>>(a);
  });
}

// dw (and db, where given) from `partial_rows` workspace rows of `columns`; partial_rows 0 writes zeros
static inline int norm_launch_dwdb(const float* partial, int partial_rows, int columns, int wdtype, void* dw, void* db,
                                   hipStream_t stream) {
  const dim3 grid((unsigned)ceil_div(columns, 64), db ? 2 : 1);
  if (wdtype == kF32) hstu_norm_dwdb_kernel<kF32><<<grid, dim3(1024), 0, stream>>>(partial, partial_rows, columns, dw, db);
  else if (wdtype == kBF16) hstu_norm_dwdb_kernel<kBF16><<<grid, dim3(1024), 0, stream>>>(partial, partial_rows, columns, dw, db);
  else hstu_norm_dwdb_kernel<kF16><<<grid, dim3(1024), 0, stream>>>(partial, partial_rows, columns, dw, db);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

static inline void norm_set_dropout(NormDropout& a, double p, int training, uint64_t seed) {
  a.thr = (uint32_t)(uint64_t)(p * 4294967296.0);   // floor(p 2^32), p in [0, 1)
  a.den = 1.0f - (float)p;
  a.drop = training != 0 && a.thr > 0;
  a.seed_lo = (uint32_t)seed;
  a.seed_hi = (uint32_t)(seed >> 32);
}

// WEIGHTS: how the message names them, "weight and bias are" or "weights are"
#define NORM_CHECK_COMMON(NAME, rows, D, dtype, wdtype, WEIGHTS)                                             \
  MI355_CHECK_ARG(D > 0 && D <= kNormMaxD, NAME ": D must be in 1 .. 8192");                                 \
  MI355_CHECK_ARG(elem_bytes(dtype) != 0, NAME ": unsupported dtype");                                       \
  MI355_CHECK_ARG(wdtype == kF32 || wdtype == dtype, NAME ": " WEIGHTS " fp32 or have the dtype of the rows"); \
  MI355_CHECK_ARG(rows >= 0 && rows < ((int64_t)1 << 31), NAME ": rows must be in 0 .. 2^31")

}  // namespace mi355
