// HSTU layer norms: layer norm and layer-norm-mul-dropout over rows [N, D], forward and backward.
//
// Replaces (reference, examples/hstu/ops/triton_ops): _layer_norm_fwd / _weighted_layer_norm_fwd and their backwards
// (triton_layer_norm.py:313-481), _ln_mul_dropout_fwd and _ln_mul_dropout_bwd_dx_du / _dwdb (triton_norm_mul_dropout.py:36-525).
// Written for wave64 from the arithmetic; the reference is Triton.
//
// Values (all arithmetic fp32, every stored value rounded once):
//   mean = sum(x) / D;  var = sum((x - mean)^2) / D from the registers that hold the row;  rstd = 1 / sqrtf(var + eps)
//   xh = (x - mean) * rstd;  ln = fmaf(xh, w, b)  (w = 1, b = 0: not learnable);  t = ln * u
//   backward, gp the gradient that reaches ln (dy, or dt * u):  g = w * gp;  c1 = sum(xh * g) / D;  c2 = sum(g) / D;
//   dx = (g - (xh * c1 + c2)) * rstd (+ extra);  dw = sum over rows of gp * xh;  db = sum over rows of gp
//
// Dropout (this project's definition; Triton's tl.rand stream is not reproduced).  Element (row, col) of mask `which`
// (0 / 1 / 2 = the u / x / t part of a concat_ux output; 0 without concat_ux) takes one 32-bit draw r of Philox4x32-10
// (init_dev.h) with
//   key     = (seed & 0xffffffff, seed >> 32)
//   counter = (row & 0xffffffff, row >> 32, col >> 2, which)
//   r       = word (col & 3) of the four output words, in the order x, y, z, w
// and is kept iff r >= floor(p * 2^32) as unsigned integers; a kept value is v / (1.0f - (float)p) (IEEE division), a
// dropped one +0.  The mask is a function of (seed, row, col, which, p) alone.
//
// Layout of a call.  A thread keeps CAP elements of a row in registers, as pieces of V elements (V = 16 bytes' worth where
// D, every base pointer and every stride allow, else 1); piece i of the row belongs to thread i mod T.
//   D <= 2048: a wave owns a row (T = 64), CAP = 8 / 16 / 32 for D <= 512 / 1024 / 2048 (V = 1: always 32), four waves a block;
//   D >  2048: a workgroup owns a row (T = 256), CAP = 16 / 32 for D <= 4096 / 8192 (V = 1: always 32), sums through LDS.
// Both run a resident grid that strides over the rows with w and b held in registers.  Wave sums are the DPP pattern of
// scan_dev.h on floats.  The backward keeps fp32 dw / db partials per thread, folds a block's four waves in wave order
// through LDS and writes one workspace row per block; hstu_norm_dwdb_kernel then sums the rows of a column as 16 runs of
// consecutive blocks, each in block order, and the 16 runs in order.  No atomics: the result depends on (N, D) alone.
#include "norm_dev.h"
#include "../../include/recsys_amd.h"

namespace mi355 {

struct NormArgs {
  uintptr_t x, u, y, w, b, dy, dx, du, extra;         // extra: dx_accumulate (layer norm); y 0: not written
  int64_t x_stride, u_s0, u_s1, y_stride, dy_stride, dx_stride, du_s0, du_s1, extra_stride;   // bytes
  float* mean;
  float* rstd;
  float* partial;      // backward: [2][gridDim.x][D] fp32
  int64_t N;
  int D, UD;
  float eps, den;      // den = 1 - p
  uint32_t thr, seed_lo, seed_hi;
  int w_f32, learnable, stats_given, drop, concat;
};

// The forward's stores of one piece (also the backward's compute_y): y = ln (layer norm), drop(ln * u), or the three parts
template <int DT, int V, bool MUL>
__device__ __forceinline__ void store_y(const NormArgs& a, int64_t row, int c, const float (&x)[V], const float (&u)[V],
                                        const float (&w)[V], const float (&b)[V], float mean, float rstd) {
  constexpr uintptr_t EB = Vec<DT, V>::EB;
  const uintptr_t yr = a.y + (uintptr_t)row * a.y_stride + (uintptr_t)c * EB;
  float t[V];
#pragma unroll
  for (int e = 0; e < V; ++e) {
    const float ln = norm_ln(norm_xh(x[e], mean, rstd), w[e], b[e]);
    t[e] = MUL ? __fmul_rn(ln, u[e]) : ln;
  }
  if constexpr (MUL) {
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
  }
  Vec<DT, V>::st(yr, t);
}

template <int DT, int V, int CAP, bool BLOCK, bool MUL>
__global__ __launch_bounds__(256) void hstu_norm_fwd_kernel(const NormArgs a) {
  constexpr int NP = CAP / V, T = BLOCK ? 256 : 64;
  constexpr uintptr_t EB = Vec<DT, V>::EB;
  __shared__ float s_red[16];
  const int tid = BLOCK ? (int)threadIdx.x : lane_id();
  const int64_t row0 = BLOCK ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t step = BLOCK ? (int64_t)gridDim.x : (int64_t)gridDim.x * 4;
  const float fD = (float)a.D;
  float w[NP][V], b[NP][V];
  uint32_t uo[NP];
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    const int c = (tid + k * T) * V;
#pragma unroll
    for (int e = 0; e < V; ++e) { w[k][e] = 1.f; b[k][e] = 0.f; }
    uo[k] = 0;
    if (c < a.D) {
      if (a.learnable) {
        ld_param<DT, V>(a.w, c, a.w_f32, w[k]);
        ld_param<DT, V>(a.b, c, a.w_f32, b[k]);
      }
      if constexpr (MUL) {
        const int h = c / a.UD;
        uo[k] = (uint32_t)((int64_t)h * a.u_s1 + (int64_t)(c - h * a.UD) * (int64_t)EB);
      }
    }
  }
  int slot = 0;
  for (int64_t row = row0; row < a.N; row += step) {
    float x[NP][V], u[NP][V];
    const uintptr_t xr = a.x + (uintptr_t)row * a.x_stride, ur = a.u + (uintptr_t)row * a.u_s0;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      const int c = (tid + k * T) * V;
#pragma unroll
      for (int e = 0; e < V; ++e) { x[k][e] = 0.f; u[k][e] = 0.f; }
      if (c < a.D) {
        Vec<DT, V>::ld(xr + (uintptr_t)c * EB, x[k]);
        if constexpr (MUL) Vec<DT, V>::ld(ur + uo[k], u[k]);
      }
    }
    float mean, rstd;
    if (a.stats_given) {
      mean = a.mean[row];
      rstd = a.rstd[row];
    } else {
      float s[1] = {0.f}, q[1] = {0.f};
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
      row_sum<BLOCK, 1>(q, s_red, slot);
      slot ^= 1;
      rstd = 1.f / sqrtf(q[0] / fD + a.eps);
      if (tid == 0) {
        a.mean[row] = mean;
        a.rstd[row] = rstd;
      }
    }
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      const int c = (tid + k * T) * V;
      if (c < a.D) store_y<DT, V, MUL>(a, row, c, x[k], u[k], w[k], b[k], mean, rstd);
    }
  }
}

template <int DT, int V, int CAP, bool BLOCK, bool MUL>
__global__ __launch_bounds__(256) void hstu_norm_bwd_kernel(const NormArgs a) {
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
  uint32_t uo[NP], duo[NP];
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    const int c = (tid + k * T) * V;
#pragma unroll
    for (int e = 0; e < V; ++e) { w[k][e] = 1.f; b[k][e] = 0.f; dwp[k][e] = 0.f; dbp[k][e] = 0.f; }
    uo[k] = duo[k] = 0;
    if (c < a.D) {
      if (a.learnable) {
        ld_param<DT, V>(a.w, c, a.w_f32, w[k]);
        if constexpr (MUL) ld_param<DT, V>(a.b, c, a.w_f32, b[k]);
      }
      if constexpr (MUL) {
        const int h = c / a.UD;
        uo[k] = (uint32_t)((int64_t)h * a.u_s1 + (int64_t)(c - h * a.UD) * (int64_t)EB);
        duo[k] = (uint32_t)((int64_t)h * a.du_s1 + (int64_t)(c - h * a.UD) * (int64_t)EB);
      }
    }
  }
  const bool cat = MUL && a.concat;
  const bool have_extra = MUL ? cat : a.extra != 0;
  int slot = 0;
  for (int64_t row = row0; row < a.N; row += step) {
    float x[NP][V], g[NP][V], u[NP][V], ex[NP][V];
    const uintptr_t xr = a.x + (uintptr_t)row * a.x_stride, ur = a.u + (uintptr_t)row * a.u_s0;
    const uintptr_t dyr = a.dy + (uintptr_t)row * a.dy_stride;
    const uintptr_t exr = MUL ? dyr + (uintptr_t)a.D * EB : a.extra + (uintptr_t)row * a.extra_stride;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      const int c = (tid + k * T) * V;
#pragma unroll
      for (int e = 0; e < V; ++e) { x[k][e] = 0.f; g[k][e] = 0.f; u[k][e] = 0.f; ex[k][e] = 0.f; }
      if (c < a.D) {
        Vec<DT, V>::ld(xr + (uintptr_t)c * EB, x[k]);
        Vec<DT, V>::ld(dyr + (uintptr_t)(cat ? 2 * a.D + c : c) * EB, g[k]);
        if constexpr (MUL) Vec<DT, V>::ld(ur + uo[k], u[k]);
        if (have_extra) Vec<DT, V>::ld(exr + (uintptr_t)c * EB, ex[k]);
      }
    }
    const float mean = a.mean[row], rstd = a.rstd[row];
    float sums[2] = {0.f, 0.f};   // sum(xh g), sum(g)
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      const int c = (tid + k * T) * V;
      if (c < a.D) {
        if constexpr (MUL) {
          if (a.y) store_y<DT, V, true>(a, row, c, x[k], u[k], w[k], b[k], mean, rstd);
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
          const float xh = norm_xh(x[k][e], mean, rstd), gp = g[k][e];
          dwp[k][e] = __fmaf_rn(gp, xh, dwp[k][e]);
          dbp[k][e] += gp;
          const float gg = w[k][e] * gp;
          g[k][e] = gg;
          sums[0] = __fmaf_rn(xh, gg, sums[0]);
          sums[1] += gg;
        }
      }
    }
    row_sum<BLOCK, 2>(sums, s_red, slot);
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
          o[e] = (g[k][e] - __fmaf_rn(xh, c1, c2)) * rstd + ex[k][e];
        }
        Vec<DT, V>::st(a.dx + (uintptr_t)row * a.dx_stride + (uintptr_t)c * EB, o);
      }
    }
  }
  if (!a.learnable) return;
  // one workspace row per block: a thread's own columns (BLOCK), or the four waves folded in wave order through LDS
  float* pw = a.partial + (size_t)blockIdx.x * a.D;
  float* pb = pw + (size_t)gridDim.x * a.D;
  if constexpr (BLOCK) {
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      const int c = (tid + k * T) * V;
      if (c < a.D) {
#pragma unroll
        for (int e = 0; e < V; ++e) { pw[c + e] = dwp[k][e]; pb[c + e] = dbp[k][e]; }
      }
    }
  } else {
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
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

// blocks of the resident grids; the backward's is also the number of workspace rows
static inline int norm_fwd_blocks(int64_t rows, int64_t D) {
  const int64_t g = D <= kNormWaveMaxD ? ceil_div(rows, 4) : rows;
  return (int)(g < 1 ? 1 : g > 2048 ? 2048 : g);
}
static inline int norm_bwd_blocks(int64_t rows, int64_t D) {
  const int64_t g = D <= kNormWaveMaxD ? ceil_div(rows, 4) : rows, cap = D <= kNormWaveMaxD ? 512 : 1024;
  return (int)(g < 1 ? 1 : g > cap ? cap : g);
}

}  // namespace mi355

using namespace mi355;

template <int DT, int V, int CAP, bool BLOCK, bool MUL, bool BWD>
static void norm_go(int grid, const NormArgs& a, hipStream_t stream) {
  if constexpr (BWD) hstu_norm_bwd_kernel<DT, V, CAP, BLOCK, MUL><<<dim3(grid), dim3(256), 0, stream>>>(a);
  else hstu_norm_fwd_kernel<DT, V, CAP, BLOCK, MUL><<<dim3(grid), dim3(256), 0, stream>>>(a);
}
// the elements a thread holds, by D (header comment); the element-wise path V = 1 always holds 32
template <int DT, int V, bool MUL, bool BWD>
static void norm_launch_cap(int grid, const NormArgs& a, hipStream_t stream) {
  const bool wave = a.D <= kNormWaveMaxD;
  if constexpr (V == 1) {
    if (wave) norm_go<DT, 1, 32, false, MUL, BWD>(grid, a, stream);
    else norm_go<DT, 1, 32, true, MUL, BWD>(grid, a, stream);
  } else {
    if (a.D <= 512) norm_go<DT, V, 8, false, MUL, BWD>(grid, a, stream);
    else if (a.D <= 1024) norm_go<DT, V, 16, false, MUL, BWD>(grid, a, stream);
    else if (wave) norm_go<DT, V, 32, false, MUL, BWD>(grid, a, stream);
    else if (a.D <= 4096) norm_go<DT, V, 16, true, MUL, BWD>(grid, a, stream);
    else norm_go<DT, V, 32, true, MUL, BWD>(grid, a, stream);
  }
}
// v: 16 bytes of the row dtype, or 1
template <bool MUL, bool BWD>
static void norm_launch(int dtype, int v, int grid, const NormArgs& a, hipStream_t stream) {
  if (dtype == kF32) {
    if (v != 1) norm_launch_cap<kF32, 4, MUL, BWD>(grid, a, stream);
    else norm_launch_cap<kF32, 1, MUL, BWD>(grid, a, stream);
  } else if (dtype == kBF16) {
    if (v != 1) norm_launch_cap<kBF16, 8, MUL, BWD>(grid, a, stream);
    else norm_launch_cap<kBF16, 1, MUL, BWD>(grid, a, stream);
  } else {
    if (v != 1) norm_launch_cap<kF16, 8, MUL, BWD>(grid, a, stream);
    else norm_launch_cap<kF16, 1, MUL, BWD>(grid, a, stream);
  }
}

#define NORM_CHECK_COMMON(NAME, rows, D, dtype, wdtype)                                                              \
  MI355_CHECK_ARG(D > 0 && D <= kNormMaxD, NAME ": D must be in 1 .. 8192");                                         \
  MI355_CHECK_ARG(norm_ebytes(dtype) != 0, NAME ": unsupported dtype");                                              \
  MI355_CHECK_ARG(wdtype == kF32 || wdtype == dtype, NAME ": weight and bias are fp32 or have the dtype of the rows"); \
  MI355_CHECK_ARG(rows >= 0 && rows < ((int64_t)1 << 31), NAME ": rows must be in 0 .. 2^31")
#define NORM_CHECK_MUL(NAME, H, UD, D, p)                                                                            \
  MI355_CHECK_ARG(H >= 1 && UD >= 1 && H * UD == D, NAME ": u must hold H * UD == D elements per row");              \
  MI355_CHECK_ARG(p >= 0.0 && p < 1.0, NAME ": dropout_ratio must be in [0, 1)")

static void norm_set_dropout(NormArgs& a, double p, int training, uint64_t seed) {
  a.thr = (uint32_t)(uint64_t)(p * 4294967296.0);   // floor(p 2^32), p in [0, 1)
  a.den = 1.0f - (float)p;
  a.drop = training != 0 && a.thr > 0;
  a.seed_lo = (uint32_t)seed;
  a.seed_hi = (uint32_t)(seed >> 32);
}

static int norm_dwdb(const NormArgs& a, int blocks, int wdtype, void* dweight, void* dbias, hipStream_t stream) {
  const dim3 grid((unsigned)ceil_div(a.D, 64), 2);
  if (wdtype == kF32) hstu_norm_dwdb_kernel<kF32><<<grid, dim3(1024), 0, stream>>>(a.partial, blocks, a.D, dweight, dbias);
  else if (wdtype == kBF16) hstu_norm_dwdb_kernel<kBF16><<<grid, dim3(1024), 0, stream>>>(a.partial, blocks, a.D, dweight, dbias);
  else hstu_norm_dwdb_kernel<kF16><<<grid, dim3(1024), 0, stream>>>(a.partial, blocks, a.D, dweight, dbias);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

extern "C" int mi355_hstu_layer_norm_fwd(const void* x, int64_t x_stride, int64_t rows, int64_t D, int dtype, const void* weight,
                                         const void* bias, int weight_dtype, float eps, void* y, int64_t y_stride, float* mean,
                                         float* rstd, int stats_given, hipStream_t stream) {
  NORM_CHECK_COMMON("hstu_layer_norm_fwd", rows, D, dtype, weight_dtype);
  MI355_CHECK_ARG((weight == nullptr) == (bias == nullptr), "hstu_layer_norm_fwd: weight and bias are given together or not at all");
  MI355_CHECK_ARG(x_stride >= D && y_stride >= D, "hstu_layer_norm_fwd: a row stride is smaller than D");
  if (rows == 0) return MI355_OK;
  MI355_CHECK_ARG(x && y && mean && rstd, "hstu_layer_norm_fwd: null buffer with rows > 0");
  const int eb = norm_ebytes(dtype), web = norm_ebytes(weight_dtype);
  MI355_CHECK_ARG(norm_aligned(x, eb) && norm_aligned(y, eb) && norm_aligned(weight, web) && norm_aligned(bias, web),
                  "hstu_layer_norm_fwd: a base pointer is not aligned to the element size");
  NormVec nv{D % (16 / eb) == 0 ? 16 / eb : 1};
  nv.need(x, x_stride * eb); nv.need(y, y_stride * eb); nv.need(weight, 0); nv.need(bias, 0);
  NormArgs a{};
  a.x = (uintptr_t)x; a.y = (uintptr_t)y; a.w = (uintptr_t)weight; a.b = (uintptr_t)bias;
  a.x_stride = x_stride * eb; a.y_stride = y_stride * eb;
  a.mean = mean; a.rstd = rstd; a.N = rows; a.D = (int)D; a.UD = (int)D; a.eps = eps;
  a.w_f32 = weight_dtype == kF32; a.learnable = weight != nullptr; a.stats_given = stats_given != 0;
  const int grid = norm_fwd_blocks(rows, D);
  norm_launch<false, false>(dtype, nv.v, grid, a, stream);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

extern "C" int64_t mi355_hstu_layer_norm_bwd_workspace_bytes(int64_t rows, int64_t D) {
  if (rows < 0 || D <= 0 || D > kNormMaxD) return 0;
  return (int64_t)2 * norm_bwd_blocks(rows, D) * D * 4;
}
extern "C" int64_t mi355_hstu_ln_mul_dropout_bwd_workspace_bytes(int64_t rows, int64_t D) {
  return mi355_hstu_layer_norm_bwd_workspace_bytes(rows, D);
}

extern "C" int mi355_hstu_layer_norm_bwd(const void* dy, int64_t dy_stride, const void* x, int64_t x_stride, int64_t rows, int64_t D,
                                         int dtype, const void* weight, int weight_dtype, const float* mean, const float* rstd,
                                         const void* dx_accumulate, int64_t dx_accumulate_stride, void* dx, int64_t dx_stride,
                                         void* dweight, void* dbias, void* workspace, int64_t workspace_bytes,
                                         hipStream_t stream) {
  NORM_CHECK_COMMON("hstu_layer_norm_bwd", rows, D, dtype, weight_dtype);
  const bool learnable = weight != nullptr;
  MI355_CHECK_ARG(!learnable || (dweight && dbias), "hstu_layer_norm_bwd: a learnable norm needs dweight and dbias");
  MI355_CHECK_ARG(dy_stride >= D && x_stride >= D && dx_stride >= D && (!dx_accumulate || dx_accumulate_stride >= D),
                  "hstu_layer_norm_bwd: a row stride is smaller than D");
  MI355_CHECK_ARG(!learnable || (workspace && ((uintptr_t)workspace & 15) == 0 &&
                                 workspace_bytes >= mi355_hstu_layer_norm_bwd_workspace_bytes(rows, D)),
                  "hstu_layer_norm_bwd: workspace is null, not 16-byte aligned or too small");
  MI355_CHECK_ARG(rows == 0 || (dy && x && dx && mean && rstd), "hstu_layer_norm_bwd: null buffer with rows > 0");
  const int eb = norm_ebytes(dtype), web = norm_ebytes(weight_dtype);
  MI355_CHECK_ARG(norm_aligned(dy, eb) && norm_aligned(x, eb) && norm_aligned(dx, eb) && norm_aligned(dx_accumulate, eb) &&
                      norm_aligned(weight, web) && norm_aligned(dweight, web) && norm_aligned(dbias, web),
                  "hstu_layer_norm_bwd: a base pointer is not aligned to the element size");
  NormVec nv{D % (16 / eb) == 0 ? 16 / eb : 1};
  nv.need(dy, dy_stride * eb); nv.need(x, x_stride * eb); nv.need(dx, dx_stride * eb); nv.need(weight, 0);
  if (dx_accumulate) nv.need(dx_accumulate, dx_accumulate_stride * eb);
  NormArgs a{};
  a.dy = (uintptr_t)dy; a.x = (uintptr_t)x; a.dx = (uintptr_t)dx; a.w = (uintptr_t)weight; a.extra = (uintptr_t)dx_accumulate;
  a.dy_stride = dy_stride * eb; a.x_stride = x_stride * eb; a.dx_stride = dx_stride * eb; a.extra_stride = dx_accumulate_stride * eb;
  a.mean = const_cast<float*>(mean); a.rstd = const_cast<float*>(rstd); a.partial = (float*)workspace;
  a.N = rows; a.D = (int)D; a.UD = (int)D;
  a.w_f32 = weight_dtype == kF32; a.learnable = learnable;
  const int grid = norm_bwd_blocks(rows, D);
  if (rows > 0) {
    norm_launch<false, true>(dtype, nv.v, grid, a, stream);
    MI355_LAUNCH_CHECK();
  }
  if (learnable) return norm_dwdb(a, rows > 0 ? grid : 0, weight_dtype, dweight, dbias, stream);
  return MI355_OK;
}

extern "C" int mi355_hstu_ln_mul_dropout_fwd(const void* x, int64_t x_stride, const void* u, int64_t u_stride0, int64_t u_stride1,
                                             int64_t H, int64_t UD, int64_t rows, int64_t D, int dtype, const void* weight,
                                             const void* bias, int weight_dtype, float eps, double dropout_ratio, int training,
                                             uint64_t seed, int concat_ux, void* y, int64_t y_stride, float* mean, float* rstd,
                                             hipStream_t stream) {
  NORM_CHECK_COMMON("hstu_ln_mul_dropout_fwd", rows, D, dtype, weight_dtype);
  NORM_CHECK_MUL("hstu_ln_mul_dropout_fwd", H, UD, D, dropout_ratio);
  const int64_t yw = concat_ux ? 3 * D : D;
  MI355_CHECK_ARG(x_stride >= D && y_stride >= yw && u_stride1 >= UD && u_stride0 >= (H - 1) * u_stride1 + UD,
                  "hstu_ln_mul_dropout_fwd: a stride is smaller than the extent it steps over");
  if (rows == 0) return MI355_OK;
  MI355_CHECK_ARG(x && u && y && weight && bias && mean && rstd, "hstu_ln_mul_dropout_fwd: null buffer with rows > 0");
  const int eb = norm_ebytes(dtype), web = norm_ebytes(weight_dtype);
  MI355_CHECK_ARG(norm_aligned(x, eb) && norm_aligned(u, eb) && norm_aligned(y, eb) && norm_aligned(weight, web) && norm_aligned(bias, web),
                  "hstu_ln_mul_dropout_fwd: a base pointer is not aligned to the element size");
  MI355_CHECK_ARG((H - 1) * u_stride1 * eb < ((int64_t)1 << 31), "hstu_ln_mul_dropout_fwd: u head stride too large");
  NormVec nv{D % (16 / eb) == 0 && UD % (16 / eb) == 0 ? 16 / eb : 1};
  nv.need(x, x_stride * eb); nv.need(y, y_stride * eb); nv.need(u, u_stride0 * eb); nv.need(nullptr, u_stride1 * eb);
  nv.need(weight, 0); nv.need(bias, 0);
  NormArgs a{};
  a.x = (uintptr_t)x; a.u = (uintptr_t)u; a.y = (uintptr_t)y; a.w = (uintptr_t)weight; a.b = (uintptr_t)bias;
  a.x_stride = x_stride * eb; a.u_s0 = u_stride0 * eb; a.u_s1 = u_stride1 * eb; a.y_stride = y_stride * eb;
  a.mean = mean; a.rstd = rstd; a.N = rows; a.D = (int)D; a.UD = (int)UD; a.eps = eps;
  a.w_f32 = weight_dtype == kF32; a.learnable = 1; a.concat = concat_ux != 0;
  norm_set_dropout(a, dropout_ratio, training, seed);
  const int grid = norm_fwd_blocks(rows, D);
  norm_launch<true, false>(dtype, nv.v, grid, a, stream);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

extern "C" int mi355_hstu_ln_mul_dropout_bwd(const void* dy, int64_t dy_stride, const void* x, int64_t x_stride, const void* u,
                                             int64_t u_stride0, int64_t u_stride1, int64_t H, int64_t UD, int64_t rows, int64_t D,
                                             int dtype, const void* weight, const void* bias, int weight_dtype, const float* mean,
                                             const float* rstd, double dropout_ratio, int training, uint64_t seed, int concat_ux,
                                             void* dx, int64_t dx_stride, void* du, int64_t du_stride0, int64_t du_stride1,
                                             void* dweight, void* dbias, void* y, int64_t y_stride, void* workspace,
                                             int64_t workspace_bytes, hipStream_t stream) {
  NORM_CHECK_COMMON("hstu_ln_mul_dropout_bwd", rows, D, dtype, weight_dtype);
  NORM_CHECK_MUL("hstu_ln_mul_dropout_bwd", H, UD, D, dropout_ratio);
  const int64_t yw = concat_ux ? 3 * D : D;
  MI355_CHECK_ARG(dy_stride >= yw && x_stride >= D && dx_stride >= D && (!y || y_stride >= yw) && u_stride1 >= UD &&
                      u_stride0 >= (H - 1) * u_stride1 + UD && du_stride1 >= UD && du_stride0 >= (H - 1) * du_stride1 + UD,
                  "hstu_ln_mul_dropout_bwd: a stride is smaller than the extent it steps over");
  MI355_CHECK_ARG(dweight && dbias, "hstu_ln_mul_dropout_bwd: null dweight or dbias");
  MI355_CHECK_ARG(workspace && ((uintptr_t)workspace & 15) == 0 &&
                      workspace_bytes >= mi355_hstu_ln_mul_dropout_bwd_workspace_bytes(rows, D),
                  "hstu_ln_mul_dropout_bwd: workspace is null, not 16-byte aligned or too small");
  MI355_CHECK_ARG(rows == 0 || (dy && x && u && dx && du && weight && bias && mean && rstd),
                  "hstu_ln_mul_dropout_bwd: null buffer with rows > 0");
  const int eb = norm_ebytes(dtype), web = norm_ebytes(weight_dtype);
  MI355_CHECK_ARG(norm_aligned(dy, eb) && norm_aligned(x, eb) && norm_aligned(u, eb) && norm_aligned(dx, eb) && norm_aligned(du, eb) &&
                      norm_aligned(y, eb) && norm_aligned(weight, web) && norm_aligned(bias, web) && norm_aligned(dweight, web) &&
                      norm_aligned(dbias, web),
                  "hstu_ln_mul_dropout_bwd: a base pointer is not aligned to the element size");
  MI355_CHECK_ARG((H - 1) * u_stride1 * eb < ((int64_t)1 << 31) && (H - 1) * du_stride1 * eb < ((int64_t)1 << 31),
                  "hstu_ln_mul_dropout_bwd: u head stride too large");
  NormVec nv{D % (16 / eb) == 0 && UD % (16 / eb) == 0 ? 16 / eb : 1};
  nv.need(dy, dy_stride * eb); nv.need(x, x_stride * eb); nv.need(dx, dx_stride * eb);
  nv.need(u, u_stride0 * eb); nv.need(nullptr, u_stride1 * eb); nv.need(du, du_stride0 * eb); nv.need(nullptr, du_stride1 * eb);
  if (y) nv.need(y, y_stride * eb);
  nv.need(weight, 0); nv.need(bias, 0);
  NormArgs a{};
  a.dy = (uintptr_t)dy; a.x = (uintptr_t)x; a.u = (uintptr_t)u; a.dx = (uintptr_t)dx; a.du = (uintptr_t)du; a.y = (uintptr_t)y;
  a.w = (uintptr_t)weight; a.b = (uintptr_t)bias;
  a.dy_stride = dy_stride * eb; a.x_stride = x_stride * eb; a.u_s0 = u_stride0 * eb; a.u_s1 = u_stride1 * eb;
  a.dx_stride = dx_stride * eb; a.du_s0 = du_stride0 * eb; a.du_s1 = du_stride1 * eb; a.y_stride = y_stride * eb;
  a.mean = const_cast<float*>(mean); a.rstd = const_cast<float*>(rstd); a.partial = (float*)workspace;
  a.N = rows; a.D = (int)D; a.UD = (int)UD;
  a.w_f32 = weight_dtype == kF32; a.learnable = 1; a.concat = concat_ux != 0;
  norm_set_dropout(a, dropout_ratio, training, seed);
  const int grid = norm_bwd_blocks(rows, D);
  if (rows > 0) {
    norm_launch<true, true>(dtype, nv.v, grid, a, stream);
    MI355_LAUNCH_CHECK();
  }
  return norm_dwdb(a, rows > 0 ? grid : 0, weight_dtype, dweight, dbias, stream);
}
