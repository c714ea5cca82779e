// HSTU group norm mul dropout over rows [N, H * L], forward and backward: layer-norm-mul-dropout with the statistics of
// every head of L columns taken apart and one weight / bias per head.
//
// Replaces (reference, examples/hstu/ops/triton_ops/triton_norm_mul_dropout.py): _group_norm_mul_dropout_fwd,
// _group_norm_mul_dropout_bwd_dx_du and _group_norm_bwd_dwdb with their wrappers (:600-1143).  Written for wave64 from the
// arithmetic; the reference is Triton.
//
// Values (all arithmetic fp32, every stored value rounded once), per (row, head h):
//   mean = sum(x) / L;  var = sum((x - mean)^2) / L in a second pass;  rstd = 1 / sqrtf(var + eps)
//   xh = (x - mean) * rstd;  gn = fmaf(xh, w_h, b_h);  t = gn * u;  y = drop(t), or [drop0(u) | drop1(x) | drop2(t)]
//   backward: dt = drop2'(dy_t);  du = fmaf(dt, gn, drop0'(dy_u));  gp = dt * u;  g = w_h * gp;  c1 = sum(xh * g) / L;
//   c2 = sum(g) / L;  dx = (g - (xh * c1 + c2)) * rstd + drop1'(dy_x);  dw_h = sum of gp * xh;  db_h = sum of gp
// The dropout is that of norm_ops.hip (norm_dev.h) with col the column in the whole row.  Decomposition, the forward's stores, the
// ladder, the grid rule and the dw / db launch are those of norm_dev.h.
//
// Two layouts.
//   Fast: a head is a whole number of 16-byte pieces, their count PPH = L / V a power of two <= 64, every base pointer and
//   stride a multiple of 16 bytes.  The decomposition is that of norm_dev.h (piece i of the row belongs to thread i mod T; a
//   wave owns a row for D <= 2048, a workgroup above), so a head is PPH neighbouring lanes of one round and never leaves its
//   wave: the per-head sums are butterflies over lane groups (DPP quad_perm / row_half_mirror / row_mirror for 2 .. 16 lanes,
//   ds_bpermute for 32 and 64), every lane of a group ends with the same bits, nothing goes through LDS.  The backward keeps
//   one dw / db partial per round and thread, folds lane groups and the four waves in a fixed order and writes [2][H] per block.
//   General (any H >= 1, L >= 1): two kernels without LDS or barriers.  The first gives 2^lg lanes (lg from L alone) to each
//   (row, head), which walk the head's columns with stride 2^lg and butterfly: forward mean and rstd, backward c1 and c2
//   (workspace) and the dw / db partials; a lane group visits (row, head) pairs with a stride that is a multiple of H, so it
//   stays on one head and owns one partial, [2][slots][H].  The second kernel is element-wise over pieces (V = 16 bytes' worth
//   when L and the addresses allow, else 1).  hstu_norm_dwdb_kernel (norm_dev.h) folds the partial rows of either layout.
// No atomics: every sum has an order fixed by (rows, H, L) and the layout, which the pointers' alignment selects.
#include "norm_dev.h"
#include "../../include/recsys_amd.h"

namespace mi355 {

struct GnArgs : NormDropout {
  uintptr_t x, u, y, w, b, dy, dx, du;                // y 0: not written
  int64_t x_stride, u_s0, u_s1, y_stride, dy_stride, dx_stride, du_s0, du_s1;   // bytes
  float* mean;
  float* rstd;
  float* partial;      // backward: [2][P][H] fp32, P = gridDim.x (fast) or slots (general)
  float* cc;           // general backward: [rows * H][2] = (c1, c2)
  int64_t N;
  int D, H, L;
  int lg;              // fast: log2 of the pieces of a head; general: log2 of the lanes of a (row, head)
  int slots;           // general backward: lane groups = slots * H
  float eps;
  int w_f32, concat;
};

#define GN_DPP(v, ctrl) v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), ctrl, 0xf, 0xf, false))
// sum over aligned groups of 2^lg lanes, the same bits in every lane of a group; every lane of the wave must be active
__device__ __forceinline__ float seg_sum(float v, int lg) {
  if (lg >= 1) GN_DPP(v, 0xB1);    // quad_perm [1, 0, 3, 2]
  if (lg >= 2) GN_DPP(v, 0x4E);    // quad_perm [2, 3, 0, 1]
  if (lg >= 3) GN_DPP(v, 0x141);   // row_half_mirror
  if (lg >= 4) GN_DPP(v, 0x140);   // row_mirror
  if (lg >= 5) v += __shfl_xor(v, 16, 64);
  if (lg >= 6) v += __shfl_xor(v, 32, 64);
  return v;
}

__device__ __forceinline__ float ld_param1(uintptr_t p, int i, int f32, int dt) {
  if (f32) return *(const float*)(p + (uintptr_t)i * 4);
  const uint16_t h = *(const uint16_t*)(p + (uintptr_t)i * 2);
  return dt == kBF16 ? bf16_to_f32(h) : f16_to_f32(h);
}

// The backward of one piece up to the sums: y again, the masks, du stored (at byte offset duo of the row); g: dy_t in,
// gp = dt u out; ex: dy_x in, dropped out.  Two statement orders, chosen per instantiation by measurement; the values are the same.
// gn_bwd_head: the masks of dt and dy_x before the du load, the order of the LN-mul-dropout backward (norm_dev.h).  Every fast
// kernel but one and the general layout's apply kernel use it.  At CAP 32 wave rows (D = 2048) it takes 165 us where the order
// below takes 585 (16 384 x (8, 256) bf16): the order decides how hipcc stages that kernel's AGPR copies.
// gn_bwd_head_cap16: the du load before the masks, the order this file had from the start.  hstu_gn_bwd_kernel<DT, V, 16, false>
// (wave rows, D in 513 .. 1024) alone keeps it: with the order above that kernel took 54.4 us against 52.1 at 16 384 x (8, 128)
// bf16 and 106.5 against 102.9 at 32 768.
template <int DT, int V, class A, class W>
__device__ __forceinline__ void gn_bwd_head(const A& a, int64_t row, int c, uint32_t duo, const float (&x)[V], float (&g)[V],
                                             const float (&u)[V], float (&ex)[V], const W& w, const W& b, float mean, float rstd) {
  constexpr uintptr_t EB = Vec<DT, V>::EB;
  const bool cat = a.concat != 0;
  if (a.y) mul_store_y<DT, V>(a, row, c, x, u, w, b, mean, rstd);
  if (a.drop) {
    drop_apply<V>(a, row, c, cat ? 2u : 0u, g);   // dt
    if (cat) drop_apply<V>(a, row, c, 1u, ex);
  }
  float duv[V];
  if (cat) {
    Vec<DT, V>::ld(a.dy + (uintptr_t)row * a.dy_stride + (uintptr_t)c * EB, duv);
    if (a.drop) drop_apply<V>(a, row, c, 0u, duv);
  } else {
#pragma unroll
    for (int e = 0; e < V; ++e) duv[e] = 0.f;
  }
#pragma unroll
  for (int e = 0; e < V; ++e) {
    const float ln = norm_ln(norm_xh(x[e], mean, rstd), norm_par(w, e), norm_par(b, e));
    duv[e] = __fmaf_rn(g[e], ln, duv[e]);
    g[e] *= u[e];
  }
  Vec<DT, V>::st(a.du + (uintptr_t)row * a.du_s0 + duo, duv);
}

template <int DT, int V>
__device__ __forceinline__ void gn_bwd_head_cap16(const GnArgs& a, int64_t row, int c, uint32_t duo, const float (&x)[V],
                                                  float (&g)[V], const float (&u)[V], float (&ex)[V], float w, float b, float mean,
                                                  float rstd) {
  constexpr uintptr_t EB = Vec<DT, V>::EB;
  const bool cat = a.concat != 0;
  if (a.y) mul_store_y<DT, V>(a, row, c, x, u, w, b, mean, rstd);
  float duv[V];
  if (cat) Vec<DT, V>::ld(a.dy + (uintptr_t)row * a.dy_stride + (uintptr_t)c * EB, duv);
  else {
#pragma unroll
    for (int e = 0; e < V; ++e) duv[e] = 0.f;
  }
  if (a.drop) {
    drop_apply<V>(a, row, c, cat ? 2u : 0u, g);   // dt
    if (cat) {
      drop_apply<V>(a, row, c, 1u, ex);
      drop_apply<V>(a, row, c, 0u, duv);
    }
  }
#pragma unroll
  for (int e = 0; e < V; ++e) {
    const float gn = norm_ln(norm_xh(x[e], mean, rstd), w, b);
    duv[e] = __fmaf_rn(g[e], gn, duv[e]);
    g[e] *= u[e];
  }
  Vec<DT, V>::st(a.du + (uintptr_t)row * a.du_s0 + duo, duv);
}

// ---- the fast layout: RowPieces and mul_store_y of norm_dev.h; the statistics are per head ----
template <int DT, int V, int CAP, bool BLOCK>
__global__ __launch_bounds__(256) void hstu_gn_fwd_kernel(const GnArgs a) {
  constexpr int NP = CAP / V;
  constexpr uintptr_t EB = Vec<DT, V>::EB;
  const RowPieces<V, CAP, BLOCK> p;
  const float fL = (float)a.L;
  const int lg = a.lg;
  float w[NP], b[NP];
  uint32_t uo[NP];
  int hd[NP];
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    const int c = p.col(k);
    w[k] = 1.f; b[k] = 0.f; uo[k] = 0; hd[k] = 0;
    if (c < a.D) {
      const int h = p.piece(k) >> lg;
      hd[k] = h;
      w[k] = ld_param1(a.w, h, a.w_f32, DT);
      b[k] = ld_param1(a.b, h, a.w_f32, DT);
      uo[k] = (uint32_t)((int64_t)h * a.u_s1 + (int64_t)(c - h * a.L) * (int64_t)EB);
    }
  }
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
        Vec<DT, V>::ld(ur + uo[k], u[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      const int c = p.col(k);
      float s = 0.f, q = 0.f;
#pragma unroll
      for (int e = 0; e < V; ++e) s += x[k][e];
      const float mean = seg_sum(s, lg) / fL;
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const float d = x[k][e] - mean;
        q = __fmaf_rn(d, d, q);
      }
      const float rstd = 1.f / sqrtf(seg_sum(q, lg) / fL + a.eps);
      if (c < a.D) {
        if ((p.piece(k) & ((1 << lg) - 1)) == 0) {
          a.mean[row * a.H + hd[k]] = mean;
          a.rstd[row * a.H + hd[k]] = rstd;
        }
        mul_store_y<DT, V>(a, row, c, x[k], u[k], w[k], b[k], mean, rstd);
      }
    }
  }
}

template <int DT, int V, int CAP, bool BLOCK>
__global__ __launch_bounds__(256) void hstu_gn_bwd_kernel(const GnArgs a) {
  constexpr int NP = CAP / V;
  constexpr uintptr_t EB = Vec<DT, V>::EB;
  constexpr int kFoldH = kNormWaveMaxD / 4;   // heads of a wave row at most: fp32 pieces of 4, one piece a head
  __shared__ float s_fold[BLOCK ? 1 : 4 * 2 * kFoldH];
  const RowPieces<V, CAP, BLOCK> p;
  const float fL = (float)a.L;
  const int lg = a.lg;
  const bool cat = a.concat != 0;
  float w[NP], b[NP], dwp[NP], dbp[NP];
  uint32_t uo[NP], duo[NP];
  int hd[NP];
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    const int c = p.col(k);
    w[k] = 1.f; b[k] = 0.f; dwp[k] = 0.f; dbp[k] = 0.f; uo[k] = duo[k] = 0; hd[k] = 0;
    if (c < a.D) {
      const int h = p.piece(k) >> lg;
      hd[k] = h;
      w[k] = ld_param1(a.w, h, a.w_f32, DT);
      b[k] = ld_param1(a.b, h, a.w_f32, DT);
      uo[k] = (uint32_t)((int64_t)h * a.u_s1 + (int64_t)(c - h * a.L) * (int64_t)EB);
      duo[k] = (uint32_t)((int64_t)h * a.du_s1 + (int64_t)(c - h * a.L) * (int64_t)EB);
    }
  }
  for (int64_t row = p.row0; row < a.N; row += p.step) {
    float x[NP][V], g[NP][V], u[NP][V], ex[NP][V];
    const uintptr_t xr = a.x + (uintptr_t)row * a.x_stride, ur = a.u + (uintptr_t)row * a.u_s0;
    const uintptr_t dyr = a.dy + (uintptr_t)row * a.dy_stride;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      const int c = p.col(k);
#pragma unroll
      for (int e = 0; e < V; ++e) { x[k][e] = 0.f; g[k][e] = 0.f; u[k][e] = 0.f; ex[k][e] = 0.f; }
      if (c < a.D) {
        Vec<DT, V>::ld(xr + (uintptr_t)c * EB, x[k]);
        Vec<DT, V>::ld(dyr + (uintptr_t)(cat ? 2 * a.D + c : c) * EB, g[k]);
        Vec<DT, V>::ld(ur + uo[k], u[k]);
        if (cat) Vec<DT, V>::ld(dyr + (uintptr_t)(a.D + c) * EB, ex[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      const int c = p.col(k);
      const bool live = c < a.D;
      float mean = 0.f, rstd = 0.f, s0 = 0.f, s1 = 0.f;   // sum(xh g), sum(g) of this thread's piece
      if (live) {
        mean = a.mean[row * a.H + hd[k]];
        rstd = a.rstd[row * a.H + hd[k]];
        if constexpr (CAP == 16 && !BLOCK) gn_bwd_head_cap16<DT, V>(a, row, c, duo[k], x[k], g[k], u[k], ex[k], w[k], b[k], mean, rstd);
        else gn_bwd_head<DT, V>(a, row, c, duo[k], x[k], g[k], u[k], ex[k], w[k], b[k], mean, rstd);
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const float xh = norm_xh(x[k][e], mean, rstd), gp = g[k][e];
          dwp[k] = __fmaf_rn(gp, xh, dwp[k]);
          dbp[k] += gp;
          const float gg = w[k] * gp;
          g[k][e] = gg;
          s0 = __fmaf_rn(xh, gg, s0);
          s1 += gg;
        }
      }
      const float c1 = seg_sum(s0, lg) / fL, c2 = seg_sum(s1, lg) / fL;
      if (live) {
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
  // [2][H] per block: the lane groups of a head, then (wave rows) the four waves in wave order through LDS
  float* pw = a.partial + (size_t)blockIdx.x * a.H;
  float* pb = pw + (size_t)gridDim.x * a.H;
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    const float sw = seg_sum(dwp[k], lg), sb = seg_sum(dbp[k], lg);
    if (p.col(k) < a.D && (p.piece(k) & ((1 << lg) - 1)) == 0) {
      if constexpr (BLOCK) {
        pw[hd[k]] = sw;
        pb[hd[k]] = sb;
      } else {
        s_fold[(p.wv * 2) * kFoldH + hd[k]] = sw;
        s_fold[(p.wv * 2 + 1) * kFoldH + hd[k]] = sb;
      }
    }
  }
  if constexpr (!BLOCK) {
    __syncthreads();
    for (int h = (int)threadIdx.x; h < a.H; h += 256) {
      pw[h] = ((s_fold[h] + s_fold[2 * kFoldH + h]) + s_fold[4 * kFoldH + h]) + s_fold[6 * kFoldH + h];
      pb[h] = ((s_fold[kFoldH + h] + s_fold[3 * kFoldH + h]) + s_fold[5 * kFoldH + h]) + s_fold[7 * kFoldH + h];
    }
  }
}

// ---- the general layout ----
// (row, head) pairs of a lane group: pair = group + i * groups, groups = gridDim.x * 256 >> lg (forward) or slots * H (backward)
template <int DT, bool BWD>
__global__ __launch_bounds__(256) void hstu_gn_stats_kernel(const GnArgs a) {
  constexpr uintptr_t EB = Vec<DT, 1>::EB;
  const int lg = a.lg, P = 1 << lg;
  const int64_t gid = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> lg;   // lane group
  const int j = (int)threadIdx.x & (P - 1);
  const int64_t groups = BWD ? (int64_t)a.slots * a.H : ((int64_t)gridDim.x * 256) >> lg;
  const int64_t pairs = a.N * a.H;
  const int64_t wave_first = (((int64_t)blockIdx.x * 256 + (threadIdx.x & ~63u)) >> lg);   // the wave's first group
  const float fL = (float)a.L;
  const bool cat = a.concat != 0;
  float dw = 0.f, db = 0.f;
  // the trip count is the wave's (its first group's), so that every lane stays active for the butterflies
  for (int64_t base = 0; wave_first + base < pairs; base += groups) {
    const int64_t pair = gid + base;
    const bool live = pair < pairs && (!BWD || gid < groups);
    const int64_t row = live ? pair / a.H : 0;
    const int h = live ? (int)(pair - row * a.H) : 0;
    const int c0 = h * a.L;
    const uintptr_t xr = a.x + (uintptr_t)row * a.x_stride + (uintptr_t)c0 * EB;
    if constexpr (!BWD) {
      float s = 0.f, q = 0.f;
      if (live) {
        for (int i = j; i < a.L; i += P) {
          float v[1];
          Vec<DT, 1>::ld(xr + (uintptr_t)i * EB, v);
          s += v[0];
        }
      }
      const float mean = seg_sum(s, lg) / fL;
      if (live) {
        for (int i = j; i < a.L; i += P) {
          float v[1];
          Vec<DT, 1>::ld(xr + (uintptr_t)i * EB, v);
          const float d = v[0] - mean;
          q = __fmaf_rn(d, d, q);
        }
      }
      const float rstd = 1.f / sqrtf(seg_sum(q, lg) / fL + a.eps);
      if (live && j == 0) {
        a.mean[pair] = mean;
        a.rstd[pair] = rstd;
      }
    } else {
      float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;   // sum(xh g), sum(g), sum(gp xh), sum(gp)
      if (live) {
        const float mean = a.mean[pair], rstd = a.rstd[pair], w = ld_param1(a.w, h, a.w_f32, DT);
        const uintptr_t ur = a.u + (uintptr_t)row * a.u_s0 + (uintptr_t)h * a.u_s1;
        const uintptr_t gr = a.dy + (uintptr_t)row * a.dy_stride + (uintptr_t)(cat ? 2 * a.D + c0 : c0) * EB;
        for (int i = j; i < a.L; i += P) {
          float x[1], g[1], u[1];
          Vec<DT, 1>::ld(xr + (uintptr_t)i * EB, x);
          Vec<DT, 1>::ld(gr + (uintptr_t)i * EB, g);
          Vec<DT, 1>::ld(ur + (uintptr_t)i * EB, u);
          if (a.drop) drop_apply<1>(a, row, c0 + i, cat ? 2u : 0u, g);
          const float xh = norm_xh(x[0], mean, rstd), gp = g[0] * u[0], gg = w * gp;
          s0 = __fmaf_rn(xh, gg, s0);
          s1 += gg;
          s2 = __fmaf_rn(gp, xh, s2);
          s3 += gp;
        }
      }
      s0 = seg_sum(s0, lg); s1 = seg_sum(s1, lg); s2 = seg_sum(s2, lg); s3 = seg_sum(s3, lg);
      if (live && j == 0) {
        a.cc[2 * pair] = s0 / fL;
        a.cc[2 * pair + 1] = s1 / fL;
      }
      dw += s2;   // (groups is a multiple of H: the group stays on head gid % H)
      db += s3;
    }
  }
  if constexpr (BWD) {
    if (j == 0 && gid < groups) {
      a.partial[gid] = dw;
      a.partial[groups + gid] = db;
    }
  }
}

// element-wise over the pieces of all rows, statistics (and c1, c2) read back
template <int DT, int V, bool BWD>
__global__ __launch_bounds__(256) void hstu_gn_apply_kernel(const GnArgs a) {
  constexpr uintptr_t EB = Vec<DT, V>::EB;
  const int ppr = a.D / V;   // pieces per row
  const int64_t pieces = a.N * ppr, stride = (int64_t)gridDim.x * 256;
  const bool cat = a.concat != 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < pieces; i += stride) {
    const int64_t row = i / ppr;
    const int c = (int)(i - row * ppr) * V, h = c / a.L;
    const float mean = a.mean[row * a.H + h], rstd = a.rstd[row * a.H + h];
    const float w = ld_param1(a.w, h, a.w_f32, DT), b = ld_param1(a.b, h, a.w_f32, DT);
    float x[V], u[V];
    Vec<DT, V>::ld(a.x + (uintptr_t)row * a.x_stride + (uintptr_t)c * EB, x);
    Vec<DT, V>::ld(a.u + (uintptr_t)row * a.u_s0 + (uintptr_t)h * a.u_s1 + (uintptr_t)(c - h * a.L) * EB, u);
    if constexpr (!BWD) {
      mul_store_y<DT, V>(a, row, c, x, u, w, b, mean, rstd);
    } else {
      const uintptr_t dyr = a.dy + (uintptr_t)row * a.dy_stride;
      float g[V], ex[V];
      Vec<DT, V>::ld(dyr + (uintptr_t)(cat ? 2 * a.D + c : c) * EB, g);
      if (cat) Vec<DT, V>::ld(dyr + (uintptr_t)(a.D + c) * EB, ex);
      else {
#pragma unroll
        for (int e = 0; e < V; ++e) ex[e] = 0.f;
      }
      const uint32_t duo = (uint32_t)((int64_t)h * a.du_s1 + (int64_t)(c - h * a.L) * (int64_t)EB);
      gn_bwd_head<DT, V>(a, row, c, duo, x, g, u, ex, w, b, mean, rstd);
      const float c1 = a.cc[2 * (row * a.H + h)], c2 = a.cc[2 * (row * a.H + h) + 1];
      float o[V];
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const float xh = norm_xh(x[e], mean, rstd);
        o[e] = (w * g[e] - __fmaf_rn(xh, c1, c2)) * rstd + ex[e];
      }
      Vec<DT, V>::st(a.dx + (uintptr_t)row * a.dx_stride + (uintptr_t)c * EB, o);
    }
  }
}

// ---- host ----
// general layout: log2 of the lanes of a (row, head): the largest power of two <= L / 4, in 1 .. 64
static inline int gn_gen_lg(int64_t L) {
  int lg = 0;
  while (lg < 6 && ((int64_t)8 << lg) <= L) ++lg;
  return lg;
}
// general backward: lane groups = slots * H, about 2048 blocks' worth at most and no more slots than rows
static inline int gn_gen_slots(int64_t rows, int64_t H, int64_t L) {
  const int64_t most = ((int64_t)2048 * 256 >> gn_gen_lg(L)) / H;
  const int64_t s = rows < most ? rows : most;
  return (int)(s < 1 ? 1 : s);
}
static inline int gn_apply_blocks(int64_t pieces) {
  const int64_t g = ceil_div(pieces, 256);
  return (int)(g < 1 ? 1 : g > 4096 ? 4096 : g);
}

}  // namespace mi355

using namespace mi355;

// the fast kernels through the ladder of norm_dev.h, without its V = 1 arm: the fast layout is made of 16-byte pieces
template <bool BWD>
static void gn_fast(int dtype, int grid, const GnArgs& a, hipStream_t stream) {
  norm_dispatch<false>(dtype, 0, a.D, [&](auto s) {
    using S = decltype(s);
    if constexpr (BWD) hstu_gn_bwd_kernel<S::DT, S::V, S::CAP, S::BLOCK><<<dim3(grid), dim3(256), 0, stream>>>(a);
    else hstu_gn_fwd_kernel<S::DT, S::V, S::CAP, S::BLOCK><<<dim3(grid), dim3(256), 0, stream>>>(a);
  });
}
template <int DT, int V, bool BWD>
static void gn_general_dt(int v, int stats_grid, const GnArgs& a, hipStream_t stream) {
  hstu_gn_stats_kernel<DT, BWD><<<dim3(stats_grid), dim3(256), 0, stream>>>(a);
  const int grid = gn_apply_blocks(a.N * (a.D / v));
  if (v != 1) hstu_gn_apply_kernel<DT, V, BWD><<<dim3(grid), dim3(256), 0, stream>>>(a);
  else hstu_gn_apply_kernel<DT, 1, BWD><<<dim3(grid), dim3(256), 0, stream>>>(a);
}
template <bool BWD>
static void gn_general(int dtype, int v, int stats_grid, const GnArgs& a, hipStream_t stream) {
  if (dtype == kF32) gn_general_dt<kF32, 4, BWD>(v, stats_grid, a, stream);
  else if (dtype == kBF16) gn_general_dt<kBF16, 8, BWD>(v, stats_grid, a, stream);
  else gn_general_dt<kF16, 8, BWD>(v, stats_grid, a, stream);
}

// lg of the fast layout, or -1: L a power-of-two number (<= 64) of 16-byte pieces
static int gn_fast_lg(int64_t L, int v) {
  if (L % v != 0) return -1;
  const int64_t pph = L / v;
  if (pph > 64 || (pph & (pph - 1)) != 0) return -1;
  int lg = 0;
  while (((int64_t)1 << lg) < pph) ++lg;
  return lg;
}

#define GN_CHECK_COMMON(NAME, rows, H, L, D, dtype, wdtype, p)                                       \
  NORM_CHECK_COMMON(NAME, rows, D, dtype, wdtype, "weight and bias are");                            \
  MI355_CHECK_ARG(H >= 1 && L >= 1 && H * L == D, NAME ": the heads must fill the row, H * L == D"); \
  MI355_CHECK_ARG(p >= 0.0 && p < 1.0, NAME ": dropout_ratio must be in [0, 1)")

extern "C" int mi355_hstu_gn_mul_dropout_fwd(const void* x, int64_t x_stride, const void* u, int64_t u_stride0, int64_t u_stride1,
                                             int64_t H, int64_t L, int64_t rows, int64_t D, int dtype, const void* weight,
                                             const void* bias, int weight_dtype, float eps, double dropout_ratio, int training,
                                             uint64_t seed, int concat_ux, void* y, int64_t y_stride, float* mean, float* rstd,
                                             hipStream_t stream) {
  GN_CHECK_COMMON("hstu_gn_mul_dropout_fwd", rows, H, L, D, dtype, weight_dtype, dropout_ratio);
  const int64_t yw = concat_ux ? 3 * D : D;
  MI355_CHECK_ARG(x_stride >= D && y_stride >= yw && u_stride1 >= L && u_stride0 >= (H - 1) * u_stride1 + L,
                  "hstu_gn_mul_dropout_fwd: a stride is smaller than the extent it steps over");
  if (rows == 0) return MI355_OK;
  MI355_CHECK_ARG(x && u && y && weight && bias && mean && rstd, "hstu_gn_mul_dropout_fwd: null buffer with rows > 0");
  const int eb = elem_bytes(dtype), web = elem_bytes(weight_dtype);
  MI355_CHECK_ARG(norm_aligned(x, eb) && norm_aligned(u, eb) && norm_aligned(y, eb) && norm_aligned(weight, web) && norm_aligned(bias, web),
                  "hstu_gn_mul_dropout_fwd: a base pointer is not aligned to the element size");
  MI355_CHECK_ARG((H - 1) * u_stride1 * eb < ((int64_t)1 << 31), "hstu_gn_mul_dropout_fwd: u head stride too large");
  NormVec nv{L % (16 / eb) == 0 ? 16 / eb : 1};
  nv.need(x, x_stride * eb); nv.need(y, y_stride * eb); nv.need(u, u_stride0 * eb); nv.need(nullptr, u_stride1 * eb);
  GnArgs a{};
  a.x = (uintptr_t)x; a.u = (uintptr_t)u; a.y = (uintptr_t)y; a.w = (uintptr_t)weight; a.b = (uintptr_t)bias;
  a.x_stride = x_stride * eb; a.u_s0 = u_stride0 * eb; a.u_s1 = u_stride1 * eb; a.y_stride = y_stride * eb;
  a.mean = mean; a.rstd = rstd; a.N = rows; a.D = (int)D; a.H = (int)H; a.L = (int)L; a.eps = eps;
  a.w_f32 = weight_dtype == kF32; a.concat = concat_ux != 0;
  norm_set_dropout(a, dropout_ratio, training, seed);
  const int flg = nv.v != 1 ? gn_fast_lg(L, nv.v) : -1;
  if (flg >= 0) {
    a.lg = flg;
    gn_fast<false>(dtype, norm_row_blocks(rows, D, false), a, stream);
  } else {
    a.lg = gn_gen_lg(L);
    const int64_t blocks = ceil_div((rows * H) << a.lg, 256);
    gn_general<false>(dtype, nv.v, (int)(blocks > 2048 ? 2048 : blocks), a, stream);
  }
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

// the partials of either layout and the general layout's (c1, c2) of every (row, head)
extern "C" int64_t mi355_hstu_gn_mul_dropout_bwd_workspace_bytes(int64_t rows, int64_t H, int64_t L) {
  if (rows < 0 || H < 1 || L < 1 || H * L > kNormMaxD) return 0;
  const int64_t fast = (int64_t)norm_row_blocks(rows, H * L, true) * H, gen = (int64_t)gn_gen_slots(rows, H, L) * H;
  return ((fast > gen ? fast : gen) * 2 + rows * H * 2) * 4;
}

extern "C" int mi355_hstu_gn_mul_dropout_bwd(const void* dy, int64_t dy_stride, const void* x, int64_t x_stride, const void* u,
                                             int64_t u_stride0, int64_t u_stride1, int64_t H, int64_t L, int64_t rows, int64_t D,
                                             int dtype, const void* weight, const void* bias, int weight_dtype, const float* mean,
                                             const float* rstd, double dropout_ratio, int training, uint64_t seed, int concat_ux,
                                             void* dx, int64_t dx_stride, void* du, int64_t du_stride0, int64_t du_stride1,
                                             void* dweight, void* dbias, void* y, int64_t y_stride, void* workspace,
                                             int64_t workspace_bytes, hipStream_t stream) {
  GN_CHECK_COMMON("hstu_gn_mul_dropout_bwd", rows, H, L, D, dtype, weight_dtype, dropout_ratio);
  const int64_t yw = concat_ux ? 3 * D : D;
  MI355_CHECK_ARG(dy_stride >= yw && x_stride >= D && dx_stride >= D && (!y || y_stride >= yw) && u_stride1 >= L &&
                      u_stride0 >= (H - 1) * u_stride1 + L && du_stride1 >= L && du_stride0 >= (H - 1) * du_stride1 + L,
                  "hstu_gn_mul_dropout_bwd: a stride is smaller than the extent it steps over");
  MI355_CHECK_ARG(dweight && dbias && (rows == 0 || (dy && x && u && dx && du && weight && bias && mean && rstd)),
                  "hstu_gn_mul_dropout_bwd: null buffer (dweight and dbias are needed for rows == 0 too)");
  MI355_CHECK_ARG(rows == 0 || (workspace && ((uintptr_t)workspace & 15) == 0 &&
                                workspace_bytes >= mi355_hstu_gn_mul_dropout_bwd_workspace_bytes(rows, H, L)),
                  "hstu_gn_mul_dropout_bwd: workspace is null, not 16-byte aligned or too small");
  const int eb = elem_bytes(dtype), web = elem_bytes(weight_dtype);
  MI355_CHECK_ARG(norm_aligned(dy, eb) && norm_aligned(x, eb) && norm_aligned(u, eb) && norm_aligned(dx, eb) && norm_aligned(du, eb) &&
                      norm_aligned(y, eb) && norm_aligned(weight, web) && norm_aligned(bias, web) && norm_aligned(dweight, web) &&
                      norm_aligned(dbias, web),
                  "hstu_gn_mul_dropout_bwd: a base pointer is not aligned to the element size");
  MI355_CHECK_ARG((H - 1) * u_stride1 * eb < ((int64_t)1 << 31) && (H - 1) * du_stride1 * eb < ((int64_t)1 << 31),
                  "hstu_gn_mul_dropout_bwd: u head stride too large");
  NormVec nv{L % (16 / eb) == 0 ? 16 / eb : 1};
  nv.need(dy, dy_stride * eb); nv.need(x, x_stride * eb); nv.need(dx, dx_stride * eb);
  nv.need(u, u_stride0 * eb); nv.need(nullptr, u_stride1 * eb); nv.need(du, du_stride0 * eb); nv.need(nullptr, du_stride1 * eb);
  if (y) nv.need(y, y_stride * eb);
  GnArgs a{};
  a.dy = (uintptr_t)dy; a.x = (uintptr_t)x; a.u = (uintptr_t)u; a.dx = (uintptr_t)dx; a.du = (uintptr_t)du; a.y = (uintptr_t)y;
  a.w = (uintptr_t)weight; a.b = (uintptr_t)bias;
  a.dy_stride = dy_stride * eb; a.x_stride = x_stride * eb; a.u_s0 = u_stride0 * eb; a.u_s1 = u_stride1 * eb;
  a.dx_stride = dx_stride * eb; a.du_s0 = du_stride0 * eb; a.du_s1 = du_stride1 * eb; a.y_stride = y_stride * eb;
  a.mean = const_cast<float*>(mean); a.rstd = const_cast<float*>(rstd); a.partial = (float*)workspace;
  a.N = rows; a.D = (int)D; a.H = (int)H; a.L = (int)L;
  a.w_f32 = weight_dtype == kF32; a.concat = concat_ux != 0;
  norm_set_dropout(a, dropout_ratio, training, seed);
  int partial_rows = 0;
  if (rows > 0) {
    const int flg = nv.v != 1 ? gn_fast_lg(L, nv.v) : -1;
    if (flg >= 0) {
      a.lg = flg;
      partial_rows = norm_row_blocks(rows, D, true);
      gn_fast<true>(dtype, partial_rows, a, stream);
    } else {
      a.lg = gn_gen_lg(L);
      a.slots = partial_rows = gn_gen_slots(rows, H, L);
      a.cc = a.partial + (size_t)2 * a.slots * H;
      gn_general<true>(dtype, nv.v, (int)ceil_div(((int64_t)a.slots * H) << a.lg, 256), a, stream);
    }
    MI355_LAUNCH_CHECK();
  }
  return norm_launch_dwdb(a.partial, partial_rows, (int)H, weight_dtype, dweight, dbias, stream);
}
