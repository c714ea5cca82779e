// Device helpers shared by the row-norm kernels (norm_ops.hip, norm_family_ops.hip, group_norm_ops.hip): the DPP wave sum,
// the row sum through LDS, the Philox draw of the dropout masks, parameter loads, the kernel that folds the dw / db partial
// rows, and the host-side piece-width choice.  Moved here from norm_ops.hip unchanged (its device code compiles to the same
// instructions as before the move).
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

// the draw of one element; not inlined: the element-wise kernels hold 32 elements a thread, and 32 generators expanded in
// line and interleaved by the scheduler spill thousands of bytes a lane
static __device__ __noinline__ uint32_t philox_draw1(uint32_t rl, uint32_t rh, uint32_t c, uint32_t which, uint32_t k0, uint32_t k1) {
  const uint4 r = philox4x32(make_uint4(rl, rh, c >> 2, which), make_uint2(k0, k1));
  return (c & 3) == 0 ? r.x : (c & 3) == 1 ? r.y : (c & 3) == 2 ? r.z : r.w;
}

// the keep / scale of V elements from column c of `row` under mask `which`; A carries seed_lo, seed_hi, thr and den
template <int V, class A>
__device__ __forceinline__ void drop_apply(const A& a, int64_t row, int c, uint32_t which, float (&v)[V]) {
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

static inline int norm_ebytes(int dtype) { return dtype == kF32 ? 4 : (dtype == kBF16 || dtype == kF16) ? 2 : 0; }

// the elements of one access: 16 bytes' worth, or 1 as soon as a base pointer or a stride is not a multiple of 16 bytes
struct NormVec {
  int v;
  void need(const void* p, int64_t stride_bytes) {
    if ((((uint64_t)(uintptr_t)p | (uint64_t)stride_bytes) % 16) != 0) v = 1;
  }
};

static inline bool norm_aligned(const void* p, int eb) { return ((uintptr_t)p % eb) == 0; }

}  // namespace mi355
