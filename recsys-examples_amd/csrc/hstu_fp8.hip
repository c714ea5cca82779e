// HSTU jagged attention on FP8 (OCP e4m3fn) operands for gfx950: the quantisers, the forward and the backward.
//
// Replaces (reference): hopper/hstu_attn_interface.py:32-292 (quantize_for_two_directions, quantize_for_block_scale,
// get_bm_and_bn_block_size_fwd, quantize_for_head_batch_tensor: Python loops over the batch) and the quant_mode >= 0 arms
// of hstu_hopper_cuda.varlen_fwd (hopper/hstu_api.cpp:520-566, mainloop_fwd_sm90_tma_gmma_ws.hpp:1342-1470).
//
// Quantisers: the same fp8 bytes and descales as the reference's PyTorch statements.
//  * every descale is max(amax / 448, 1e-6); modes 1 (per token) and 2 divide the amax in fp32, mode 1's vt descale and
//    modes 3 / 4 / 5 divide it in the INPUT dtype (bf16 / fp16, round to nearest even) before widening;
//  * x / descale is an fp32 division, rounded to e4m3fn as torch's Tensor.to(float8_e4m3fn) does (f32_to_e4m3); in mode 4
//    the reference's quotient keeps the input dtype (a 0-dim fp32 descale does not promote), so it is rounded there first;
//  * one launch per tensor (modes 0, 1, 2), two for modes 3 / 4 / 5 (an amax over 128-token tiles with one atomic per
//    tile, then the cast).  Tiles are found from cu_blocks (the per-sequence count of 128- or block-size-token tiles).
//
// Forward (self-attention, head_dim 64 / 128 / 256): one workgroup = 4 wave64 = 128 query rows of one (sequence, head),
// 64-key tiles, v_mfma_scale_f32_32x32x64_f8f6f4 with unit e8m0 scales (127) for both products and the descales applied
// in fp32 around them, as the reference applies them around its GMMA:
//  * GEMM 1: S^T = K Q^T (A = K tile from LDS, B = Q fragment kept in registers): the accumulator has the query row in the
//    lane and 16 keys per tile in the registers, ({0-3, 8-11, 16-19, 24-27} + 4 * lane half);
//  * S *= the mode's descale product, *= alpha, mask, SiLU; modes 1-5 divide P by s_P = max(1e-6, max |P|) / 448 over
//    the wave's 32 rows x the 64-key tile (the P group); P to e4m3 saturating at +-448 (v_cvt_pk_fp8_f32);
//  * GEMM 2: O^T += V^T P^T: the converted accumulator is the B operand as it stands; V is transposed on its way into
//    LDS with the accumulator's key permutation, so the A operand is one 32-byte row read.  Modes 1-5 compute each
//    tile's partial into a zeroed accumulator and add it times s_P * v_descale (mode 1: per column, descale_vt).
//  * O / scaling_seqlen written as fp16.
#include "common.h"
#include "../../include/recsys_amd.h"

namespace mi355 {
namespace hstu_fp8 {

typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));

constexpr float kFp8Max = 448.0f;
constexpr float kDescaleFloor = 1e-6f;

// fp32 -> e4m3fn, round to nearest even, as torch's float -> Float8_e4m3fn conversion: |f| >= 480 (and NaN) give 0x7f
// (NaN), values in [448, 480) round to 448, subnormals through an fp32 add that leaves the e4m3 subnormal step (2^-9) as
// the last bit of a number in [2^14, 2^15).
__device__ __forceinline__ uint32_t f32_to_e4m3(float f) {
  uint32_t bits = __float_as_uint(f);
  const uint32_t sign = bits & 0x80000000u;
  bits ^= sign;
  uint32_t r;
  if (bits >= (1087u << 20)) {
    r = 0x7f;
  } else if (bits < (121u << 23)) {
    const float t = __uint_as_float(bits) + __uint_as_float(141u << 23);
    r = (__float_as_uint(t) - (141u << 23)) & 0xffu;
  } else {
    const uint32_t odd = (bits >> 20) & 1u;
    bits += ((uint32_t)(7 - 127) << 23) + 0x7ffffu + odd;
    r = (bits >> 20) & 0xffu;
  }
  return r | (sign >> 24);
}

template <bool F16>
__device__ __forceinline__ float ld16(uint16_t u) { return F16 ? f16_to_f32(u) : bf16_to_f32(u); }
// a / 448 computed in the input dtype (torch: opmath fp32, then one rounding to bf16 / fp16)
template <bool F16>
__device__ __forceinline__ float div_in_dtype(float amax) {
  const float d = amax / kFp8Max;
  return F16 ? f16_to_f32(f32_to_f16(d)) : bf16_to_f32(f32_to_bf16(d));
}

// 8 consecutive 16-bit inputs -> 8 floats
template <bool F16>
__device__ __forceinline__ void load8(const uint16_t* p, float* f) {
  const uint4 u = *(const uint4*)p;
  const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = ld16<F16>((uint16_t)(w[i] & 0xffffu));
    f[2 * i + 1] = ld16<F16>((uint16_t)(w[i] >> 16));
  }
}
// x / descale to e4m3; in_dtype: the quotient is rounded to the input dtype first (mode 4 of the reference divides a bf16 /
// fp16 slice by a 0-dim fp32 descale, which keeps the slice's dtype: two roundings)
template <bool F16>
__device__ __forceinline__ uint2 cvt8(const float* f, float descale, bool scaled, bool in_dtype = false) {
  uint32_t w[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    uint32_t v = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float y = scaled ? f[4 * i + e] / descale : f[4 * i + e];
      if (in_dtype) y = F16 ? f16_to_f32(f32_to_f16(y)) : bf16_to_f32(f32_to_bf16(y));
      v |= f32_to_e4m3(y) << (8 * e);
    }
    w[i] = v;
  }
  return make_uint2(w[0], w[1]);
}

// the sequence b whose tiles [cu[b], cu[b+1]) hold tile g
__device__ __forceinline__ int tile_seq(const int32_t* cu, int B, int g) {
  int lo = 0, hi = B;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (cu[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
// max over the 256 threads of the block (every thread gets it)
__device__ __forceinline__ float block_max(float v, float* red) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

__global__ void cu_blocks_kernel(const int32_t* off, int B, int bs, int32_t* cu) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int s = 0;
  cu[0] = 0;
  for (int b = 0; b < B; ++b) {
    s += (off[b + 1] - off[b] + bs - 1) / bs;
    cu[b + 1] = s;
  }
}

// mode 0: plain cast
template <bool F16>
__global__ void __launch_bounds__(256) cast_kernel(const uint16_t* x, uint8_t* y, int64_t n8) {
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
    float f[8];
    load8<F16>(x + 8 * i, f);
    *(uint2*)(y + 8 * i) = cvt8<F16>(f, 1.0f, false);
  }
}

// mode 1, q / k: one descale per (token, head) row; descale[h * ds + t]
template <bool F16>
__global__ void __launch_bounds__(256) token_kernel(const uint16_t* x, uint8_t* y, int64_t rows, int H, int D, float* ds,
                                                    int64_t dstride) {
  const int tpr = D / 8;                       // threads per row: 4 .. 32, a power of two inside one wave
  const int rpb = 256 / tpr;
  const int sub = threadIdx.x % tpr;
  for (int64_t r0 = (int64_t)blockIdx.x * rpb; r0 < rows; r0 += (int64_t)gridDim.x * rpb) {
    const int64_t r = r0 + threadIdx.x / tpr;
    float f[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (r < rows) load8<F16>(x + r * D + 8 * sub, f);
    float m = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) m = fmaxf(m, fabsf(f[i]));
    for (int o = tpr >> 1; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    const float d = fmaxf(m / kFp8Max, kDescaleFloor);
    if (r < rows) {
      *(uint2*)(y + r * D + 8 * sub) = cvt8<F16>(f, d, true);
      if (sub == 0) ds[(r % H) * dstride + r / H] = d;
    }
  }
}

// mode 1, vt: one descale per (128-token tile, head, column); descale_vt[g * H * D + h * D + c]
template <bool F16>
__global__ void __launch_bounds__(256) vt_kernel(const uint16_t* x, uint8_t* y, const int32_t* off, const int32_t* cu, int B,
                                                 int HD, float* ds) {
  const int g = blockIdx.x;
  if (g >= cu[B]) return;
  const int col = blockIdx.y * 256 + threadIdx.x;
  if (col >= HD) return;
  const int b = tile_seq(cu, B, g);
  const int t0 = off[b] + (g - cu[b]) * 128, t1 = min(t0 + 128, off[b + 1]);
  float m = 0.f;
  for (int t = t0; t < t1; ++t) m = fmaxf(m, fabsf(ld16<F16>(x[(int64_t)t * HD + col])));
  const float d = fmaxf(div_in_dtype<F16>(m), kDescaleFloor);
  ds[(int64_t)g * HD + col] = d;
  for (int t = t0; t < t1; ++t) y[(int64_t)t * HD + col] = (uint8_t)f32_to_e4m3(ld16<F16>(x[(int64_t)t * HD + col]) / d);
}

// amax of the [t0, t1) x D tile of head h (256 threads)
template <bool F16>
__device__ __forceinline__ float tile_amax(const uint16_t* x, int t0, int t1, int h, int H, int D, float* red) {
  const int vpr = D / 8;
  const int n = (t1 - t0) * vpr;
  float m = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) {
    float f[8];
    load8<F16>(x + ((int64_t)(t0 + i / vpr) * H + h) * D + 8 * (i % vpr), f);
#pragma unroll
    for (int e = 0; e < 8; ++e) m = fmaxf(m, fabsf(f[e]));
  }
  return block_max(m, red);
}
template <bool F16>
__device__ __forceinline__ void tile_cast(const uint16_t* x, uint8_t* y, int t0, int t1, int h, int H, int D, float d,
                                          bool in_dtype = false) {
  const int vpr = D / 8;
  const int n = (t1 - t0) * vpr;
  for (int i = threadIdx.x; i < n; i += 256) {
    const int64_t e = ((int64_t)(t0 + i / vpr) * H + h) * D + 8 * (i % vpr);
    float f[8];
    load8<F16>(x + e, f);
    *(uint2*)(y + e) = cvt8<F16>(f, d, true, in_dtype);
  }
}

// mode 2: one descale per (block of bs tokens, head); descale[h * ds + g]
template <bool F16>
__global__ void __launch_bounds__(256) block_kernel(const uint16_t* x, uint8_t* y, const int32_t* off, const int32_t* cu, int B,
                                                    int bs, int H, int D, float* ds, int64_t dstride) {
  __shared__ float red[4];
  const int g = blockIdx.x, h = blockIdx.y;
  if (g >= cu[B]) return;
  const int b = tile_seq(cu, B, g);
  const int t0 = off[b] + (g - cu[b]) * bs, t1 = min(t0 + bs, off[b + 1]);
  const float d = fmaxf(tile_amax<F16>(x, t0, t1, h, H, D, red) / kFp8Max, kDescaleFloor);
  if (threadIdx.x == 0) ds[h * dstride + g] = d;
  tile_cast<F16>(x, y, t0, t1, h, H, D, d);
}

// modes 3 / 4 / 5 (kind 4 / 5 / 6): the group of a (sequence, head) tile
__device__ __forceinline__ int group_of(int kind, int b, int h, int H) { return kind == 4 ? b * H + h : kind == 5 ? b : 0; }

template <bool F16>
__global__ void __launch_bounds__(256) group_amax_kernel(const uint16_t* x, const int32_t* off, const int32_t* cu, int B, int H,
                                                         int D, int kind, uint32_t* amax) {
  __shared__ float red[4];
  const int g = blockIdx.x, h = blockIdx.y;
  if (g >= cu[B]) return;
  const int b = tile_seq(cu, B, g);
  const int t0 = off[b] + (g - cu[b]) * 128, t1 = min(t0 + 128, off[b + 1]);
  const float m = tile_amax<F16>(x, t0, t1, h, H, D, red);
  if (threadIdx.x == 0) atomicMax(amax + group_of(kind, b, h, H), __float_as_uint(m));   // (m >= 0: bits order as values)
}
template <bool F16>
__global__ void __launch_bounds__(256) group_cast_kernel(const uint16_t* x, uint8_t* y, const int32_t* off, const int32_t* cu,
                                                         int B, int H, int D, int kind, const uint32_t* amax, float* ds) {
  const int g = blockIdx.x, h = blockIdx.y;
  if (g >= cu[B]) return;
  const int b = tile_seq(cu, B, g);
  const int t0 = off[b] + (g - cu[b]) * 128, t1 = min(t0 + 128, off[b + 1]);
  const int grp = group_of(kind, b, h, H);
  const float d = fmaxf(div_in_dtype<F16>(__uint_as_float(amax[grp])), kDescaleFloor);
  const bool writer = kind == 6 ? g == 0 && h == 0 : g == cu[b] && (kind == 4 || h == 0);
  if (writer && threadIdx.x == 0) ds[grp] = d;
  tile_cast<F16>(x, y, t0, t1, h, H, D, d, kind == 5);
}

template <bool F16>
static int quantize(int kind, const void* xv, int64_t T, int64_t H, int64_t D, const int32_t* off, int64_t B, int64_t bs,
                    const int32_t* cu, int64_t nblk, void* yv, float* ds, int64_t dstride, uint32_t* amax,
                    hipStream_t st) {
  const uint16_t* x = (const uint16_t*)xv;
  uint8_t* y = (uint8_t*)yv;
  const int HD = (int)(H * D);
  if (T == 0) return MI355_OK;
  switch (kind) {
    case 0:
      cast_kernel<F16><<<grid_for(T * HD / 8, 256), 256, 0, st>>>(x, y, T * HD / 8);
      break;
    case 1:
      token_kernel<F16><<<grid_for(T * H, 256 / (D / 8)), 256, 0, st>>>(x, y, T * H, (int)H, (int)D, ds, dstride);
      break;
    case 2:
      if (nblk > 0) vt_kernel<F16><<<dim3((unsigned)nblk, (unsigned)ceil_div(HD, 256)), 256, 0, st>>>(x, y, off, cu, (int)B, HD, ds);
      break;
    case 3:
      if (nblk > 0)
        block_kernel<F16><<<dim3((unsigned)nblk, (unsigned)H), 256, 0, st>>>(x, y, off, cu, (int)B, (int)bs, (int)H, (int)D, ds,
                                                                             dstride);
      break;
    default:
      if (nblk > 0) {
        group_amax_kernel<F16><<<dim3((unsigned)nblk, (unsigned)H), 256, 0, st>>>(x, off, cu, (int)B, (int)H, (int)D, kind, amax);
        group_cast_kernel<F16><<<dim3((unsigned)nblk, (unsigned)H), 256, 0, st>>>(x, y, off, cu, (int)B, (int)H, (int)D, kind,
                                                                                  amax, ds);
      }
  }
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

// ---------------------------------------------------------------------------------------------------------------- forward

struct Fp8FwdArgs {
  const uint8_t *q, *k, *v;
  uint16_t* out;
  int64_t q_rs, k_rs, v_rs, o_rs, q_hs, k_hs, v_hs, o_hs;
  const int32_t* cu;
  int B, H, nqb;
  const int32_t *nc, *nt;
  int group, wl, wr;
  float alpha, scaling;
  const float *dq, *dk, *dv;
  int64_t dq_s, dk_s, dv_s;
  const int32_t *cu_vt, *cu_bq, *cu_bkv;
  int block_kv;
};

__device__ __forceinline__ v8i lds32(const uint8_t* p) {
  const uint4 a = *(const uint4*)p, b = *(const uint4*)(p + 16);
  v8i r;
  r[0] = a.x; r[1] = a.y; r[2] = a.z; r[3] = a.w; r[4] = b.x; r[5] = b.y; r[6] = b.z; r[7] = b.w;
  return r;
}
__device__ __forceinline__ v16f mfma_fp8(v8i a, v8i b, v16f c) {
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 0, 0, 0, 127, 0, 127);
}
// 4 floats (already inside +-448) -> 4 e4m3 bytes
__device__ __forceinline__ int pack4(float a, float b, float c, float d) {
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
  return __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
}
// the position of key k (0..63) of a tile in a V^T row: the accumulator's key order (see the head of this file)
__device__ __forceinline__ int vt_pos(int k) { return 32 * ((k >> 2) & 1) + 16 * (k >> 5) + 4 * ((k >> 3) & 3) + (k & 3); }

struct Mask {
  int nc, hist, group, wl, wr;
  bool ctx, tgt;
  __device__ __forceinline__ bool operator()(int i, int j) const {
    if (ctx || tgt) {   // contextual / target rows come with the causal mask (hstu_attn_varlen_func checks it)
      const int ii = ctx ? max(i - nc + 1, 0) : i, jj = ctx ? max(j - nc + 1, 0) : j;
      bool m = i == j || jj < ii;
      if (tgt) {
        const int gi = i >= hist ? (i - hist) / group : -1, gj = j >= hist ? (j - hist) / group : -1;
        m = m && (gi == gj || gi < 0 || gj < 0);
      }
      if (ctx) m = m || (ii == 0 && j < hist);
      return m;
    }
    return (wl < 0 || j >= i - wl) && (wr < 0 || j <= i + wr);
  }
};

template <int D, int MODE>
__global__ void __launch_bounds__(256) hstu_fp8_fwd_kernel(Fp8FwdArgs a) {
  constexpr int KP = D + 16;   // K tile row pitch (bytes)
  constexpr int VP = 64 + 16;  // V^T tile row pitch
  constexpr int NC = D / 64;   // 64-deep k steps of GEMM 1
  constexpr int NO = D / 32;   // 32-column blocks of O
  __shared__ __attribute__((aligned(16))) uint8_t sK[64 * KP];
  __shared__ __attribute__((aligned(16))) uint8_t sV[D * VP];
  __shared__ float sDk[64];
  __shared__ float sDv[D];

  const int b = blockIdx.x / a.nqb, qb = blockIdx.x % a.nqb, h = blockIdx.y;
  const int s0 = a.cu[b], L = a.cu[b + 1] - s0;
  const int r0 = qb * 128;
  if (r0 >= L) return;   // uniform over the workgroup, ahead of every barrier
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, lr = lane & 31, lh = lane >> 5;
  const int row = r0 + 32 * w + lr;
  const bool row_ok = row < L;

  Mask mk;
  mk.ctx = a.nc != nullptr;
  mk.tgt = a.nt != nullptr;
  mk.nc = mk.ctx ? a.nc[b] : 0;
  mk.hist = L - (mk.tgt ? a.nt[b] : 0);
  mk.group = a.group;
  mk.wl = a.wl;
  mk.wr = a.wr;

  const int rlast = min(r0 + 128, L) - 1;
  int kmin = a.wl >= 0 ? max(0, r0 - a.wl) : 0;
  int kmax = a.wr >= 0 ? min(L, rlast + a.wr + 1) : L;
  if (mk.ctx && r0 < mk.nc) kmax = L;
  kmin &= ~63;   // tiles start on 64-key boundaries of the sequence: inside one mode-1 / mode-2 descale block

  // Q: B operand of GEMM 1, lane (row lr, half lh) holds dims 64c + 32lh .. +31
  v8i qf[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    if (row_ok) qf[c] = lds32(a.q + (int64_t)(s0 + row) * a.q_rs + h * a.q_hs + 64 * c + 32 * lh);
    else qf[c] = v8i{0, 0, 0, 0, 0, 0, 0, 0};
  }
  float dq_row = 1.f, dqk = 1.f, dv_u = 1.f;
  if (MODE == 1) dq_row = row_ok ? a.dq[h * a.dq_s + s0 + row] : 0.f;
  if (MODE == 2) dq_row = a.dq[h * a.dq_s + a.cu_bq[b] + r0 / 128];
  if (MODE == 3) { dqk = a.dq[b * a.H + h] * a.dk[b * a.H + h]; dv_u = a.dv[b * a.H + h]; }
  if (MODE == 4) { dqk = a.dq[b] * a.dk[b]; dv_u = a.dv[b]; }
  if (MODE == 5) { dqk = a.dq[0] * a.dk[0]; dv_u = a.dv[0]; }

  v16f o[NO];
#pragma unroll
  for (int n = 0; n < NO; ++n) o[n] = v16f{};

  const int wr0 = r0 + 32 * w, wr1 = wr0 + 31;
  for (int kt = kmin; kt < kmax; kt += 64) {
    __syncthreads();
    // K tile [64 keys][D], zero past the sequence
    for (int i = tid; i < 64 * D / 16; i += 256) {
      const int r = i / (D / 16), c = i % (D / 16), key = kt + r;
      uint4 val = make_uint4(0, 0, 0, 0);
      if (key < L) val = *(const uint4*)(a.k + (int64_t)(s0 + key) * a.k_rs + h * a.k_hs + 16 * c);
      *(uint4*)(sK + r * KP + 16 * c) = val;
    }
    // V^T tile [D][64 keys in the accumulator's order]: 4 keys x 16 columns per thread, transposed in registers
    for (int i = tid; i < D; i += 256) {
      const int cg = i % (D / 16), kg = i / (D / 16);
      uint32_t rw[4][4];
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const int key = kt + 4 * kg + x;
        uint4 val = make_uint4(0, 0, 0, 0);
        if (key < L) val = *(const uint4*)(a.v + (int64_t)(s0 + key) * a.v_rs + h * a.v_hs + 16 * cg);
        rw[x][0] = val.x; rw[x][1] = val.y; rw[x][2] = val.z; rw[x][3] = val.w;
      }
      const int pos = vt_pos(4 * kg);
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const uint32_t t = ((rw[0][u] >> (8 * e)) & 0xffu) | (((rw[1][u] >> (8 * e)) & 0xffu) << 8) |
                             (((rw[2][u] >> (8 * e)) & 0xffu) << 16) | (((rw[3][u] >> (8 * e)) & 0xffu) << 24);
          *(uint32_t*)(sV + (16 * cg + 4 * u + e) * VP + pos) = t;
        }
    }
    if (MODE == 1) {
      if (tid < 64) sDk[tid] = kt + tid < L ? a.dk[h * a.dk_s + s0 + kt + tid] : 0.f;
      const float* dvt = a.dv + (int64_t)(a.cu_vt[b] + kt / 128) * a.dv_s + h * D;
      for (int c = tid; c < D; c += 256) sDv[c] = dvt[c];
    }
    __syncthreads();

    // GEMM 1: S^T (two 32-key tiles)
    v16f s[2] = {v16f{}, v16f{}};
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int t = 0; t < 2; ++t) s[t] = mfma_fp8(lds32(sK + (32 * t + lr) * KP + 64 * c + 32 * lh), qf[c], s[t]);

    float sc = a.alpha;
    if (MODE == 2) sc *= dq_row * a.dk[h * a.dk_s + a.cu_bkv[b] + kt / a.block_kv];
    if (MODE >= 3) sc *= dqk;
    const bool interior = !mk.ctx && !mk.tgt && (a.wl < 0 || kt >= wr1 - a.wl) && (a.wr < 0 || kt + 63 <= wr0 + a.wr);
    float pmax = 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kk = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * lh;
        float x = s[t][r];
        if (MODE == 1) x = x * (dq_row * sDk[kk]);
        x *= sc;
        x = x / (1.f + __expf(-x));
        if (!interior && !mk(row, kt + kk)) x = 0.f;
        s[t][r] = x;
        pmax = fmaxf(pmax, fabsf(x));
      }
    float sp = 1.f;
    if (MODE != 0) {
      const float m = fmaxf(wave_max(pmax), kDescaleFloor);
      sp = m / kFp8Max;
      const float inv = kFp8Max / m;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) s[t][r] *= inv;
    }
    v8i pf;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        float f[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) f[e] = fminf(fmaxf(s[t][4 * g + e], -kFp8Max), kFp8Max);
        pf[4 * t + g] = pack4(f[0], f[1], f[2], f[3]);
      }

    // GEMM 2: O^T += V^T P^T
    float mult = sp * dv_u;
    if (MODE == 2) mult = sp * a.dv[h * a.dv_s + a.cu_bkv[b] + kt / a.block_kv];
#pragma unroll
    for (int n = 0; n < NO; ++n) {
      const v8i va = lds32(sV + (32 * n + lr) * VP + 32 * lh);
      if (MODE == 0) {
        o[n] = mfma_fp8(va, pf, o[n]);
      } else {
        const v16f part = mfma_fp8(va, pf, v16f{});
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float m = MODE == 1 ? sp * sDv[32 * n + (r & 3) + 8 * (r >> 2) + 4 * lh] : mult;
          o[n][r] += part[r] * m;
        }
      }
    }
  }

  if (!row_ok) return;
  uint16_t* op = a.out + (int64_t)(s0 + row) * a.o_rs + h * a.o_hs;
#pragma unroll
  for (int n = 0; n < NO; ++n)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int col = 32 * n + 8 * g + 4 * lh;
      uint32_t lo = (uint32_t)f32_to_f16(o[n][4 * g] / a.scaling) | ((uint32_t)f32_to_f16(o[n][4 * g + 1] / a.scaling) << 16);
      uint32_t hi = (uint32_t)f32_to_f16(o[n][4 * g + 2] / a.scaling) | ((uint32_t)f32_to_f16(o[n][4 * g + 3] / a.scaling) << 16);
      *(uint2*)(op + col) = make_uint2(lo, hi);
    }
}

template <int D>
static void launch_fwd(int mode, const Fp8FwdArgs& a, dim3 grid, hipStream_t st) {
  switch (mode) {
    case 0: hstu_fp8_fwd_kernel<D, 0><<<grid, 256, 0, st>>>(a); break;
    case 1: hstu_fp8_fwd_kernel<D, 1><<<grid, 256, 0, st>>>(a); break;
    case 2: hstu_fp8_fwd_kernel<D, 2><<<grid, 256, 0, st>>>(a); break;
    case 3: hstu_fp8_fwd_kernel<D, 3><<<grid, 256, 0, st>>>(a); break;
    case 4: hstu_fp8_fwd_kernel<D, 4><<<grid, 256, 0, st>>>(a); break;
    default: hstu_fp8_fwd_kernel<D, 5><<<grid, 256, 0, st>>>(a); break;
  }
}


// --------------------------------------------------------------------------------------------------------------- backward
//
// Two passes, both recomputing S = alpha Q K^T and dP = dO V^T on the fp8 operands (seven GEMMs instead of five, but no P /
// dS exchange between workgroups, no atomics and no workspace):
//  * key-major (hstu_fp8_bwd_dkdv_kernel): one workgroup = 4 waves x 32 keys = 128 keys of one (sequence, head), aligned
//    to the sequence start so that they lie in one 128-token k / kt / v descale block; 64-query steps, aligned likewise
//    (one 64-token q / dout block of mode 2, one 128-token qt / dout_t block of mode 1).  S and dP come out with the key in
//    the lane and 16 queries per 32-query tile in the registers; converted, they are the B operand of
//    dV^T += dO^T P^T and dK^T += Q^T dS^T, whose A operands are dO^T / Q^T (dout_t / qt in mode 1) transposed into LDS
//    with the accumulator's query permutation (vt_pos), as the forward fills V^T.
//  * query-major (hstu_fp8_bwd_dq_kernel): the forward's shape, 4 waves x 32 queries, 64-key tiles; dQ^T += K^T dS^T with
//    K^T (kt in mode 1) transposed into LDS.
// P and dS are divided by s = max(1e-6, max |x|) / 448 over their group before the e4m3 cast (modes 1-5; mode 0 casts
// straight, saturating at +-448): the wave's 32 keys x 64 queries in the key-major pass, its 32 queries x 64 keys in the
// query-major one; each tile's partial product is computed into a zeroed accumulator and added times s and the partner's
// descale.  dS = dP SiLU'(S) alpha / N, dV = P^T dO / N; dq / dk / dv are written as fp16.

struct Fp8BwdArgs {
  const uint8_t *q, *k, *v, *dout, *qt, *kt, *dot;   // qt / kt / dot alias q / k / dout outside mode 1
  uint16_t *dq, *dk, *dv;
  int64_t q_rs, k_rs, v_rs, do_rs, qt_rs, kt_rs, dot_rs, dq_rs, dk_rs, dv_rs;   // token strides (bytes / fp16 elements)
  int64_t q_hs, k_hs, v_hs, do_hs, qt_hs, kt_hs, dot_hs, dq_hs, dk_hs, dv_hs;   // head strides
  const int32_t* cu;
  int B, H, nqb, nkb;
  const int32_t *nc, *nt;
  int group, wl, wr;
  float alpha, scaling;
  const float *s_q, *s_qt, *s_k, *s_kt, *s_v, *s_do, *s_dot;
  int64_t s_q_s, s_qt_s, s_k_s, s_kt_s, s_v_s, s_do_s, s_dot_s;
  const int32_t *cu_qt, *cu_kt, *cu_bq, *cu_bkv;
};

// rows [t0, t0 + 64) of x (one head; x already offset by it) into s[64][D + 16], zero past the sequence
template <int D>
__device__ __forceinline__ void fill_rows(uint8_t* s, const uint8_t* x, int64_t rs, int t0, int L) {
  for (int i = threadIdx.x; i < 64 * D / 16; i += 256) {
    const int r = i / (D / 16), c = i % (D / 16), t = t0 + r;
    uint4 val = make_uint4(0, 0, 0, 0);
    if (t < L) val = *(const uint4*)(x + (int64_t)t * rs + 16 * c);
    *(uint4*)(s + r * (D + 16) + 16 * c) = val;
  }
}
// the same rows transposed into s[D][64 + 16], token t0 + k at vt_pos(k): 4 tokens x 16 columns per thread
template <int D>
__device__ __forceinline__ void fill_t(uint8_t* s, const uint8_t* x, int64_t rs, int t0, int L) {
  for (int i = threadIdx.x; i < D; i += 256) {
    const int cg = i % (D / 16), kg = i / (D / 16);
    uint32_t rw[4][4];
#pragma unroll
    for (int y = 0; y < 4; ++y) {
      const int t = t0 + 4 * kg + y;
      uint4 val = make_uint4(0, 0, 0, 0);
      if (t < L) val = *(const uint4*)(x + (int64_t)t * rs + 16 * cg);
      rw[y][0] = val.x; rw[y][1] = val.y; rw[y][2] = val.z; rw[y][3] = val.w;
    }
    const int pos = vt_pos(4 * kg);
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const uint32_t t = ((rw[0][u] >> (8 * e)) & 0xffu) | (((rw[1][u] >> (8 * e)) & 0xffu) << 8) |
                           (((rw[2][u] >> (8 * e)) & 0xffu) << 16) | (((rw[3][u] >> (8 * e)) & 0xffu) << 24);
        *(uint32_t*)(s + (16 * cg + 4 * u + e) * 80 + pos) = t;
      }
  }
}

__device__ __forceinline__ Mask make_mask(const Fp8BwdArgs& a, int b, int L) {
  Mask mk;
  mk.ctx = a.nc != nullptr;
  mk.tgt = a.nt != nullptr;
  mk.nc = mk.ctx ? a.nc[b] : 0;
  mk.hist = L - (mk.tgt ? a.nt[b] : 0);
  mk.group = a.group;
  mk.wl = a.wl;
  mk.wr = a.wr;
  return mk;
}
// the modes-3 / 4 / 5 descale index of (sequence b, head h)
__device__ __forceinline__ int grp_idx(int mode, int b, int h, int H) { return mode == 3 ? b * H + h : mode == 4 ? b : 0; }

// x [2 tiles][16] -> e4m3 B operand; modes 1-5 divide by the group scale first (returned; 1 in mode 0)
template <int MODE>
__device__ __forceinline__ float to_fp8(v16f* x, float amax, v8i& f) {
  float sc = 1.f;
  if (MODE != 0) {
    const float m = fmaxf(wave_max(amax), kDescaleFloor);
    sc = m / kFp8Max;
    const float inv = kFp8Max / m;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) x[t][r] *= inv;
  }
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = fminf(fmaxf(x[t][4 * g + e], -kFp8Max), kFp8Max);
      f[4 * t + g] = pack4(v[0], v[1], v[2], v[3]);
    }
  return sc;
}
// acc[n] += A(n) x f, times mult (MODE 0: unscaled) or, in mode 1, times sc * col_ds[column]
template <int D, int MODE>
__device__ __forceinline__ void gemm_t(v16f* acc, const uint8_t* sA, v8i f, float sc, float mult, const float* col_ds,
                                       int lr, int lh) {
#pragma unroll
  for (int n = 0; n < D / 32; ++n) {
    const v8i va = lds32(sA + (32 * n + lr) * 80 + 32 * lh);
    if (MODE == 0) {
      acc[n] = mfma_fp8(va, f, acc[n]);
    } else {
      const v16f part = mfma_fp8(va, f, v16f{});
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float m = MODE == 1 ? sc * col_ds[32 * n + (r & 3) + 8 * (r >> 2) + 4 * lh] : mult;
        acc[n][r] += part[r] * m;
      }
    }
  }
}
// acc (lane = row, registers = columns) / div -> fp16 row of out
template <int D>
__device__ __forceinline__ void store_row(uint16_t* op, const v16f* acc, float div, int lh) {
#pragma unroll
  for (int n = 0; n < D / 32; ++n)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int col = 32 * n + 8 * g + 4 * lh;
      const uint32_t lo = (uint32_t)f32_to_f16(acc[n][4 * g] / div) | ((uint32_t)f32_to_f16(acc[n][4 * g + 1] / div) << 16);
      const uint32_t hi = (uint32_t)f32_to_f16(acc[n][4 * g + 2] / div) | ((uint32_t)f32_to_f16(acc[n][4 * g + 3] / div) << 16);
      *(uint2*)(op + col) = make_uint2(lo, hi);
    }
}

// PART: 3 computes dV and dK; at d = 256, where 2 x 128 accumulators and the S / dP tiles spill, the pass is two kernels,
// 1 (S, dV) and 2 (S, dP, dK): eight GEMMs instead of seven.
template <int D, int MODE, int PART>
__global__ void __launch_bounds__(256) hstu_fp8_bwd_dkdv_kernel(Fp8BwdArgs a) {
  constexpr int KP = D + 16, NC = D / 64, NO = D / 32;
  constexpr bool DV = PART & 1, DK = PART & 2;
  __shared__ __attribute__((aligned(16))) uint8_t sQ[64 * KP];
  __shared__ __attribute__((aligned(16))) uint8_t sDo[DK ? 64 * KP : 16];
  __shared__ __attribute__((aligned(16))) uint8_t sQT[DK ? D * 80 : 16];
  __shared__ __attribute__((aligned(16))) uint8_t sDoT[DV ? D * 80 : 16];
  __shared__ float sDq[64], sDdo[64], sDqt[MODE == 1 && DK ? D : 1], sDdot[MODE == 1 && DV ? D : 1];

  const int b = blockIdx.x / a.nkb, kb = blockIdx.x % a.nkb, h = blockIdx.y;
  const int s0 = a.cu[b], L = a.cu[b + 1] - s0;
  const int k0 = kb * 128;
  if (k0 >= L) return;   // uniform over the workgroup, ahead of every barrier
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, lr = lane & 31, lh = lane >> 5;
  const int key = k0 + 32 * w + lr;
  const bool key_ok = key < L;
  const Mask mk = make_mask(a, b, L);

  const int klast = min(k0 + 128, L) - 1;
  int qmin = a.wr >= 0 ? max(0, k0 - a.wr) : 0;
  const int qmax = a.wl >= 0 ? min(L, klast + a.wl + 1) : L;
  if (mk.ctx) qmin = 0;
  qmin &= ~63;

  const uint8_t* qh = a.q + (int64_t)s0 * a.q_rs + h * a.q_hs;
  const uint8_t* doh = a.dout + (int64_t)s0 * a.do_rs + h * a.do_hs;
  const uint8_t* qth = a.qt + (int64_t)s0 * a.qt_rs + h * a.qt_hs;
  const uint8_t* doth = a.dot + (int64_t)s0 * a.dot_rs + h * a.dot_hs;

  // K and V: B operands, lane (key lr, half lh) holds dims 64c + 32lh .. +31
  const uint8_t* kp = a.k + (int64_t)(s0 + key) * a.k_rs + h * a.k_hs + 32 * lh;
  const uint8_t* vp = a.v + (int64_t)(s0 + key) * a.v_rs + h * a.v_hs + 32 * lh;
  v8i kf[NC], vf[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    kf[c] = key_ok ? lds32(kp + 64 * c) : v8i{0, 0, 0, 0, 0, 0, 0, 0};
    vf[c] = key_ok && DK ? lds32(vp + 64 * c) : v8i{0, 0, 0, 0, 0, 0, 0, 0};
  }
  float dk_key = 1.f, dv_key = 1.f, u_q = 1.f, u_do = 1.f;
  if (MODE == 1) {
    dk_key = key_ok ? a.s_k[h * a.s_k_s + s0 + key] : 0.f;
    dv_key = key_ok ? a.s_v[h * a.s_v_s + s0 + key] : 0.f;
  }
  if (MODE == 2) {
    dk_key = a.s_k[h * a.s_k_s + a.cu_bkv[b] + k0 / 128];
    dv_key = a.s_v[h * a.s_v_s + a.cu_bkv[b] + k0 / 128];
  }
  if (MODE >= 3) {
    const int gi = grp_idx(MODE, b, h, a.H);
    dk_key = a.s_k[gi]; dv_key = a.s_v[gi]; u_q = a.s_q[gi]; u_do = a.s_do[gi];
  }
  const float dsc = a.alpha / a.scaling;

  v16f dva[DV ? NO : 1], dka[DK ? NO : 1];
#pragma unroll
  for (int n = 0; n < NO; ++n) {
    if (DV) dva[n] = v16f{};
    if (DK) dka[n] = v16f{};
  }

  for (int q0 = qmin; q0 < qmax; q0 += 64) {
    __syncthreads();
    fill_rows<D>(sQ, qh, a.q_rs, q0, L);
    if (DK) fill_rows<D>(sDo, doh, a.do_rs, q0, L);
    if (DK) fill_t<D>(sQT, qth, a.qt_rs, q0, L);
    if (DV) fill_t<D>(sDoT, doth, a.dot_rs, q0, L);
    if (MODE == 1) {
      if (tid < 64) {
        const bool ok = q0 + tid < L;
        sDq[tid] = ok ? a.s_q[h * a.s_q_s + s0 + q0 + tid] : 0.f;
        if (DK) sDdo[tid] = ok ? a.s_do[h * a.s_do_s + s0 + q0 + tid] : 0.f;
      }
      const int64_t tq = (int64_t)(a.cu_qt[b] + q0 / 128);
      for (int c = tid; c < D; c += 256) {
        if (DK) sDqt[c] = a.s_qt[tq * a.s_qt_s + h * D + c];
        if (DV) sDdot[c] = a.s_dot[tq * a.s_dot_s + h * D + c];
      }
    }
    __syncthreads();

    // S and dP, key in the lane: tile t, register r -> query q0 + 32t + (r & 3) + 8 (r >> 2) + 4 lh
    v16f s[2] = {v16f{}, v16f{}}, dp[2] = {v16f{}, v16f{}};
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        s[t] = mfma_fp8(lds32(sQ + (32 * t + lr) * KP + 64 * c + 32 * lh), kf[c], s[t]);
        if (DK) dp[t] = mfma_fp8(lds32(sDo + (32 * t + lr) * KP + 64 * c + 32 * lh), vf[c], dp[t]);
      }
    float ss = a.alpha, sd = 1.f, mq = u_q, mdo = u_do;
    if (MODE == 2) {
      mq = a.s_q[h * a.s_q_s + a.cu_bq[b] + q0 / 64];
      mdo = a.s_do[h * a.s_do_s + a.cu_bq[b] + q0 / 64];
    }
    if (MODE >= 2) { ss *= mq * dk_key; sd = mdo * dv_key; }
    float pmax = 0.f, dmax = 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int qq = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * lh, row = q0 + qq;
        float x = s[t][r] * ss, y = dp[t][r] * sd;
        if (MODE == 1) { x *= sDq[qq] * dk_key; if (DK) y *= sDdo[qq] * dv_key; }
        const float sg = 1.f / (1.f + __expf(-x));
        float p = x * sg, ds = DK ? y * sg * (1.f + x * (1.f - sg)) * dsc : 0.f;
        if (!key_ok || row >= L || !mk(row, key)) { p = 0.f; ds = 0.f; }
        s[t][r] = p;
        dp[t][r] = ds;
        pmax = fmaxf(pmax, fabsf(p));
        dmax = fmaxf(dmax, fabsf(ds));
      }
    if (DV) {   // dV^T += dO^T P^T
      v8i pf;
      const float sp = to_fp8<MODE>(s, pmax, pf);
      gemm_t<D, MODE>(dva, sDoT, pf, sp, sp * mdo, sDdot, lr, lh);
    }
    if (DK) {   // dK^T += Q^T dS^T
      v8i df;
      const float sds = to_fp8<MODE>(dp, dmax, df);
      gemm_t<D, MODE>(dka, sQT, df, sds, sds * mq, sDqt, lr, lh);
    }
  }

  if (!key_ok) return;
  if (DV) store_row<D>(a.dv + (int64_t)(s0 + key) * a.dv_rs + h * a.dv_hs, dva, a.scaling, lh);
  if (DK) store_row<D>(a.dk + (int64_t)(s0 + key) * a.dk_rs + h * a.dk_hs, dka, 1.f, lh);
}

template <int D, int MODE>
__global__ void __launch_bounds__(256) hstu_fp8_bwd_dq_kernel(Fp8BwdArgs a) {
  constexpr int KP = D + 16, NC = D / 64, NO = D / 32;
  __shared__ __attribute__((aligned(16))) uint8_t sK[64 * KP];
  __shared__ __attribute__((aligned(16))) uint8_t sV[64 * KP];
  __shared__ __attribute__((aligned(16))) uint8_t sKT[D * 80];
  __shared__ float sDk[64], sDv[64], sDkt[MODE == 1 ? D : 1];

  const int b = blockIdx.x / a.nqb, qb = blockIdx.x % a.nqb, h = blockIdx.y;
  const int s0 = a.cu[b], L = a.cu[b + 1] - s0;
  const int r0 = qb * 128;
  if (r0 >= L) return;   // uniform over the workgroup, ahead of every barrier
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, lr = lane & 31, lh = lane >> 5;
  const int row = r0 + 32 * w + lr;
  const bool row_ok = row < L;
  const Mask mk = make_mask(a, b, L);

  const int rlast = min(r0 + 128, L) - 1;
  int kmin = a.wl >= 0 ? max(0, r0 - a.wl) : 0;
  int kmax = a.wr >= 0 ? min(L, rlast + a.wr + 1) : L;
  if (mk.ctx && r0 < mk.nc) kmax = L;
  kmin &= ~63;

  const uint8_t* kh = a.k + (int64_t)s0 * a.k_rs + h * a.k_hs;
  const uint8_t* vh = a.v + (int64_t)s0 * a.v_rs + h * a.v_hs;
  const uint8_t* kth = a.kt + (int64_t)s0 * a.kt_rs + h * a.kt_hs;

  // Q and dO: B operands, lane (row lr, half lh) holds dims 64c + 32lh .. +31
  v8i qf[NC], of[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    if (row_ok) {
      qf[c] = lds32(a.q + (int64_t)(s0 + row) * a.q_rs + h * a.q_hs + 64 * c + 32 * lh);
      of[c] = lds32(a.dout + (int64_t)(s0 + row) * a.do_rs + h * a.do_hs + 64 * c + 32 * lh);
    } else {
      qf[c] = v8i{0, 0, 0, 0, 0, 0, 0, 0};
      of[c] = v8i{0, 0, 0, 0, 0, 0, 0, 0};
    }
  }
  float dq_row = 1.f, ddo_row = 1.f, u_k = 1.f, u_v = 1.f;
  if (MODE == 1) {
    dq_row = row_ok ? a.s_q[h * a.s_q_s + s0 + row] : 0.f;
    ddo_row = row_ok ? a.s_do[h * a.s_do_s + s0 + row] : 0.f;
  }
  if (MODE == 2) {   // the wave's 32 rows lie in one 64-row block
    dq_row = a.s_q[h * a.s_q_s + a.cu_bq[b] + (r0 + 32 * w) / 64];
    ddo_row = a.s_do[h * a.s_do_s + a.cu_bq[b] + (r0 + 32 * w) / 64];
  }
  if (MODE >= 3) {
    const int gi = grp_idx(MODE, b, h, a.H);
    dq_row = a.s_q[gi]; ddo_row = a.s_do[gi]; u_k = a.s_k[gi]; u_v = a.s_v[gi];
  }
  const float dsc = a.alpha / a.scaling;

  v16f dqa[NO];
#pragma unroll
  for (int n = 0; n < NO; ++n) dqa[n] = v16f{};

  for (int kt = kmin; kt < kmax; kt += 64) {
    __syncthreads();
    fill_rows<D>(sK, kh, a.k_rs, kt, L);
    fill_rows<D>(sV, vh, a.v_rs, kt, L);
    fill_t<D>(sKT, kth, a.kt_rs, kt, L);
    if (MODE == 1) {
      if (tid < 64) {
        const bool ok = kt + tid < L;
        sDk[tid] = ok ? a.s_k[h * a.s_k_s + s0 + kt + tid] : 0.f;
        sDv[tid] = ok ? a.s_v[h * a.s_v_s + s0 + kt + tid] : 0.f;
      }
      const int64_t tk = (int64_t)(a.cu_kt[b] + kt / 128);
      for (int c = tid; c < D; c += 256) sDkt[c] = a.s_kt[tk * a.s_kt_s + h * D + c];
    }
    __syncthreads();

    // S^T and dP^T, query in the lane: tile t, register r -> key kt + 32t + (r & 3) + 8 (r >> 2) + 4 lh
    v16f s[2] = {v16f{}, v16f{}}, dp[2] = {v16f{}, v16f{}};
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        s[t] = mfma_fp8(lds32(sK + (32 * t + lr) * KP + 64 * c + 32 * lh), qf[c], s[t]);
        dp[t] = mfma_fp8(lds32(sV + (32 * t + lr) * KP + 64 * c + 32 * lh), of[c], dp[t]);
      }
    float ss = a.alpha, sd = 1.f, mk_ = u_k;
    if (MODE == 2) {
      mk_ = a.s_k[h * a.s_k_s + a.cu_bkv[b] + kt / 128];
      u_v = a.s_v[h * a.s_v_s + a.cu_bkv[b] + kt / 128];
    }
    if (MODE >= 2) { ss *= dq_row * mk_; sd = ddo_row * u_v; }
    float dmax = 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kk = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * lh, key = kt + kk;
        float x = s[t][r] * ss, y = dp[t][r] * sd;
        if (MODE == 1) { x *= dq_row * sDk[kk]; y *= ddo_row * sDv[kk]; }
        const float sg = 1.f / (1.f + __expf(-x));
        float ds = y * sg * (1.f + x * (1.f - sg)) * dsc;
        if (!row_ok || key >= L || !mk(row, key)) ds = 0.f;
        dp[t][r] = ds;
        dmax = fmaxf(dmax, fabsf(ds));
      }
    v8i df;
    const float sds = to_fp8<MODE>(dp, dmax, df);
    gemm_t<D, MODE>(dqa, sKT, df, sds, sds * mk_, sDkt, lr, lh);   // dQ^T += K^T dS^T
  }

  if (!row_ok) return;
  store_row<D>(a.dq + (int64_t)(s0 + row) * a.dq_rs + h * a.dq_hs, dqa, 1.f, lh);
}

template <int D, int MODE>
static void launch_bwd_mode(const Fp8BwdArgs& a, dim3 gk, dim3 gq, hipStream_t st) {
  if constexpr (D == 256) {
    hstu_fp8_bwd_dkdv_kernel<D, MODE, 1><<<gk, 256, 0, st>>>(a);
    hstu_fp8_bwd_dkdv_kernel<D, MODE, 2><<<gk, 256, 0, st>>>(a);
  } else {
    hstu_fp8_bwd_dkdv_kernel<D, MODE, 3><<<gk, 256, 0, st>>>(a);
  }
  hstu_fp8_bwd_dq_kernel<D, MODE><<<gq, 256, 0, st>>>(a);
}
template <int D>
static void launch_bwd(int mode, const Fp8BwdArgs& a, dim3 gk, dim3 gq, hipStream_t st) {
  switch (mode) {
    case 0: launch_bwd_mode<D, 0>(a, gk, gq, st); break;
    case 1: launch_bwd_mode<D, 1>(a, gk, gq, st); break;
    case 2: launch_bwd_mode<D, 2>(a, gk, gq, st); break;
    case 3: launch_bwd_mode<D, 3>(a, gk, gq, st); break;
    case 4: launch_bwd_mode<D, 4>(a, gk, gq, st); break;
    default: launch_bwd_mode<D, 5>(a, gk, gq, st); break;
  }
}

}  // namespace hstu_fp8
}  // namespace mi355

using namespace mi355;
using namespace mi355::hstu_fp8;

extern "C" int mi355_hstu_fp8_cu_blocks(const int32_t* seq_offsets, int64_t batch, int64_t block_size, int32_t* cu_blocks,
                                        hipStream_t stream) {
  MI355_CHECK_ARG(seq_offsets && cu_blocks && batch >= 0, "hstu_fp8_cu_blocks: null pointer or negative batch");
  MI355_CHECK_ARG(block_size > 0, "hstu_fp8_cu_blocks: block_size must be positive");
  cu_blocks_kernel<<<1, 1, 0, stream>>>(seq_offsets, (int)batch, (int)block_size, cu_blocks);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

extern "C" int64_t mi355_hstu_fp8_blocks_bound(int64_t total, int64_t batch, int64_t block_size) {
  return block_size > 0 ? total / block_size + batch : 0;
}

extern "C" int mi355_hstu_fp8_quantize(int kind, const void* x, int x_is_f16, int64_t total, int64_t num_heads,
                                       int64_t head_dim, const int32_t* seq_offsets, int64_t batch, int64_t block_size,
                                       const int32_t* cu_blocks, int64_t num_blocks_bound, void* out_fp8, float* descale,
                                       int64_t descale_stride, uint32_t* amax_work, hipStream_t stream) {
  MI355_CHECK_ARG(kind >= 0 && kind <= 6, "hstu_fp8_quantize: kind must be 0 .. 6");
  MI355_CHECK_ARG(x && out_fp8 && total >= 0 && num_heads > 0, "hstu_fp8_quantize: null tensor or bad shape");
  MI355_CHECK_ARG(head_dim == 32 || head_dim == 64 || head_dim == 128 || head_dim == 256,
                  "hstu_fp8_quantize: head_dim must be 32, 64, 128 or 256");
  MI355_CHECK_ARG(kind == 0 || descale, "hstu_fp8_quantize: descale is null");
  MI355_CHECK_ARG(kind <= 1 || (seq_offsets && cu_blocks && batch > 0), "hstu_fp8_quantize: seq_offsets / cu_blocks missing");
  MI355_CHECK_ARG(kind != 3 || block_size > 0, "hstu_fp8_quantize: block_size must be positive");
  MI355_CHECK_ARG(kind < 4 || amax_work, "hstu_fp8_quantize: modes 3 / 4 / 5 need a zeroed amax workspace");
  MI355_CHECK_ARG(num_blocks_bound >= 0 && num_blocks_bound < (1ll << 31), "hstu_fp8_quantize: num_blocks_bound out of range");
  return x_is_f16 ? quantize<true>(kind, x, total, num_heads, head_dim, seq_offsets, batch, block_size, cu_blocks,
                                   num_blocks_bound, out_fp8, descale, descale_stride, amax_work, stream)
                  : quantize<false>(kind, x, total, num_heads, head_dim, seq_offsets, batch, block_size, cu_blocks,
                                    num_blocks_bound, out_fp8, descale, descale_stride, amax_work, stream);
}

extern "C" int mi355_hstu_attn_fwd_fp8(int quant_mode, const void* q, const void* k, const void* v, void* out,
                                       int64_t q_row_stride, int64_t k_row_stride, int64_t v_row_stride, int64_t o_row_stride,
                                       int64_t q_head_stride, int64_t k_head_stride, int64_t v_head_stride,
                                       int64_t o_head_stride, const int32_t* cu_seqlens, int64_t batch, int64_t num_heads,
                                       int64_t head_dim, int64_t max_seqlen, const int32_t* num_contexts,
                                       const int32_t* num_targets, int64_t target_group_size, int64_t window_left,
                                       int64_t window_right, float alpha, float scaling_seqlen, const float* descale_q,
                                       const float* descale_k, const float* descale_v, int64_t descale_q_stride,
                                       int64_t descale_k_stride, int64_t descale_v_stride,
                                       const int32_t* cu_seqlens_descale_vt, const int32_t* cu_seqlens_block_descale_q,
                                       const int32_t* cu_seqlens_block_descale_kv, int64_t block_kv, hipStream_t stream) {
  MI355_CHECK_ARG(quant_mode >= 0 && quant_mode <= 5, "hstu_attn_fwd_fp8: quant_mode must be 0 .. 5");
  MI355_CHECK_ARG(q && k && v && out && cu_seqlens, "hstu_attn_fwd_fp8: null tensor");
  MI355_CHECK_ARG(head_dim == 64 || head_dim == 128 || head_dim == 256, "hstu_attn_fwd_fp8: head_dim must be 64, 128 or 256");
  MI355_CHECK_ARG(batch > 0 && num_heads > 0 && max_seqlen >= 0, "hstu_attn_fwd_fp8: bad batch / heads / max_seqlen");
  MI355_CHECK_ARG(((q_row_stride | k_row_stride | v_row_stride | q_head_stride | k_head_stride | v_head_stride) & 15) == 0 &&
                      (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) & 15) == 0,
                  "hstu_attn_fwd_fp8: q / k / v strides and pointers must be 16-byte aligned");
  MI355_CHECK_ARG(((o_row_stride | o_head_stride) & 3) == 0 && ((uintptr_t)out & 7) == 0,
                  "hstu_attn_fwd_fp8: out strides must be multiples of 4 elements");
  MI355_CHECK_ARG(quant_mode == 0 || (descale_q && descale_k && descale_v), "hstu_attn_fwd_fp8: descale tensors missing");
  MI355_CHECK_ARG(quant_mode != 1 || cu_seqlens_descale_vt, "hstu_attn_fwd_fp8: mode 1 needs cu_seqlens_descale_vt");
  MI355_CHECK_ARG(quant_mode != 2 || (cu_seqlens_block_descale_q && cu_seqlens_block_descale_kv &&
                                      (block_kv == 64 || block_kv == 128)),
                  "hstu_attn_fwd_fp8: mode 2 needs the block cu_seqlens and a kv block of 64 or 128");
  MI355_CHECK_ARG(num_targets == nullptr || target_group_size >= 1, "hstu_attn_fwd_fp8: target_group_size must be >= 1");
  MI355_CHECK_ARG(scaling_seqlen != 0.f, "hstu_attn_fwd_fp8: scaling_seqlen is 0");
  if (max_seqlen == 0) return MI355_OK;
  Fp8FwdArgs a;
  a.q = (const uint8_t*)q; a.k = (const uint8_t*)k; a.v = (const uint8_t*)v; a.out = (uint16_t*)out;
  a.q_rs = q_row_stride; a.k_rs = k_row_stride; a.v_rs = v_row_stride; a.o_rs = o_row_stride;
  a.q_hs = q_head_stride; a.k_hs = k_head_stride; a.v_hs = v_head_stride; a.o_hs = o_head_stride;
  a.cu = cu_seqlens; a.B = (int)batch; a.H = (int)num_heads; a.nqb = (int)ceil_div(max_seqlen, 128);
  a.nc = num_contexts; a.nt = num_targets; a.group = (int)target_group_size;
  a.wl = window_left < 0 ? -1 : (int)window_left; a.wr = window_right < 0 ? -1 : (int)window_right;
  a.alpha = alpha; a.scaling = scaling_seqlen;
  a.dq = descale_q; a.dk = descale_k; a.dv = descale_v;
  a.dq_s = descale_q_stride; a.dk_s = descale_k_stride; a.dv_s = descale_v_stride;
  a.cu_vt = cu_seqlens_descale_vt; a.cu_bq = cu_seqlens_block_descale_q; a.cu_bkv = cu_seqlens_block_descale_kv;
  a.block_kv = (int)block_kv;
  MI355_CHECK_ARG(batch * a.nqb < (1ll << 31) && num_heads < 65536, "hstu_attn_fwd_fp8: grid too large");
  const dim3 grid((unsigned)(batch * a.nqb), (unsigned)num_heads);
  if (head_dim == 64) launch_fwd<64>(quant_mode, a, grid, stream);
  else if (head_dim == 128) launch_fwd<128>(quant_mode, a, grid, stream);
  else launch_fwd<256>(quant_mode, a, grid, stream);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

extern "C" int mi355_hstu_attn_bwd_fp8(int quant_mode, const void* dout, const void* dout_t, const void* q, const void* q_t,
                                       const void* k, const void* k_t, const void* v, void* dq, void* dk, void* dv,
                                       const int64_t* row_strides, const int64_t* head_strides, const int32_t* cu_seqlens,
                                       int64_t batch, int64_t num_heads, int64_t head_dim, int64_t max_seqlen,
                                       const int32_t* num_contexts, const int32_t* num_targets, int64_t target_group_size,
                                       int64_t window_left, int64_t window_right, float alpha, float scaling_seqlen,
                                       const float* descale_q, const float* descale_qt, const float* descale_k,
                                       const float* descale_kt, const float* descale_v, const float* descale_do,
                                       const float* descale_dot, const int64_t* descale_strides,
                                       const int32_t* cu_seqlens_descale_qt, const int32_t* cu_seqlens_descale_kt,
                                       const int32_t* cu_seqlens_block_descale_q, const int32_t* cu_seqlens_block_descale_kv,
                                       hipStream_t stream) {
  MI355_CHECK_ARG(quant_mode >= 0 && quant_mode <= 5, "hstu_attn_bwd_fp8: quant_mode must be 0 .. 5");
  MI355_CHECK_ARG(dout && q && k && v && dq && dk && dv && cu_seqlens && row_strides && head_strides,
                  "hstu_attn_bwd_fp8: null tensor or stride array");
  MI355_CHECK_ARG(quant_mode != 1 || (dout_t && q_t && k_t), "hstu_attn_bwd_fp8: mode 1 needs dout_t, q_t and k_t");
  MI355_CHECK_ARG(head_dim == 64 || head_dim == 128 || head_dim == 256, "hstu_attn_bwd_fp8: head_dim must be 64, 128 or 256");
  MI355_CHECK_ARG(batch > 0 && num_heads > 0 && num_heads < 65536 && max_seqlen >= 0,
                  "hstu_attn_bwd_fp8: bad batch / heads / max_seqlen");
  if (quant_mode != 1) { dout_t = dout; q_t = q; k_t = k; }
  const void* in[7] = {dout, dout_t, q, q_t, k, k_t, v};
  int64_t acc = 0;
  uintptr_t pacc = 0;
  for (int i = 0; i < 7; ++i) { acc |= row_strides[i] | head_strides[i]; pacc |= (uintptr_t)in[i]; }
  MI355_CHECK_ARG((acc & 15) == 0 && (pacc & 15) == 0,
                  "hstu_attn_bwd_fp8: fp8 operand strides and pointers must be 16-byte aligned");
  MI355_CHECK_ARG(((row_strides[7] | row_strides[8] | row_strides[9] | head_strides[7] | head_strides[8] | head_strides[9]) &
                   3) == 0 && (((uintptr_t)dq | (uintptr_t)dk | (uintptr_t)dv) & 7) == 0,
                  "hstu_attn_bwd_fp8: dq / dk / dv strides must be multiples of 4 elements");
  MI355_CHECK_ARG(quant_mode == 0 || (descale_q && descale_k && descale_v && descale_do && descale_strides),
                  "hstu_attn_bwd_fp8: descale tensors missing");
  MI355_CHECK_ARG(quant_mode != 1 || (descale_qt && descale_kt && descale_dot && cu_seqlens_descale_qt && cu_seqlens_descale_kt),
                  "hstu_attn_bwd_fp8: mode 1 needs descale_qt / descale_kt / descale_dot and their cu_seqlens");
  MI355_CHECK_ARG(quant_mode != 2 || (cu_seqlens_block_descale_q && cu_seqlens_block_descale_kv),
                  "hstu_attn_bwd_fp8: mode 2 needs the block cu_seqlens");
  MI355_CHECK_ARG(num_targets == nullptr || target_group_size >= 1, "hstu_attn_bwd_fp8: target_group_size must be >= 1");
  MI355_CHECK_ARG(scaling_seqlen != 0.f, "hstu_attn_bwd_fp8: scaling_seqlen is 0");
  if (max_seqlen == 0) return MI355_OK;
  Fp8BwdArgs a;
  a.dout = (const uint8_t*)dout; a.dot = (const uint8_t*)dout_t; a.q = (const uint8_t*)q; a.qt = (const uint8_t*)q_t;
  a.k = (const uint8_t*)k; a.kt = (const uint8_t*)k_t; a.v = (const uint8_t*)v;
  a.dq = (uint16_t*)dq; a.dk = (uint16_t*)dk; a.dv = (uint16_t*)dv;
  a.do_rs = row_strides[0]; a.dot_rs = row_strides[1]; a.q_rs = row_strides[2]; a.qt_rs = row_strides[3];
  a.k_rs = row_strides[4]; a.kt_rs = row_strides[5]; a.v_rs = row_strides[6];
  a.dq_rs = row_strides[7]; a.dk_rs = row_strides[8]; a.dv_rs = row_strides[9];
  a.do_hs = head_strides[0]; a.dot_hs = head_strides[1]; a.q_hs = head_strides[2]; a.qt_hs = head_strides[3];
  a.k_hs = head_strides[4]; a.kt_hs = head_strides[5]; a.v_hs = head_strides[6];
  a.dq_hs = head_strides[7]; a.dk_hs = head_strides[8]; a.dv_hs = head_strides[9];
  if (quant_mode != 1) {   // (the aliases' strides are the originals')
    a.dot_rs = a.do_rs; a.qt_rs = a.q_rs; a.kt_rs = a.k_rs; a.dot_hs = a.do_hs; a.qt_hs = a.q_hs; a.kt_hs = a.k_hs;
  }
  a.cu = cu_seqlens; a.B = (int)batch; a.H = (int)num_heads;
  a.nqb = a.nkb = (int)ceil_div(max_seqlen, 128);
  a.nc = num_contexts; a.nt = num_targets; a.group = (int)target_group_size;
  a.wl = window_left < 0 ? -1 : (int)window_left; a.wr = window_right < 0 ? -1 : (int)window_right;
  a.alpha = alpha; a.scaling = scaling_seqlen;
  a.s_q = descale_q; a.s_qt = descale_qt; a.s_k = descale_k; a.s_kt = descale_kt; a.s_v = descale_v; a.s_do = descale_do;
  a.s_dot = descale_dot;
  const int64_t zero[7] = {0, 0, 0, 0, 0, 0, 0};
  const int64_t* ds = descale_strides ? descale_strides : zero;
  a.s_q_s = ds[0]; a.s_qt_s = ds[1]; a.s_k_s = ds[2]; a.s_kt_s = ds[3]; a.s_v_s = ds[4]; a.s_do_s = ds[5]; a.s_dot_s = ds[6];
  a.cu_qt = cu_seqlens_descale_qt; a.cu_kt = cu_seqlens_descale_kt;
  a.cu_bq = cu_seqlens_block_descale_q; a.cu_bkv = cu_seqlens_block_descale_kv;
  MI355_CHECK_ARG(batch * a.nqb < (1ll << 31), "hstu_attn_bwd_fp8: grid too large");
  const dim3 grid((unsigned)(batch * a.nqb), (unsigned)num_heads);
  if (head_dim == 64) launch_bwd<64>(quant_mode, a, grid, grid, stream);
  else if (head_dim == 128) launch_bwd<128>(quant_mode, a, grid, grid, stream);
  else launch_bwd<256>(quant_mode, a, grid, grid, stream);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}
