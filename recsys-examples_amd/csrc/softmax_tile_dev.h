// The key-tile core of the softmax flash-attention forwards.  beam_decode.hip (beam_ctx_kernel) is written on all of it;
// prefill_attn.hip (prefill_attn_kernel) takes the types, SmMma, sm_key_of and scores() and keeps the other pieces written
// out, line for line equal to the ones here, for a measured reason given in that file: edit both.  A kernel keeps what is
// its own -- block-to-work mapping, sequence bounds, tile ranges, masks, epilogue -- and writes its tile loop from the pieces
// here, in this order:
//
//     __syncthreads();  T::store_tile(st, sK, sV, tid);  __syncthreads();       (barriers stay in the kernel)
//     T::load_tile(st, kb, vb, k_ss, v_ss, next, len, tid);                     (one tile ahead, in registers)
//     T::scores(sK, qf, scale_log2, r, h, p);
//     ... mask: p[j] = -inf for the keys sm_key_of(j, h) a row does not see ...
//     alpha = T::template softmax_step<EMPTY_ROWS>(p, m, lsum);   o[i] *= alpha;
//     T::pv(sV, r, h, p, o);
//
// Shape.  v_mfma_f32_32x32x16_{bf16,f16}; a workgroup of 4 waves owns kSmRows = 128 query rows, a wave 32 of them
// (r = lane & 31 is the row, h = lane >> 5 the lane half), its Q fragments in registers: qf[s] holds elements
// 16 s + 8 h .. + 7 of the row.  A tile is kSmKeys = 64 keys, two 32-key sub-blocks.
//
// LDS.  K is written as [key][KS], KS = D + 8 elements: the padding keeps every row 16-byte aligned for the 128-bit fragment
// reads and makes the row stride no multiple of 32 dwords, so that consecutive keys start on different banks (reasoned from
// the 64-bank LDS, (byte address / 4) mod 64 for 128-bit reads; the conflict counter was not read).
// V is written transposed as [d][VS], VS = 64 + 4 elements = 34 dwords: the 32 rows d that a half-wave reads hit 64 banks,
// and the transposing write -- a lane holds one 16-byte chunk of keys 2p and 2p + 1 and writes 8 dwords [d][2p, 2p + 1],
// two keys per 32-bit write -- is conflict-free.  Keys at or past the end of the sequence are never read from memory; they
// enter LDS as zeros.
//
// Registers.  S^T = K Q^T: K is the A operand, so the key index lies in the accumulator registers and the query row on the
// lane.  A row's max and sum are reductions over the 32 registers p[] of a lane plus one exchange between the two lane
// halves.  Register j of lane half h is key sm_key_of(j, h) = 32 (j >> 4) + 8 ((j & 15) >> 2) + 4 h + (j & 3) of the tile.
// P, rounded once to the operand type (the row sum is taken from the fp32 P), is the B operand of O^T += V^T P^T with no trip
// through LDS: k-step ks (sub-block ks >> 1, step ks & 1) packs registers 8 ks .. 8 ks + 7, which are keys
// 16 ks + 4 h + {0..3} and 16 ks + 8 + 4 h + {0..3}; pv() reads the V^T fragment of row d at exactly these two groups of four
// keys.  A change to sm_key_of, to the packing order or to that read has to be made to all three.
//
// Running max m and sum lsum are fp32, per lane half (the halves' sums are added in the epilogue), in log2 units: scores are
// pre-scaled by softmax_scale log2 e and the exponential is v_exp_f32.  1 / l is applied once, in the epilogue.
#pragma once
#include "common.h"

#include <math.h>

namespace mi355 {

typedef float sm_f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t sm_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t sm_u32x2 __attribute__((ext_vector_type(2)));
typedef float sm_f32x2 __attribute__((ext_vector_type(2)));

constexpr int kSmKeys = 64;     // keys per tile
constexpr int kSmRows = 128;    // query rows per workgroup (4 waves x 32)
constexpr float kSmLog2e = 1.4426950408889634f;
constexpr float kSmLn2 = 0.6931471805599453f;

template <int DT> struct SmMma;
template <> struct SmMma<kBF16> {
  typedef __bf16 V8 __attribute__((ext_vector_type(8)));
  typedef __bf16 V2 __attribute__((ext_vector_type(2)));
  static __device__ __forceinline__ sm_f32x16 mma(sm_u32x4 a, sm_u32x4 b, sm_f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(V8, a), __builtin_bit_cast(V8, b), c, 0, 0, 0);
  }
  static __device__ __forceinline__ uint32_t pack2(float lo, float hi) {   // v_cvt_pk_bf16_f32: round to nearest even
    const sm_f32x2 x = {lo, hi};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(x, V2));
  }
};
template <> struct SmMma<kF16> {
  typedef _Float16 V8 __attribute__((ext_vector_type(8)));
  typedef _Float16 V2 __attribute__((ext_vector_type(2)));
  static __device__ __forceinline__ sm_f32x16 mma(sm_u32x4 a, sm_u32x4 b, sm_f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(V8, a), __builtin_bit_cast(V8, b), c, 0, 0, 0);
  }
  static __device__ __forceinline__ uint32_t pack2(float lo, float hi) {   // v_cvt_pk_f16_f32: round to nearest even
    const sm_f32x2 x = {lo, hi};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(x, V2));
  }
};

// 16-byte rows: base aligned, strides multiples of 8 elements
static inline bool sm_aligned(const void* p, int64_t s0, int64_t s1, int64_t s2) {
  return ((uintptr_t)p % 16 == 0) && s0 % 8 == 0 && s1 % 8 == 0 && s2 % 8 == 0;
}

// the key inside its tile of score register j (0 .. 31) of lane half h
__device__ __forceinline__ constexpr int sm_key_of(int j, int h) { return 32 * (j >> 4) + (j & 3) + 8 * ((j & 15) >> 2) + 4 * h; }

template <int DT, int D>
struct SmTile {
  using M = SmMma<DT>;
  static constexpr int KS = D + 8;          // K row stride in LDS (elements)
  static constexpr int VS = kSmKeys + 4;    // V^T row stride in LDS (elements)
  static constexpr int kSK = kSmKeys * KS, kSV = D * VS;   // elements of sK / sV (uint16_t, 16-byte aligned)
  static constexpr int CH = D / 8;          // 16-byte chunks per row
  static constexpr int NK = kSmKeys * CH / 256, NV = 32 * CH / 256;

  // One tile of K / V in registers.  K: consecutive lanes take consecutive 16-byte chunks of a row.  V: a lane takes one
  // chunk of keys 2p and 2p + 1.
  struct Stage { sm_u32x4 k[NK], v[NV][2]; };

  // qp: element 8 h of the lane's query row
  static __device__ __forceinline__ void load_q(const uint16_t* qp, bool valid, sm_u32x4 (&qf)[D / 16]) {
#pragma unroll
    for (int s = 0; s < D / 16; ++s) {
      sm_u32x4 z = {0u, 0u, 0u, 0u};
      qf[s] = valid ? *reinterpret_cast<const sm_u32x4*>(qp + 16 * s) : z;
    }
  }

  static __device__ __forceinline__ void zero_acc(sm_f32x16 (&o)[D / 32]) {
#pragma unroll
    for (int i = 0; i < D / 32; ++i)
#pragma unroll
      for (int j = 0; j < 16; ++j) o[i][j] = 0.f;
  }

  // chunk c of row `row` (key `key` of its tile) of a K or V whose key 0 is at base; zeros for a key at or past the nv valid ones
  static __device__ __forceinline__ sm_u32x4 ld_row(const uint16_t* base, int64_t stride, int row, int nv, int key, int c) {
    sm_u32x4 val = {0u, 0u, 0u, 0u};
    if (key < nv) val = *reinterpret_cast<const sm_u32x4*>(base + (int64_t)row * stride + 8 * c);
    return val;
  }

  // tile t of a sequence of len keys whose key 0 is at kb / vb
  static __device__ __forceinline__ void load_tile(Stage& st, const uint16_t* kb, const uint16_t* vb, int64_t k_ss, int64_t v_ss,
                                                   int t, int len, int tid) {
    const int nv = len - t * kSmKeys;
#pragma unroll
    for (int i = 0; i < NK; ++i) {
      const int u = tid + 256 * i, key = u / CH, c = u % CH;
      st.k[i] = ld_row(kb, k_ss, t * kSmKeys + key, nv, key, c);
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int u = tid + 256 * i, p = u & 31, c = u >> 5;
      st.v[i][0] = ld_row(vb, v_ss, t * kSmKeys + 2 * p, nv, 2 * p, c);
      st.v[i][1] = ld_row(vb, v_ss, t * kSmKeys + 2 * p + 1, nv, 2 * p + 1, c);
    }
  }

  // the staged tile to LDS; the caller puts a barrier before (the previous tile is no longer read) and after.  The split of
  // tid + 256 i into (key, c) and (p, c) is the one of load_tile above.
  static __device__ __forceinline__ void store_tile(const Stage& st, uint16_t* sK, uint16_t* sV, int tid) {
#pragma unroll
    for (int i = 0; i < NK; ++i) {
      const int u = tid + 256 * i, key = u / CH, c = u % CH;
      *reinterpret_cast<sm_u32x4*>(sK + key * KS + 8 * c) = st.k[i];
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {   // V transposed: 8 dwords [d][2p, 2p + 1] per chunk pair
      const int u = tid + 256 * i, p = u & 31, c = u >> 5;
      const sm_u32x4 va = st.v[i][0], vc = st.v[i][1];
      uint32_t* dst = reinterpret_cast<uint32_t*>(sV + (8 * c) * VS + 2 * p);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        dst[(2 * e) * (VS / 2)] = (va[e] & 0xffffu) | (vc[e] << 16);
        dst[(2 * e + 1) * (VS / 2)] = (va[e] >> 16) | (vc[e] & 0xffff0000u);
      }
    }
  }

  // p = scale_log2 * S^T = scale_log2 * K Q^T for the two 32-key sub-blocks
  static __device__ __forceinline__ void scores(const uint16_t* sK, const sm_u32x4 (&qf)[D / 16], float scale_log2, int r, int h,
                                                float (&p)[32]) {
    sm_f32x16 s0, s1;
#pragma unroll
    for (int j = 0; j < 16; ++j) { s0[j] = 0.f; s1[j] = 0.f; }
#pragma unroll
    for (int s = 0; s < D / 16; ++s) {
      const sm_u32x4 k0 = *reinterpret_cast<const sm_u32x4*>(sK + r * KS + 16 * s + 8 * h);
      const sm_u32x4 k1 = *reinterpret_cast<const sm_u32x4*>(sK + (32 + r) * KS + 16 * s + 8 * h);
      s0 = M::mma(k0, qf[s], s0);
      s1 = M::mma(k1, qf[s], s1);
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) { p[j] = s0[j] * scale_log2; p[16 + j] = s1[j] * scale_log2; }
  }

  // The online-softmax update: masked scores in p (-inf: not seen) become the fp32 P, m and lsum are updated, and the factor
  // alpha = exp2(m_old - m_new) is returned: the caller multiplies its accumulators by it before pv().  (That multiply stays
  // in the kernel's loop: with it behind a helper that takes o by reference, prefill_attn_kernel, when tried on this step,
  // compiled to 24 more VGPRs.)  EMPTY_ROWS: a row may have seen no key yet (m_new = -inf); the exponent is then taken against 0, so that
  // P = exp2(-inf) = 0 and no inf - inf arises.  Without it m_new must be finite (a visible key in every tile).
  template <bool EMPTY_ROWS>
  static __device__ __forceinline__ float softmax_step(float (&p)[32], float& m, float& lsum) {
    float mx = p[0];
#pragma unroll
    for (int j = 1; j < 32; ++j) mx = fmaxf(mx, p[j]);
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m, mx);
    float m_use = m_new;
    if constexpr (EMPTY_ROWS) m_use = m_new == -INFINITY ? 0.f : m_new;
    const float alpha = __builtin_amdgcn_exp2f(m - m_use);
    m = m_new;
    float ts = 0.f;
#pragma unroll
    for (int j = 0; j < 32; ++j) { p[j] = __builtin_amdgcn_exp2f(p[j] - m_use); ts += p[j]; }
    lsum = lsum * alpha + ts;
    return alpha;
  }

  // O^T += V^T P^T
  static __device__ __forceinline__ void pv(const uint16_t* sV, int r, int h, const float (&p)[32], sm_f32x16 (&o)[D / 32]) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {   // k-step: sub-block ks >> 1, step ks & 1: registers 8 ks .. 8 ks + 7 of p
      sm_u32x4 pf;
#pragma unroll
      for (int e = 0; e < 4; ++e) pf[e] = M::pack2(p[8 * ks + 2 * e], p[8 * ks + 2 * e + 1]);
#pragma unroll
      for (int i = 0; i < D / 32; ++i) {
        const uint16_t* vp = sV + (32 * i + r) * VS + 16 * ks + 4 * h;
        const sm_u32x2 lo = *reinterpret_cast<const sm_u32x2*>(vp);
        const sm_u32x2 hi = *reinterpret_cast<const sm_u32x2*>(vp + 8);
        const sm_u32x4 vf = {lo[0], lo[1], hi[0], hi[1]};
        o[i] = M::mma(vf, pf, o[i]);
      }
    }
  }
};

}  // namespace mi355
