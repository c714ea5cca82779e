// Jagged x dense products of the HSTU op layer: the per-sample GEMM of jagged rows with a dense [K, N] matrix (+ bias), its
// weight gradient (jagged^T x jagged, reduced over the sequence), the per-sample broadcast add and the per-sample row sum.
//
// Replaces (reference, examples/commons/ops/triton_ops/triton_jagged.py): jagged_dense_bmm_broadcast_add_kernel (:77-153),
// _jagged_jagged_bmm_reduce_sum (:161-255), jagged_dense_broadcast_add_kernel (:387-437) and jagged_reduce_sum (:440-477).
// Written for wave64 and the gfx950 matrix cores from the arithmetic; nothing of the reference's launch shape is kept: its
// grid is cdiv(max_seq_len, BLOCK_M) x B and rows at or past max_seq_len stay uninitialised, here max_seq_len does not exist.
//
// (a) jagged_dense_bmm.  The unit of work is a tile of 32 rows x 128 columns, one block of four waves, wave w owning the
//     32 x 32 accumulator of columns [32 w, 32 w + 32).  Sample b owns the tile slots [off[b] / 32 + b, off[b + 1] / 32 + b + 1)
//     (integer division): at least ceil(len_b / 32) of them, L / 32 + B + 1 in all with the pseudo-sample B that owns the rows
//     [off[B], L) and fills them with zeros.  The grid is sized from L and B alone; a block finds its sample with a binary
//     search of that strictly increasing key and leaves if its tile starts past the sample's end.  Offsets are clamped to
//     [0, L], so whatever they hold no row outside the buffers is touched.
//     K runs in stages of 32 (16-bit) or 16 (fp32) through LDS: As[32][k] and Bs[128][k], both with k contiguous, which is how
//     the MFMA wants its operands (lane l = (r, h): 8 consecutive k of row r, cf. hstu_attn.hip).  The jagged rows have k
//     contiguous in memory and go in as 16-byte pieces; the dense matrix goes in the same way when its k stride is 1 (the
//     backward's D^T, read in place) and is transposed on the way into LDS when its n stride is 1 (the forward).  The pieces of
//     stage s + 1 are loaded into registers before the MFMAs of stage s.  Everything outside K, N and the sample's rows is
//     staged as zero, so the tails need no other mask.  Where a base pointer or a stride is not 16-byte aligned, or a piece
//     crosses the end of a row, the piece is loaded element by element: same values, same arithmetic.
//     bf16 / fp16: v_mfma_f32_32x32x16_{bf16,f16}.  fp32: v_mfma_f32_32x32x2_f32 (an fmaf chain in k order, full precision).
//     The bias is added to the fp32 accumulator, then the one rounding.
// (b) jagged_jagged_bmm.  One block per (chunk of a sample, 64 x 64 tile of Out_b), 2 x 2 waves of 32 x 32; the sequence is the
//     k of the MFMA, walked in row order in stages of 32 (16) rows, both operands transposed on the way into LDS.  A sample is
//     cut into chunks of C rows counted from its first row, C = 64 x (tiles of Out_b) clamped to [256, 4096]: a function of
//     (M, N) alone, so that a 4096-row sample with a 128 x 128 product is 16 blocks per tile and not one.  The chunks get their
//     blocks by the slot scheme of (a) with C in place of 32 (L / C + B slots, every sample at least one: an empty sample has a
//     block that writes its zeros).  A sample of one chunk is rounded and written by its block; the chunks of a longer one go
//     to an fp32 workspace [slot][M][N] and a second kernel adds them in chunk order and rounds once.  No atomics: the order
//     of the additions is a function of (length, M, N) alone.  The optional column sum rides in the blocks of the first m
//     tile as one more MFMA per stage with a tile of ones for the first operand (exact products), and takes the same path
//     through the workspace ([slot][N], behind the chunk sums of Out).
// (c) jagged_broadcast_add: a thread owns one 16-byte piece of columns and walks down rows (act_ops.hip); the sample of a row
//     is found by binary search, wave-uniformly.  Rows at or past off[B] are written as zeros.
// (d) jagged_row_sum: one block of 16 waves per (sample, 64 pieces of columns); wave w sums the rows w, w + 16, ... of the
//     sample in that order, four loads in flight, the 16 sums are folded in wave order through LDS and rounded once.
#include "common.h"
#include "jagged_dev.h"
#include "vec_dev.h"
#include "../../include/recsys_amd.h"

namespace mi355 {

typedef __attribute__((ext_vector_type(16))) float jb_f32x16_t;
typedef __attribute__((ext_vector_type(4))) uint32_t jb_u32x4_t;
typedef __attribute__((ext_vector_type(8))) __bf16 jb_bf16x8_t;
typedef __attribute__((ext_vector_type(8))) _Float16 jb_f16x8_t;

constexpr int kJbRows = 32;     // rows of a tile slot of (a)
constexpr int kJbCols = 128;    // columns of a tile of (a)
constexpr int kJbOut = 64;      // Out_b tile edge of (b)

template <int DT> struct JbGeom {
  static constexpr int EB = DT == kF32 ? 4 : 2;
  static constexpr int VE = 16 / EB;                 // elements of a 16-byte piece
  static constexpr int BK = DT == kF32 ? 16 : 32;    // k of a stage: four pieces
  static constexpr int LDK = BK + VE;                // LDS row in elements (80 bytes: rows stay 16-byte aligned)
};

// VE consecutive elements at `a`, the first `cnt` of them valid (the rest zero); one 16-byte load where allowed
template <int EB>
__device__ __forceinline__ jb_u32x4_t jb_ld_piece(uintptr_t a, int cnt, bool vec) {
  constexpr int VE = 16 / EB;
  jb_u32x4_t v = {0u, 0u, 0u, 0u};
  if (cnt >= VE && vec) return *(const __attribute__((address_space(1))) jb_u32x4_t*)a;
#pragma unroll
  for (int e = 0; e < VE; ++e) {
    if (e < cnt) {
      if constexpr (EB == 4) {
        v[e] = *(const __attribute__((address_space(1))) uint32_t*)(a + 4 * e);
      } else {
        const uint32_t x = *(const __attribute__((address_space(1))) uint16_t*)(a + 2 * e);
        v[e >> 1] |= x << (16 * (e & 1));
      }
    }
  }
  return v;
}

// the same piece of elements `es` bytes apart
template <int EB>
__device__ __forceinline__ jb_u32x4_t jb_ld_piece_strided(uintptr_t a, int64_t es, int cnt) {
  constexpr int VE = 16 / EB;
  jb_u32x4_t v = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int e = 0; e < VE; ++e) {
    if (e < cnt) {
      if constexpr (EB == 4) {
        v[e] = *(const __attribute__((address_space(1))) uint32_t*)(a + (uintptr_t)(es * e));
      } else {
        const uint32_t x = *(const __attribute__((address_space(1))) uint16_t*)(a + (uintptr_t)(es * e));
        v[e >> 1] |= x << (16 * (e & 1));
      }
    }
  }
  return v;
}

__device__ __forceinline__ int jb_clamp(int64_t v, int hi) { return v < 0 ? 0 : v > hi ? hi : (int)v; }

// A [C x BK] block whose element (c, k) lies at base + c sc + k EB goes to lds[c][k]: pieces run along k.  C * 4 pieces,
// piece p of thread tid + 256 i.  ccount / kcount: the valid extent of the block; the rest is staged as zero.
template <int DT, int C> struct JbDirect {
  typedef JbGeom<DT> G;
  static constexpr int NP = (C * 4 + 255) / 256;
  static __device__ __forceinline__ void ld(jb_u32x4_t (&r)[NP], uintptr_t base, int64_t sc, int ccount, int kcount, bool vec,
                                            int tid) {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int p = tid + 256 * i;
      const int c = p >> 2, kv = p & 3;
      const int cnt = (p < C * 4 && c < ccount) ? jb_clamp(kcount - kv * G::VE, G::VE) : 0;
      r[i] = jb_ld_piece<G::EB>(base + (uintptr_t)(c * sc) + (uintptr_t)(kv * 16), cnt, vec);
    }
  }
  static __device__ __forceinline__ void st(const jb_u32x4_t (&r)[NP], void* lds, int tid) {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int p = tid + 256 * i;
      if (p < C * 4) *(jb_u32x4_t*)((char*)lds + ((p >> 2) * G::LDK + (p & 3) * G::VE) * G::EB) = r[i];
    }
  }
};

// A [BK x C] block whose element (k, c) lies at base + k sk + c sc goes to lds[c][k]: pieces run along c and are transposed
// by the LDS writes.  Four neighbouring lanes take four neighbouring pieces of one k (64 contiguous bytes when sc is the
// element size), the next lanes the next k.
template <int DT, int C> struct JbTrans {
  typedef JbGeom<DT> G;
  static constexpr int NP = (C / G::VE * G::BK) / 256;
  static_assert((C / G::VE * G::BK) % 256 == 0 && (C / G::VE) % 4 == 0, "piece count");
  static __device__ __forceinline__ void map(int p, int& k, int& cv) {
    k = (p >> 2) % G::BK;
    cv = (p / (4 * G::BK)) * 4 + (p & 3);
  }
  static __device__ __forceinline__ void ld(jb_u32x4_t (&r)[NP], uintptr_t base, int64_t sk, int64_t sc, int kcount, int ccount,
                                            bool vec, int tid) {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      int k, cv;
      map(tid + 256 * i, k, cv);
      const int cnt = k < kcount ? jb_clamp(ccount - cv * G::VE, G::VE) : 0;
      const uintptr_t a = base + (uintptr_t)(k * sk) + (uintptr_t)(cv * G::VE * sc);
      r[i] = sc == G::EB ? jb_ld_piece<G::EB>(a, cnt, vec) : jb_ld_piece_strided<G::EB>(a, sc, cnt);
    }
  }
  static __device__ __forceinline__ void st(const jb_u32x4_t (&r)[NP], void* lds, int tid) {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      int k, cv;
      map(tid + 256 * i, k, cv);
#pragma unroll
      for (int e = 0; e < G::VE; ++e) {
        const int idx = (cv * G::VE + e) * G::LDK + k;
        if constexpr (G::EB == 4) ((uint32_t*)lds)[idx] = r[i][e];
        else ((uint16_t*)lds)[idx] = (uint16_t)(r[i][e >> 1] >> (16 * (e & 1)));
      }
    }
  }
};

// acc += As[arow + r][.] x Bs[brow + r][.] over one stage (lds rows of LDK elements, k contiguous)
template <int DT>
__device__ __forceinline__ void jb_mma_stage(jb_f32x16_t& acc, const void* As, int arow, const void* Bs, int brow, int lane) {
  typedef JbGeom<DT> G;
  const int r = lane & 31, h = lane >> 5;
  if constexpr (DT == kF32) {
    const float* a = (const float*)As + (arow + r) * G::LDK + h;
    const float* b = (const float*)Bs + (brow + r) * G::LDK + h;
#pragma unroll
    for (int kk = 0; kk < G::BK; kk += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk], b[kk], acc, 0, 0, 0);
  } else {
    const uint16_t* a = (const uint16_t*)As + (arow + r) * G::LDK + 8 * h;
    const uint16_t* b = (const uint16_t*)Bs + (brow + r) * G::LDK + 8 * h;
#pragma unroll
    for (int ks = 0; ks < G::BK; ks += 16) {
      const jb_u32x4_t av = *(const jb_u32x4_t*)(a + ks), bv = *(const jb_u32x4_t*)(b + ks);
      if constexpr (DT == kBF16)
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(jb_bf16x8_t, av), __builtin_bit_cast(jb_bf16x8_t, bv), acc, 0, 0, 0);
      else
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(jb_f16x8_t, av), __builtin_bit_cast(jb_f16x8_t, bv), acc, 0, 0, 0);
    }
  }
}

// acc += 1 x Bs[brow + r][.] over one stage: every row of acc is the column sum of the stage's rows (the products are exact)
template <int DT>
__device__ __forceinline__ void jb_mma_ones_stage(jb_f32x16_t& acc, const void* Bs, int brow, int lane) {
  typedef JbGeom<DT> G;
  const int r = lane & 31, h = lane >> 5;
  if constexpr (DT == kF32) {
    const float* b = (const float*)Bs + (brow + r) * G::LDK + h;
#pragma unroll
    for (int kk = 0; kk < G::BK; kk += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(1.f, b[kk], acc, 0, 0, 0);
  } else {
    constexpr uint32_t one2 = DT == kBF16 ? 0x3f803f80u : 0x3c003c00u;   // two 1.0 of the dtype
    const jb_u32x4_t ones = {one2, one2, one2, one2};
    const uint16_t* b = (const uint16_t*)Bs + (brow + r) * G::LDK + 8 * h;
#pragma unroll
    for (int ks = 0; ks < G::BK; ks += 16) {
      const jb_u32x4_t bv = *(const jb_u32x4_t*)(b + ks);
      if constexpr (DT == kBF16)
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(jb_bf16x8_t, ones), __builtin_bit_cast(jb_bf16x8_t, bv), acc, 0, 0, 0);
      else
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(jb_f16x8_t, ones), __builtin_bit_cast(jb_f16x8_t, bv), acc, 0, 0, 0);
    }
  }
}

// row of accumulator register `reg` of lane half h in the 32 x 32 tile; the column is lane & 31
__device__ __forceinline__ int jb_acc_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

__device__ __forceinline__ int64_t jb_off(const int64_t* off, int64_t i, int64_t L) {
  const int64_t v = off[i];
  return v < 0 ? 0 : v > L ? L : v;
}

struct JbmmArgs {
  uintptr_t j, d, bias, out;
  const int64_t* off;
  int64_t L, B, K, N;
  int64_t j_stride, out_stride;   // bytes per row
  int64_t d_sb, d_sk, d_sn;       // bytes
  int64_t bias_sb;                // bytes
  int j_vec, d_vec;               // 16-byte pieces allowed
};

template <int DT>
__global__ __launch_bounds__(256) void jagged_dense_bmm_kernel(const JbmmArgs a) {
  typedef JbGeom<DT> G;
  constexpr int EB = G::EB;
  __shared__ __attribute__((aligned(16))) char s_a[kJbRows * G::LDK * EB];
  __shared__ __attribute__((aligned(16))) char s_b[kJbCols * G::LDK * EB];
  const int tid = (int)threadIdx.x, lane = lane_id(), wv = tid >> 6;
  const int64_t slot = blockIdx.x;
  const int64_t n0 = (int64_t)blockIdx.y * kJbCols;
  // largest b in [0, B] with off[b] / 32 + b <= slot
  int64_t lo = 0, hi = a.B;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (jb_off(a.off, mid, a.L) / kJbRows + mid <= slot) lo = mid; else hi = mid - 1;
  }
  const int64_t b = lo;
  const int64_t start = jb_off(a.off, b, a.L);
  const int64_t t = slot - (start / kJbRows + b);
  if (t < 0) return;
  const int64_t r0 = start + t * kJbRows;
  const int64_t rend = b < a.B ? jb_off(a.off, b + 1, a.L) : a.L;
  if (r0 >= rend) return;   // (block-uniform)
  const int rows = rend - r0 < kJbRows ? (int)(rend - r0) : kJbRows;
  const int cols = a.N - n0 < kJbCols ? (int)(a.N - n0) : kJbCols;
  if (b == a.B) {
    // rows past the last offset: defined, and zero
    for (int i = tid; i < rows * cols; i += 256) {
      const int rr = i / cols, cc = i - rr * cols;
      st1<DT>((void*)(a.out + (uintptr_t)(r0 + rr) * a.out_stride), n0 + cc, 0.f);
    }
    return;
  }
  const uintptr_t jbase = a.j + (uintptr_t)r0 * a.j_stride;
  const uintptr_t dbase = a.d + (uintptr_t)(b * a.d_sb) + (uintptr_t)(n0 * a.d_sn);
  const bool d_along_k = a.d_sk == EB;
  jb_u32x4_t pa[1], pb[2];
  auto load = [&](int64_t k0) {
    const int kc = a.K - k0 < G::BK ? (int)(a.K - k0) : G::BK;
    JbDirect<DT, kJbRows>::ld(pa, jbase + (uintptr_t)k0 * EB, a.j_stride, rows, kc, a.j_vec != 0, tid);
    if (d_along_k) JbDirect<DT, kJbCols>::ld(pb, dbase + (uintptr_t)k0 * EB, a.d_sn, cols, kc, a.d_vec != 0, tid);
    else JbTrans<DT, kJbCols>::ld(pb, dbase + (uintptr_t)(k0 * a.d_sk), a.d_sk, a.d_sn, kc, cols, a.d_vec != 0, tid);
  };
  jb_f32x16_t acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  const bool wave_on = wv * 32 < cols;
  load(0);
  for (int64_t k0 = 0; k0 < a.K; k0 += G::BK) {
    JbDirect<DT, kJbRows>::st(pa, s_a, tid);
    if (d_along_k) JbDirect<DT, kJbCols>::st(pb, s_b, tid);
    else JbTrans<DT, kJbCols>::st(pb, s_b, tid);
    __syncthreads();
    if (k0 + G::BK < a.K) load(k0 + G::BK);
    if (wave_on) jb_mma_stage<DT>(acc, s_a, 0, s_b, wv * 32, lane);
    __syncthreads();
  }
  if (!wave_on) return;
  const int c = wv * 32 + (lane & 31), h = lane >> 5;
  if (c >= cols) return;
  const float bias = a.bias ? ld1<DT>((const void*)(a.bias + (uintptr_t)(b * a.bias_sb)), n0 + c) : 0.f;
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int rr = jb_acc_row(reg, h);
    if (rr < rows) st1<DT>((void*)(a.out + (uintptr_t)(r0 + rr) * a.out_stride), n0 + c, a.bias ? acc[reg] + bias : acc[reg]);
  }
}

struct JjArgs {
  uintptr_t a, bm, out, colsum;   // colsum: 0 when no column sum is wanted
  const int64_t* off;
  float* partial;                 // [slots][M][N] fp32: the chunk sums of the samples that have more than one chunk
  float* partial_r;               // [slots][N] fp32: the same for the column sum
  int64_t colsum_sb;              // bytes
  int64_t L, B, M, N, chunk;
  int64_t a_stride, b_stride;     // bytes per row
  int64_t out_sb, out_sm;         // bytes
  int a_vec, b_vec;
};

// chunks of sample b: at least one, so that an empty sample has a block that writes its zeros
__device__ __forceinline__ int64_t jj_chunks(int64_t len, int64_t chunk) { return len <= chunk ? 1 : (len + chunk - 1) / chunk; }

template <int DT>
__global__ __launch_bounds__(256) void jagged_jagged_bmm_kernel(const JjArgs a) {
  typedef JbGeom<DT> G;
  constexpr int EB = G::EB;
  __shared__ __attribute__((aligned(16))) char s_a[kJbOut * G::LDK * EB];
  __shared__ __attribute__((aligned(16))) char s_b[kJbOut * G::LDK * EB];
  const int tid = (int)threadIdx.x, lane = lane_id(), wv = tid >> 6;
  const int64_t slot = blockIdx.x;
  const int64_t m0 = (int64_t)blockIdx.y * kJbOut, n0 = (int64_t)blockIdx.z * kJbOut;
  // largest b in [0, B - 1] with off[b] / chunk + b <= slot
  int64_t lo = 0, hi = a.B - 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (jb_off(a.off, mid, a.L) / a.chunk + mid <= slot) lo = mid; else hi = mid - 1;
  }
  const int64_t b = lo;
  const int64_t first = jb_off(a.off, b, a.L), last = jb_off(a.off, b + 1, a.L);
  const int64_t t = slot - (first / a.chunk + b);
  const int64_t len = last > first ? last - first : 0;
  const int64_t chunks = jj_chunks(len, a.chunk);
  if (t < 0 || t >= chunks) return;   // (block-uniform)
  const int64_t rs = first + t * a.chunk;
  const int64_t re = rs + a.chunk < first + len ? rs + a.chunk : first + len;
  const int mc = a.M - m0 < kJbOut ? (int)(a.M - m0) : kJbOut;
  const int nc = a.N - n0 < kJbOut ? (int)(a.N - n0) : kJbOut;
  const uintptr_t abase = a.a + (uintptr_t)m0 * EB, bbase = a.bm + (uintptr_t)n0 * EB;
  jb_u32x4_t pa[1], pb[1];
  auto load = [&](int64_t r0) {
    const int kc = re - r0 < G::BK ? (int)(re - r0) : G::BK;
    JbTrans<DT, kJbOut>::ld(pa, abase + (uintptr_t)r0 * a.a_stride, a.a_stride, EB, kc, mc, a.a_vec != 0, tid);
    JbTrans<DT, kJbOut>::ld(pb, bbase + (uintptr_t)r0 * a.b_stride, a.b_stride, EB, kc, nc, a.b_vec != 0, tid);
  };
  jb_f32x16_t acc, acc_r;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = acc_r[i] = 0.f;
  const int wm = (wv >> 1) * 32, wn = (wv & 1) * 32;
  const bool wave_on = wm < mc && wn < nc;
  // the column sum of the n tile rides in the blocks of the first m tile: one more MFMA with a tile of ones
  const bool sum_on = a.colsum != 0 && blockIdx.y == 0 && wm == 0 && wave_on;
  if (rs < re) load(rs);
  for (int64_t r0 = rs; r0 < re; r0 += G::BK) {
    JbTrans<DT, kJbOut>::st(pa, s_a, tid);
    JbTrans<DT, kJbOut>::st(pb, s_b, tid);
    __syncthreads();
    if (r0 + G::BK < re) load(r0 + G::BK);
    if (wave_on) jb_mma_stage<DT>(acc, s_a, wm, s_b, wn, lane);
    if (sum_on) jb_mma_ones_stage<DT>(acc_r, s_b, wn, lane);
    __syncthreads();
  }
  if (!wave_on) return;
  const int c = wn + (lane & 31), h = lane >> 5;
  if (c >= nc) return;
  if (sum_on && h == 0) {   // (register 0 of the lower lane half is row 0 of the tile)
    if (chunks == 1) st1<DT>((void*)(a.colsum + (uintptr_t)(b * a.colsum_sb)), n0 + c, acc_r[0]);
    else a.partial_r[(size_t)slot * a.N + n0 + c] = acc_r[0];
  }
  if (chunks == 1) {
    const uintptr_t obase = a.out + (uintptr_t)(b * a.out_sb);
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int rr = wm + jb_acc_row(reg, h);
      if (rr < mc) st1<DT>((void*)(obase + (uintptr_t)(m0 + rr) * a.out_sm), n0 + c, acc[reg]);
    }
  } else {
    float* p = a.partial + (size_t)slot * a.M * a.N;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int rr = wm + jb_acc_row(reg, h);
      if (rr < mc) p[(size_t)(m0 + rr) * a.N + n0 + c] = acc[reg];
    }
  }
}

// Out_b of a sample with more than one chunk: its chunk sums added in chunk order, rounded once
template <int DT>
__global__ __launch_bounds__(256) void jagged_jagged_bmm_fold_kernel(const JjArgs a) {
  const int64_t b = blockIdx.y;
  const int64_t first = jb_off(a.off, b, a.L), last = jb_off(a.off, b + 1, a.L);
  const int64_t chunks = jj_chunks(last > first ? last - first : 0, a.chunk);
  if (chunks == 1) return;
  const int64_t mn = a.M * a.N;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= mn) return;
  const float* p = a.partial + (size_t)(first / a.chunk + b) * mn + i;
  float t = 0.f;
  for (int64_t c = 0; c < chunks; ++c) t += p[(size_t)c * mn];
  const int64_t m = i / a.N;
  st1<DT>((void*)(a.out + (uintptr_t)(b * a.out_sb) + (uintptr_t)m * a.out_sm), i - m * a.N, t);
  if (a.colsum != 0 && i < a.N) {
    const float* q = a.partial_r + (size_t)(first / a.chunk + b) * a.N + i;
    float r = 0.f;
    for (int64_t c = 0; c < chunks; ++c) r += q[(size_t)c * a.N];
    st1<DT>((void*)(a.colsum + (uintptr_t)(b * a.colsum_sb)), i, r);
  }
}

struct JaddArgs {
  uintptr_t j, dense, out;
  const int64_t* off;
  int64_t L, B, D;
  int64_t j_stride, out_stride, dense_sb;   // bytes
};

template <int DT, int V>
__global__ __launch_bounds__(256) void jagged_broadcast_add_kernel(const JaddArgs a) {
  constexpr uintptr_t EB = Vec<DT, V>::EB;
  const int lane = lane_id(), wv = threadIdx.x >> 6;
  const int64_t c = ((int64_t)blockIdx.x * 64 + lane) * V;
  if (c >= a.D) return;
  const uintptr_t co = (uintptr_t)c * EB;
  const int64_t last = jb_off(a.off, a.B, a.L);
  for (int64_t row = (int64_t)blockIdx.y * 4 + wv; row < a.L; row += (int64_t)gridDim.y * 4) {
    float o[V];
    if (row < last) {
      const int64_t b = sample_of(a.off, a.B, row);   // (wave-uniform)
      float x[V], y[V];
      Vec<DT, V>::ld(a.j + (uintptr_t)row * a.j_stride + co, x);
      Vec<DT, V>::ld(a.dense + (uintptr_t)(b * a.dense_sb) + co, y);
#pragma unroll
      for (int e = 0; e < V; ++e) o[e] = x[e] + y[e];
    } else {
#pragma unroll
      for (int e = 0; e < V; ++e) o[e] = 0.f;
    }
    Vec<DT, V>::st(a.out + (uintptr_t)row * a.out_stride + co, o);
  }
}

struct JsumArgs {
  uintptr_t j, out;
  const int64_t* off;
  int64_t L, B, D;
  int64_t j_stride, out_sb;   // bytes
};

template <int DT, int V>
__global__ __launch_bounds__(1024) void jagged_row_sum_kernel(const JsumArgs a) {
  constexpr uintptr_t EB = Vec<DT, V>::EB;
  constexpr int UN = 4;
  __shared__ float s_fold[16 * 64 * V];
  const int lane = lane_id(), wv = threadIdx.x >> 6;
  const int64_t b = blockIdx.y;
  const int64_t c0 = (int64_t)blockIdx.x * 64 * V;
  const int64_t c = c0 + (int64_t)lane * V;
  const int64_t rs = jb_off(a.off, b, a.L), re = jb_off(a.off, b + 1, a.L);
  float acc[V];
#pragma unroll
  for (int e = 0; e < V; ++e) acc[e] = 0.f;
  if (c < a.D) {
    const uintptr_t co = (uintptr_t)c * EB;
    for (int64_t row = rs + wv; row < re; row += 16 * UN) {
      float x[UN][V];
#pragma unroll
      for (int i = 0; i < UN; ++i)
        if (row + 16 * i < re) Vec<DT, V>::ld(a.j + (uintptr_t)(row + 16 * i) * a.j_stride + co, x[i]);
#pragma unroll
      for (int i = 0; i < UN; ++i)
        if (row + 16 * i < re) {
#pragma unroll
          for (int e = 0; e < V; ++e) acc[e] += x[i][e];
        }
    }
  }
#pragma unroll
  for (int e = 0; e < V; ++e) s_fold[wv * 64 * V + lane * V + e] = acc[e];
  __syncthreads();
  for (int j = (int)threadIdx.x; j < 64 * V; j += 1024) {
    if (c0 + j < a.D) {
      float t = 0.f;
#pragma unroll
      for (int k = 0; k < 16; ++k) t += s_fold[k * 64 * V + j];
      st1<DT>((void*)(a.out + (uintptr_t)(b * a.out_sb)), c0 + j, t);
    }
  }
}

static inline bool jb_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static inline bool jb_al16(int64_t bytes) { return (bytes & 15) == 0; }
// the stride of a single row (or a single sample) is never used
static inline bool jb_stride_ok(int64_t count, int64_t width, int64_t stride) { return count <= 1 || stride >= width; }

}  // namespace mi355

using namespace mi355;

#define JB_CHECK_COMMON(NAME, dtype, batch, L, offsets)                                                   \
  MI355_CHECK_ARG(elem_bytes(dtype) != 0, NAME ": unsupported dtype");                                    \
  MI355_CHECK_ARG(batch >= 1 && batch < ((int64_t)1 << 31), NAME ": batch must be in 1 .. 2^31");         \
  MI355_CHECK_ARG(L >= 0 && L < ((int64_t)1 << 34), NAME ": rows must be in 0 .. 2^34");                  \
  MI355_CHECK_ARG(offsets != nullptr, NAME ": null offsets")

#define JB_DISPATCH(dtype, KERNEL, grid, block, stream, args)                                             \
  do {                                                                                                    \
    if (dtype == kF32) KERNEL<kF32><<<grid, block, 0, stream>>>(args);                                    \
    else if (dtype == kBF16) KERNEL<kBF16><<<grid, block, 0, stream>>>(args);                             \
    else KERNEL<kF16><<<grid, block, 0, stream>>>(args);                                                  \
  } while (0)

#define JB_DISPATCH_V(dtype, vec, KERNEL, grid, block, stream, args)                                      \
  do {                                                                                                    \
    if (dtype == kF32) { if (vec) KERNEL<kF32, 4><<<grid, block, 0, stream>>>(args); else KERNEL<kF32, 1><<<grid, block, 0, stream>>>(args); } \
    else if (dtype == kBF16) { if (vec) KERNEL<kBF16, 8><<<grid, block, 0, stream>>>(args); else KERNEL<kBF16, 1><<<grid, block, 0, stream>>>(args); } \
    else { if (vec) KERNEL<kF16, 8><<<grid, block, 0, stream>>>(args); else KERNEL<kF16, 1><<<grid, block, 0, stream>>>(args); } \
  } while (0)

extern "C" int mi355_jagged_dense_bmm(const void* jagged, int64_t jagged_stride, const int64_t* offsets, int64_t batch, int64_t L,
                                      int64_t K, int64_t N, const void* dense, int64_t stride_db, int64_t stride_dk,
                                      int64_t stride_dn, const void* bias, int64_t bias_stride, void* out, int64_t out_stride,
                                      int dtype, hipStream_t stream) {
  JB_CHECK_COMMON("jagged_dense_bmm", dtype, batch, L, offsets);
  MI355_CHECK_ARG(K >= 1 && N >= 1 && K < ((int64_t)1 << 31) && N <= (int64_t)kJbCols * 65535,
                  "jagged_dense_bmm: K must be in 1 .. 2^31 and N in 1 .. 128 * 65535");
  MI355_CHECK_ARG(jb_stride_ok(L, K, jagged_stride) && jb_stride_ok(L, N, out_stride),
                  "jagged_dense_bmm: a row stride is smaller than the width");
  MI355_CHECK_ARG(stride_db >= 0 && stride_dk >= 1 && stride_dn >= 1, "jagged_dense_bmm: a stride of dense is not positive");
  MI355_CHECK_ARG(!bias || jb_stride_ok(batch, N, bias_stride), "jagged_dense_bmm: the stride of bias is smaller than N");
  if (L == 0) return MI355_OK;
  MI355_CHECK_ARG(jagged && dense && out, "jagged_dense_bmm: null buffer with rows > 0");
  const int eb = elem_bytes(dtype);
  MI355_CHECK_ARG((((uintptr_t)jagged | (uintptr_t)dense | (uintptr_t)bias | (uintptr_t)out) & (uintptr_t)(eb - 1)) == 0,
                  "jagged_dense_bmm: a base pointer is not aligned to the element size");
  JbmmArgs a{};
  a.j = (uintptr_t)jagged; a.d = (uintptr_t)dense; a.bias = (uintptr_t)bias; a.out = (uintptr_t)out;
  a.off = offsets; a.L = L; a.B = batch; a.K = K; a.N = N;
  a.j_stride = (L <= 1 ? K : jagged_stride) * eb; a.out_stride = (L <= 1 ? N : out_stride) * eb;
  a.d_sb = stride_db * eb; a.d_sk = stride_dk * eb; a.d_sn = stride_dn * eb;
  a.bias_sb = (batch <= 1 ? N : bias_stride) * eb;
  a.j_vec = jb_al16(jagged) && jb_al16(a.j_stride);
  // the unit-stride dimension of dense carries the pieces; every other stride must keep them 16-byte aligned
  a.d_vec = jb_al16(dense) && jb_al16(a.d_sb) && jb_al16(stride_dk == 1 ? a.d_sn : a.d_sk);
  const int64_t slots = L / kJbRows + batch + 1;
  MI355_CHECK_ARG(slots < ((int64_t)1 << 31), "jagged_dense_bmm: too many rows for one launch");
  const dim3 grid((unsigned)slots, (unsigned)ceil_div(N, kJbCols));
  JB_DISPATCH(dtype, jagged_dense_bmm_kernel, grid, dim3(256), stream, a);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

extern "C" int mi355_jagged_row_sum(const void* jagged, int64_t jagged_stride, const int64_t* offsets, int64_t batch, int64_t L,
                                    int64_t D, void* out, int64_t out_stride, int dtype, hipStream_t stream) {
  JB_CHECK_COMMON("jagged_row_sum", dtype, batch, L, offsets);
  MI355_CHECK_ARG(batch <= 65535, "jagged_row_sum: batch is limited to 65535 samples");
  MI355_CHECK_ARG(D >= 1 && D < ((int64_t)1 << 31), "jagged_row_sum: D must be in 1 .. 2^31");
  MI355_CHECK_ARG(jb_stride_ok(L, D, jagged_stride) && jb_stride_ok(batch, D, out_stride),
                  "jagged_row_sum: a row stride is smaller than the width");
  MI355_CHECK_ARG(out != nullptr, "jagged_row_sum: null out");
  MI355_CHECK_ARG(L == 0 || jagged, "jagged_row_sum: null buffer with rows > 0");
  const int eb = elem_bytes(dtype);
  MI355_CHECK_ARG((((uintptr_t)jagged | (uintptr_t)out) & (uintptr_t)(eb - 1)) == 0,
                  "jagged_row_sum: a base pointer is not aligned to the element size");
  JsumArgs a{};
  a.j = (uintptr_t)jagged; a.out = (uintptr_t)out; a.off = offsets; a.L = L; a.B = batch; a.D = D;
  a.j_stride = (L <= 1 ? D : jagged_stride) * eb; a.out_sb = (batch <= 1 ? D : out_stride) * eb;
  const bool vec = D % (16 / eb) == 0 && (L == 0 || (jb_al16(jagged) && jb_al16(a.j_stride)));
  const dim3 grid((unsigned)ceil_div(D, (int64_t)64 * (vec ? 16 / eb : 1)), (unsigned)batch);
  JB_DISPATCH_V(dtype, vec, jagged_row_sum_kernel, grid, dim3(1024), stream, a);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

// rows of a chunk of the sequence: 64 per output tile, so that about as many blocks work on a sample whatever M and N are; at
// least 256 and at most 4096
static inline int64_t jj_chunk_rows(int64_t M, int64_t N) {
  const int64_t c = 64 * ceil_div(M, kJbOut) * ceil_div(N, kJbOut);
  return c < 256 ? 256 : c > 4096 ? 4096 : c;
}

extern "C" int64_t mi355_jagged_jagged_bmm_workspace_bytes(int64_t batch, int64_t L, int64_t M, int64_t N) {
  if (batch < 1 || L < 0 || M < 1 || N < 1) return 0;
  const int64_t b = (L / jj_chunk_rows(M, N) + batch) * (M * N + N) * 4;   // per slot: the chunk sum of out, then of col_sum
  return b < 16 ? 16 : b;
}

extern "C" int mi355_jagged_jagged_bmm(const void* a_rows, int64_t a_stride, const void* b_rows, int64_t b_stride,
                                       const int64_t* offsets, int64_t batch, int64_t L, int64_t M, int64_t N, void* out,
                                       int64_t out_stride_b, int64_t out_stride_m, void* col_sum, int64_t col_sum_stride,
                                       int dtype, void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  JB_CHECK_COMMON("jagged_jagged_bmm", dtype, batch, L, offsets);
  MI355_CHECK_ARG(M >= 1 && N >= 1 && M <= (int64_t)kJbOut * 65535 && N <= (int64_t)kJbOut * 65535,
                  "jagged_jagged_bmm: M and N must be in 1 .. 64 * 65535");
  MI355_CHECK_ARG(batch <= 65535, "jagged_jagged_bmm: batch is limited to 65535 samples");
  MI355_CHECK_ARG(jb_stride_ok(L, M, a_stride) && jb_stride_ok(L, N, b_stride) && jb_stride_ok(M, N, out_stride_m),
                  "jagged_jagged_bmm: a row stride is smaller than the width");
  MI355_CHECK_ARG(jb_stride_ok(batch, M * N, out_stride_b) && (!col_sum || jb_stride_ok(batch, N, col_sum_stride)),
                  "jagged_jagged_bmm: a batch stride is smaller than the sample");
  MI355_CHECK_ARG(out != nullptr, "jagged_jagged_bmm: null out");
  MI355_CHECK_ARG(L == 0 || (a_rows && b_rows), "jagged_jagged_bmm: null buffer with rows > 0");
  MI355_CHECK_ARG(workspace && ((uintptr_t)workspace & 15) == 0 &&
                  workspace_bytes >= mi355_jagged_jagged_bmm_workspace_bytes(batch, L, M, N),
                  "jagged_jagged_bmm: workspace is null, not 16-byte aligned or too small");
  const int eb = elem_bytes(dtype);
  MI355_CHECK_ARG((((uintptr_t)a_rows | (uintptr_t)b_rows | (uintptr_t)out | (uintptr_t)col_sum) & (uintptr_t)(eb - 1)) == 0,
                  "jagged_jagged_bmm: a base pointer is not aligned to the element size");
  JjArgs a{};
  a.a = (uintptr_t)a_rows; a.bm = (uintptr_t)b_rows; a.out = (uintptr_t)out; a.colsum = (uintptr_t)col_sum;
  a.colsum_sb = (batch <= 1 ? N : col_sum_stride) * eb;
  a.off = offsets; a.partial = (float*)workspace; a.L = L; a.B = batch; a.M = M; a.N = N; a.chunk = jj_chunk_rows(M, N);
  a.a_stride = (L <= 1 ? M : a_stride) * eb; a.b_stride = (L <= 1 ? N : b_stride) * eb;
  a.out_sb = (batch <= 1 ? M * N : out_stride_b) * eb; a.out_sm = (M <= 1 ? N : out_stride_m) * eb;
  a.a_vec = jb_al16(a_rows) && jb_al16(a.a_stride);
  a.b_vec = jb_al16(b_rows) && jb_al16(a.b_stride);
  const int64_t slots = L / a.chunk + batch;
  MI355_CHECK_ARG(slots < ((int64_t)1 << 31), "jagged_jagged_bmm: too many rows for one launch");
  a.partial_r = a.partial + (size_t)slots * M * N;
  const dim3 grid((unsigned)slots, (unsigned)ceil_div(M, kJbOut), (unsigned)ceil_div(N, kJbOut));
  JB_DISPATCH(dtype, jagged_jagged_bmm_kernel, grid, dim3(256), stream, a);
  MI355_LAUNCH_CHECK();
  if (L > a.chunk) {   // (no sample has a second chunk otherwise)
    const dim3 fold((unsigned)ceil_div(M * N, 256), (unsigned)batch);
    MI355_CHECK_ARG(ceil_div(M * N, 256) < ((int64_t)1 << 31), "jagged_jagged_bmm: M N too large");
    JB_DISPATCH(dtype, jagged_jagged_bmm_fold_kernel, fold, dim3(256), stream, a);
    MI355_LAUNCH_CHECK();
  }
  return MI355_OK;
}

extern "C" int mi355_jagged_broadcast_add(const void* jagged, int64_t jagged_stride, const int64_t* offsets, int64_t batch,
                                          int64_t L, int64_t D, const void* dense, int64_t dense_stride, void* out,
                                          int64_t out_stride, int dtype, hipStream_t stream) {
  JB_CHECK_COMMON("jagged_broadcast_add", dtype, batch, L, offsets);
  MI355_CHECK_ARG(D >= 1 && D < ((int64_t)1 << 31), "jagged_broadcast_add: D must be in 1 .. 2^31");
  MI355_CHECK_ARG(jb_stride_ok(L, D, jagged_stride) && jb_stride_ok(L, D, out_stride) && jb_stride_ok(batch, D, dense_stride),
                  "jagged_broadcast_add: a row stride is smaller than the width");
  if (L == 0) return MI355_OK;
  MI355_CHECK_ARG(jagged && dense && out, "jagged_broadcast_add: null buffer with rows > 0");
  const int eb = elem_bytes(dtype);
  MI355_CHECK_ARG((((uintptr_t)jagged | (uintptr_t)dense | (uintptr_t)out) & (uintptr_t)(eb - 1)) == 0,
                  "jagged_broadcast_add: a base pointer is not aligned to the element size");
  JaddArgs a{};
  a.j = (uintptr_t)jagged; a.dense = (uintptr_t)dense; a.out = (uintptr_t)out; a.off = offsets; a.L = L; a.B = batch; a.D = D;
  a.j_stride = (L <= 1 ? D : jagged_stride) * eb; a.out_stride = (L <= 1 ? D : out_stride) * eb;
  a.dense_sb = (batch <= 1 ? D : dense_stride) * eb;
  const bool vec = D % (16 / eb) == 0 && jb_al16(jagged) && jb_al16(dense) && jb_al16(out) && jb_al16(a.j_stride) &&
                   jb_al16(a.out_stride) && jb_al16(a.dense_sb);
  int64_t gy = ceil_div(L, 4);
  gy = gy > 2048 ? 2048 : gy;
  const dim3 grid((unsigned)ceil_div(D, (int64_t)64 * (vec ? 16 / eb : 1)), (unsigned)gy);
  JB_DISPATCH_V(dtype, vec, jagged_broadcast_add_kernel, grid, dim3(256), stream, a);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}
