// Softmax attention backward of the semantic-ID generative-retrieval family: dQ, dK, dV of the forward in prefill_attn.hip
// (out = softmax(scale q k^T over the visible keys) v), for training through the flash-attention calls of
// examples/sid_gr/model/jagged_flash_attn_block.py.  Same coverage as the forward: bf16 / fp16, D = 64 / 128, GQA / MQA, dense
// with every stride an argument, jagged with clamped cu_seqlens, masks none / causal bottom-right / arbitrary_func.
//
// Two launches, no atomics, no fp32 dQ buffer: bitwise reproducible.  The only workspace is delta [Hq, rows] fp32 (laid out
// like lse), written by launch 1 and read by launch 2.  Both recompute P = exp2(scale log2e s - lse log2e) from the saved lse
// (no second online softmax) and dP = dO V^T, form dS = P (dP - delta), round P once (dV) and dS once (dQ, dK) to the operand
// type, accumulate in fp32, and round each gradient once on the way out; softmax_scale multiplies the fp32 sums of dQ and dK.
//
// Launch 1, sm_bwd_dq_kernel: the forward's layout (softmax_tile_dev.h).  A workgroup owns 128 query rows of one query head,
//   a wave 32 rows, the row on the lane; Q and dO fragments in registers.  Per key tile of 64: S^T = K Q^T and dP^T = V dO^T
//   (SmTile::scores over the [key][D + 8] images of K and of V) come out in sm_key_of register order, and dS^T goes from the
//   registers into dQ^T += K^T dS^T (SmTile::pv with the transposed K image in the place of V^T).  delta_i = sum_d dO_id out_id
//   is taken in fp32 from the fragments (one __shfl_xor 32) and written for launch 2.  Key tiles are skipped by the rule of
//   prefill_attn_kernel: both expand SM_NEXT_TILE and call sm_hits of softmax_mask_dev.h, where the mask semantics are stated.
// Launch 2, sm_bwd_dkdv_kernel: the mirror image.  A workgroup owns 128 keys of one kv head, a wave 32 keys, the key on the
//   lane; K and V fragments in registers; the dK^T and dV^T accumulators stay live across the G query heads of the group (in
//   head order: the GQA sum has a fixed order and stays inside the workgroup) and the query tiles of 64 rows.  Per tile Q and
//   dO are staged in both images: load_tile / store_tile with (Q, dO) gives Q by rows and dO^T, with (dO, Q) dO by rows and
//   Q^T.  S = Q K^T and dP = dO V^T (scores with the key fragments as the B operand) put the query in the register index;
//   dV^T += dO^T P and dK^T += Q^T dS take P / dS from the registers (pv).  lse, delta and the rows' mask values are per
//   register here, not per lane: they are staged in LDS per tile (interval ends already clamped) and read as broadcasts.
//   The four images are 68 KB at D = 128, so the LDS is dynamic and the function's limit is raised at its first launch.
//   A tile that does not reach the workgroup's keys is not loaded, and that is known before its loads are issued: under the
//   func kind the rows' extents (largest prefix, hull of the bands) are reduced straight from `func`, four tiles per step;
//   under the causal kind the largest prefix of a tile is that of its last row.  All global loads of a tile that is needed
//   (both stagings, lse, delta, the mask values) are then issued together.  From the staged values every wave reduces the
//   tile's extents once more (smallest prefix included) for its own decisions: it computes only tiles that reach its 32 keys
//   and tests elements only where some row does not see all of them through its prefix.
//
// A skipped tile would have had P = 0 everywhere, and adding the exact zeros changes no accumulator bit: skip_tiles = 0 gives
// the same bits.  A row with lse = -inf (no visible key) takes +inf as its exponent offset: P = exp2(s - inf) = 0, dS = 0,
// dQ = 0 exactly and no NaN.  A masked element is SELECTED to 0, not multiplied.  Every key of every sequence lies in one
// workgroup of launch 2 whether or not a query sees it, and every row of dq in one of launch 1: every element of dq / dk / dv
// inside the sequences is written, the caller zeroes nothing.  (Jagged: Sq / Sk are max_seqlen_q / max_seqlen_k and bound the
// launches as Sq bounds the forward's; rows of a sequence at or past max_seqlen_q are treated as absent, as the forward does.)
#include "common.h"
#include "softmax_mask_dev.h"
#include "../../include/recsys_amd.h"

#include <math.h>

namespace mi355 {

constexpr int kBwQRows = kSmKeys;      // query rows per tile of launch 2 (the tile that SmTile stages)
constexpr int kBwKeys = 128;           // keys per workgroup of launch 2 (4 waves x 32)
constexpr int kBwMaxFunc = 129;        // launch 2 stages n_func values per row in LDS

struct BwdArgs {
  const uint16_t* q;
  const uint16_t* k;
  const uint16_t* v;
  const uint16_t* out;      // contiguous, the forward's
  const uint16_t* dout;
  const int32_t* cu_q;      // [B + 1] or null (dense)
  const int32_t* cu_k;
  const int32_t* func;      // kSmMaskFunc only
  const float* lse;         // [B, Hq, Sq] / [Hq, total_q], natural log
  float* delta;             // same layout
  uint16_t* dq;             // [B, Sq, Hq, D] / [total_q, Hq, D]
  uint16_t* dk;             // [B, Sk, Hkv, D] / [total_k, Hkv, D]
  uint16_t* dv;
  int64_t q_sb, q_ss, q_sh, k_sb, k_ss, k_sh, v_sb, v_ss, v_sh, do_sb, do_ss, do_sh;
  int64_t f_sb, f_sh, f_sp, f_si;
  int64_t total_q, total_k;
  int B, Sq, Sk, Hq, Hkv, G, nqt, nkt, n_func, skip;
  float scale_log2, scale;
};

template <int DT> __device__ __forceinline__ void bw_unpack(uint32_t u, float& lo, float& hi);
template <> __device__ __forceinline__ void bw_unpack<kBF16>(uint32_t u, float& lo, float& hi) {
  lo = __uint_as_float(u << 16);
  hi = __uint_as_float(u & 0xffff0000u);
}
template <> __device__ __forceinline__ void bw_unpack<kF16>(uint32_t u, float& lo, float& hi) {
  const typename SmMma<kF16>::V2 x = __builtin_bit_cast(typename SmMma<kF16>::V2, u);
  lo = (float)x[0];
  hi = (float)x[1];
}

template <int DT, int D, int MK>
__global__ void __launch_bounds__(256) sm_bwd_dq_kernel(BwdArgs a) {
  using T = SmTile<DT, D>;
  constexpr int KS = T::KS, CH = T::CH;
  __shared__ __attribute__((aligned(16))) uint16_t sK[T::kSK];    // [key][KS]
  __shared__ __attribute__((aligned(16))) uint16_t sVr[T::kSK];   // [key][KS]
  __shared__ __attribute__((aligned(16))) uint16_t sKt[T::kSV];   // [d][VS]
  __shared__ int sExt[16];

  const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, h = lane >> 5;
  int64_t id = blockIdx.x;
  const int hq = (int)(id % a.Hq); id /= a.Hq;
  const int b = (int)(id % a.B);
  const int qi = (int)(id / a.B);
  const int qt = a.nqt - 1 - qi;   // late query tiles first, heads fastest (the forward's order)
  const int hk = hq / a.G;
  const bool skip = a.skip != 0;

  int64_t qrow0 = 0, krow0 = 0;
  int Lq = a.Sq, Lk = a.Sk;
  if (a.cu_q) {
    sm_seq_bounds(a.cu_q, b, a.total_q, qrow0, Lq);
    sm_seq_bounds(a.cu_k, b, a.total_k, krow0, Lk);
  }
  if (qt * kSmRows >= Lq) return;   // (block-uniform: no barrier has been passed)

  const int i = qt * kSmRows + wv * 32 + r;   // query row of this lane inside its sequence
  const bool valid = i < Lq;
  const int32_t* frow = nullptr;
  if constexpr (MK == kSmMaskFunc) frow = a.func + (int64_t)b * a.f_sb + (int64_t)hq * a.f_sh + (int64_t)i * a.f_si;

  // ---- the row's extents, the wave's, the workgroup's
  int pre = 0; SmExt we{0, 0, kSmIntMax, 0};   // (a row past the sequence end sees nothing)
  SM_ROW_EXT(MK, we, pre, valid, i, Lq, Lk, frow, a.f_sp, a.n_func);
  sm_ext_reduce<32>(we);
  SmExt be[4];
  sm_ext_exchange_sync(sExt, wv, lane, we, be);
  sm_ext_uniform(we);

  const int nt = (Lk + kSmKeys - 1) / kSmKeys;
  auto next_tile = [&](int t) { SM_NEXT_TILE(skip, t, nt, be); return t; };

  // ---- the row's operands and constants: Q, dO, delta = dO . out (written for launch 2), the exponent offset lse log2 e
  const int64_t orow = (a.cu_q ? qrow0 : (int64_t)b * a.Sq) + i;
  const int64_t li = a.cu_q ? (int64_t)hq * a.total_q + qrow0 + i : ((int64_t)b * a.Hq + hq) * a.Sq + i;
  sm_u32x4 qf[D / 16], dof[D / 16];
  T::load_q(a.q + (int64_t)b * a.q_sb + (qrow0 + i) * a.q_ss + (int64_t)hq * a.q_sh + 8 * h, valid, qf);
  T::load_q(a.dout + (int64_t)b * a.do_sb + (qrow0 + i) * a.do_ss + (int64_t)hq * a.do_sh + 8 * h, valid, dof);
  float dl = 0.f, l2 = INFINITY;   // a row without a visible key (lse = -inf), or past the end: P = exp2(s - inf) = 0
  {
    sm_u32x4 of[D / 16];
    T::load_q(a.out + (orow * a.Hq + hq) * D + 8 * h, valid, of);
#pragma unroll
    for (int s = 0; s < D / 16; ++s)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float x0, x1, y0, y1;
        bw_unpack<DT>(dof[s][e], x0, x1);
        bw_unpack<DT>(of[s][e], y0, y1);
        dl = fmaf(x0, y0, dl);
        dl = fmaf(x1, y1, dl);
      }
    dl += __shfl_xor(dl, 32, 64);
    if (valid) {
      const float l = a.lse[li];
      if (l != -INFINITY) l2 = l * kSmLog2e;
      if (h == 0) a.delta[li] = dl;
    }
  }

  sm_f32x16 acc[D / 32];
  T::zero_acc(acc);

  const uint16_t* kb = a.k + (int64_t)b * a.k_sb + (int64_t)hk * a.k_sh + krow0 * a.k_ss;
  const uint16_t* vb = a.v + (int64_t)b * a.v_sb + (int64_t)hk * a.v_sh + krow0 * a.v_ss;

  // register staging, one tile ahead: K by rows and K^T (load_tile with K in both places), V by rows
  typename T::Stage st;
  sm_u32x4 vreg[T::NK];
  auto load_tile = [&](int t) {
    T::load_tile(st, kb, kb, a.k_ss, a.k_ss, t, Lk, tid);
    const int nv = Lk - t * kSmKeys;
#pragma unroll
    for (int ii = 0; ii < T::NK; ++ii) {
      const int u = tid + 256 * ii, key = u / CH, c = u % CH;
      vreg[ii] = T::ld_row(vb, a.v_ss, t * kSmKeys + key, nv, key, c);
    }
  };

  int t = next_tile(0);
  if (t < nt) load_tile(t);
  while (t < nt) {
    const int n0 = t * kSmKeys, n1 = n0 + kSmKeys;
    __syncthreads();
    T::store_tile(st, sK, sKt, tid);
#pragma unroll
    for (int ii = 0; ii < T::NK; ++ii) {
      const int u = tid + 256 * ii, key = u / CH, c = u % CH;
      *reinterpret_cast<sm_u32x4*>(sVr + key * KS + 8 * c) = vreg[ii];
    }
    __syncthreads();
    const int tn = next_tile(t + 1);
    if (tn < nt) load_tile(tn);

    if (!skip || sm_hits(we, n0, n1)) {   // (wave-uniform; no barrier inside)
      float p[32], dp[32];
      T::scores(sK, qf, a.scale_log2, r, h, p);
      T::scores(sVr, dof, 1.0f, r, h, dp);
      uint32_t ok = 0xffffffffu;
      if (!skip || n1 > we.pmin) {   // some row of the wave does not see the whole tile through its prefix
        ok = 0;
        SM_MASK_BITS(MK, ok, skip, we, n0, n1, h, valid, pre, Lk, frow, a.f_sp, a.n_func);
      }
#pragma unroll
      for (int j = 0; j < 32; ++j) {   // dS = P (dP - delta), in place of the score
        const float pj = ((ok >> j) & 1u) ? __builtin_amdgcn_exp2f(p[j] - l2) : 0.f;
        p[j] = pj * (dp[j] - dl);
      }
      T::pv(sKt, r, h, p, acc);   // dQ^T += K^T dS^T
    }
    t = tn;
  }

  if (valid) sm_store_row<DT, D>(a.dq + (orow * a.Hq + hq) * D + 4 * h, acc, a.scale);
}

template <int DT, int D, int MK>
__global__ void __launch_bounds__(256) sm_bwd_dkdv_kernel(BwdArgs a) {
  using T = SmTile<DT, D>;
  extern __shared__ __attribute__((aligned(16))) uint16_t bw_smem[];
  uint16_t* const sQ = bw_smem;              // [row][KS]
  uint16_t* const sdO = sQ + T::kSK;         // [row][KS]
  uint16_t* const sQt = sdO + T::kSK;        // [d][VS]
  uint16_t* const sdOt = sQt + T::kSV;       // [d][VS]
  float* const sL = reinterpret_cast<float*>(sdOt + T::kSV);   // [64] lse log2 e (+inf: the row sees nothing or is absent)
  float* const sDl = sL + kBwQRows;                            // [64] delta
  int* const sHit = reinterpret_cast<int*>(sDl + kBwQRows);    // [2][4] the scan's answers
  int* const sF = sHit + 8;                                    // [nf][64] prefix bound, band ends, clamped to [0, Lk]

  const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, h = lane >> 5;
  int64_t id = blockIdx.x;
  const int hk = (int)(id % a.Hkv); id /= a.Hkv;
  const int b = (int)(id % a.B);
  const int kt = (int)(id / a.B);   // early key tiles (the longest under a causal mask) first
  const bool skip = a.skip != 0;

  int64_t qrow0 = 0, krow0 = 0;
  int Lq = a.Sq, Lk = a.Sk;
  if (a.cu_q) {
    sm_seq_bounds(a.cu_q, b, a.total_q, qrow0, Lq);
    sm_seq_bounds(a.cu_k, b, a.total_k, krow0, Lk);
  }
  const int key0 = kt * kBwKeys;
  if (key0 >= Lk) return;   // (block-uniform: no barrier has been passed)
  const int Lqv = Lq < a.Sq ? Lq : a.Sq;   // jagged: rows at or past max_seqlen_q were not computed by the forward

  const int kw0 = key0 + wv * 32, key = kw0 + r;
  const bool kvalid = key < Lk;
  sm_u32x4 kf[D / 16], vf[D / 16];
  T::load_q(a.k + (int64_t)b * a.k_sb + (krow0 + key) * a.k_ss + (int64_t)hk * a.k_sh + 8 * h, kvalid, kf);
  T::load_q(a.v + (int64_t)b * a.v_sb + (krow0 + key) * a.v_ss + (int64_t)hk * a.v_sh + 8 * h, kvalid, vf);

  sm_f32x16 dk[D / 32], dv[D / 32];
  T::zero_acc(dk);
  T::zero_acc(dv);

  const int nf = MK == kSmMaskFunc ? a.n_func : 1;
  const int nqt = (Lqv + kBwQRows - 1) / kBwQRows;
  int t0 = 0;
  if (MK == kSmMaskCausal && skip) {   // rows before key0 - (Lk - Lq) see none of this workgroup's keys
    const int64_t first = (int64_t)key0 - ((int64_t)Lk - Lq);
    t0 = first > 0 ? (int)(first / kBwQRows) : 0;
  }

  int scan = 0;   // steps of the scan below so far
  for (int g = 0; g < a.G; ++g) {
    const int hq = hk * a.G + g;
    const uint16_t* qb = a.q + (int64_t)b * a.q_sb + (int64_t)hq * a.q_sh + qrow0 * a.q_ss;
    const uint16_t* dob = a.dout + (int64_t)b * a.do_sb + (int64_t)hq * a.do_sh + qrow0 * a.do_ss;
    const int64_t lbase = a.cu_q ? (int64_t)hq * a.total_q + qrow0 : ((int64_t)b * a.Hq + hq) * a.Sq;
    const int32_t* fb = nullptr;
    if constexpr (MK == kSmMaskFunc) fb = a.func + (int64_t)b * a.f_sb + (int64_t)hq * a.f_sh;

    for (int t = t0; t < nqt; ++t) {
      if constexpr (MK == kSmMaskFunc) {
        if (skip) {
          // Scan ahead to the next tile that reaches this workgroup's keys, four tiles per step: wave w takes tile t + w, a
          // lane one of its rows straight from `func`, and one barrier publishes the four answers (slots alternate by step, so
          // a step's answers are never overwritten while a slower wave still reads them).  On a flattened batch most tiles
          // belong to other sequences; staging each of them to find that out cost two barriers and a round trip apiece.
          while (t < nqt) {
            const int tt = t + wv, i = tt * kBwQRows + lane;
            SmExt x{0, 0, kSmIntMax, 0};
            if (tt < nqt && i < Lqv) {   // (equal to SM_ROW_EXT less pmin; edit both)
              const int32_t* fr = fb + (int64_t)i * a.f_si;
              x.pmax = sm_clamp(fr[0], Lk);
              for (int pp = 1; pp + 1 < nf; pp += 2) {
                const int lo = sm_clamp(fr[(int64_t)pp * a.f_sp], Lk), up = sm_clamp(fr[(int64_t)(pp + 1) * a.f_sp], Lk);
                sm_ext_band(x, lo, up);
              }
            }
            sm_ext_reduce<64, false>(x);   // (pmin is not needed to find a tile)
            int* const slot = sHit + 4 * (scan & 1);
            ++scan;
            if (lane == 0) slot[wv] = sm_hits(x, key0, key0 + kBwKeys) ? 1 : 0;   // (a tile past the end has no rows: no hit)
            __syncthreads();
            const int first = slot[0] ? 0 : (slot[1] ? 1 : (slot[2] ? 2 : (slot[3] ? 3 : 4)));
            t += first;
            if (first < 4) break;
          }
          if (t >= nqt) break;
        }
      }
      const int q0 = t * kBwQRows;
      if constexpr (MK != kSmMaskFunc) {
        if (skip) {   // the last row of the tile has its largest prefix: a tile that does not reach key0 is not loaded
          const int il = (q0 + kBwQRows < Lqv ? q0 + kBwQRows : Lqv) - 1;
          const int pmax = MK == kSmMaskNone ? Lk : sm_clamp((int64_t)il + 1 + Lk - Lq, Lk);
          if (pmax <= key0) continue;   // (block-uniform; no barrier has been passed in this step)
        }
      }
      // Every tile that gets here is needed (func: found by the scan above).  Its global loads are issued together, before the
      // barrier that waits for the previous tile's readers: Q and dO in both stagings, and the rows' constants.
      typename T::Stage sa, sb;
      T::load_tile(sa, qb, dob, a.q_ss, a.do_ss, t, Lqv, tid);    // Q by rows, dO^T
      T::load_tile(sb, dob, qb, a.do_ss, a.q_ss, t, Lqv, tid);    // dO by rows, Q^T
      float l2 = INFINITY, dl = 0.f;
      int pre = 0;
      if (tid < kBwQRows) {
        const int i = q0 + tid;
        if (i < Lqv) {
          const float l = a.lse[lbase + i];
          if (l != -INFINITY) l2 = l * kSmLog2e;
          dl = a.delta[lbase + i];
          if constexpr (MK == kSmMaskNone) pre = Lk;
          if constexpr (MK == kSmMaskCausal) pre = sm_clamp((int64_t)i + 1 + Lk - Lq, Lk);
        }
      }
      __syncthreads();   // the previous tile is no longer read
      if (tid < kBwQRows) {
        sL[tid] = l2;
        sDl[tid] = dl;
        if constexpr (MK != kSmMaskFunc) sF[tid] = pre;
      }
      if constexpr (MK == kSmMaskFunc) {
        for (int idx = tid; idx < kBwQRows * nf; idx += 256) {
          const int row = idx & (kBwQRows - 1), p = idx >> 6, i = q0 + row;
          sF[idx] = i < Lqv ? sm_clamp(fb[(int64_t)p * a.f_sp + (int64_t)i * a.f_si], Lk) : 0;
        }
      }
      T::store_tile(sa, sQ, sdOt, tid);
      T::store_tile(sb, sdO, sQt, tid);
      __syncthreads();

      // the extents of the tile's 64 rows, for the wave's own decisions (every wave reduces the same staged values)
      SmExt e{sF[lane], 0, kSmIntMax, 0};
      e.pmin = e.pmax;
      for (int pp = 1; pp + 1 < nf; pp += 2) {
        const int lo = sF[pp * kBwQRows + lane], up = sF[(pp + 1) * kBwQRows + lane];
        sm_ext_band(e, lo, up);
      }
      SM_EXT_REDUCE(e, 64);
      sm_ext_uniform(e);

      if (!skip || sm_hits(e, kw0, kw0 + 32)) {   // (wave-uniform; no barrier inside)
        float p[32], dp[32];
        T::scores(sQ, kf, a.scale_log2, r, h, p);     // register j: query row sm_key_of(j, h) of the tile
        T::scores(sdO, vf, 1.0f, r, h, dp);
        uint32_t ok = 0xffffffffu;
        if (!skip || kw0 + 32 > e.pmin) {   // some row does not see all of the wave's keys through its prefix
          ok = 0;
#pragma unroll
          for (int j = 0; j < 32; ++j) ok |= (uint32_t)(key < sF[sm_key_of(j, h)]) << j;
          if constexpr (MK == kSmMaskFunc) {
            if (!skip || (e.lo < kw0 + 32 && e.hi > kw0)) {
              for (int pp = 1; pp + 1 < nf; pp += 2) {
                const int* flo = sF + pp * kBwQRows;
                const int* fup = flo + kBwQRows;
#pragma unroll
                for (int j = 0; j < 32; ++j) {
                  const int qr = sm_key_of(j, h);
                  ok |= (uint32_t)((flo[qr] <= key) & (key < fup[qr])) << j;
                }
              }
            }
          }
        }
#pragma unroll
        for (int j = 0; j < 32; ++j) {
          const int qr = sm_key_of(j, h);
          const float pj = ((ok >> j) & 1u) ? __builtin_amdgcn_exp2f(p[j] - sL[qr]) : 0.f;
          p[j] = pj;
          dp[j] = pj * (dp[j] - sDl[qr]);
        }
        // The two fences keep the fragment reads of one product from being hoisted over the other: without them the D = 128
        // instantiation without a mask spilled 7 registers.
        __builtin_amdgcn_sched_barrier(0);
        T::pv(sdOt, r, h, p, dv);    // dV^T += dO^T P
        __builtin_amdgcn_sched_barrier(0);
        T::pv(sQt, r, h, dp, dk);    // dK^T += Q^T dS
      }
    }
  }

  if (kvalid) {
    const int64_t krow = (a.cu_q ? krow0 : (int64_t)b * a.Sk) + key;
    sm_store_row<DT, D>(a.dk + (krow * a.Hkv + hk) * D + 4 * h, dk, a.scale);
    sm_store_row<DT, D>(a.dv + (krow * a.Hkv + hk) * D + 4 * h, dv, 1.0f);
  }
}

template <int DT, int D>
static size_t bw_dkdv_lds(int nf) {
  using T = SmTile<DT, D>;
  return 2 * (size_t)(2 * T::kSK + 2 * T::kSV) + 4 * (size_t)kBwQRows * (2 + nf) + 4 * 8;
}

// launches kernel instance K with `smem` bytes of dynamic LDS; the instance's limit is raised to the largest size asked so far
template <auto K>
static int bw_launch_lds(dim3 grid, size_t smem, hipStream_t stream, const BwdArgs& c) {
  static size_t limit = 0;
  if (smem > limit) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(K), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (e != hipSuccess) { mi355_set_error(hipGetErrorString(e)); return MI355_ELAUNCH; }
    limit = smem;
  }
  hipLaunchKernelGGL(K, grid, dim3(256), smem, stream, c);
  return MI355_OK;
}

template <int DT, int D, int MK>
static int bw_launch_mask(dim3 gq, dim3 gk, hipStream_t stream, const BwdArgs& c) {
  if (gq.x > 0) hipLaunchKernelGGL((sm_bwd_dq_kernel<DT, D, MK>), gq, dim3(256), 0, stream, c);
  if (gk.x > 0) return bw_launch_lds<sm_bwd_dkdv_kernel<DT, D, MK>>(gk, bw_dkdv_lds<DT, D>(MK == kSmMaskFunc ? c.n_func : 1), stream, c);
  return MI355_OK;
}

template <int DT, int D>
static int bw_launch(int mask, dim3 gq, dim3 gk, hipStream_t stream, const BwdArgs& c) {
  if (mask == kSmMaskNone) return bw_launch_mask<DT, D, kSmMaskNone>(gq, gk, stream, c);
  if (mask == kSmMaskCausal) return bw_launch_mask<DT, D, kSmMaskCausal>(gq, gk, stream, c);
  return bw_launch_mask<DT, D, kSmMaskFunc>(gq, gk, stream, c);
}

}  // namespace mi355

using namespace mi355;

int mi355_softmax_attn_bwd(const void* q, int64_t q_stride_b, int64_t q_stride_s, int64_t q_stride_h, const void* k,
                           int64_t k_stride_b, int64_t k_stride_s, int64_t k_stride_h, const void* v, int64_t v_stride_b,
                           int64_t v_stride_s, int64_t v_stride_h, const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k,
                           int64_t B, int64_t Sq, int64_t Sk, int64_t total_q, int64_t total_k, int64_t Hq, int64_t Hkv, int64_t D,
                           int mask, const int32_t* func, int64_t n_func, int64_t func_heads, int64_t func_stride_b,
                           int64_t func_stride_h, int64_t func_stride_f, int64_t func_stride_s, float softmax_scale,
                           int skip_tiles, const void* out, const void* dout, int64_t dout_stride_b, int64_t dout_stride_s,
                           int64_t dout_stride_h, const float* lse, float* delta, void* dq, void* dk, void* dv, int dtype,
                           hipStream_t stream) {
  SM_ATTN_CHECK_COMMON("softmax_attn_bwd", kBwKeys, kBwMaxFunc, "n_func above 129 (64 bands) is not supported by the dK/dV pass");
  const int64_t qrows = jagged ? total_q : B * Sq, krows = jagged ? total_k : B * Sk;
  const bool has_q = B > 0 && qrows > 0 && Sq > 0, has_k = B > 0 && krows > 0 && Sk > 0;
  if (!has_q && !has_k) return MI355_OK;
  if (has_q) {
    MI355_CHECK_ARG(q && out && dout && lse && delta && dq, "softmax_attn_bwd: null pointer (q, out, dout, lse, delta or dq)");
    MI355_CHECK_ARG(sm_aligned(q, q_stride_b, q_stride_s, q_stride_h) && (uintptr_t)out % 16 == 0 && (uintptr_t)dq % 16 == 0,
                    "softmax_attn_bwd: q, out and dq need 16-byte aligned rows (base aligned, strides multiples of 8 elements)");
    MI355_CHECK_ARG(sm_aligned(dout, dout_stride_b, dout_stride_s, dout_stride_h),
                    "softmax_attn_bwd: dout needs 16-byte aligned rows (base aligned, strides multiples of 8 elements)");
    MI355_CHECK_ARG((uintptr_t)lse % 4 == 0 && (uintptr_t)delta % 4 == 0, "softmax_attn_bwd: lse or delta is misaligned");
  }
  if (has_k) {
    MI355_CHECK_ARG(k && v && dk && dv, "softmax_attn_bwd: null pointer (k, v, dk or dv)");
    MI355_CHECK_ARG(sm_aligned(k, k_stride_b, k_stride_s, k_stride_h) && sm_aligned(v, v_stride_b, v_stride_s, v_stride_h) &&
                        (uintptr_t)dk % 16 == 0 && (uintptr_t)dv % 16 == 0,
                    "softmax_attn_bwd: k / v / dk / dv rows need 16-byte alignment (base aligned, strides multiples of 8 elements)");
  }
  if (mask == kSmMaskFunc && has_q) MI355_CHECK_ARG(func && (uintptr_t)func % 4 == 0, "softmax_attn_bwd: func is null or misaligned");
  const int64_t nqt = has_q ? ceil_div(Sq, (int64_t)kSmRows) : 0;   // jagged: Sq / Sk are max_seqlen_q / max_seqlen_k
  const int64_t nkt = has_k ? ceil_div(Sk, (int64_t)kBwKeys) : 0;
  MI355_CHECK_ARG(nqt * B * Hq <= INT32_MAX && nkt * B * Hkv <= INT32_MAX, "softmax_attn_bwd: launch too large");

  BwdArgs c;
  SM_ATTN_FILL_COMMON(c);
  c.out = (const uint16_t*)out; c.dout = (const uint16_t*)dout; c.lse = lse; c.delta = delta;
  c.dq = (uint16_t*)dq; c.dk = (uint16_t*)dk; c.dv = (uint16_t*)dv;
  c.do_sb = jagged ? 0 : dout_stride_b; c.do_ss = dout_stride_s; c.do_sh = dout_stride_h;
  c.Hkv = (int)Hkv; c.nqt = (int)nqt; c.nkt = (int)nkt; c.scale = softmax_scale;
  const dim3 gq((unsigned)(nqt * B * Hq)), gk((unsigned)(nkt * B * Hkv));
  int rc;
  if (dtype == kBF16) rc = D == 64 ? bw_launch<kBF16, 64>(mask, gq, gk, stream, c) : bw_launch<kBF16, 128>(mask, gq, gk, stream, c);
  else rc = D == 64 ? bw_launch<kF16, 64>(mask, gq, gk, stream, c) : bw_launch<kF16, 128>(mask, gq, gk, stream, c);
  if (rc != MI355_OK) return rc;
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}
