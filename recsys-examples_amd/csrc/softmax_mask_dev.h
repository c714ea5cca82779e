// The mask and extent layer of the softmax attention family: everything between a kernel's block-to-work mapping and its
// MFMA tile loop (softmax_tile_dev.h).  prefill_attn.hip (prefill_attn_kernel), softmax_attn_bwd.hip (sm_bwd_dq_kernel,
// sm_bwd_dkdv_kernel) and beam_decode.hip (the sequence bounds) are written on it, and so are the argument checks of their
// entry points.  This is the one statement of the semantics.
//
// Masks.  Every query row has a prefix bound `pre` (keys j < pre are seen) and, for the arbitrary kind, bands [lo, up):
//   none     pre = Lk
//   causal   pre = clamp(i + 1 + Lk - Lq, 0, Lk)                              (bottom-right aligned)
//   func     pre = clamp(F[0][i], 0, Lk), bands clamp(F[2p-1][i]) .. clamp(F[2p][i]), an interval with start >= end is empty
// A row past the end of its sequence sees nothing (pre = 0, no band).
//
// Extents.  SmExt describes a group of rows: the largest and the smallest prefix and the hull of the bands.  A wave reduces
// the extents of its rows (sm_ext_reduce); the forward and the dQ kernel exchange the four waves' extents through LDS once
// (sm_ext_exchange_sync).  A key tile [n0, n1) is loaded only if some wave's extent reaches it (SM_NEXT_TILE), a wave computes
// only the tiles its own rows reach (sm_hits), and the per-element test (SM_MASK_BITS) runs only on tiles that are not inside
// the smallest prefix of the wave.  A tile that is skipped would have had P = 0 for every row: in the forward the running
// max is unchanged, in the backward exact zeros are added, so skipping changes no bit of a result (skip_tiles = 0 turns the
// skipping off: every tile is loaded, computed and tested).
//
// The forward and the backward MUST skip by the same rule: a tile the forward skipped has to have P = 0 in the backward.
// They do because both are written on the functions and macros below; a kernel that keeps a piece written out (for a
// measured reason stated where it does) names the function it equals and has to be edited with it.
#pragma once
#include "common.h"
#include "softmax_tile_dev.h"

namespace mi355 {

constexpr int kSmMaskNone = 0, kSmMaskCausal = 1, kSmMaskFunc = 2;   // the `mask` argument of the C ABI
constexpr int kSmIntMax = 0x7fffffff;                                 // lo of an empty hull

struct SmExt { int pmax, pmin, lo, hi; };   // largest / smallest prefix of a group of rows, hull [lo, hi) of their bands (lo >= hi: none)

__device__ __forceinline__ int sm_clamp(int64_t x, int hi) { return x < 0 ? 0 : (x > hi ? hi : (int)x); }
__device__ __forceinline__ bool sm_hits(const SmExt& e, int n0, int n1) { return n0 < e.pmax || (e.lo < n1 && e.hi > n0); }

// Six pieces below are statement macros: SM_SEQ_BOUNDS, SM_ROW_EXT, SM_EXT_REDUCE, SM_NEXT_TILE, SM_MASK_BITS, SM_STORE_ROW.
// The kernels that use them are at the SGPR limit (func) or close to it in scheduling (D = 64): behind a __forceinline__
// function the same statements compiled to other vector instruction orders, more AGPRs or scalar changes that measured
// slower (per piece: profiles/softmax_mask_refactor.txt, section 0); expanded in place they compile to the instructions
// the kernels had with the lines written out, and there is still one definition.  Each is one statement (do { } while (0),
// used with its semicolon), its arguments are parenthesised, and its own locals end in an underscore.

// sequence b of a jagged batch: bounds clamped into the tensor and made monotone, so that no row outside it is ever touched
#define SM_SEQ_BOUNDS(cu, b, total, row0, len)                         \
  do {                                                                 \
    int64_t s_ = (cu)[(b)], e_ = (cu)[(b) + 1];                        \
    s_ = s_ < 0 ? 0 : (s_ > (total) ? (total) : s_);                   \
    e_ = e_ < s_ ? s_ : (e_ > (total) ? (total) : e_);                 \
    (row0) = s_; (len) = (int)(e_ - s_);                               \
  } while (0)
__device__ __forceinline__ void sm_seq_bounds(const int32_t* cu, int b, int64_t total, int64_t& row0, int& len) {
  SM_SEQ_BOUNDS(cu, b, total, row0, len);
}

// band [lo, up) (already clamped) joins the hull of e; an empty one does not
__device__ __forceinline__ void sm_ext_band(SmExt& e, int lo, int up) {
  if (lo < up) { e.lo = lo < e.lo ? lo : e.lo; e.hi = up > e.hi ? up : e.hi; }
}

// The extent of one row into `we` and its prefix bound into `pre`: we.pmax = we.pmin = pre, we.lo / we.hi the hull of its
// bands.  The caller declares `int pre = 0; SmExt we{0, 0, kSmIntMax, 0};` (a row that does not exist keeps these).
// i: the row inside its sequence, valid: it exists; frow: F[.][i] of the func kind (element p at frow[p * f_sp]), not read otherwise.
#define SM_ROW_EXT(MK, we, pre, valid, i, Lq, Lk, frow, f_sp, n_func)                                                 \
  do {                                                                                                               \
    if (valid) {                                                                                                     \
      if constexpr ((MK) == kSmMaskNone) (pre) = (Lk);                                                               \
      if constexpr ((MK) == kSmMaskCausal) (pre) = sm_clamp((int64_t)(i) + 1 + (Lk) - (Lq), (Lk));                   \
      if constexpr ((MK) == kSmMaskFunc) {                                                                           \
        (pre) = sm_clamp((frow)[0], (Lk));                                                                           \
        for (int p_ = 1; p_ + 1 < (n_func); p_ += 2) {                                                               \
          const int lo_ = sm_clamp((frow)[(int64_t)p_ * (f_sp)], (Lk)), up_ = sm_clamp((frow)[(int64_t)(p_ + 1) * (f_sp)], (Lk)); \
          sm_ext_band((we), lo_, up_);                                                                               \
        }                                                                                                            \
      }                                                                                                              \
    }                                                                                                                \
    (we).pmax = (pre); (we).pmin = (pre);                                                                            \
  } while (0)

// the extent of LANES consecutive lanes' rows (32: each half of the wave its own; 64: the wave), in every one of them
#define SM_EXT_REDUCE(e, LANES)                                                                     \
  do {                                                                                              \
    _Pragma("unroll") for (int off_ = 1; off_ < (LANES); off_ <<= 1) {                              \
      const int x0_ = __shfl_xor((e).pmax, off_, 64), x1_ = __shfl_xor((e).pmin, off_, 64);         \
      const int x2_ = __shfl_xor((e).lo, off_, 64), x3_ = __shfl_xor((e).hi, off_, 64);             \
      (e).pmax = x0_ > (e).pmax ? x0_ : (e).pmax; (e).pmin = x1_ < (e).pmin ? x1_ : (e).pmin;       \
      (e).lo = x2_ < (e).lo ? x2_ : (e).lo; (e).hi = x3_ > (e).hi ? x3_ : (e).hi;                   \
    }                                                                                               \
  } while (0)
// PMIN = false leaves pmin alone, for a caller that does not read it.
template <int LANES, bool PMIN = true>
__device__ __forceinline__ void sm_ext_reduce(SmExt& e) {
  if constexpr (PMIN) {
    SM_EXT_REDUCE(e, LANES);
  } else {
#pragma unroll
    for (int off = 1; off < LANES; off <<= 1) {
      const int x0 = __shfl_xor(e.pmax, off, 64), x2 = __shfl_xor(e.lo, off, 64), x3 = __shfl_xor(e.hi, off, 64);
      e.pmax = x0 > e.pmax ? x0 : e.pmax; e.lo = x2 < e.lo ? x2 : e.lo; e.hi = x3 > e.hi ? x3 : e.hi;
    }
  }
}

// a wave-uniform extent into scalar registers
__device__ __forceinline__ void sm_ext_uniform(SmExt& e) {
  e.pmax = __builtin_amdgcn_readfirstlane(e.pmax); e.pmin = __builtin_amdgcn_readfirstlane(e.pmin);
  e.lo = __builtin_amdgcn_readfirstlane(e.lo); e.hi = __builtin_amdgcn_readfirstlane(e.hi);
}

// The four waves' extents to every wave, through sExt[16].  CONTAINS A __syncthreads(): every thread of the workgroup calls it.
__device__ __forceinline__ void sm_ext_exchange_sync(int* sExt, int wv, int lane, const SmExt& we, SmExt (&be)[4]) {
  if (lane == 0) { sExt[4 * wv] = we.pmax; sExt[4 * wv + 1] = we.pmin; sExt[4 * wv + 2] = we.lo; sExt[4 * wv + 3] = we.hi; }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    be[w].pmax = __builtin_amdgcn_readfirstlane(sExt[4 * w]);
    be[w].pmin = __builtin_amdgcn_readfirstlane(sExt[4 * w + 1]);
    be[w].lo = __builtin_amdgcn_readfirstlane(sExt[4 * w + 2]);
    be[w].hi = __builtin_amdgcn_readfirstlane(sExt[4 * w + 3]);
  }
}

// Advances t to the first key tile at or after t, of nt, that some wave reaches (nt: none); be: the four waves' extents
#define SM_NEXT_TILE(skip, t, nt, be)                                                          \
  do {                                                                                         \
    if (!(skip)) { (t) = (t) < (nt) ? (t) : (nt); break; }                                     \
    for (; (t) < (nt); ++(t)) {                                                                \
      const int n0_ = (t) * kSmKeys, n1_ = n0_ + kSmKeys;                                      \
      if (sm_hits((be)[0], n0_, n1_) || sm_hits((be)[1], n0_, n1_) || sm_hits((be)[2], n0_, n1_) || sm_hits((be)[3], n0_, n1_)) break; \
    }                                                                                          \
  } while (0)

// Ors into `ok` bit j if the lane's row (prefix bound pre, bands in frow as for SM_ROW_EXT) sees the key of score register j
// of lane half h in the tile [n0, n1).  we: the extent of the wave's rows; the bands are walked only if their hull reaches the tile.
#define SM_MASK_BITS(MK, ok, skip, we, n0, n1, h, valid, pre, Lk, frow, f_sp, n_func)                                  \
  do {                                                                                                                 \
    _Pragma("unroll") for (int j_ = 0; j_ < 32; ++j_) {                                                                \
      const int key_ = (n0) + sm_key_of(j_, (h));                                                                      \
      (ok) |= (uint32_t)(key_ < (pre)) << j_;                                                                          \
    }                                                                                                                  \
    if constexpr ((MK) == kSmMaskFunc) {                                                                               \
      if (!(skip) || ((we).lo < (n1) && (we).hi > (n0))) {                                                             \
        for (int pp_ = 1; pp_ + 1 < (n_func); pp_ += 2) {                                                              \
          int lo_ = 0, up_ = 0;                                                                                        \
          if (valid) { lo_ = sm_clamp((frow)[(int64_t)pp_ * (f_sp)], (Lk)); up_ = sm_clamp((frow)[(int64_t)(pp_ + 1) * (f_sp)], (Lk)); } \
          _Pragma("unroll") for (int j_ = 0; j_ < 32; ++j_) {                                                          \
            const int key_ = (n0) + sm_key_of(j_, (h));                                                                \
            (ok) |= (uint32_t)((lo_ <= key_) & (key_ < up_)) << j_;                                                    \
          }                                                                                                            \
        }                                                                                                              \
      }                                                                                                                \
    }                                                                                                                  \
  } while (0)

// fp32 accumulators (d in the registers, the row or key r on the lane) times c, rounded once, to row `dst` (element 4 h).
// M: SmMma<DT>.  (The macro for the forward, see above; sm_store_row for everyone else.)
#define SM_STORE_ROW(M, D, dst, o, c)                                                        \
  do {                                                                                       \
    _Pragma("unroll") for (int ii_ = 0; ii_ < (D) / 32; ++ii_)                               \
      _Pragma("unroll") for (int g_ = 0; g_ < 4; ++g_) {                                     \
        sm_u32x2 x_;                                                                         \
        x_[0] = M::pack2((o)[ii_][4 * g_] * (c), (o)[ii_][4 * g_ + 1] * (c));                \
        x_[1] = M::pack2((o)[ii_][4 * g_ + 2] * (c), (o)[ii_][4 * g_ + 3] * (c));            \
        *reinterpret_cast<sm_u32x2*>((dst) + 32 * ii_ + 8 * g_) = x_;                        \
      }                                                                                      \
  } while (0)
template <int DT, int D>
__device__ __forceinline__ void sm_store_row(uint16_t* dst, const sm_f32x16 (&o)[D / 32], float c) {
  using M = SmMma<DT>;
  SM_STORE_ROW(M, D, dst, o, c);
}

}  // namespace mi355

// ---- host side.  mi355_prefill_attn and mi355_softmax_attn_bwd take the same leading arguments under the same names
// (include/recsys_amd.h); the two macros below read those names.

// The argument checks the two entry points share, in their order; defines `jagged`.  NAME: the op's message prefix;
// KTILE: keys per workgroup of the launch that Sk bounds; NFUNC_MAX / NFUNC_MSG: the op's own limit on n_func.
#define SM_ATTN_CHECK_COMMON(NAME, KTILE, NFUNC_MAX, NFUNC_MSG)                                                            \
  MI355_CHECK_ARG(dtype == kBF16 || dtype == kF16, NAME ": dtype must be bf16 or fp16");                                    \
  MI355_CHECK_ARG(D == 64 || D == 128, NAME ": head dim must be 64 or 128");                                                \
  MI355_CHECK_ARG(B >= 0 && Hq > 0 && Hkv > 0 && Hq % Hkv == 0, NAME ": Hq must be a multiple of Hkv");                     \
  MI355_CHECK_ARG(Sq >= 0 && Sk >= 0 && total_q >= 0 && total_k >= 0, NAME ": negative length");                            \
  MI355_CHECK_ARG(mask == kSmMaskNone || mask == kSmMaskCausal || mask == kSmMaskFunc,                                      \
                  NAME ": mask must be 0 (none), 1 (causal) or 2 (arbitrary func)");                                        \
  MI355_CHECK_ARG((cu_seqlens_q == nullptr) == (cu_seqlens_k == nullptr),                                                   \
                  NAME ": cu_seqlens_q and cu_seqlens_k come together (jagged) or not at all (dense)");                     \
  const bool jagged = cu_seqlens_q != nullptr;                                                                              \
  if (mask == kSmMaskFunc) {                                                                                                \
    MI355_CHECK_ARG(!jagged, NAME ": the arbitrary func mask applies to the dense form only (no cu_seqlens)");              \
    MI355_CHECK_ARG(n_func >= 1 && n_func % 2 == 1, NAME ": n_func must be odd and >= 1");                                  \
    MI355_CHECK_ARG(func_heads == 1 || func_heads == Hq, NAME ": func must have 1 or Hq heads");                            \
    MI355_CHECK_ARG(n_func <= NFUNC_MAX, NAME ": " NFUNC_MSG);                                                              \
  } else {                                                                                                                  \
    MI355_CHECK_ARG(func == nullptr, NAME ": func is given but the mask kind is not 2 (a causal or plain call takes none)"); \
  }                                                                                                                         \
  MI355_CHECK_ARG(skip_tiles == 0 || skip_tiles == 1, NAME ": skip_tiles must be 0 or 1");                                  \
  MI355_CHECK_ARG(B <= INT32_MAX && Hq <= INT32_MAX && Sq <= INT32_MAX - kSmRows && Sk <= INT32_MAX - KTILE &&              \
                      total_q <= INT32_MAX - kSmRows && total_k <= INT32_MAX - KTILE,                                       \
                  NAME ": a dimension does not fit 31 bits")

// The fields PrefillArgs and BwdArgs share, from the arguments (a jagged tensor has no batch stride; a func with one head
// serves every query head).
#define SM_ATTN_FILL_COMMON(c)                                                                                              \
  c.q = (const uint16_t*)q; c.k = (const uint16_t*)k; c.v = (const uint16_t*)v;                                             \
  c.cu_q = cu_seqlens_q; c.cu_k = cu_seqlens_k; c.func = func;                                                              \
  c.q_sb = jagged ? 0 : q_stride_b; c.q_ss = q_stride_s; c.q_sh = q_stride_h;                                               \
  c.k_sb = jagged ? 0 : k_stride_b; c.k_ss = k_stride_s; c.k_sh = k_stride_h;                                               \
  c.v_sb = jagged ? 0 : v_stride_b; c.v_ss = v_stride_s; c.v_sh = v_stride_h;                                               \
  c.f_sb = func_stride_b; c.f_sh = func_heads == 1 ? 0 : func_stride_h; c.f_sp = func_stride_f; c.f_si = func_stride_s;     \
  c.total_q = total_q; c.total_k = total_k;                                                                                 \
  c.B = (int)B; c.Sq = (int)Sq; c.Sk = (int)Sk; c.Hq = (int)Hq; c.G = (int)(Hq / Hkv);                                      \
  c.n_func = (int)n_func; c.skip = skip_tiles;                                                                              \
  c.scale_log2 = softmax_scale * kSmLog2e
