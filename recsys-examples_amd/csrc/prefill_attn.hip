// Softmax prefill attention (forward) of the semantic-ID generative-retrieval family: the kernel that builds the context the
// beam-search decode kernels (beam_decode.hip) attend over.
//
// Replaces (reference): the three flash-attention calls of examples/sid_gr/model/jagged_flash_attn_block.py and
// examples/sid-gr-inference/.../gr_kernels/prefill/flash_attn_backend.py -- flash_attn_varlen_func(causal=True) on a
// flattened jagged batch, flash_attn_func(causal=True) on a padded batch, and flash_attn.cute's flash_attn_func(arbitrary=True,
// aux_tensors=[arbitrary_func]) for the beam-isolation / target-aware masks.  flash_attn is CUDA / CuTe DSL; this is written
// for gfx950 from the semantics (bottom-right aligned causal as in flash-attn >= 2.1; the interval encoding of arbitrary_func,
// examples/sid_gr/model/attention_mask.py:210-275, which is the `func` of hstu_attn.hip).
//
// One launch, no workspace, no atomics: bitwise reproducible.  prefill_attn_kernel has the tile loop of beam_ctx_kernel, whose
// pieces are SmTile of softmax_tile_dev.h (LDS layout, register-to-key mapping, online softmax and P V are described there):
// one workgroup (4 waves) owns one (sequence, query head, tile of 128 query rows); K / V come from kv head h / G; the global
// loads of the next tile are issued before the MFMAs of this one and written to LDS after them.  From the header this kernel
// takes the types, the constants, SmMma, sm_key_of and SmTile::scores; the Q load, the K / V staging, the softmax step and
// the P V loop are WRITTEN OUT below, equal line for line to SmTile's.  Measured reason: the arbitrary-mask instantiations
// are at the SGPR limit and the D = 64 ones close to it in scheduling; with any of those pieces taken from SmTile the
// compiler placed scalar spill reloads and the schedule differently, and some shape lost 0.5 - 3 % (arbitrary mask with
// skip_tiles = 0, or dense D = 64 at S = 8192).  As it stands the kernel compiles to the instructions it had before the
// header existed.  A change to one of these pieces in the header has to be made here as well.
//
// Masks, row extents and tile skipping are those of softmax_mask_dev.h, the one statement of their semantics, shared with
// the backward (softmax_attn_bwd.hip).  This kernel takes that layer's functions where they leave its instructions alone
// and its statement macros (SM_SEQ_BOUNDS, SM_ROW_EXT, SM_EXT_REDUCE, SM_NEXT_TILE, SM_MASK_BITS, SM_STORE_ROW) where a call
// did not -- by the rule above: as it stands the kernel still compiles to the instructions it had.  One piece, the wave
// exchange, is WRITTEN OUT and marked "equal to sm_ext_exchange_sync; edit both" (profiles/softmax_mask_refactor.txt).
//
// A row with no visible key -- in a tile (m stays -inf: the exponent is taken against 0, so P = exp2(-inf) = 0 and no
// inf - inf arises) or at all (l = 0: out = 0, lse = -inf).
#include "common.h"
#include "softmax_mask_dev.h"
#include "../../include/recsys_amd.h"

#include <math.h>

namespace mi355 {

struct PrefillArgs {
  const uint16_t* q;
  const uint16_t* k;
  const uint16_t* v;
  const int32_t* cu_q;      // [B + 1] or null (dense)
  const int32_t* cu_k;
  const int32_t* func;      // kSmMaskFunc only
  uint16_t* out;            // [B, Sq, Hq, D] / [total_q, Hq, D]
  float* lse;               // [B, Hq, Sq] / [Hq, total_q], natural log
  int64_t q_sb, q_ss, q_sh, k_sb, k_ss, k_sh, v_sb, v_ss, v_sh;
  int64_t f_sb, f_sh, f_sp, f_si;
  int64_t total_q, total_k;
  int B, Sq, Sk, Hq, G, nqt, n_func, skip;
  float scale_log2;
};

template <int DT, int D, int MK>
__global__ void __launch_bounds__(256) prefill_attn_kernel(PrefillArgs a) {
  constexpr int KS = D + 8;          // = SmTile::KS
  constexpr int VS = kSmKeys + 4;    // = SmTile::VS
  constexpr int CH = D / 8;          // 16-byte chunks per row
  __shared__ __attribute__((aligned(16))) uint16_t sK[kSmKeys * KS];
  __shared__ __attribute__((aligned(16))) uint16_t sV[D * VS];
  __shared__ int sExt[16];
  using M = SmMma<DT>;
  using T = SmTile<DT, D>;

  const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, h = lane >> 5;
  int64_t id = blockIdx.x;
  const int hq = (int)(id % a.Hq); id /= a.Hq;
  const int b = (int)(id % a.B);
  const int qi = (int)(id / a.B);
  const int qt = a.nqt - 1 - qi;   // late query tiles (the longest under a causal mask) first; heads fastest: a group shares K / V in L2
  const int hk = hq / a.G;
  const bool skip = a.skip != 0;

  int64_t qrow0 = 0, krow0 = 0;
  int Lq = a.Sq, Lk = a.Sk;
  if (a.cu_q) {   // jagged
    SM_SEQ_BOUNDS(a.cu_q, b, a.total_q, qrow0, Lq);
    SM_SEQ_BOUNDS(a.cu_k, b, a.total_k, krow0, Lk);
  }
  if (qt * kSmRows >= Lq) return;   // (block-uniform: no barrier has been passed)

  const int i = qt * kSmRows + wv * 32 + r;   // query row of this lane inside its sequence
  const bool valid = i < Lq;
  const int32_t* frow = nullptr;
  if constexpr (MK == kSmMaskFunc) frow = a.func + (int64_t)b * a.f_sb + (int64_t)hq * a.f_sh + (int64_t)i * a.f_si;

  // ---- the row's extents, the wave's, the workgroup's
  int pre = 0; SmExt we{0, 0, kSmIntMax, 0};   // (a row past the sequence end sees nothing)
  SM_ROW_EXT(MK, we, pre, valid, i, Lq, Lk, frow, a.f_sp, a.n_func);
  SM_EXT_REDUCE(we, 32);
  // (equal to sm_ext_exchange_sync; edit both)
  if (lane == 0) { sExt[4 * wv] = we.pmax; sExt[4 * wv + 1] = we.pmin; sExt[4 * wv + 2] = we.lo; sExt[4 * wv + 3] = we.hi; }
  __syncthreads();
  SmExt be[4];
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    be[w].pmax = __builtin_amdgcn_readfirstlane(sExt[4 * w]);
    be[w].pmin = __builtin_amdgcn_readfirstlane(sExt[4 * w + 1]);
    be[w].lo = __builtin_amdgcn_readfirstlane(sExt[4 * w + 2]);
    be[w].hi = __builtin_amdgcn_readfirstlane(sExt[4 * w + 3]);
  }
  sm_ext_uniform(we);

  const int nt = (Lk + kSmKeys - 1) / kSmKeys;
  auto next_tile = [&](int t) { SM_NEXT_TILE(skip, t, nt, be); return t; };

  sm_u32x4 qf[D / 16];
  {
    const uint16_t* qp = a.q + (int64_t)b * a.q_sb + (qrow0 + i) * a.q_ss + (int64_t)hq * a.q_sh + 8 * h;
#pragma unroll
    for (int s = 0; s < D / 16; ++s) {
      sm_u32x4 z = {0u, 0u, 0u, 0u};
      qf[s] = valid ? *reinterpret_cast<const sm_u32x4*>(qp + 16 * s) : z;
    }
  }

  sm_f32x16 o[D / 32];
#pragma unroll
  for (int ii = 0; ii < D / 32; ++ii)
#pragma unroll
    for (int j = 0; j < 16; ++j) o[ii][j] = 0.f;
  float m = -INFINITY, lsum = 0.f;

  const uint16_t* kb = a.k + (int64_t)b * a.k_sb + (int64_t)hk * a.k_sh + krow0 * a.k_ss;
  const uint16_t* vb = a.v + (int64_t)b * a.v_sb + (int64_t)hk * a.v_sh + krow0 * a.v_ss;

  // Register staging, one tile ahead (SmTile::load_tile / store_tile, written out): keys at or past Lk enter LDS as zeros.
  constexpr int NK = kSmKeys * CH / 256, NV = 32 * CH / 256;
  sm_u32x4 kreg[NK], vreg[NV][2];
  auto load_tile = [&](int t) {
    const int nv = Lk - t * kSmKeys;
#pragma unroll
    for (int ii = 0; ii < NK; ++ii) {
      const int u = tid + 256 * ii, key = u / CH, c = u % CH;
      sm_u32x4 val = {0u, 0u, 0u, 0u};
      if (key < nv) val = *reinterpret_cast<const sm_u32x4*>(kb + (int64_t)(t * kSmKeys + key) * a.k_ss + 8 * c);
      kreg[ii] = val;
    }
#pragma unroll
    for (int ii = 0; ii < NV; ++ii) {
      const int u = tid + 256 * ii, p = u & 31, c = u >> 5;
      sm_u32x4 va = {0u, 0u, 0u, 0u}, vc = {0u, 0u, 0u, 0u};
      if (2 * p < nv) va = *reinterpret_cast<const sm_u32x4*>(vb + (int64_t)(t * kSmKeys + 2 * p) * a.v_ss + 8 * c);
      if (2 * p + 1 < nv) vc = *reinterpret_cast<const sm_u32x4*>(vb + (int64_t)(t * kSmKeys + 2 * p + 1) * a.v_ss + 8 * c);
      vreg[ii][0] = va; vreg[ii][1] = vc;
    }
  };

  int t = next_tile(0);
  if (t < nt) load_tile(t);
  while (t < nt) {
    const int n0 = t * kSmKeys, n1 = n0 + kSmKeys;
    __syncthreads();
#pragma unroll
    for (int ii = 0; ii < NK; ++ii) {
      const int u = tid + 256 * ii, key = u / CH, c = u % CH;
      *reinterpret_cast<sm_u32x4*>(sK + key * KS + 8 * c) = kreg[ii];
    }
#pragma unroll
    for (int ii = 0; ii < NV; ++ii) {   // V transposed: 8 dwords [d][2p, 2p + 1] per chunk pair
      const int u = tid + 256 * ii, p = u & 31, c = u >> 5;
      const sm_u32x4 va = vreg[ii][0], vc = vreg[ii][1];
      uint32_t* dst = reinterpret_cast<uint32_t*>(sV + (8 * c) * VS + 2 * p);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        dst[(2 * e) * (VS / 2)] = (va[e] & 0xffffu) | (vc[e] << 16);
        dst[(2 * e + 1) * (VS / 2)] = (va[e] >> 16) | (vc[e] & 0xffff0000u);
      }
    }
    __syncthreads();
    const int tn = next_tile(t + 1);
    if (tn < nt) load_tile(tn);

    if (!skip || sm_hits(we, n0, n1)) {   // (wave-uniform; no barrier inside)
      float p[32];
      T::scores(sK, qf, a.scale_log2, r, h, p);
      if (!skip || n1 > we.pmin) {   // some row of the wave does not see the whole tile through its prefix
        uint32_t ok = 0;
        SM_MASK_BITS(MK, ok, skip, we, n0, n1, h, valid, pre, Lk, frow, a.f_sp, a.n_func);
#pragma unroll
        for (int j = 0; j < 32; ++j) p[j] = ((ok >> j) & 1u) ? p[j] : -INFINITY;
      }
      float mx = p[0];
#pragma unroll
      for (int j = 1; j < 32; ++j) mx = fmaxf(mx, p[j]);
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float m_new = fmaxf(m, mx);
      const float m_use = m_new == -INFINITY ? 0.f : m_new;   // a row that has seen no key yet: P = exp2(-inf - 0) = 0, not NaN
      const float alpha = __builtin_amdgcn_exp2f(m - m_use);
      m = m_new;
      float ts = 0.f;
#pragma unroll
      for (int j = 0; j < 32; ++j) { p[j] = __builtin_amdgcn_exp2f(p[j] - m_use); ts += p[j]; }
      lsum = lsum * alpha + ts;
#pragma unroll
      for (int ii = 0; ii < D / 32; ++ii)
#pragma unroll
        for (int j = 0; j < 16; ++j) o[ii][j] *= alpha;

      // O^T += V^T P^T
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {   // k-step: sub-block ks >> 1, step ks & 1: registers 8 ks .. 8 ks + 7 of p
        sm_u32x4 pf;
#pragma unroll
        for (int e = 0; e < 4; ++e) pf[e] = M::pack2(p[8 * ks + 2 * e], p[8 * ks + 2 * e + 1]);
#pragma unroll
        for (int ii = 0; ii < D / 32; ++ii) {
          const uint16_t* vp = sV + (32 * ii + r) * VS + 16 * ks + 4 * h;
          const sm_u32x2 lo = *reinterpret_cast<const sm_u32x2*>(vp);
          const sm_u32x2 hi = *reinterpret_cast<const sm_u32x2*>(vp + 8);
          const sm_u32x4 vf = {lo[0], lo[1], hi[0], hi[1]};
          o[ii] = M::mma(vf, pf, o[ii]);
        }
      }
    }
    t = tn;
  }

  const float l = lsum + __shfl_xor(lsum, 32, 64);
  const float inv = l > 0.f ? 1.0f / l : 0.f;   // a row with no visible key: out = 0, lse = -inf
  if (valid) {
    const int64_t orow = (a.cu_q ? qrow0 : (int64_t)b * a.Sq) + i;
    uint16_t* op = a.out + (orow * a.Hq + hq) * D + 4 * h;
    SM_STORE_ROW(M, D, op, o, inv);
    if (h == 0) {
      const int64_t li = a.cu_q ? (int64_t)hq * a.total_q + qrow0 + i : ((int64_t)b * a.Hq + hq) * a.Sq + i;
      a.lse[li] = l > 0.f ? (m + __builtin_amdgcn_logf(l)) * kSmLn2 : -INFINITY;   // v_log_f32 is log2
    }
  }
}

template <int DT, int D>
static void pf_launch(int mask, dim3 grid, hipStream_t stream, const PrefillArgs& c) {
  const dim3 block(256);
  if (mask == kSmMaskNone) hipLaunchKernelGGL((prefill_attn_kernel<DT, D, kSmMaskNone>), grid, block, 0, stream, c);
  else if (mask == kSmMaskCausal) hipLaunchKernelGGL((prefill_attn_kernel<DT, D, kSmMaskCausal>), grid, block, 0, stream, c);
  else hipLaunchKernelGGL((prefill_attn_kernel<DT, D, kSmMaskFunc>), grid, block, 0, stream, c);
}

}  // namespace mi355

using namespace mi355;

int mi355_prefill_attn(const void* q, int64_t q_stride_b, int64_t q_stride_s, int64_t q_stride_h, const void* k,
                       int64_t k_stride_b, int64_t k_stride_s, int64_t k_stride_h, const void* v, int64_t v_stride_b,
                       int64_t v_stride_s, int64_t v_stride_h, const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k,
                       int64_t B, int64_t Sq, int64_t Sk, int64_t total_q, int64_t total_k, int64_t Hq, int64_t Hkv, int64_t D,
                       int mask, const int32_t* func, int64_t n_func, int64_t func_heads, int64_t func_stride_b,
                       int64_t func_stride_h, int64_t func_stride_f, int64_t func_stride_s, float softmax_scale,
                       int skip_tiles, void* out, float* lse, int dtype, hipStream_t stream) {
  SM_ATTN_CHECK_COMMON("prefill_attn", kSmKeys, INT32_MAX, "n_func does not fit 31 bits");
  const int64_t rows = jagged ? total_q : B * Sq;
  if (B == 0 || rows == 0 || Sq == 0) return MI355_OK;
  MI355_CHECK_ARG(q && out && lse, "prefill_attn: null pointer");
  MI355_CHECK_ARG(sm_aligned(q, q_stride_b, q_stride_s, q_stride_h) && (uintptr_t)out % 16 == 0,
                  "prefill_attn: q and out need 16-byte aligned rows (base aligned, strides multiples of 8 elements)");
  if (jagged ? total_k > 0 : Sk > 0) {
    MI355_CHECK_ARG(k && v, "prefill_attn: null k / v pointer");
    MI355_CHECK_ARG(sm_aligned(k, k_stride_b, k_stride_s, k_stride_h) && sm_aligned(v, v_stride_b, v_stride_s, v_stride_h),
                    "prefill_attn: k / v rows need 16-byte alignment (base aligned, strides multiples of 8 elements)");
  }
  if (mask == kSmMaskFunc) MI355_CHECK_ARG(func && (uintptr_t)func % 4 == 0, "prefill_attn: func is null or misaligned");
  const int64_t nqt = ceil_div(Sq, (int64_t)kSmRows);   // jagged: Sq is max_seqlen_q
  const int64_t nblocks = nqt * B * Hq;
  MI355_CHECK_ARG(nblocks <= INT32_MAX, "prefill_attn: launch too large");

  PrefillArgs c;
  SM_ATTN_FILL_COMMON(c);
  c.out = (uint16_t*)out; c.lse = lse; c.nqt = (int)nqt;
  const dim3 grid((unsigned)nblocks);
  if (dtype == kBF16) {
    if (D == 64) pf_launch<kBF16, 64>(mask, grid, stream, c);
    else pf_launch<kBF16, 128>(mask, grid, stream, c);
  } else {
    if (D == 64) pf_launch<kF16, 64>(mask, grid, stream, c);
    else pf_launch<kF16, 128>(mask, grid, stream, c);
  }
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}
