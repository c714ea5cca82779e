// Beam-search decode attention of the semantic-ID generative-retrieval family: softmax attention of the W beams of a sample
// over its shared context KV, plus each beam's own top-k gather from the beam KV, merged by log-sum-exp.
//
// Replaces (reference): corelib/gr_decode_atten -- interface.py (BeamDecodeAttn: context attention, sparse beam attention,
// combine), which is CuTe DSL for SM80-SM120 only.  Written for gfx950 from the semantics of tests/reference.py there.
//
// Two launches per call, no float atomics, bitwise reproducible for a given split count:
//
// 1. beam_ctx_kernel: flash-decoding on the shared key-tile core of softmax_tile_dev.h (LDS layout, register-to-key mapping,
//    online softmax and P V are described there).  One workgroup (4 waves) owns one (batch, kv head, tile of 128 packed query
//    rows, KV split).  The packed row of beam w and group head g is w G + g, so the K / V tile of a kv head serves all W G
//    rows of its group.  A split is a range of the sample's OWN key tiles (seqused_k and jagged contexts included), tiles
//    [s nt / ns, (s + 1) nt / ns); a split with no tile writes lse = -inf and nothing else.  Every split writes a normalised
//    fp32 partial O and its LSE (log2 units).  Only the last tile of a sequence is masked (key >= nvalid), and key 0 of every
//    tile exists, so the running max is always finite.
//
// 2. beam_merge_kernel: 16 lanes per row (b, w, h).  Gathers the decode_nums beam rows through the index list, scores and
//    softmax in fp32 on the vector ALU (online), then folds in the ns context partials by log-sum-exp and writes `out` in
//    the dtype of q and `lse` in fp32.  An index outside [0, decode_nums W) is never dereferenced: that key is absent.
#include "common.h"
#include "softmax_mask_dev.h"
#include "../../include/recsys_amd.h"

#include <math.h>

namespace mi355 {

struct BeamCtxArgs {
  const uint16_t* q;
  const uint16_t* k;
  const uint16_t* v;
  const int32_t* seqused;   // [B] or null
  const int32_t* cu;        // [B + 1] or null (jagged)
  float* o_part;            // [ns][rows][D]
  float* lse_part;          // [ns][rows], log2 units
  int64_t q_sb, q_sw, q_sh;
  int64_t k_sb, k_ss, k_sh, v_sb, v_ss, v_sh;
  int64_t total_k, rows;
  int B, W, Hq, Hkv, G, Sk, ns, nqt;
  float scale_log2;
};

template <int DT, int D>
__global__ void __launch_bounds__(256) beam_ctx_kernel(BeamCtxArgs a) {
  using T = SmTile<DT, D>;
  __shared__ __attribute__((aligned(16))) uint16_t sK[T::kSK];
  __shared__ __attribute__((aligned(16))) uint16_t sV[T::kSV];

  const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, h = lane >> 5;
  int64_t id = blockIdx.x;
  const int qt = (int)(id % a.nqt); id /= a.nqt;
  const int sp = (int)(id % a.ns); id /= a.ns;
  const int hk = (int)(id % a.Hkv);
  const int b = (int)(id / a.Hkv);

  int64_t row0 = 0;
  int len = a.Sk;
  if (a.cu) {
    SM_SEQ_BOUNDS(a.cu, b, a.total_k, row0, len);
  } else if (a.seqused) {
    const int u = a.seqused[b];
    len = u < 0 ? 0 : (u < a.Sk ? u : a.Sk);
  }
  const int nt = (len + kSmKeys - 1) / kSmKeys;
  const int t0 = (int)((int64_t)sp * nt / a.ns), t1 = (int)((int64_t)(sp + 1) * nt / a.ns);

  const int rr = qt * kSmRows + wv * 32 + r;       // packed row of this lane
  const bool valid = rr < a.W * a.G;
  const int w = valid ? rr / a.G : 0, hq = hk * a.G + (valid ? rr % a.G : 0);
  const int64_t prow = ((int64_t)b * a.W + w) * a.Hq + hq;

  if (t0 >= t1) {   // (block-uniform: no barrier has been passed)
    if (valid && h == 0) a.lse_part[(int64_t)sp * a.rows + prow] = -INFINITY;
    return;
  }

  sm_u32x4 qf[D / 16];
  T::load_q(a.q + (int64_t)b * a.q_sb + (int64_t)w * a.q_sw + (int64_t)hq * a.q_sh + 8 * h, valid, qf);
  sm_f32x16 o[D / 32];
  T::zero_acc(o);
  float m = -INFINITY, lsum = 0.f;

  const uint16_t* kb = a.k + (int64_t)b * a.k_sb + (int64_t)hk * a.k_sh + row0 * a.k_ss;
  const uint16_t* vb = a.v + (int64_t)b * a.v_sb + (int64_t)hk * a.v_sh + row0 * a.v_ss;

  // Register staging, one tile ahead: the global loads of tile t + 1 are issued before the MFMAs of tile t and written to
  // LDS after them, so that their latency lies under the compute of a workgroup that has its CU to itself.
  typename T::Stage st;
  auto load_tile = [&](int t) { T::load_tile(st, kb, vb, a.k_ss, a.v_ss, t, len, tid); };   // (only shortens the two calls)
  load_tile(t0);

  for (int t = t0; t < t1; ++t) {
    const int nvalid = len - t * kSmKeys;   // >= 1
    __syncthreads();
    T::store_tile(st, sK, sV, tid);
    __syncthreads();
    if (t + 1 < t1) load_tile(t + 1);

    float p[32];
    T::scores(sK, qf, a.scale_log2, r, h, p);
    if (nvalid < kSmKeys) {
#pragma unroll
      for (int j = 0; j < 32; ++j)
        if (sm_key_of(j, h) >= nvalid) p[j] = -INFINITY;
    }
    const float alpha = T::template softmax_step<false>(p, m, lsum);   // m stays finite: key 0 of a tile always exists
#pragma unroll
    for (int i = 0; i < D / 32; ++i) o[i] *= alpha;
    T::pv(sV, r, h, p, o);
  }

  const float l = lsum + __shfl_xor(lsum, 32, 64);
  const float inv = 1.0f / l;
  if (valid) {
    float* op = a.o_part + ((int64_t)sp * a.rows + prow) * D + 4 * h;
#pragma unroll
    for (int i = 0; i < D / 32; ++i)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        float4 x;
        x.x = o[i][4 * g] * inv; x.y = o[i][4 * g + 1] * inv; x.z = o[i][4 * g + 2] * inv; x.w = o[i][4 * g + 3] * inv;
        *reinterpret_cast<float4*>(op + 32 * i + 8 * g) = x;
      }
    if (h == 0) a.lse_part[(int64_t)sp * a.rows + prow] = m + __builtin_amdgcn_logf(l);   // v_log_f32 is log2
  }
}

struct BeamMergeArgs {
  const uint16_t* q;
  const uint16_t* kbeam;
  const uint16_t* vbeam;
  const void* topk;
  const float* o_part;
  const float* lse_part;
  uint16_t* out;
  float* lse;
  int64_t q_sb, q_sw, q_sh;
  int64_t kb_sb, kb_ss, kb_sh, vb_sb, vb_ss, vb_sh;
  int64_t tk_sb, tk_sh, tk_sn, tk_sw;
  int64_t rows;
  int W, Hq, G, dn, ns;
  float scale_log2;
};

template <int DT, int E>
__device__ __forceinline__ void bd_load(const uint16_t* p, float (&x)[E]) {
#pragma unroll
  for (int i = 0; i < E / 4; ++i) {
    const float4 f = ld4<DT>(p, 4 * i);
    x[4 * i] = f.x; x[4 * i + 1] = f.y; x[4 * i + 2] = f.z; x[4 * i + 3] = f.w;
  }
}

template <int DT, int D, typename IT>
__global__ void __launch_bounds__(256) beam_merge_kernel(BeamMergeArgs a) {
  constexpr int E = D / 16;   // elements of a row per lane
  const int sub = (int)threadIdx.x & 15;
  const int64_t row = (int64_t)blockIdx.x * 16 + ((int)threadIdx.x >> 4);
  if (row >= a.rows) return;   // (a whole 16-lane group leaves together; the exchanges below stay inside a group)
  const int hq = (int)(row % a.Hq), w = (int)((row / a.Hq) % a.W);
  const int64_t b = row / ((int64_t)a.Hq * a.W);
  const int hk = hq / a.G;

  float qf[E], acc[E];
  bd_load<DT, E>(a.q + b * a.q_sb + (int64_t)w * a.q_sw + (int64_t)hq * a.q_sh + sub * E, qf);
#pragma unroll
  for (int i = 0; i < E; ++i) acc[i] = 0.f;
  float m = -INFINITY, l = 0.f;

  const IT* tk = reinterpret_cast<const IT*>(a.topk) + b * a.tk_sb + (int64_t)(hk * a.G) * a.tk_sh + (int64_t)w * a.tk_sw;
  const uint64_t nbeam = (uint64_t)a.dn * (uint64_t)a.W;
  for (int n = 0; n < a.dn; ++n) {
    const int64_t idx = (int64_t)tk[(int64_t)n * a.tk_sn];
    if ((uint64_t)idx >= nbeam) continue;   // (negative indices wrap above the bound): the key is absent
    float kf[E], vf[E];
    bd_load<DT, E>(a.kbeam + b * a.kb_sb + idx * a.kb_ss + (int64_t)hk * a.kb_sh + sub * E, kf);
    bd_load<DT, E>(a.vbeam + b * a.vb_sb + idx * a.vb_ss + (int64_t)hk * a.vb_sh + sub * E, vf);
    float d = 0.f;
#pragma unroll
    for (int i = 0; i < E; ++i) d = fmaf(qf[i], kf[i], d);
    d += __shfl_xor(d, 8, 64); d += __shfl_xor(d, 4, 64); d += __shfl_xor(d, 2, 64); d += __shfl_xor(d, 1, 64);
    const float s2 = d * a.scale_log2;
    const float m_new = fmaxf(m, s2);
    const float alpha = __builtin_amdgcn_exp2f(m - m_new), e = __builtin_amdgcn_exp2f(s2 - m_new);
    m = m_new;
    l = l * alpha + e;
#pragma unroll
    for (int i = 0; i < E; ++i) acc[i] = fmaf(e, vf[i], acc[i] * alpha);
  }
  // the context partials: weight 2^lse_s on a normalised O_s
  for (int s = 0; s < a.ns; ++s) {
    const float ls = a.lse_part[(int64_t)s * a.rows + row];
    if (ls == -INFINITY) continue;   // an empty split wrote no O
    const float* op = a.o_part + ((int64_t)s * a.rows + row) * D + sub * E;
    float of[E];
#pragma unroll
    for (int i = 0; i < E / 4; ++i) {
      const float4 f = *reinterpret_cast<const float4*>(op + 4 * i);
      of[4 * i] = f.x; of[4 * i + 1] = f.y; of[4 * i + 2] = f.z; of[4 * i + 3] = f.w;
    }
    const float m_new = fmaxf(m, ls);
    const float alpha = __builtin_amdgcn_exp2f(m - m_new), e = __builtin_amdgcn_exp2f(ls - m_new);
    m = m_new;
    l = l * alpha + e;
#pragma unroll
    for (int i = 0; i < E; ++i) acc[i] = fmaf(e, of[i], acc[i] * alpha);
  }
  const float inv = l > 0.f ? 1.0f / l : 0.f;   // a row with no key at all: out = 0, lse = -inf
  uint16_t* outp = a.out + row * D + sub * E;
#pragma unroll
  for (int i = 0; i < E / 4; ++i) {
    float4 f;
    f.x = acc[4 * i] * inv; f.y = acc[4 * i + 1] * inv; f.z = acc[4 * i + 2] * inv; f.w = acc[4 * i + 3] * inv;
    st4<DT>(outp, 4 * i, f);
  }
  if (sub == 0) a.lse[row] = l > 0.f ? (m + __builtin_amdgcn_logf(l)) * kSmLn2 : -INFINITY;
}

}  // namespace mi355

using namespace mi355;

int64_t mi355_beam_decode_workspace_bytes(int64_t B, int64_t W, int64_t Hq, int64_t D, int64_t num_splits) {
  if (B < 0 || W < 0 || Hq < 0 || D < 0 || num_splits < 1) return 0;
  const int64_t rows = B * W * Hq;
  return ((num_splits * rows * (D + 1) * 4 + 15) / 16) * 16;
}

int mi355_beam_decode_attn(const void* q, int64_t q_stride_b, int64_t q_stride_w, int64_t q_stride_h, const void* k_context,
                           const void* v_context, int64_t kc_stride_b, int64_t kc_stride_s, int64_t kc_stride_h,
                           int64_t vc_stride_b, int64_t vc_stride_s, int64_t vc_stride_h, int64_t Sk, int64_t total_k,
                           const int32_t* seqused_k, const int32_t* cu_seqlens_k, const void* k_beam, const void* v_beam,
                           int64_t kb_stride_b, int64_t kb_stride_s, int64_t kb_stride_h, int64_t vb_stride_b,
                           int64_t vb_stride_s, int64_t vb_stride_h, const void* topk_indices, int topk_itype,
                           int64_t tk_stride_b, int64_t tk_stride_h, int64_t tk_stride_n, int64_t tk_stride_w, int64_t B,
                           int64_t W, int64_t Hq, int64_t Hkv, int64_t D, int64_t decode_nums, float softmax_scale,
                           int64_t num_splits, void* out, float* lse, int dtype, void* workspace, int64_t workspace_bytes,
                           hipStream_t stream) {
  MI355_CHECK_ARG(dtype == kBF16 || dtype == kF16, "beam_decode_attn: dtype must be bf16 or fp16");
  MI355_CHECK_ARG(D == 64 || D == 128, "beam_decode_attn: head dim must be 64 or 128");
  MI355_CHECK_ARG(B >= 0 && W >= 0 && Hq > 0 && Hkv > 0 && Hq % Hkv == 0, "beam_decode_attn: Hq must be a multiple of Hkv");
  MI355_CHECK_ARG(decode_nums >= 0 && Sk >= 0 && total_k >= 0, "beam_decode_attn: negative length");
  MI355_CHECK_ARG(!(seqused_k && cu_seqlens_k), "beam_decode_attn: seqused_k and cu_seqlens_k are mutually exclusive");
  MI355_CHECK_ARG(topk_itype == 0 || topk_itype == 1, "beam_decode_attn: topk_itype must be 0 (int32) or 1 (int64)");
  MI355_CHECK_ARG(num_splits >= 1 && num_splits <= 65535, "beam_decode_attn: num_splits must be in [1, 65535]");
  const int64_t rows = B * W * Hq;
  if (rows == 0) return MI355_OK;
  const int64_t G = Hq / Hkv;
  MI355_CHECK_ARG(B <= INT32_MAX && W * G <= INT32_MAX - kSmRows && Sk <= INT32_MAX - kSmKeys && Hq <= INT32_MAX &&
                      decode_nums <= INT32_MAX, "beam_decode_attn: a dimension does not fit 31 bits");
  MI355_CHECK_ARG(q && out && lse, "beam_decode_attn: null pointer");
  MI355_CHECK_ARG(sm_aligned(q, q_stride_b, q_stride_w, q_stride_h) && (uintptr_t)out % 16 == 0,
                  "beam_decode_attn: q and out need 16-byte aligned rows");
  const bool has_ctx = cu_seqlens_k ? total_k > 0 : Sk > 0;
  if (has_ctx) {
    MI355_CHECK_ARG(k_context && v_context, "beam_decode_attn: null context pointer");
    MI355_CHECK_ARG(sm_aligned(k_context, kc_stride_b, kc_stride_s, kc_stride_h) &&
                        sm_aligned(v_context, vc_stride_b, vc_stride_s, vc_stride_h),
                    "beam_decode_attn: context rows need 16-byte alignment (strides multiples of 8 elements)");
  }
  if (decode_nums > 0) {
    MI355_CHECK_ARG(k_beam && v_beam && topk_indices, "beam_decode_attn: null beam pointer");
    MI355_CHECK_ARG(sm_aligned(k_beam, kb_stride_b, kb_stride_s, kb_stride_h) &&
                        sm_aligned(v_beam, vb_stride_b, vb_stride_s, vb_stride_h),
                    "beam_decode_attn: beam rows need 16-byte alignment (strides multiples of 8 elements)");
  }
  MI355_CHECK_ARG(workspace && (uintptr_t)workspace % 16 == 0 &&
                      workspace_bytes >= mi355_beam_decode_workspace_bytes(B, W, Hq, D, num_splits),
                  "beam_decode_attn: workspace missing, misaligned or too small");
  const int64_t nqt = ceil_div(W * G, (int64_t)kSmRows);
  const int64_t nblocks = nqt * num_splits * Hkv * B;
  MI355_CHECK_ARG(nblocks <= INT32_MAX && ceil_div(rows, (int64_t)16) <= INT32_MAX, "beam_decode_attn: launch too large");

  float* o_part = reinterpret_cast<float*>(workspace);
  float* lse_part = o_part + num_splits * rows * D;
  const float scale_log2 = softmax_scale * kSmLog2e;

  BeamCtxArgs c;
  c.q = (const uint16_t*)q; c.k = (const uint16_t*)k_context; c.v = (const uint16_t*)v_context;
  c.seqused = seqused_k; c.cu = cu_seqlens_k; c.o_part = o_part; c.lse_part = lse_part;
  c.q_sb = q_stride_b; c.q_sw = q_stride_w; c.q_sh = q_stride_h;
  c.k_sb = cu_seqlens_k ? 0 : kc_stride_b; c.k_ss = kc_stride_s; c.k_sh = kc_stride_h;
  c.v_sb = cu_seqlens_k ? 0 : vc_stride_b; c.v_ss = vc_stride_s; c.v_sh = vc_stride_h;
  c.total_k = total_k; c.rows = rows;
  c.B = (int)B; c.W = (int)W; c.Hq = (int)Hq; c.Hkv = (int)Hkv; c.G = (int)G; c.Sk = cu_seqlens_k ? 0 : (int)Sk;
  c.ns = (int)num_splits; c.nqt = (int)nqt; c.scale_log2 = scale_log2;
  {
    const dim3 grid((unsigned)nblocks), block(256);
    if (dtype == kBF16) {
      if (D == 64) hipLaunchKernelGGL((beam_ctx_kernel<kBF16, 64>), grid, block, 0, stream, c);
      else hipLaunchKernelGGL((beam_ctx_kernel<kBF16, 128>), grid, block, 0, stream, c);
    } else {
      if (D == 64) hipLaunchKernelGGL((beam_ctx_kernel<kF16, 64>), grid, block, 0, stream, c);
      else hipLaunchKernelGGL((beam_ctx_kernel<kF16, 128>), grid, block, 0, stream, c);
    }
    MI355_LAUNCH_CHECK();
  }

  BeamMergeArgs g;
  g.q = (const uint16_t*)q; g.kbeam = (const uint16_t*)k_beam; g.vbeam = (const uint16_t*)v_beam; g.topk = topk_indices;
  g.o_part = o_part; g.lse_part = lse_part; g.out = (uint16_t*)out; g.lse = lse;
  g.q_sb = q_stride_b; g.q_sw = q_stride_w; g.q_sh = q_stride_h;
  g.kb_sb = kb_stride_b; g.kb_ss = kb_stride_s; g.kb_sh = kb_stride_h;
  g.vb_sb = vb_stride_b; g.vb_ss = vb_stride_s; g.vb_sh = vb_stride_h;
  g.tk_sb = tk_stride_b; g.tk_sh = tk_stride_h; g.tk_sn = tk_stride_n; g.tk_sw = tk_stride_w;
  g.rows = rows; g.W = (int)W; g.Hq = (int)Hq; g.G = (int)G; g.dn = (int)decode_nums; g.ns = (int)num_splits;
  g.scale_log2 = scale_log2;
  {
    const dim3 grid((unsigned)ceil_div(rows, (int64_t)16)), block(256);
#define BD_MERGE(DT_, D_)                                                                              \
  do {                                                                                                 \
    if (topk_itype == 0) hipLaunchKernelGGL((beam_merge_kernel<DT_, D_, int32_t>), grid, block, 0, stream, g); \
    else hipLaunchKernelGGL((beam_merge_kernel<DT_, D_, int64_t>), grid, block, 0, stream, g);         \
  } while (0)
    if (dtype == kBF16) { if (D == 64) BD_MERGE(kBF16, 64); else BD_MERGE(kBF16, 128); }
    else { if (D == 64) BD_MERGE(kF16, 64); else BD_MERGE(kF16, 128); }
#undef BD_MERGE
    MI355_LAUNCH_CHECK();
  }
  return MI355_OK;
}
