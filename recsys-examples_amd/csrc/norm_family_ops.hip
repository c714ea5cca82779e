// HSTU swish layer norm and RMS norm over rows [N, D], forward and backward.
//
// Replaces (reference, examples/hstu/ops/triton_ops/triton_layer_norm.py): SwishLayerNormFunction (:763-877, the IS_SWISH
// branches of _weighted_layer_norm_fwd and _weighted_layer_norm_bwd_dx, :229-253) and RMSNormFunction with
// _weighted_rms_norm_fwd / _weighted_rms_norm_bwd_dx / _rms_norm_bwd_dwdb (:537-760).  Written for wave64 from the arithmetic.
//
// Values (all arithmetic fp32, every stored value rounded once):
//   swish:  mean, rstd, xh, ln = fmaf(xh, w, b) as in norm_ops.hip;  s = 1 / (1 + expf(-ln)) (act_ops.hip's sigmoid);  y = s * x
//           backward: q = ((dy * x) * s) * (1 - s);  g = w * q;  c1 = sum(xh * g) / D;  c2 = sum(g) / D;
//           dx = (g - (xh * c1 + c2)) * rstd + dy * s;  dw = sum over rows of q * xh;  db = sum over rows of q
//   rms:    rstd = 1 / sqrtf(sum(x^2) / D + eps);  xh = x * rstd;  y = xh * w
//           backward: g = w * dy;  c1 = sum(xh * g) / D;  dx = (g - xh * c1) * rstd;  dw = sum over rows of dy * xh
//
// Layout of a call, the kernels (hstu_norm_fwd_kernel / hstu_norm_bwd_kernel, kinds kNormSwish and kNormRms here), the grid size,
// the dispatch ladder and the dw / db fold: norm_dev.h, shared with norm_ops.hip.  This file holds the argument checks and the
// argument blocks of the four entry points.
#include "norm_dev.h"
#include "../../include/recsys_amd.h"

using namespace mi355;

template <int KIND>
static int fam_fwd(const void* x, int64_t x_stride, int64_t rows, int64_t D, int dtype, const void* weight,
                   const void* bias, int weight_dtype, float eps, void* y, int64_t y_stride, float* mean, float* rstd,
                   hipStream_t stream) {
  const int eb = elem_bytes(dtype);
  NormVec nv{D % (16 / eb) == 0 ? 16 / eb : 1};
  nv.need(x, x_stride * eb); nv.need(y, y_stride * eb); nv.need(weight, 0); nv.need(bias, 0);
  NormArgs a{};
  a.x = (uintptr_t)x; a.y = (uintptr_t)y; a.w = (uintptr_t)weight; a.b = (uintptr_t)bias;
  a.x_stride = x_stride * eb; a.y_stride = y_stride * eb;
  a.mean = mean; a.rstd = rstd; a.N = rows; a.D = (int)D; a.eps = eps; a.w_f32 = weight_dtype == kF32;
  norm_launch<KIND, false>(dtype, nv.v, norm_row_blocks(rows, D, false), a, stream);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

template <int KIND>
static int fam_bwd(const void* dy, int64_t dy_stride, const void* x, int64_t x_stride, int64_t rows, int64_t D, int dtype,
                   const void* weight, const void* bias, int weight_dtype, const float* mean, const float* rstd, void* dx,
                   int64_t dx_stride, void* dweight, void* dbias, void* workspace, hipStream_t stream) {
  const int eb = elem_bytes(dtype);
  NormVec nv{D % (16 / eb) == 0 ? 16 / eb : 1};
  nv.need(dy, dy_stride * eb); nv.need(x, x_stride * eb); nv.need(dx, dx_stride * eb); nv.need(weight, 0); nv.need(bias, 0);
  NormArgs a{};
  a.dy = (uintptr_t)dy; a.x = (uintptr_t)x; a.dx = (uintptr_t)dx; a.w = (uintptr_t)weight; a.b = (uintptr_t)bias;
  a.dy_stride = dy_stride * eb; a.x_stride = x_stride * eb; a.dx_stride = dx_stride * eb;
  a.mean = const_cast<float*>(mean); a.rstd = const_cast<float*>(rstd); a.partial = (float*)workspace;
  a.N = rows; a.D = (int)D; a.w_f32 = weight_dtype == kF32;
  const int grid = norm_row_blocks(rows, D, true);
  if (rows > 0) {
    norm_launch<KIND, true>(dtype, nv.v, grid, a, stream);
    MI355_LAUNCH_CHECK();
  }
  return norm_launch_dwdb(a.partial, rows > 0 ? grid : 0, a.D, weight_dtype, dweight, dbias, stream);
}

extern "C" int mi355_hstu_swish_layer_norm_fwd(const void* x, int64_t x_stride, int64_t rows, int64_t D, int dtype,
                                               const void* weight, const void* bias, int weight_dtype, float eps, void* y,
                                               int64_t y_stride, float* mean, float* rstd, hipStream_t stream) {
  NORM_CHECK_COMMON("hstu_swish_layer_norm_fwd", rows, D, dtype, weight_dtype, "weights are");
  MI355_CHECK_ARG(x_stride >= D && y_stride >= D, "hstu_swish_layer_norm_fwd: a row stride is smaller than D");
  if (rows == 0) return MI355_OK;
  MI355_CHECK_ARG(x && y && weight && bias && mean && rstd, "hstu_swish_layer_norm_fwd: null buffer with rows > 0");
  const int eb = elem_bytes(dtype), web = elem_bytes(weight_dtype);
  MI355_CHECK_ARG(norm_aligned(x, eb) && norm_aligned(y, eb) && norm_aligned(weight, web) && norm_aligned(bias, web),
                  "hstu_swish_layer_norm_fwd: a base pointer is not aligned to the element size");
  return fam_fwd<kNormSwish>(x, x_stride, rows, D, dtype, weight, bias, weight_dtype, eps, y, y_stride, mean, rstd, stream);
}

extern "C" int64_t mi355_hstu_swish_layer_norm_bwd_workspace_bytes(int64_t rows, int64_t D) {
  if (rows < 0 || D <= 0 || D > kNormMaxD) return 0;
  return (int64_t)2 * norm_row_blocks(rows, D, true) * D * 4;
}
extern "C" int64_t mi355_hstu_rms_norm_bwd_workspace_bytes(int64_t rows, int64_t D) {
  if (rows < 0 || D <= 0 || D > kNormMaxD) return 0;
  return (int64_t)norm_row_blocks(rows, D, true) * D * 4;
}

extern "C" int mi355_hstu_swish_layer_norm_bwd(const void* dy, int64_t dy_stride, const void* x, int64_t x_stride, int64_t rows,
                                               int64_t D, int dtype, const void* weight, const void* bias, int weight_dtype,
                                               const float* mean, const float* rstd, void* dx, int64_t dx_stride, void* dweight,
                                               void* dbias, void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  NORM_CHECK_COMMON("hstu_swish_layer_norm_bwd", rows, D, dtype, weight_dtype, "weights are");
  MI355_CHECK_ARG(dy_stride >= D && x_stride >= D && dx_stride >= D, "hstu_swish_layer_norm_bwd: a row stride is smaller than D");
  MI355_CHECK_ARG(dweight && dbias && (rows == 0 || (dy && x && dx && weight && bias && mean && rstd)),
                  "hstu_swish_layer_norm_bwd: null buffer (dweight and dbias are needed for rows == 0 too)");
  MI355_CHECK_ARG(rows == 0 || (workspace && ((uintptr_t)workspace & 15) == 0 &&
                                workspace_bytes >= mi355_hstu_swish_layer_norm_bwd_workspace_bytes(rows, D)),
                  "hstu_swish_layer_norm_bwd: workspace is null, not 16-byte aligned or too small");
  const int eb = elem_bytes(dtype), web = elem_bytes(weight_dtype);
  MI355_CHECK_ARG(norm_aligned(dy, eb) && norm_aligned(x, eb) && norm_aligned(dx, eb) && norm_aligned(weight, web) &&
                      norm_aligned(bias, web) && norm_aligned(dweight, web) && norm_aligned(dbias, web),
                  "hstu_swish_layer_norm_bwd: a base pointer is not aligned to the element size");
  return fam_bwd<kNormSwish>(dy, dy_stride, x, x_stride, rows, D, dtype, weight, bias, weight_dtype, mean, rstd, dx, dx_stride,
                        dweight, dbias, workspace, stream);
}

extern "C" int mi355_hstu_rms_norm_fwd(const void* x, int64_t x_stride, int64_t rows, int64_t D, int dtype, const void* weight,
                                       int weight_dtype, float eps, void* y, int64_t y_stride, float* rstd, hipStream_t stream) {
  NORM_CHECK_COMMON("hstu_rms_norm_fwd", rows, D, dtype, weight_dtype, "weights are");
  MI355_CHECK_ARG(x_stride >= D && y_stride >= D, "hstu_rms_norm_fwd: a row stride is smaller than D");
  if (rows == 0) return MI355_OK;
  MI355_CHECK_ARG(x && y && weight && rstd, "hstu_rms_norm_fwd: null buffer with rows > 0");
  const int eb = elem_bytes(dtype), web = elem_bytes(weight_dtype);
  MI355_CHECK_ARG(norm_aligned(x, eb) && norm_aligned(y, eb) && norm_aligned(weight, web),
                  "hstu_rms_norm_fwd: a base pointer is not aligned to the element size");
  return fam_fwd<kNormRms>(x, x_stride, rows, D, dtype, weight, nullptr, weight_dtype, eps, y, y_stride, nullptr, rstd, stream);
}

extern "C" int mi355_hstu_rms_norm_bwd(const void* dy, int64_t dy_stride, const void* x, int64_t x_stride, int64_t rows, int64_t D,
                                       int dtype, const void* weight, int weight_dtype, const float* rstd, void* dx,
                                       int64_t dx_stride, void* dweight, void* workspace, int64_t workspace_bytes,
                                       hipStream_t stream) {
  NORM_CHECK_COMMON("hstu_rms_norm_bwd", rows, D, dtype, weight_dtype, "weights are");
  MI355_CHECK_ARG(dy_stride >= D && x_stride >= D && dx_stride >= D, "hstu_rms_norm_bwd: a row stride is smaller than D");
  MI355_CHECK_ARG(dweight && (rows == 0 || (dy && x && dx && weight && rstd)),
                  "hstu_rms_norm_bwd: null buffer (dweight is needed for rows == 0 too)");
  MI355_CHECK_ARG(rows == 0 || (workspace && ((uintptr_t)workspace & 15) == 0 &&
                                workspace_bytes >= mi355_hstu_rms_norm_bwd_workspace_bytes(rows, D)),
                  "hstu_rms_norm_bwd: workspace is null, not 16-byte aligned or too small");
  const int eb = elem_bytes(dtype), web = elem_bytes(weight_dtype);
  MI355_CHECK_ARG(norm_aligned(dy, eb) && norm_aligned(x, eb) && norm_aligned(dx, eb) && norm_aligned(weight, web) &&
                      norm_aligned(dweight, web),
                  "hstu_rms_norm_bwd: a base pointer is not aligned to the element size");
  return fam_bwd<kNormRms>(dy, dy_stride, x, x_stride, rows, D, dtype, weight, nullptr, weight_dtype, nullptr, rstd, dx, dx_stride,
                       dweight, nullptr, workspace, stream);
}
