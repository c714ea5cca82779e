// HSTU layer norms: layer norm and layer-norm-mul-dropout over rows [N, D], forward and backward.
//
// Replaces (reference, examples/hstu/ops/triton_ops): _layer_norm_fwd / _weighted_layer_norm_fwd and their backwards
// (triton_layer_norm.py:313-481), _ln_mul_dropout_fwd and _ln_mul_dropout_bwd_dx_du / _dwdb (triton_norm_mul_dropout.py:36-525).
// Written for wave64 from the arithmetic; the reference is Triton.
//
// Values (all arithmetic fp32, every stored value rounded once):
//   mean = sum(x) / D;  var = sum((x - mean)^2) / D from the registers that hold the row;  rstd = 1 / sqrtf(var + eps)
//   xh = (x - mean) * rstd;  ln = fmaf(xh, w, b)  (w = 1, b = 0: not learnable);  t = ln * u
//   backward, gp the gradient that reaches ln (dy, or dt * u):  g = w * gp;  c1 = sum(xh * g) / D;  c2 = sum(g) / D;
//   dx = (g - (xh * c1 + c2)) * rstd (+ extra);  dw = sum over rows of gp * xh;  db = sum over rows of gp
//
// Dropout (this project's definition; Triton's tl.rand stream is not reproduced).  Element (row, col) of mask `which`
// (0 / 1 / 2 = the u / x / t part of a concat_ux output; 0 without concat_ux) takes one 32-bit draw r of Philox4x32-10
// (init_dev.h) with
//   key     = (seed & 0xffffffff, seed >> 32)
//   counter = (row & 0xffffffff, row >> 32, col >> 2, which)
//   r       = word (col & 3) of the four output words, in the order x, y, z, w
// and is kept iff r >= floor(p * 2^32) as unsigned integers; a kept value is v / (1.0f - (float)p) (IEEE division), a
// dropped one +0.  The mask is a function of (seed, row, col, which, p) alone.
//
// Layout of a call, the kernels (hstu_norm_fwd_kernel / hstu_norm_bwd_kernel, kinds kNormLayer and kNormLnMul here), the grid
// size, the dispatch ladder and the dw / db fold: norm_dev.h, shared with norm_family_ops.hip and group_norm_ops.hip.  This file
// holds the argument checks and the argument blocks of the four entry points.
#include "norm_dev.h"
#include "../../include/recsys_amd.h"

using namespace mi355;

#define NORM_CHECK_MUL(NAME, H, UD, D, p)                                                                            \
  MI355_CHECK_ARG(H >= 1 && UD >= 1 && H * UD == D, NAME ": u must hold H * UD == D elements per row");              \
  MI355_CHECK_ARG(p >= 0.0 && p < 1.0, NAME ": dropout_ratio must be in [0, 1)")

extern "C" int mi355_hstu_layer_norm_fwd(const void* x, int64_t x_stride, int64_t rows, int64_t D, int dtype, const void* weight,
                                         const void* bias, int weight_dtype, float eps, void* y, int64_t y_stride, float* mean,
                                         float* rstd, int stats_given, hipStream_t stream) {
  NORM_CHECK_COMMON("hstu_layer_norm_fwd", rows, D, dtype, weight_dtype, "weight and bias are");
  MI355_CHECK_ARG((weight == nullptr) == (bias == nullptr), "hstu_layer_norm_fwd: weight and bias are given together or not at all");
  MI355_CHECK_ARG(x_stride >= D && y_stride >= D, "hstu_layer_norm_fwd: a row stride is smaller than D");
  if (rows == 0) return MI355_OK;
  MI355_CHECK_ARG(x && y && mean && rstd, "hstu_layer_norm_fwd: null buffer with rows > 0");
  const int eb = elem_bytes(dtype), web = elem_bytes(weight_dtype);
  MI355_CHECK_ARG(norm_aligned(x, eb) && norm_aligned(y, eb) && norm_aligned(weight, web) && norm_aligned(bias, web),
                  "hstu_layer_norm_fwd: a base pointer is not aligned to the element size");
  NormVec nv{D % (16 / eb) == 0 ? 16 / eb : 1};
  nv.need(x, x_stride * eb); nv.need(y, y_stride * eb); nv.need(weight, 0); nv.need(bias, 0);
  NormArgs a{};
  a.x = (uintptr_t)x; a.y = (uintptr_t)y; a.w = (uintptr_t)weight; a.b = (uintptr_t)bias;
  a.x_stride = x_stride * eb; a.y_stride = y_stride * eb;
  a.mean = mean; a.rstd = rstd; a.N = rows; a.D = (int)D; a.UD = (int)D; a.eps = eps;
  a.w_f32 = weight_dtype == kF32; a.learnable = weight != nullptr; a.stats_given = stats_given != 0;
  const int grid = norm_row_blocks(rows, D, false);
  norm_launch<kNormLayer, false>(dtype, nv.v, grid, a, stream);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

extern "C" int64_t mi355_hstu_layer_norm_bwd_workspace_bytes(int64_t rows, int64_t D) {
  if (rows < 0 || D <= 0 || D > kNormMaxD) return 0;
  return (int64_t)2 * norm_row_blocks(rows, D, true) * D * 4;
}
extern "C" int64_t mi355_hstu_ln_mul_dropout_bwd_workspace_bytes(int64_t rows, int64_t D) {
  return mi355_hstu_layer_norm_bwd_workspace_bytes(rows, D);
}

extern "C" int mi355_hstu_layer_norm_bwd(const void* dy, int64_t dy_stride, const void* x, int64_t x_stride, int64_t rows, int64_t D,
                                         int dtype, const void* weight, int weight_dtype, const float* mean, const float* rstd,
                                         const void* dx_accumulate, int64_t dx_accumulate_stride, void* dx, int64_t dx_stride,
                                         void* dweight, void* dbias, void* workspace, int64_t workspace_bytes,
                                         hipStream_t stream) {
  NORM_CHECK_COMMON("hstu_layer_norm_bwd", rows, D, dtype, weight_dtype, "weight and bias are");
  const bool learnable = weight != nullptr;
  MI355_CHECK_ARG(!learnable || (dweight && dbias), "hstu_layer_norm_bwd: a learnable norm needs dweight and dbias");
  MI355_CHECK_ARG(dy_stride >= D && x_stride >= D && dx_stride >= D && (!dx_accumulate || dx_accumulate_stride >= D),
                  "hstu_layer_norm_bwd: a row stride is smaller than D");
  MI355_CHECK_ARG(!learnable || (workspace && ((uintptr_t)workspace & 15) == 0 &&
                                 workspace_bytes >= mi355_hstu_layer_norm_bwd_workspace_bytes(rows, D)),
                  "hstu_layer_norm_bwd: workspace is null, not 16-byte aligned or too small");
  MI355_CHECK_ARG(rows == 0 || (dy && x && dx && mean && rstd), "hstu_layer_norm_bwd: null buffer with rows > 0");
  const int eb = elem_bytes(dtype), web = elem_bytes(weight_dtype);
  MI355_CHECK_ARG(norm_aligned(dy, eb) && norm_aligned(x, eb) && norm_aligned(dx, eb) && norm_aligned(dx_accumulate, eb) &&
                      norm_aligned(weight, web) && norm_aligned(dweight, web) && norm_aligned(dbias, web),
                  "hstu_layer_norm_bwd: a base pointer is not aligned to the element size");
  NormVec nv{D % (16 / eb) == 0 ? 16 / eb : 1};
  nv.need(dy, dy_stride * eb); nv.need(x, x_stride * eb); nv.need(dx, dx_stride * eb); nv.need(weight, 0);
  if (dx_accumulate) nv.need(dx_accumulate, dx_accumulate_stride * eb);
  NormArgs a{};
  a.dy = (uintptr_t)dy; a.x = (uintptr_t)x; a.dx = (uintptr_t)dx; a.w = (uintptr_t)weight; a.extra = (uintptr_t)dx_accumulate;
  a.dy_stride = dy_stride * eb; a.x_stride = x_stride * eb; a.dx_stride = dx_stride * eb; a.extra_stride = dx_accumulate_stride * eb;
  a.mean = const_cast<float*>(mean); a.rstd = const_cast<float*>(rstd); a.partial = (float*)workspace;
  a.N = rows; a.D = (int)D; a.UD = (int)D;
  a.w_f32 = weight_dtype == kF32; a.learnable = learnable;
  const int grid = norm_row_blocks(rows, D, true);
  if (rows > 0) {
    norm_launch<kNormLayer, true>(dtype, nv.v, grid, a, stream);
    MI355_LAUNCH_CHECK();
  }
  if (learnable) return norm_launch_dwdb(a.partial, rows > 0 ? grid : 0, a.D, weight_dtype, dweight, dbias, stream);
  return MI355_OK;
}

extern "C" int mi355_hstu_ln_mul_dropout_fwd(const void* x, int64_t x_stride, const void* u, int64_t u_stride0, int64_t u_stride1,
                                             int64_t H, int64_t UD, int64_t rows, int64_t D, int dtype, const void* weight,
                                             const void* bias, int weight_dtype, float eps, double dropout_ratio, int training,
                                             uint64_t seed, int concat_ux, void* y, int64_t y_stride, float* mean, float* rstd,
                                             hipStream_t stream) {
  NORM_CHECK_COMMON("hstu_ln_mul_dropout_fwd", rows, D, dtype, weight_dtype, "weight and bias are");
  NORM_CHECK_MUL("hstu_ln_mul_dropout_fwd", H, UD, D, dropout_ratio);
  const int64_t yw = concat_ux ? 3 * D : D;
  MI355_CHECK_ARG(x_stride >= D && y_stride >= yw && u_stride1 >= UD && u_stride0 >= (H - 1) * u_stride1 + UD,
                  "hstu_ln_mul_dropout_fwd: a stride is smaller than the extent it steps over");
  if (rows == 0) return MI355_OK;
  MI355_CHECK_ARG(x && u && y && weight && bias && mean && rstd, "hstu_ln_mul_dropout_fwd: null buffer with rows > 0");
  const int eb = elem_bytes(dtype), web = elem_bytes(weight_dtype);
  MI355_CHECK_ARG(norm_aligned(x, eb) && norm_aligned(u, eb) && norm_aligned(y, eb) && norm_aligned(weight, web) && norm_aligned(bias, web),
                  "hstu_ln_mul_dropout_fwd: a base pointer is not aligned to the element size");
  MI355_CHECK_ARG((H - 1) * u_stride1 * eb < ((int64_t)1 << 31), "hstu_ln_mul_dropout_fwd: u head stride too large");
  NormVec nv{D % (16 / eb) == 0 && UD % (16 / eb) == 0 ? 16 / eb : 1};
  nv.need(x, x_stride * eb); nv.need(y, y_stride * eb); nv.need(u, u_stride0 * eb); nv.need(nullptr, u_stride1 * eb);
  nv.need(weight, 0); nv.need(bias, 0);
  NormArgs a{};
  a.x = (uintptr_t)x; a.u = (uintptr_t)u; a.y = (uintptr_t)y; a.w = (uintptr_t)weight; a.b = (uintptr_t)bias;
  a.x_stride = x_stride * eb; a.u_s0 = u_stride0 * eb; a.u_s1 = u_stride1 * eb; a.y_stride = y_stride * eb;
  a.mean = mean; a.rstd = rstd; a.N = rows; a.D = (int)D; a.UD = (int)UD; a.eps = eps;
  a.w_f32 = weight_dtype == kF32; a.learnable = 1; a.concat = concat_ux != 0;
  norm_set_dropout(a, dropout_ratio, training, seed);
  const int grid = norm_row_blocks(rows, D, false);
  norm_launch<kNormLnMul, false>(dtype, nv.v, grid, a, stream);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

extern "C" int mi355_hstu_ln_mul_dropout_bwd(const void* dy, int64_t dy_stride, const void* x, int64_t x_stride, const void* u,
                                             int64_t u_stride0, int64_t u_stride1, int64_t H, int64_t UD, int64_t rows, int64_t D,
                                             int dtype, const void* weight, const void* bias, int weight_dtype, const float* mean,
                                             const float* rstd, double dropout_ratio, int training, uint64_t seed, int concat_ux,
                                             void* dx, int64_t dx_stride, void* du, int64_t du_stride0, int64_t du_stride1,
                                             void* dweight, void* dbias, void* y, int64_t y_stride, void* workspace,
                                             int64_t workspace_bytes, hipStream_t stream) {
  NORM_CHECK_COMMON("hstu_ln_mul_dropout_bwd", rows, D, dtype, weight_dtype, "weight and bias are");
  NORM_CHECK_MUL("hstu_ln_mul_dropout_bwd", H, UD, D, dropout_ratio);
  const int64_t yw = concat_ux ? 3 * D : D;
  MI355_CHECK_ARG(dy_stride >= yw && x_stride >= D && dx_stride >= D && (!y || y_stride >= yw) && u_stride1 >= UD &&
                      u_stride0 >= (H - 1) * u_stride1 + UD && du_stride1 >= UD && du_stride0 >= (H - 1) * du_stride1 + UD,
                  "hstu_ln_mul_dropout_bwd: a stride is smaller than the extent it steps over");
  MI355_CHECK_ARG(dweight && dbias, "hstu_ln_mul_dropout_bwd: null dweight or dbias");
  MI355_CHECK_ARG(workspace && ((uintptr_t)workspace & 15) == 0 &&
                      workspace_bytes >= mi355_hstu_ln_mul_dropout_bwd_workspace_bytes(rows, D),
                  "hstu_ln_mul_dropout_bwd: workspace is null, not 16-byte aligned or too small");
  MI355_CHECK_ARG(rows == 0 || (dy && x && u && dx && du && weight && bias && mean && rstd),
                  "hstu_ln_mul_dropout_bwd: null buffer with rows > 0");
  const int eb = elem_bytes(dtype), web = elem_bytes(weight_dtype);
  MI355_CHECK_ARG(norm_aligned(dy, eb) && norm_aligned(x, eb) && norm_aligned(u, eb) && norm_aligned(dx, eb) && norm_aligned(du, eb) &&
                      norm_aligned(y, eb) && norm_aligned(weight, web) && norm_aligned(bias, web) && norm_aligned(dweight, web) &&
                      norm_aligned(dbias, web),
                  "hstu_ln_mul_dropout_bwd: a base pointer is not aligned to the element size");
  MI355_CHECK_ARG((H - 1) * u_stride1 * eb < ((int64_t)1 << 31) && (H - 1) * du_stride1 * eb < ((int64_t)1 << 31),
                  "hstu_ln_mul_dropout_bwd: u head stride too large");
  NormVec nv{D % (16 / eb) == 0 && UD % (16 / eb) == 0 ? 16 / eb : 1};
  nv.need(dy, dy_stride * eb); nv.need(x, x_stride * eb); nv.need(dx, dx_stride * eb);
  nv.need(u, u_stride0 * eb); nv.need(nullptr, u_stride1 * eb); nv.need(du, du_stride0 * eb); nv.need(nullptr, du_stride1 * eb);
  if (y) nv.need(y, y_stride * eb);
  nv.need(weight, 0); nv.need(bias, 0);
  NormArgs a{};
  a.dy = (uintptr_t)dy; a.x = (uintptr_t)x; a.u = (uintptr_t)u; a.dx = (uintptr_t)dx; a.du = (uintptr_t)du; a.y = (uintptr_t)y;
  a.w = (uintptr_t)weight; a.b = (uintptr_t)bias;
  a.dy_stride = dy_stride * eb; a.x_stride = x_stride * eb; a.u_s0 = u_stride0 * eb; a.u_s1 = u_stride1 * eb;
  a.dx_stride = dx_stride * eb; a.du_s0 = du_stride0 * eb; a.du_s1 = du_stride1 * eb; a.y_stride = y_stride * eb;
  a.mean = const_cast<float*>(mean); a.rstd = const_cast<float*>(rstd); a.partial = (float*)workspace;
  a.N = rows; a.D = (int)D; a.UD = (int)UD;
  a.w_f32 = weight_dtype == kF32; a.learnable = 1; a.concat = concat_ux != 0;
  norm_set_dropout(a, dropout_ratio, training, seed);
  const int grid = norm_row_blocks(rows, D, true);
  if (rows > 0) {
    norm_launch<kNormLnMul, true>(dtype, nv.v, grid, a, stream);
    MI355_LAUNCH_CHECK();
  }
  return norm_launch_dwdb(a.partial, rows > 0 ? grid : 0, a.D, weight_dtype, dweight, dbias, stream);
}
