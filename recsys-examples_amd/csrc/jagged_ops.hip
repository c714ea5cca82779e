// Jagged row movers of the HSTU pre-/post-processing: the concat of n jagged 2-D tensors (forward and its inverse), the block
// workload table of the reference's Python wrapper, and the inference preprocess (item / action interleave + candidates).
//
// Replaces (reference, examples/commons/ops/cuda_ops/csrc/): concat_2D_jagged_tensors_forward_kernel / _backward_kernel and
// compute_block_workloads_kernel (jagged_tensor_op_kernel.cu), and the host loop of narrow().copy_() calls of
// hstu_inference_preprocess (jagged_tensor_op_cuda.cpp:135-240).  Written for wave64 from the semantics; the reference's
// kernels give a 32-lane warp to a row and index rows in 32 bits.
//
// The decomposition -- one wave per run of 2^k rows of the MERGED buffer, lane l resolves row l, the run is copied as one flat
// stream of pieces -- is the row run of jagged_dev.h, and so are the piece loop and the choice of k and W.  Here is the resolve
// step of the two ops:
//   concat:     binary search of merged_offsets for the row's sample, then one pass over the n tensors' offsets (the tensor index
//               is wave-uniform: the pointer tables are kernel arguments read with scalar loads, the offsets vector loads that
//               mostly share a cache line) -> the address of its row in its tensor.  The backward is the same kernel with source
//               and destination swapped: every row of every per-tensor buffer is some merged row, so every one is written.
//   preprocess: the row's place in the item / action interleave of its sample (below).
// No row outside a tensor is touched whatever the offsets hold: a row index outside [0, rows[t]) or [0, total_rows) is
// skipped.
#include "common.h"
#include "jagged_dev.h"
#include "../../include/recsys_amd.h"

namespace mi355 {

constexpr int kJagMaxN = 128;
constexpr int kJagF64 = 3;   // dtype code of these entry points only (element size 8); 0 / 1 / 2 as everywhere

struct JagArgs {
  uintptr_t vals[kJagMaxN];        // per-tensor values [rows[t], D]
  const int64_t* offs[kJagMaxN];   // per-tensor offsets [B + 1]
  int64_t rows[kJagMaxN];          // per-tensor row count (bound of every access)
  const int64_t* merged_offsets;   // [B + 1]
  uintptr_t merged;                // [total_rows, D]
  int64_t total_rows;
  int64_t B;
  uint32_t row_bytes;
  int n;
  int dir;                         // 0: tensors -> merged, 1: merged -> tensors
  RunPlan plan;                     // pieces of W bytes
};

struct PreArgs {
  uintptr_t item, action, out;
  const int64_t* item_offsets;     // [B + 1]
  const int64_t* action_offsets;   // [B + 1]
  const int64_t* out_offsets;      // [B + 1]
  int64_t item_rows, action_rows, out_rows, B;
  uint32_t row_bytes;
  RunPlan plan;
};

struct WorkArgs {
  const int64_t* offs[kJagMaxN];
  int64_t* out;
  int64_t B, nb, spb;
  int n;
};

template <int W>
__global__ __launch_bounds__(256) void jagged_concat_kernel(const JagArgs a) {
  RowRun run;
  if (!row_run(a.total_rows, a.plan.rpw_log2, run)) return;   // (wave-uniform)
  const bool have = run.have;
  const int64_t m = run.m;
  const int64_t b = sample_of(a.merged_offsets, a.B, m);
  int64_t rem = m - a.merged_offsets[b];
  bool open = have && rem >= 0;
  uintptr_t trow = 0;
#pragma unroll 4
  for (int t = 0; t < a.n; ++t) {
    const int64_t* o = a.offs[t];
    const int64_t s = o[b];
    int64_t len = o[b + 1] - s;
    len = len > 0 ? len : 0;
    const bool hit = open && rem < len;
    const int64_t r = s + rem;
    if (hit && r >= 0 && r < a.rows[t]) trow = a.vals[t] + (uintptr_t)r * a.row_bytes;
    open = open && !hit;
    rem -= len;
  }
  const uintptr_t mrow = trow ? a.merged + (uintptr_t)m * a.row_bytes : 0;
  wave_move_run<W, false>(a.dir == 0 ? trow : mrow, a.dir == 0 ? mrow : trow, run.nrows, a.plan.vpr, a.plan.vpr_shift);
}

// Output row r of a sample with I items, A actions (A - I = e in {0, 1}) and L = 2 h + e + C output rows:
//   r < e: action[0];  r' = r - e < 2 h: item[r' / 2] (even) or action[r' / 2 + e] (odd);  else item[h + r' - 2 h].
template <int W>
__global__ __launch_bounds__(256) void hstu_inference_preprocess_kernel(const PreArgs a) {
  RowRun run;
  if (!row_run(a.out_rows, a.plan.rpw_log2, run)) return;   // (wave-uniform)
  const bool have = run.have;
  const int64_t m = run.m;
  const int64_t b = sample_of(a.out_offsets, a.B, m);
  const int64_t o0 = a.out_offsets[b], L = a.out_offsets[b + 1] - o0;
  const int64_t i0 = a.item_offsets[b], I = a.item_offsets[b + 1] - i0;
  const int64_t a0 = a.action_offsets[b], A = a.action_offsets[b + 1] - a0;
  const int64_t e = A - I, h = L - e - I;
  const int64_t r = m - o0, rp = r - e;
  bool from_action;
  int64_t k;
  if (r < e) { from_action = true; k = 0; }
  else if (rp < 2 * h) { from_action = (rp & 1) != 0; k = (rp >> 1) + (from_action ? e : 0); }
  else { from_action = false; k = rp - h; }
  const int64_t cnt = from_action ? A : I;
  const int64_t g = (from_action ? a0 : i0) + k;
  const bool ok = have && r >= 0 && r < L && k >= 0 && k < cnt && g >= 0 && g < (from_action ? a.action_rows : a.item_rows);
  const uintptr_t src = ok ? (from_action ? a.action : a.item) + (uintptr_t)g * a.row_bytes : 0;
  const uintptr_t dst = ok ? a.out + (uintptr_t)m * a.row_bytes : 0;
  wave_move_run<W, false>(src, dst, run.nrows, a.plan.vpr, a.plan.vpr_shift);
}

// work_id = (b n + t) nb + idx -> rows of block idx of segment (b, t); blockIdx.y = t keeps the table index wave-uniform
__global__ __launch_bounds__(256) void jagged_block_workloads_kernel(const WorkArgs a) {
  const int t = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.B * a.nb) return;
  const int64_t b = i / a.nb, idx = i - b * a.nb;
  const int64_t* o = a.offs[t];
  int64_t w = o[b + 1] - o[b] - idx * a.spb;
  w = w < a.spb ? w : a.spb;
  a.out[(b * a.n + t) * a.nb + idx] = w > 0 ? w : 0;
}

static inline int elem_bytes_of(int dtype) { return dtype == kJagF64 ? 8 : elem_bytes(dtype); }

}  // namespace mi355

using namespace mi355;

extern "C" int mi355_jagged_concat(int n, const void* const* values, const int64_t* const* offsets, const int64_t* rows,
                                   int64_t batch, const int64_t* merged_offsets, void* merged, int64_t total_rows, int64_t D,
                                   int dtype, int direction, hipStream_t stream) {
  MI355_CHECK_ARG(n >= 1 && n <= kJagMaxN, "jagged_concat: n must be in 1..128");
  MI355_CHECK_ARG(D > 0, "jagged_concat: D must be > 0");
  const int eb = elem_bytes_of(dtype);
  MI355_CHECK_ARG(eb != 0, "jagged_concat: unsupported dtype");
  MI355_CHECK_ARG(direction == 0 || direction == 1, "jagged_concat: direction must be 0 (concat) or 1 (split)");
  MI355_CHECK_ARG(batch >= 1 && total_rows >= 0, "jagged_concat: batch must be >= 1 and total_rows >= 0");
  MI355_CHECK_ARG(D <= (int64_t)(1 << 24) / eb, "jagged_concat: a row is limited to 16 MiB");
  MI355_CHECK_ARG(values && offsets && rows && merged_offsets, "jagged_concat: null argument array");
  MI355_CHECK_ARG(merged || total_rows == 0, "jagged_concat: null merged buffer");
  JagArgs a{};
  uintptr_t bits = (uintptr_t)merged;
  for (int t = 0; t < n; ++t) {
    MI355_CHECK_ARG(offsets[t], "jagged_concat: null offsets pointer");
    MI355_CHECK_ARG(rows[t] >= 0 && (values[t] || rows[t] == 0), "jagged_concat: null values pointer with rows > 0");
    a.vals[t] = (uintptr_t)values[t];
    a.offs[t] = offsets[t];
    a.rows[t] = values[t] ? rows[t] : 0;
    if (a.rows[t]) bits |= a.vals[t];
  }
  MI355_CHECK_ARG((bits & (uintptr_t)(eb - 1)) == 0, "jagged_concat: a base pointer is not aligned to the element size");
  if (total_rows == 0) return MI355_OK;
  const uint64_t rb = (uint64_t)D * eb;
  const int w = access_width(rb | bits);
  a.merged_offsets = merged_offsets;
  a.merged = (uintptr_t)merged;
  a.total_rows = total_rows;
  a.B = batch;
  a.row_bytes = (uint32_t)rb;
  a.n = n;
  a.dir = direction;
  unsigned grid;
  if (const int rc = plan_run(total_rows, rb, rb / w, "jagged_concat", a.plan, grid)) return rc;
  MI355_SWITCH_W(w, jagged_concat_kernel<W><<<dim3(grid), dim3(256), 0, stream>>>(a));
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

extern "C" int mi355_jagged_block_workloads(int n, const int64_t* const* offsets, int64_t batch, int64_t seqlen_per_block,
                                            int64_t max_seqlen, int64_t* workloads, int64_t workloads_numel,
                                            hipStream_t stream) {
  MI355_CHECK_ARG(n >= 1 && n <= kJagMaxN, "jagged_block_workloads: n must be in 1..128");
  MI355_CHECK_ARG(batch >= 1, "jagged_block_workloads: batch must be >= 1");
  MI355_CHECK_ARG(seqlen_per_block > 0 && max_seqlen >= 0, "jagged_block_workloads: seqlen_per_block must be > 0 and max_seqlen >= 0");
  const int64_t nb = ceil_div(max_seqlen, seqlen_per_block);
  MI355_CHECK_ARG(batch * nb < ((int64_t)1 << 38), "jagged_block_workloads: batch * blocks too large");
  MI355_CHECK_ARG(workloads_numel >= batch * n * nb, "jagged_block_workloads: workloads is smaller than batch * n * blocks");
  MI355_CHECK_ARG(offsets, "jagged_block_workloads: null argument array");
  if (nb == 0) return MI355_OK;
  MI355_CHECK_ARG(workloads, "jagged_block_workloads: null workloads");
  WorkArgs a{};
  for (int t = 0; t < n; ++t) {
    MI355_CHECK_ARG(offsets[t], "jagged_block_workloads: null offsets pointer");
    a.offs[t] = offsets[t];
  }
  a.out = workloads;
  a.B = batch; a.nb = nb; a.spb = seqlen_per_block; a.n = n;
  hipLaunchKernelGGL(jagged_block_workloads_kernel, dim3((unsigned)ceil_div(batch * nb, 256), (unsigned)n), dim3(256), 0, stream, a);
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

extern "C" int mi355_hstu_inference_preprocess(const void* item_values, int64_t item_rows, const int64_t* item_offsets,
                                               const void* action_values, int64_t action_rows, const int64_t* action_offsets,
                                               const int64_t* out_offsets, int64_t batch, void* out, int64_t out_rows,
                                               int64_t D, int dtype, hipStream_t stream) {
  MI355_CHECK_ARG(D > 0, "hstu_inference_preprocess: D must be > 0");
  const int eb = elem_bytes_of(dtype);
  MI355_CHECK_ARG(eb != 0, "hstu_inference_preprocess: unsupported dtype");
  MI355_CHECK_ARG(batch >= 1, "hstu_inference_preprocess: batch must be >= 1");
  MI355_CHECK_ARG(item_rows >= 0 && action_rows >= 0 && out_rows >= 0, "hstu_inference_preprocess: negative row count");
  MI355_CHECK_ARG(D <= (int64_t)(1 << 24) / eb, "hstu_inference_preprocess: a row is limited to 16 MiB");
  MI355_CHECK_ARG(item_offsets && action_offsets && out_offsets, "hstu_inference_preprocess: null offsets");
  MI355_CHECK_ARG((item_values || item_rows == 0) && (action_values || action_rows == 0) && (out || out_rows == 0),
                  "hstu_inference_preprocess: null buffer with rows > 0");
  const uintptr_t bits = (uintptr_t)out | (item_rows ? (uintptr_t)item_values : 0) | (action_rows ? (uintptr_t)action_values : 0);
  MI355_CHECK_ARG((bits & (uintptr_t)(eb - 1)) == 0, "hstu_inference_preprocess: a base pointer is not aligned to the element size");
  if (out_rows == 0) return MI355_OK;
  const uint64_t rb = (uint64_t)D * eb;
  const int w = access_width(rb | bits);
  PreArgs a{};
  a.item = (uintptr_t)item_values; a.action = (uintptr_t)action_values; a.out = (uintptr_t)out;
  a.item_offsets = item_offsets; a.action_offsets = action_offsets; a.out_offsets = out_offsets;
  a.item_rows = item_rows; a.action_rows = action_rows; a.out_rows = out_rows; a.B = batch;
  a.row_bytes = (uint32_t)rb;
  unsigned grid;
  if (const int rc = plan_run(out_rows, rb, rb / w, "hstu_inference_preprocess", a.plan, grid)) return rc;
  MI355_SWITCH_W(w, hstu_inference_preprocess_kernel<W><<<dim3(grid), dim3(256), 0, stream>>>(a));
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}
