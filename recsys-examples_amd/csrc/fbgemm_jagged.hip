// The FBGEMM sparse / jagged ops that examples/hstu calls under torch.ops.fbgemm.* (fbgemm_jagged_ops.py): the three cumulative
// sums of a lengths vector, jagged <-> padded dense, and the batch select of a KeyedJaggedTensor.  All of them move data: the
// results are bit-exact, nothing is atomic (no read-modify-write), nothing is read on the host, everything is addressed in 64
// bits and offsets / lengths / indices are read as int32 or int64 by template (a conversion launch would cost what the op does).
// Written for wave64 from the semantics of the ops; FBGEMM's kernels are not the model.
//
// Scan (mi355_cumsum).  A tile is 4096 elements of one row: 256 threads x 16 consecutive elements, staged through LDS so that
// the global accesses are coalesced whatever the alignment of a row ([R, N] in, [R, N + 1] out in complete mode).  Sums are
// carried in 64 bits for both dtypes (an int32 sum is the low half of the 64-bit one, so it wraps as torch.cumsum does); the
// wave scan of a 64-bit value is three wave_incl_scan (scan_dev.h) of its 21 / 21 / 22-bit pieces, which cannot overflow over
// 64 lanes.  While a row has at most kSerialTiles tiles one block walks them with a running carry.  Above that every tile is
// a work item of a resident grid and takes its prefix by decoupled look-back: a tile publishes {status, low half} and
// {status, high half} as two 8-byte granules (status 1: sum of the tile, 2: sum of the row up to and including it) with one
// relaxed agent-scope store each -- the data is the flag, so there is no fence -- and a wave of the consumer reads the 256
// tiles before its own in one step.  A launch takes at most as many tiles as the device holds resident blocks (2 per CU of
// the queried CU count), ONE tile per block and no grid-stride loop, so a block only ever waits for lower-numbered blocks of
// its own launch: they are resident with it, and were it otherwise (CUs masked off or held by another stream's kernel) they
// are the blocks the dispatcher starts first.  A longer input is scanned in consecutive launches on the stream; the first
// tile of a launch that begins inside a row takes its prefix from the output the launch before wrote.  Every poll loop is
// bounded all the same, and a poll that runs out sets the first word of the workspace.  The granules
// are zeroed by a small launch in front (the same write-through stores that publish them; a captured hipMemsetAsync node was
// not seen by the polls of a graph replay -- suspected, not pursued: the node's zeros are still in flight or in a cache that
// the polls' device-scope loads do not look in when the scan starts -- so the look-back does not lean on one).
//
// Padded dense (mi355_jagged_to_padded, mi355_padded_to_jagged).  The row run of jagged_dev.h over the rows of the OUTPUT, moved by
// its wave_move_run in the fill form.  Their own is the resolve step: a division for the dense side, a binary search of the
// offsets for the jagged side, into a source address or "fill"; the strides of the dense side count for the access width.  Every
// output element is written exactly once, the fill included: there is no memset.
//
// Select (mi355_kjt_select_lengths / _values).  Output bag (f, j) is input bag (f, indices[j]).  The values kernel gives every
// OUTPUT ELEMENT a lane (its bag by a binary search of the output offsets), so a bag of 3000 ids is 3000 lanes like any other
// 3000 elements; weights ride in the same launch.
#include "common.h"
#include "jagged_dev.h"
#include "scan_dev.h"
#include "vec_dev.h"
#include "../../include/recsys_amd.h"

namespace mi355 {

// ---------------------------------------------------------------------------------------------------------------------
// scan
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kCsItems = 16;
constexpr int kCsTile = kScanThreads * kCsItems;   // 4096
constexpr int kSerialTiles = 2;                    // a row of up to 8192 elements is one block's (a tile more costs it ~1.5 us)
constexpr int kScanBlocksPerCU = 2;                // resident look-back blocks per CU (154 VGPRs, 37 KB of LDS admit 3)
constexpr int64_t kScanHeaderBytes = 16;           // workspace: {timeout word, pad}, then the granules
constexpr unsigned kSpinLimit = 1u << 22;

struct ScanArgs {
  const void* in;
  void* out;
  uint64_t* granules;   // [rows * tiles * 2] (look-back only)
  uint64_t* timeouts;   // set to 1 by a block whose poll ran out (look-back only)
  int64_t item_begin;   // first work item (row * tiles + tile) of this launch (look-back only)
  int64_t rows, n, tiles;
  int mode;             // 0 complete, 1 inclusive, 2 exclusive
  int lookback;
};

__device__ __forceinline__ int lds_slot(int i) { return i + (i >> 3); }   // 8-byte slots, one of pad per 8: a thread's run is conflict-free

__device__ __forceinline__ uint64_t wave_incl_scan_u64(uint64_t v) {
  const int a = wave_incl_scan((int)(v & 0x1fffffu));
  const int b = wave_incl_scan((int)((v >> 21) & 0x1fffffu));
  const int c = wave_incl_scan((int)(v >> 42));
  return (uint64_t)(uint32_t)a + ((uint64_t)(uint32_t)b << 21) + ((uint64_t)(uint32_t)c << 42);
}

__device__ __forceinline__ uint64_t shfl_u64(uint64_t v, int src) { return (uint64_t)shfl_addr((uintptr_t)v, src); }

// The sum of the row before tile `t`, by wave 0; false when a poll ran out.  `lo` (< t) is the row's first tile inside this
// launch: it publishes its inclusive prefix at once, and nothing before it is read.  One round reads the kLookWindows * 64
// tiles before `hi` with all loads in flight together (a round costs one trip to memory however many tiles it reads: at 1 M
// elements, 256 tiles that start together, every tile is one round from tile 0 instead of up to four), then walks the windows
// from the nearest: up to the nearest tile that knows its inclusive prefix every tile must have published its sum.
constexpr int kLookWindows = 4;
__device__ __forceinline__ bool lookback_prefix(const uint64_t* g, int64_t t, int64_t lo, uint64_t& prefix) {
  const int lane = lane_id();
  uint64_t acc = 0;
  int64_t hi = t - 1;   // lane l reads tiles hi - l - 64 j, j = 0 .. kLookWindows - 1
  for (;;) {
    uint64_t part = 0;
    bool done = false;
    for (unsigned spins = 0;; ++spins) {
      uint64_t val[kLookWindows];
      unsigned st[kLookWindows];
#pragma unroll
      for (int j = 0; j < kLookWindows; ++j) {
        const int64_t mine = hi - lane - 64 * j;
        val[j] = 0;
        st[j] = 2;       // a lane before tile `lo`: an inclusive prefix of 0 (never reached: `lo` itself ends the walk)
        if (mine >= lo) {
          const uint64_t w0 = ald64(g + 2 * mine), w1 = ald64(g + 2 * mine + 1);
          const unsigned s0 = (unsigned)(w0 >> 32), s1 = (unsigned)(w1 >> 32);
          st[j] = s0 == s1 ? s0 : 0;   // the two halves of one publication, or not yet
          val[j] = (w0 & 0xffffffffu) | (w1 << 32);
        }
      }
      bool retry = false;
      part = 0;
      done = false;
#pragma unroll
      for (int j = 0; j < kLookWindows; ++j) {
        if (!done && !retry) {   // (wave-uniform)
          const unsigned long long full = __ballot(st[j] == 2), none = __ballot(st[j] == 0);
          const int first = full ? __builtin_ctzll(full) : 64;   // nearest tile of this window that knows its inclusive prefix
          const unsigned long long needed = first >= 63 ? ~0ull : ((2ull << first) - 1);
          if (none & needed) retry = true;
          else {
            part += lane <= first ? val[j] : 0;
            done = first < 64;
          }
        }
      }
      if (!retry) break;
      if (spins >= kSpinLimit) return false;   // (wave-uniform)
      __builtin_amdgcn_s_sleep(1);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) part += shfl_u64(part, lane ^ d);
    acc += part;
    if (done) break;
    hi -= 64 * kLookWindows;
  }
  prefix = acc;
  return true;
}

__global__ __launch_bounds__(256) void scan_clear_granules_kernel(uint64_t* g, int64_t words) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < words) ast64(g + i, 0);
}

template <typename T>
__global__ __launch_bounds__(kScanThreads) void cumsum_kernel(const ScanArgs a) {
  __shared__ uint64_t s_v[kCsTile + kCsTile / 8];
  __shared__ uint64_t s_wave[kScanThreads / 64];
  __shared__ uint64_t s_prefix;
  __shared__ int s_ok;
  const int tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
  const T* in = (const T*)a.in;
  T* out = (T*)a.out;
  const int64_t out_stride = a.n + (a.mode == 0 ? 1 : 0);
  const int64_t items = a.lookback ? a.rows * a.tiles : a.rows;
  // look-back: one item per block, no loop (the host sizes the launch); one block per row otherwise, rows are independent
  const int64_t item0 = a.lookback ? a.item_begin + blockIdx.x : blockIdx.x, step = a.lookback ? items : gridDim.x;
  for (int64_t item = item0; item < items; item += step) {
    const int64_t row = a.lookback ? item / a.tiles : item;
    const int64_t t_begin = a.lookback ? item - row * a.tiles : 0, t_end = a.lookback ? t_begin + 1 : a.tiles;
    const T* src = in + row * a.n;
    T* dst = out + row * out_stride;
    uint64_t carry = 0;
    for (int64_t t = t_begin; t < t_end; ++t) {
      const int64_t base = t * kCsTile;
      const int cnt = a.n - base < kCsTile ? (int)(a.n - base) : kCsTile;
#pragma unroll
      for (int k = 0; k < kCsItems; ++k) {
        const int i = k * kScanThreads + tid;
        s_v[lds_slot(i)] = i < cnt ? (uint64_t)(int64_t)src[base + i] : 0;
      }
      __syncthreads();
      uint64_t x[kCsItems], run = 0;
#pragma unroll
      for (int k = 0; k < kCsItems; ++k) {
        x[k] = s_v[lds_slot(tid * kCsItems + k)];
        run += x[k];
      }
      const uint64_t incl = wave_incl_scan_u64(run);
      if (lane == 63) s_wave[w] = incl;
      __syncthreads();
      uint64_t before = 0, total = 0;
#pragma unroll
      for (int k = 0; k < kScanThreads / 64; ++k) {
        const uint64_t y = s_wave[k];
        if (k < w) before += y;
        total += y;
      }
      if (a.lookback) {
        uint64_t* g = a.granules + row * a.tiles * 2;
        if (w == 0) {
          // The row's first tile inside this launch knows its inclusive prefix at once: nothing (tile 0), or what the launch
          // before left in the output at the tile's last-but-one element (stream order makes it visible).
          const int64_t lo = a.item_begin > row * a.tiles ? a.item_begin - row * a.tiles : 0;
          uint64_t p = 0;
          bool ok = true;
          if (t == lo) {
            if (t > 0) {
              const int64_t e = base - 1;
              p = (uint64_t)(int64_t)dst[e + (a.mode == 0 ? 1 : 0)];
              if (a.mode == 2) p += (uint64_t)(int64_t)src[e];
            }
          } else {
            if (lane < 2) ast64(g + 2 * t + lane, ((uint64_t)1 << 32) | (uint32_t)(lane == 0 ? total : total >> 32));
            ok = lookback_prefix(g, t, lo, p);
          }
          const uint64_t inc = p + total;
          if (ok && lane < 2) ast64(g + 2 * t + lane, ((uint64_t)2 << 32) | (uint32_t)(lane == 0 ? inc : inc >> 32));
          if (!ok && lane == 0) ast64(a.timeouts, 1);
          if (lane == 0) { s_prefix = p; s_ok = ok ? 1 : 0; }
        }
        __syncthreads();
        carry = s_prefix;
        if (!s_ok) return;   // (block-uniform) a poll ran out: the tile stays unwritten rather than wrong, the timeout word is set
      }
      uint64_t acc = carry + before + incl - run;   // the sum of everything before this thread's first element
#pragma unroll
      for (int k = 0; k < kCsItems; ++k) {
        const uint64_t e = acc;
        acc += x[k];
        s_v[lds_slot(tid * kCsItems + k)] = a.mode == 2 ? e : acc;
      }
      __syncthreads();
      const int64_t shift = a.mode == 0 ? 1 : 0;
#pragma unroll
      for (int k = 0; k < kCsItems; ++k) {
        const int i = k * kScanThreads + tid;
        if (i < cnt) dst[base + i + shift] = (T)s_v[lds_slot(i)];
      }
      if (a.mode == 0 && t == 0 && tid == 0) dst[0] = (T)0;
      carry += total;
      __syncthreads();
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// jagged <-> padded dense
// ---------------------------------------------------------------------------------------------------------------------
struct PadArgs {
  uintptr_t jagged;       // [T, D] rows of row_bytes
  uintptr_t dense;        // [B, N, D]: element (b, l) at dense + b stride_b + l stride_n (bytes)
  const void* offsets;    // [B + 1]
  int64_t T, B, N;
  int64_t stride_b, stride_n;
  int64_t out_rows;       // B N (to padded) or the jagged row count (to jagged)
  uint32_t row_bytes;
  RunPlan plan;
  FillBits fill;
};

template <int W, typename OT>
__global__ __launch_bounds__(256) void jagged_to_padded_kernel(const PadArgs a) {
  RowRun run;
  if (!row_run(a.out_rows, a.plan.rpw_log2, run)) return;   // (wave-uniform)
  const bool have = run.have;
  const int64_t m = run.m;
  const int64_t b = m / a.N, l = m - b * a.N;
  const OT* off = (const OT*)a.offsets;
  const int64_t s = (int64_t)off[b], len = (int64_t)off[b + 1] - s;
  const int64_t r = s + l;
  const bool real = have && l < len && r >= 0 && r < a.T;
  const uintptr_t src = real ? a.jagged + (uintptr_t)r * a.row_bytes : 0;
  const uintptr_t dst = have ? a.dense + (uintptr_t)m * a.row_bytes : 0;
  wave_move_run<W, true>(src, dst, run.nrows, a.plan.vpr, a.plan.vpr_shift, a.fill);
}

template <int W, typename OT>
__global__ __launch_bounds__(256) void padded_to_jagged_kernel(const PadArgs a) {
  RowRun run;
  if (!row_run(a.out_rows, a.plan.rpw_log2, run)) return;   // (wave-uniform)
  const bool have = run.have;
  const int64_t m = run.m;
  uintptr_t src = 0;
  if (a.B > 0) {
    const OT* off = (const OT*)a.offsets;
    const int64_t b = sample_of<OT>(off, a.B, m);
    const int64_t l = m - (int64_t)off[b];
    if (have && l >= 0 && l < a.N && m < (int64_t)off[b + 1])
      src = a.dense + (uintptr_t)b * (uintptr_t)a.stride_b + (uintptr_t)l * (uintptr_t)a.stride_n;
  }
  const uintptr_t dst = have ? a.jagged + (uintptr_t)m * a.row_bytes : 0;
  wave_move_run<W, true>(src, dst, run.nrows, a.plan.vpr, a.plan.vpr_shift, a.fill);
}

// ---------------------------------------------------------------------------------------------------------------------
// KeyedJaggedTensor batch select
// ---------------------------------------------------------------------------------------------------------------------
template <typename LT, typename IT>
__global__ __launch_bounds__(256) void kjt_select_lengths_kernel(const LT* __restrict__ lengths, const IT* __restrict__ indices,
                                                                 int64_t F, int64_t B, int64_t S, LT* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= F * S) return;
  const int64_t f = i / S, j = i - f * S;
  const int64_t idx = (int64_t)indices[j];
  out[i] = idx >= 0 && idx < B ? lengths[f * B + idx] : (LT)0;
}

struct SelArgs {
  const void* values;
  const void* weights;
  const void* offsets;       // [F B + 1] of the input
  const void* indices;       // [S]
  const void* out_offsets;   // [F S + 1]
  void* out_values;
  void* out_weights;
  int64_t num_values, F, B, S, total;
  int weight_bytes;
};

template <typename E>
__device__ __forceinline__ void move_elem(const void* src, void* dst, int64_t from, int64_t to, bool ok) {
  ((E*)dst)[to] = ok ? ((const E*)src)[from] : (E)0;
}

// EB: bytes of a value; OT / PT / IT: the types of the input offsets, the output offsets and the indices
template <typename E, typename OT, typename PT, typename IT>
__global__ __launch_bounds__(256) void kjt_select_values_kernel(const SelArgs a) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= a.total) return;
  const PT* po = (const PT*)a.out_offsets;
  const int64_t bags = a.F * a.S;
  const int64_t bag = sample_of<PT>(po, bags, p);   // the last bag that starts at or before p: the one that holds it
  const int64_t k = p - (int64_t)po[bag];
  const int64_t f = bag / a.S, j = bag - f * a.S;
  const int64_t idx = (int64_t)((const IT*)a.indices)[j];
  bool ok = idx >= 0 && idx < a.B && k >= 0 && p < (int64_t)po[bag + 1];
  int64_t from = 0;
  if (ok) {
    const OT* io = (const OT*)a.offsets;
    const int64_t s = (int64_t)io[f * a.B + idx];
    from = s + k;
    ok = from >= 0 && from < a.num_values && from < (int64_t)io[f * a.B + idx + 1];
    if (!ok) from = 0;
  }
  move_elem<E>(a.values, a.out_values, from, p, ok);
  if (a.weights) {   // (uniform)
    if (a.weight_bytes == 4) move_elem<uint32_t>(a.weights, a.out_weights, from, p, ok);
    else if (a.weight_bytes == 2) move_elem<uint16_t>(a.weights, a.out_weights, from, p, ok);
    else move_elem<uint64_t>(a.weights, a.out_weights, from, p, ok);
  }
}

static inline FillBits fill_bits(uint64_t pattern, int eb) {
  FillBits f;
  if (eb == 8) { f.w[0] = f.w[2] = (uint32_t)pattern; f.w[1] = f.w[3] = (uint32_t)(pattern >> 32); }
  else {
    const uint32_t x = eb == 4 ? (uint32_t)pattern : ((uint32_t)(pattern & 0xffffu) * 0x10001u);
    f.w[0] = f.w[1] = f.w[2] = f.w[3] = x;
  }
  return f;
}

}  // namespace mi355

using namespace mi355;

static inline bool itype_ok(int t) { return t == 0 || t == 1; }

extern "C" int64_t mi355_cumsum_workspace_bytes(int64_t rows, int64_t n) {
  if (rows <= 0 || n <= 0) return 0;
  const int64_t tiles = ceil_div(n, kCsTile);
  return tiles <= kSerialTiles ? 0 : kScanHeaderBytes + rows * tiles * 16;
}

// Blocks of the look-back scan that one launch may hold: kScanBlocksPerCU per CU of the current device, fewer where the
// occupancy query admits fewer (it can over-report by one: hence the cap below what hipcc's register count allows).
static int64_t scan_resident_blocks() {
  static int cached[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  if (cached[dev] > 0) return cached[dev];
  int cus = 0, per = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 1;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, cumsum_kernel<int64_t>, kScanThreads, 0) != hipSuccess || per < 1) per = 1;
  (void)hipGetLastError();
  if (per > kScanBlocksPerCU) per = kScanBlocksPerCU;
  const int g = cus * per;
  cached[dev] = g;
  return g;
}

extern "C" int mi355_cumsum(const void* in, void* out, int64_t rows, int64_t n, int itype, int mode, void* workspace,
                            int64_t workspace_bytes, hipStream_t stream) {
  MI355_CHECK_ARG(itype_ok(itype), "cumsum: unsupported dtype (0 int32, 1 int64)");
  MI355_CHECK_ARG(mode >= 0 && mode <= 2, "cumsum: mode must be 0 (complete), 1 (inclusive) or 2 (exclusive)");
  MI355_CHECK_ARG(rows >= 0 && n >= 0, "cumsum: negative size");
  MI355_CHECK_ARG(rows <= 1 || mode == 0, "cumsum: only the complete sum takes a 2-D input");
  MI355_CHECK_ARG(rows < ((int64_t)1 << 31) && n < ((int64_t)1 << 40), "cumsum: input too large");
  if (rows == 0 || n == 0) return MI355_OK;   // (the caller makes the [rows, 1] zeros of the complete sum)
  MI355_CHECK_ARG(in && out, "cumsum: null buffer");
  const int eb = itype == 1 ? 8 : 4;
  MI355_CHECK_ARG((((uintptr_t)in | (uintptr_t)out) & (uintptr_t)(eb - 1)) == 0, "cumsum: a buffer is not aligned to its element");
  ScanArgs a{};
  a.in = in; a.out = out; a.rows = rows; a.n = n; a.mode = mode;
  a.tiles = ceil_div(n, kCsTile);
  a.lookback = a.tiles > kSerialTiles ? 1 : 0;
  if (!a.lookback) {   // rows are independent: any grid will do
    const int64_t grid = rows < 4096 ? rows : 4096;
    if (itype == 1) hipLaunchKernelGGL(cumsum_kernel<int64_t>, dim3((unsigned)grid), dim3(kScanThreads), 0, stream, a);
    else hipLaunchKernelGGL(cumsum_kernel<int32_t>, dim3((unsigned)grid), dim3(kScanThreads), 0, stream, a);
    MI355_LAUNCH_CHECK();
    return MI355_OK;
  }
  const int64_t items = rows * a.tiles, need = kScanHeaderBytes + items * 16;
  MI355_CHECK_ARG(need < ((int64_t)1 << 40), "cumsum: input too large");
  MI355_CHECK_ARG(workspace && workspace_bytes >= need && ((uintptr_t)workspace & 15) == 0,
                  "cumsum: workspace is null, misaligned or smaller than mi355_cumsum_workspace_bytes");
  a.timeouts = (uint64_t*)workspace;
  a.granules = (uint64_t*)workspace + kScanHeaderBytes / 8;
  hipLaunchKernelGGL(scan_clear_granules_kernel, dim3((unsigned)ceil_div(need / 8, 256)), dim3(256), 0, stream, a.timeouts,
                     need / 8);
  MI355_LAUNCH_CHECK();
  const int64_t per_launch = scan_resident_blocks();
  for (int64_t b = 0; b < items; b += per_launch) {
    a.item_begin = b;
    const int64_t grid = items - b < per_launch ? items - b : per_launch;
    if (itype == 1) hipLaunchKernelGGL(cumsum_kernel<int64_t>, dim3((unsigned)grid), dim3(kScanThreads), 0, stream, a);
    else hipLaunchKernelGGL(cumsum_kernel<int32_t>, dim3((unsigned)grid), dim3(kScanThreads), 0, stream, a);
    MI355_LAUNCH_CHECK();
  }
  return MI355_OK;
}

// the end of both entry points: the access width, the run plan and the launch
static int pad_launch(bool to_padded, const char* name, PadArgs& a, int64_t D, int eb, uint64_t align_bits, int64_t out_rows,
                      int itype, hipStream_t stream) {
  const uint64_t rb = (uint64_t)D * eb;
  const int w = access_width(rb | align_bits);
  a.row_bytes = (uint32_t)rb;
  a.out_rows = out_rows;
  unsigned grid;
  if (const int rc = plan_run(out_rows, rb, rb / w, name, a.plan, grid)) return rc;
#define MI355_PAD_GO(OT)                                                                                        \
  MI355_SWITCH_W(w, if (to_padded) jagged_to_padded_kernel<W, OT><<<dim3(grid), dim3(256), 0, stream>>>(a);     \
                    else padded_to_jagged_kernel<W, OT><<<dim3(grid), dim3(256), 0, stream>>>(a))
  if (itype == 1) { MI355_PAD_GO(int64_t) } else { MI355_PAD_GO(int32_t) }
#undef MI355_PAD_GO
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

extern "C" int mi355_jagged_to_padded(const void* values, int64_t T, const void* offsets, int offsets_itype, int64_t B,
                                      int64_t max_len, int64_t D, int elem_bytes, uint64_t padding_bits, void* out,
                                      hipStream_t stream) {
  MI355_CHECK_ARG(elem_bytes == 2 || elem_bytes == 4 || elem_bytes == 8, "jagged_to_padded: unsupported dtype (element of 2, 4 or 8 bytes)");
  MI355_CHECK_ARG(itype_ok(offsets_itype), "jagged_to_padded: unsupported offsets dtype (0 int32, 1 int64)");
  MI355_CHECK_ARG(T >= 0 && B >= 0 && max_len >= 0, "jagged_to_padded: negative size");
  MI355_CHECK_ARG(D >= 1 && D <= (int64_t)(1 << 24) / elem_bytes, "jagged_to_padded: D must be >= 1 and a row at most 16 MiB");
  MI355_CHECK_ARG(B == 0 || max_len == 0 || B <= ((int64_t)1 << 46) / max_len, "jagged_to_padded: B * max_len too large");
  const int64_t out_rows = B * max_len;
  if (out_rows == 0) return MI355_OK;
  MI355_CHECK_ARG(offsets && out, "jagged_to_padded: null buffer");
  MI355_CHECK_ARG(values || T == 0, "jagged_to_padded: null values with T > 0");
  const uintptr_t bits = (uintptr_t)out | (T ? (uintptr_t)values : 0);
  MI355_CHECK_ARG((bits & (uintptr_t)(elem_bytes - 1)) == 0, "jagged_to_padded: a base pointer is not aligned to the element size");
  PadArgs a{};
  a.jagged = (uintptr_t)values; a.dense = (uintptr_t)out; a.offsets = offsets;
  a.T = values ? T : 0; a.B = B; a.N = max_len;
  a.fill = fill_bits(padding_bits, elem_bytes);
  return pad_launch(true, "jagged_to_padded", a, D, elem_bytes, bits, out_rows, offsets_itype, stream);
}

extern "C" int mi355_padded_to_jagged(const void* dense, int64_t stride_b, int64_t stride_n, int64_t B, int64_t N,
                                      const void* offsets, int offsets_itype, int64_t D, int elem_bytes, void* out,
                                      int64_t total, hipStream_t stream) {
  MI355_CHECK_ARG(elem_bytes == 2 || elem_bytes == 4 || elem_bytes == 8, "padded_to_jagged: unsupported dtype (element of 2, 4 or 8 bytes)");
  MI355_CHECK_ARG(itype_ok(offsets_itype), "padded_to_jagged: unsupported offsets dtype (0 int32, 1 int64)");
  MI355_CHECK_ARG(B >= 0 && N >= 0 && total >= 0, "padded_to_jagged: negative size");
  MI355_CHECK_ARG(stride_b >= 0 && stride_n >= 0, "padded_to_jagged: negative stride");
  MI355_CHECK_ARG(D >= 1 && D <= (int64_t)(1 << 24) / elem_bytes, "padded_to_jagged: D must be >= 1 and a row at most 16 MiB");
  MI355_CHECK_ARG(stride_b < ((int64_t)1 << 56) && stride_n < ((int64_t)1 << 56), "padded_to_jagged: stride too large");
  if (total == 0) return MI355_OK;
  MI355_CHECK_ARG(offsets && out, "padded_to_jagged: null buffer");
  MI355_CHECK_ARG(dense || B * N == 0, "padded_to_jagged: null dense with B * N > 0");
  const bool any = dense && B > 0 && N > 0;
  uintptr_t bits = (uintptr_t)out;
  if (any) bits |= (uintptr_t)dense;
  MI355_CHECK_ARG((bits & (uintptr_t)(elem_bytes - 1)) == 0, "padded_to_jagged: a base pointer is not aligned to the element size");
  if (any) bits |= (uintptr_t)(stride_b * elem_bytes) | (uintptr_t)(stride_n * elem_bytes);
  PadArgs a{};
  a.jagged = (uintptr_t)out; a.dense = (uintptr_t)dense; a.offsets = offsets;
  a.B = any ? B : 0; a.N = N;
  a.stride_b = stride_b * elem_bytes; a.stride_n = stride_n * elem_bytes;
  a.fill = fill_bits(0, elem_bytes);
  return pad_launch(false, "padded_to_jagged", a, D, elem_bytes, bits, total, offsets_itype, stream);
}

extern "C" int mi355_kjt_select_lengths(const void* lengths, int lengths_itype, const void* indices, int indices_itype,
                                        int64_t F, int64_t B, int64_t S, void* out_lengths, hipStream_t stream) {
  MI355_CHECK_ARG(itype_ok(lengths_itype) && itype_ok(indices_itype), "kjt_select_lengths: unsupported dtype (0 int32, 1 int64)");
  MI355_CHECK_ARG(F >= 0 && B >= 0 && S >= 0, "kjt_select_lengths: negative size");
  MI355_CHECK_ARG(F == 0 || S == 0 || F <= ((int64_t)1 << 38) / S, "kjt_select_lengths: F * S too large");
  if (F * S == 0) return MI355_OK;
  MI355_CHECK_ARG(indices && out_lengths && (lengths || B == 0), "kjt_select_lengths: null buffer");
  const unsigned grid = (unsigned)ceil_div(F * S, 256);
#define MI355_SEL_LEN(LT, IT) \
  hipLaunchKernelGGL((kjt_select_lengths_kernel<LT, IT>), dim3(grid), dim3(256), 0, stream, (const LT*)lengths, \
                     (const IT*)indices, F, B, S, (LT*)out_lengths)
  if (lengths_itype == 1) { if (indices_itype == 1) MI355_SEL_LEN(int64_t, int64_t); else MI355_SEL_LEN(int64_t, int32_t); }
  else { if (indices_itype == 1) MI355_SEL_LEN(int32_t, int64_t); else MI355_SEL_LEN(int32_t, int32_t); }
#undef MI355_SEL_LEN
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}

template <typename E>
static void launch_select_values(int ty, unsigned grid, hipStream_t stream, const SelArgs& a) {
#define MI355_SEL_VAL(OT, PT, IT) \
  hipLaunchKernelGGL((kjt_select_values_kernel<E, OT, PT, IT>), dim3(grid), dim3(256), 0, stream, a)
  switch (ty) {
    case 0: MI355_SEL_VAL(int32_t, int32_t, int32_t); break;
    case 1: MI355_SEL_VAL(int64_t, int32_t, int32_t); break;
    case 2: MI355_SEL_VAL(int32_t, int64_t, int32_t); break;
    case 3: MI355_SEL_VAL(int64_t, int64_t, int32_t); break;
    case 4: MI355_SEL_VAL(int32_t, int32_t, int64_t); break;
    case 5: MI355_SEL_VAL(int64_t, int32_t, int64_t); break;
    case 6: MI355_SEL_VAL(int32_t, int64_t, int64_t); break;
    default: MI355_SEL_VAL(int64_t, int64_t, int64_t); break;
  }
#undef MI355_SEL_VAL
}

extern "C" int mi355_kjt_select_values(const void* values, int64_t num_values, int elem_bytes, const void* weights,
                                       int weight_bytes, const void* offsets, int offsets_itype, const void* indices,
                                       int indices_itype, int64_t F, int64_t B, int64_t S, const void* out_offsets,
                                       int out_offsets_itype, void* out_values, void* out_weights, int64_t total,
                                       hipStream_t stream) {
  MI355_CHECK_ARG(elem_bytes == 1 || elem_bytes == 2 || elem_bytes == 4 || elem_bytes == 8,
                  "kjt_select_values: unsupported dtype (element of 1, 2, 4 or 8 bytes)");
  MI355_CHECK_ARG(itype_ok(offsets_itype) && itype_ok(indices_itype) && itype_ok(out_offsets_itype),
                  "kjt_select_values: unsupported offsets / indices dtype (0 int32, 1 int64)");
  MI355_CHECK_ARG(num_values >= 0 && F >= 0 && B >= 0 && S >= 0 && total >= 0, "kjt_select_values: negative size");
  MI355_CHECK_ARG(!weights || weight_bytes == 2 || weight_bytes == 4 || weight_bytes == 8,
                  "kjt_select_values: unsupported weights dtype (element of 2, 4 or 8 bytes)");
  MI355_CHECK_ARG(F == 0 || S == 0 || F <= ((int64_t)1 << 38) / S, "kjt_select_values: F * S too large");
  MI355_CHECK_ARG(total < ((int64_t)1 << 38), "kjt_select_values: too many elements for one launch");
  if (total == 0 || F * S == 0) return MI355_OK;
  MI355_CHECK_ARG(offsets && indices && out_offsets && out_values && (values || num_values == 0),
                  "kjt_select_values: null buffer");
  MI355_CHECK_ARG(!weights || out_weights, "kjt_select_values: weights without out_weights");
  MI355_CHECK_ARG((((uintptr_t)values | (uintptr_t)out_values) & (uintptr_t)(elem_bytes - 1)) == 0 &&
                  (!weights || (((uintptr_t)weights | (uintptr_t)out_weights) & (uintptr_t)(weight_bytes - 1)) == 0),
                  "kjt_select_values: a base pointer is not aligned to the element size");
  SelArgs a{};
  a.values = values; a.weights = weights; a.offsets = offsets; a.indices = indices; a.out_offsets = out_offsets;
  a.out_values = out_values; a.out_weights = out_weights;
  a.num_values = values ? num_values : 0; a.F = F; a.B = B; a.S = S; a.total = total; a.weight_bytes = weight_bytes;
  const unsigned grid = (unsigned)ceil_div(total, 256);
  const int ty = offsets_itype | (out_offsets_itype << 1) | (indices_itype << 2);
  switch (elem_bytes) {
    case 1: launch_select_values<uint8_t>(ty, grid, stream, a); break;
    case 2: launch_select_values<uint16_t>(ty, grid, stream, a); break;
    case 4: launch_select_values<uint32_t>(ty, grid, stream, a); break;
    default: launch_select_values<uint64_t>(ty, grid, stream, a); break;
  }
  MI355_LAUNCH_CHECK();
  return MI355_OK;
}
