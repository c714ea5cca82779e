// The row run: the one decomposition of the jagged row kernels -- the concat and the inference preprocess (jagged_ops.hip),
// jagged <-> padded dense (fbgemm_jagged.hip) and the position / timestamp adds (position_ops.hip).  Each of those files holds
// what is its own, the resolve step and the arithmetic; the run, its piece loop and its host plan are here and only here.
//
// Decomposition.  The unit of work is a run of 2^k consecutive rows of the OUTPUT (k = 2 .. 6, chosen per call so that a small
// call still fills the chip: rows_per_wave_log2), one wave per run -- load follows the bytes, never the length of one sample (a
// 4096-row sample next to empty ones is 64 .. 1024 waves like any other 4096 rows).  A wave works in two phases:
//   resolve: lane l owns row m0 + l (row_run gives it its row index m, clamped to the run's first row for a lane past the run's
//            end, which must then resolve to "no row").  The kernel turns m into the addresses of the row: a binary search of
//            the offsets for its sample (sample_of), then whatever the op needs.  An address of 0 means "no such row".
//   stream:  the run is one flat list of `vpr` pieces per row (wave_run_pieces); lane i of a step takes piece i, and its row's
//            addresses come from the owning lane with shuffles (shfl_addr).  UN steps' loads are issued before their stores.  All
//            lanes work whatever D is (D = 136 bf16: 17 pieces per row).
// Two rules of the piece loop are not obvious.  Loads are unconditional: a lane without a piece, or whose row has no source,
// reads the zero word g_zero_piece instead, or hipcc fences each load into its own branch (gather_dev.h, g_zero_row).  And the
// row index of a lane past the end of the run is clamped to 0 BEFORE the shuffle that takes it as a lane number.
// Everything is addressed in 64 bits.  No row outside a buffer is touched whatever the offsets hold: the resolve step gives a row
// index outside its buffer the address 0.
//
// wave_move_run is the mover of the ops that only copy (W bytes a piece, W the widest of 16 / 8 / 4 / 2 that divides the row and
// every base pointer and stride of the call: access_width; the host checks the pointers, not only D).  It is an explicit
// loop, the text of wave_run_pieces with its two steps written in, and not a caller of it as position_ops.hip's wave_add_run
// is: on the generic loop the eight copy kernels of jagged_ops.hip keep their instruction count at W = 16 / 4 / 2 but not
// their order, and at W = 8 they are four instructions and two VGPRs above (the pad kernels do not care).  Written out, every
// kernel of the three files compiles to the instructions it had while each file had a loop of its own
// (profiles/row_run_refactor.txt).  A change to the loop's rules is therefore made twice, both times in this header.
#pragma once
#include <stdio.h>
#include "common.h"

namespace mi355 {

// read by the lanes of a step that have nothing to load (position_ops.hip reads up to 32 bytes of it)
static __device__ __attribute__((aligned(32))) uint32_t g_zero_piece[8];

template <int W> struct Piece;
template <> struct Piece<16> { typedef unsigned int T __attribute__((ext_vector_type(4))); };
template <> struct Piece<8> { typedef unsigned int T __attribute__((ext_vector_type(2))); };
template <> struct Piece<4> { typedef unsigned int T; };
template <> struct Piece<2> { typedef unsigned short T; };

struct FillBits { uint32_t w[4]; };   // the padding element repeated over 16 bytes

template <int W>
__device__ __forceinline__ typename Piece<W>::T fill_piece(const FillBits& f) {
  typename Piece<W>::T v;
  if constexpr (W == 16) { v[0] = f.w[0]; v[1] = f.w[1]; v[2] = f.w[2]; v[3] = f.w[3]; }
  else if constexpr (W == 8) { v[0] = f.w[0]; v[1] = f.w[1]; }
  else if constexpr (W == 4) v = f.w[0];
  else v = (unsigned short)f.w[0];
  return v;
}

__device__ __forceinline__ uintptr_t shfl_addr(uintptr_t v, int src) {
  const int lo = __shfl((int)(v & 0xffffffffu), src, 64), hi = __shfl((int)(v >> 32), src, 64);
  return (uintptr_t)(unsigned)lo | ((uintptr_t)(unsigned)hi << 32);
}

// largest b in [0, B - 1] with off[b] <= m
template <typename OT>
__device__ __forceinline__ int64_t sample_of(const OT* off, int64_t B, int64_t m) {
  int64_t lo = 0, hi = B - 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if ((int64_t)off[mid] <= m) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// The run of this wave (blocks of 4 waves): false when it lies past the last row (wave-uniform).  Returned through the
// reference on purpose: the struct by value, tested with nrows == 0, costs every kernel 9 to 13 instructions.
struct RowRun {
  int64_t m;    // the lane's row (the run's first row for a lane that has none)
  int nrows;    // rows of the run: 2^rpw_log2, fewer in the last one
  bool have;    // lane < nrows
};
__device__ __forceinline__ bool row_run(int64_t rows, int rpw_log2, RowRun& r) {
  const int lane = lane_id();
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t m0 = wave << rpw_log2;
  if (m0 >= rows) return false;
  const int64_t left = rows - m0;
  r.nrows = left < (1 << rpw_log2) ? (int)left : (1 << rpw_log2);
  r.have = lane < r.nrows;
  r.m = m0 + (r.have ? lane : 0);
  return true;
}

// The piece loop: ld(u, in, row, piece) for the UN steps of a pass, then st(u) for each.  `in`: the lane has a piece in step u;
// `row` is the lane that owns its row (0 when !in: a valid shuffle source), `piece` its index inside the row.  ld must load
// whatever `in` says (from g_zero_piece when it has no address) and leave what st needs in per-step registers.
template <int UN, class LD, class ST>
__device__ __forceinline__ void wave_run_pieces(int nrows, uint32_t vpr, int vpr_shift, LD ld, ST st) {
  const uint32_t lane = (uint32_t)lane_id();
  const uint32_t total = (uint32_t)nrows * vpr;
  for (uint32_t base = 0; base < total; base += 64 * UN) {
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const uint32_t i = base + u * 64 + lane;
      const bool in = i < total;
      const uint32_t ic = in ? i : 0u;
      const uint32_t row = vpr_shift >= 0 ? ic >> vpr_shift : ic / vpr;
      ld(u, in, (int)row, ic - row * vpr);
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) st(u);
  }
}

// The wave moves `nrows` rows of `vpr` pieces of W bytes: lane l holds the source and the destination address of row l.
// FILL false: a row whose source or destination is 0 is skipped.  FILL true: destination 0 skips the row, source 0 writes `fill`.
template <int W, bool FILL>
__device__ __forceinline__ void wave_move_run(uintptr_t src, uintptr_t dst, int nrows, uint32_t vpr, int vpr_shift,
                                              const FillBits& fill = FillBits{}) {
  typedef typename Piece<W>::T V;
  typedef const __attribute__((address_space(1))) V* gsrc_t;
  typedef __attribute__((address_space(1))) V* gdst_t;
  constexpr int UN = 4;
  const uint32_t lane = (uint32_t)lane_id();
  const uint32_t total = (uint32_t)nrows * vpr;
  const uintptr_t zero = (uintptr_t)g_zero_piece;
  V fv;
  if constexpr (FILL) fv = fill_piece<W>(fill);
  for (uint32_t base = 0; base < total; base += 64 * UN) {
    V v[UN];
    uintptr_t d[UN];
    bool copy[UN];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const uint32_t i = base + u * 64 + lane;
      const bool in = i < total;
      const uint32_t ic = in ? i : 0u;
      const uint32_t row = vpr_shift >= 0 ? ic >> vpr_shift : ic / vpr;
      const uintptr_t col = (uintptr_t)(ic - row * vpr) * W;
      const uintptr_t s = shfl_addr(src, (int)row), dd = shfl_addr(dst, (int)row);
      copy[u] = in && s != 0 && (FILL || dd != 0);
      v[u] = *(gsrc_t)(copy[u] ? s + col : zero);
      d[u] = (FILL ? in && dd != 0 : copy[u]) ? dd + col : 0;
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      if constexpr (FILL) { if (d[u]) *(gdst_t)d[u] = copy[u] ? v[u] : fv; }
      else { if (d[u]) *(gdst_t)d[u] = v[u]; }
    }
  }
}

// Rows per wave: 64 while the call has waves to spare; halved (down to 4) while it would leave the chip short of waves and a
// wave would still move 4 KiB.
static inline int rows_per_wave_log2(int64_t rows, uint64_t row_bytes) {
  int k = 6;
  while (k > 2 && ceil_div(rows, (int64_t)1 << k) < 4096 && (row_bytes << (k - 1)) >= 4096) --k;
  return k;
}

static inline int log2_or_minus1(uint32_t v) { return (v & (v - 1)) == 0 ? __builtin_ctz(v) : -1; }

// widest access (bytes) that divides everything in `bits`: the OR of the row bytes, the base pointers and the strides of a call
static inline int access_width(uint64_t bits) { return (bits & 15) == 0 ? 16 : (bits & 7) == 0 ? 8 : (bits & 3) == 0 ? 4 : 2; }

// The host side of a run, as the kernels read it (their argument structs embed it), and the grid of 256-thread blocks.
struct RunPlan {
  uint32_t vpr;    // pieces per row
  int vpr_shift;   // log2(vpr) when it is a power of two, else -1
  int rpw_log2;    // rows per wave
};
static inline int plan_run(int64_t rows, uint64_t row_bytes, uint64_t pieces_per_row, const char* name, RunPlan& p, unsigned& grid) {
  p.vpr = (uint32_t)pieces_per_row;
  p.vpr_shift = log2_or_minus1(p.vpr);
  p.rpw_log2 = rows_per_wave_log2(rows, row_bytes);
  const int64_t g = ceil_div(ceil_div(rows, (int64_t)1 << p.rpw_log2), 4);
  if (g >= ((int64_t)1 << 31)) {
    char msg[128];
    snprintf(msg, sizeof(msg), "%s: too many rows for one launch", name);
    mi355_set_error(msg);
    return MI355_EINVAL;
  }
  grid = (unsigned)g;
  return MI355_OK;
}

// `w` (an access_width) as the constant W of the statement
#define MI355_SWITCH_W(w, ...)                                  \
  switch (w) {                                                  \
    case 16: { constexpr int W = 16; __VA_ARGS__; } break;      \
    case 8: { constexpr int W = 8; __VA_ARGS__; } break;        \
    case 4: { constexpr int W = 4; __VA_ARGS__; } break;        \
    default: { constexpr int W = 2; __VA_ARGS__; } break;       \
  }

}  // namespace mi355
