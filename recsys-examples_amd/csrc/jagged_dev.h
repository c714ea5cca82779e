// Device / host helpers shared by the jagged row kernels (jagged_ops.hip, position_ops.hip): one wave per run of rows, lane l
// resolves row l of the run, the row's addresses travel to the copying lanes with shuffles.
#pragma once
#include "common.h"

namespace mi355 {

__device__ __forceinline__ uintptr_t shfl_addr(uintptr_t v, int src) {
  const int lo = __shfl((int)(v & 0xffffffffu), src, 64), hi = __shfl((int)(v >> 32), src, 64);
  return (uintptr_t)(unsigned)lo | ((uintptr_t)(unsigned)hi << 32);
}

// largest b in [0, B - 1] with off[b] <= m
__device__ __forceinline__ int64_t sample_of(const int64_t* off, int64_t B, int64_t m) {
  int64_t lo = 0, hi = B - 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (off[mid] <= m) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// Rows per wave: 64 while the call has waves to spare; halved (down to 4) while it would leave the chip short of waves and a
// wave would still move 4 KiB.
static inline int rows_per_wave_log2(int64_t rows, uint64_t row_bytes) {
  int k = 6;
  while (k > 2 && ceil_div(rows, (int64_t)1 << k) < 4096 && (row_bytes << (k - 1)) >= 4096) --k;
  return k;
}

static inline int log2_or_minus1(uint32_t v) { return (v & (v - 1)) == 0 ? __builtin_ctz(v) : -1; }

}  // namespace mi355
