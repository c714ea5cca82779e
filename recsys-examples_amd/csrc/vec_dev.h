// V consecutive elements of a row <-> fp32 registers in one access: shared by position_ops.hip and norm_ops.hip.
#pragma once
#include "common.h"

namespace mi355 {

template <int NW> struct Words { typedef uint32_t T __attribute__((ext_vector_type(NW))); };
template <> struct Words<1> { typedef uint32_t T; };

// V consecutive elements of dtype DT <-> fp32, one access of V * sizeof(element) bytes
template <int DT, int V> struct Vec {
  static constexpr int EB = DT == kF32 ? 4 : 2;
  static constexpr int BYTES = V * EB;
  static __device__ __forceinline__ float up(uint32_t h) {
    return DT == kBF16 ? __uint_as_float(h << 16) : f16_to_f32((uint16_t)h);
  }
  static __device__ __forceinline__ uint32_t down(float f) {
    return DT == kBF16 ? (uint32_t)f32_to_bf16(f) : (uint32_t)f32_to_f16(f);
  }
  static __device__ __forceinline__ void ld(uintptr_t a, float (&f)[V]) {
    if constexpr (BYTES == 2) {
      f[0] = up(*(const __attribute__((address_space(1))) uint16_t*)a);
    } else {
      constexpr int NW = BYTES / 4;
      typedef typename Words<NW>::T W;
      const W w = *(const __attribute__((address_space(1))) W*)a;
      uint32_t u[NW];
      if constexpr (NW == 1) {
        u[0] = w;
      } else {
#pragma unroll
        for (int i = 0; i < NW; ++i) u[i] = w[i];
      }
#pragma unroll
      for (int i = 0; i < NW; ++i) {
        if constexpr (DT == kF32) {
          f[i] = __uint_as_float(u[i]);
        } else {
          f[2 * i] = up(u[i] & 0xffffu);
          f[2 * i + 1] = up(u[i] >> 16);
        }
      }
    }
  }
  static __device__ __forceinline__ void st(uintptr_t a, const float (&f)[V]) {
    if constexpr (BYTES == 2) {
      *(__attribute__((address_space(1))) uint16_t*)a = (uint16_t)down(f[0]);
    } else {
      constexpr int NW = BYTES / 4;
      typedef typename Words<NW>::T W;
      uint32_t u[NW];
#pragma unroll
      for (int i = 0; i < NW; ++i) {
        if constexpr (DT == kF32) u[i] = __float_as_uint(f[i]);
        else u[i] = down(f[2 * i]) | (down(f[2 * i + 1]) << 16);
      }
      W w;
      if constexpr (NW == 1) {
        w = u[0];
      } else {
#pragma unroll
        for (int i = 0; i < NW; ++i) w[i] = u[i];
      }
      *(__attribute__((address_space(1))) W*)a = w;
    }
  }
};

}  // namespace mi355
