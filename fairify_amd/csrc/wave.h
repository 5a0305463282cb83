// Device helpers shared by the wave64 kernels: the gamma of the rounding terms and the cross-lane
// reductions (butterfly sum, arg-max, prefix sum).  All force-inlined.
#pragma once
#include <hip/hip_runtime.h>

// the gamma of the kernels' rounding terms: ku / (1 - ku) for k + 2 operations at unit roundoff u,
// inflated by (1 + 4u) for its own rounding
__device__ __forceinline__ float fa_gam(int k, float u) {
#pragma clang fp contract(off)   // (k + 2) u and 4 u are exact: fused or not, the same value
  const float ku = (float)(k + 2) * u;
  return ku / (1.f - ku) * (1.f + 4.f * u);
}

// butterfly sum within aligned groups of G lanes (every lane of the group gets the total)
template <int G, typename T>
__device__ __forceinline__ T fa_group_sum(T v) {
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// (value, index) arg-max within aligned groups of G lanes (G = 64: the wave): the larger value wins,
// ties go to the lower index (a sequential scan's first strict maximum); every lane gets the winner
template <int G, typename T>
__device__ __forceinline__ void fa_group_argmax(T& s, int& i) {
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) {
    const T s2 = __shfl_xor(s, off, 64);
    const int i2 = __shfl_xor(i, off, 64);
    if (s2 > s || (s2 == s && i2 < i)) { s = s2; i = i2; }
  }
}

// inclusive wave64 prefix sum
__device__ __forceinline__ int fa_wave_incl_scan(int v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(v, o);
    if (lane >= o) v += u;
  }
  return v;
}
