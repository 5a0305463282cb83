// The parts the leaf-enumeration kernels share (fa_count_enum_kernel in count.hip, fa_gap_enum_kernel
// in gap.hip): which PA / RA slot each of a lane's input coordinates is, the leaf's mixed-radix
// decode table, a point's coordinates and the rigorous forward of one row of 16 points.  The point s
// of a leaf is the mixed-radix decode over the non-PA dims in increasing dim order, last dim
// fastest (ops/count.lattice_points_at).  All force-inlined.
#pragma once
#include "pointfwd.h"
#include "regfwd.h"

// per lane: the PA slot of input coordinate 16 t + 4 grp + i (-1: none) and the stride of its digit
// in the offset index (0: not an RA dim); fixed for the launch
template <int XT>
struct FaEnumSlots {
  int8_t pslot[XT][4];
  int rstride[XT][4];
  int base;                 // 2 tau + 1
};

template <int XT, typename Args>
__device__ __forceinline__ void fa_enum_slots(const Args& a, int grp, FaEnumSlots<XT>& s) {
  s.base = 2 * a.tau + 1;
#pragma unroll
  for (int t = 0; t < XT; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k = 16 * t + 4 * grp + i;
      int q = -1, rs = 0, st = 1;
      for (int m = 0; m < a.npa; ++m)
        if (a.pa_idx[m] == k) q = m;
      for (int m = a.nra - 1; m >= 0; --m) {
        if (a.ra_idx[m] == k) rs = st;
        st *= s.base;
      }
      s.pslot[t][i] = (int8_t)q;
      s.rstride[t][i] = rs;
    }
}

// one thread: the leaf's lo / width / digit stride per dim into LDS; returns its volume, or 0 for an
// empty box or one over a.max_vol.  A PA dim has width 1 (its coordinate is overwritten).
template <typename Args>
__device__ __forceinline__ int fa_enum_decode(const Args& a, int leaf, int n0, float* s_lo, int* s_w, int* s_st) {
  long long vol = 1;
  for (int k = n0 - 1; k >= 0; --k) {
    const float l = a.lo[(size_t)leaf * n0 + k], h = a.hi[(size_t)leaf * n0 + k];
    bool pa = false;
    for (int m = 0; m < a.npa; ++m) pa = pa || a.pa_idx[m] == k;
    const int w = pa ? 1 : (int)(h - l) + 1;
    s_lo[k] = l;
    s_w[k] = w;
    s_st[k] = (int)vol;
    if (w < 1) vol = 0;
    if (vol <= a.max_vol) vol *= w;
  }
  return (vol >= 1 && vol <= a.max_vol) ? (int)vol : 0;
}

// this lane's coordinates of point s (0 where the point or the dim does not exist)
template <int XT>
__device__ __forceinline__ void fa_enum_point(float (&Xb)[XT][4], int s, bool sv, int grp, int n0, const float* s_lo,
                                              const int* s_w, const int* s_st) {
#pragma unroll
  for (int t = 0; t < XT; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k = 16 * t + 4 * grp + i;
      Xb[t][i] = (k < n0 && sv) ? s_lo[k] + (float)((s / s_st[k]) % s_w[k]) : 0.f;
    }
}

// rigorous forward of the 16 points' row (PA assignment v, offset vector e or -1) into the slab row
// out = [lb x 16 | ub x 16]
template <int TM, int XT, typename Args>
__device__ __forceinline__ void fa_enum_run_row(const NetDesc& net, const Args& a, BoundArgs& ba, const PointCfg& cfg,
                                                const float* smem, int lane, const float (&Xb)[XT][4],
                                                const FaEnumSlots<XT>& sl, float g0, int v, int e, float* out,
                                                float (&HA)[TM][4], float (&EA)[TM][4], float (&HB)[TM][4],
                                                float (&EB)[TM][4]) {
#pragma unroll
  for (int t = 0; t < XT; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float x = Xb[t][i];
      const int q = sl.pslot[t][i];
      if (q >= 0) x = (float)a.values[v * a.npa + q];
      const int rs = sl.rstride[t][i];
      if (e >= 0 && rs > 0) x += (float)((e / rs) % sl.base - a.tau);
      HA[t][i] = x;
      EA[t][i] = g0 * fabsf(x);      // inputs are exact: only the GEMM rounding term
    }
  ba.out_lb = out;
  ba.out_ub = out + 16;
  for (int l = 0; l < net.n_layers; ++l) {
    if (l & 1) fa_point_layer<TM>(net, ba, cfg, smem, l, 0, lane, HB, EB, HA, EA);
    else fa_point_layer<TM>(net, ba, cfg, smem, l, 0, lane, HA, EA, HB, EB);
  }
}
