// The row-forward layer of the six rigorous point kernels: fa_rate_kernel (rate.hip),
// fa_count_enum_kernel (count.hip), fa_gap_enum_kernel (gap.hip), fa_audit_kernel (audit.hip),
// fa_neighbour_kernel (neighbours.hip) and fa_causal_kernel (causal.hip).
//
// Work shape, common to the six: W is staged once per workgroup in MFMA operand order with the padded
// bias copy (fa_stage_wperm, regfwd.h).  Each of the four waves owns 16 rows per pass = the 16 MFMA
// columns; a lane keeps the base row's coordinates 16 t + 4 grp + i in Xb[t][i] (n0 <= 32: at most two
// tiles).  A row to bound is the base row with a few coordinates overwritten: a query's PA assignment
// and RA offset vector, a neighbour's coordinate, a causal set's values.  It runs through the rigorous
// point forward (fa_point_layer, pointfwd.h: fp32 logit +- the running Higham bound) into a
// wave-private LDS slab row [lb x 16 | ub x 16], written by lanes 0..15 and read back by the same lane
// only, and is tested on the spot against its counterpart -- through a V x V pair table in LDS where
// the kernel takes a query.  What differs per kernel is the outer loop: where the base rows come from
// (the hash stream, a leaf's mixed-radix decode, a table in HBM), what is kept of a row's bounds and
// how the flags are reduced.  (fa_rate_kernel and fa_causal_kernel keep fa_row_forward's few lines in
// place, around the shared and their own coordinate rule: rate.hip and causal.hip say why.)
//
// Device code is force-inlined and templated on the kernel's Args type through its field names (npa,
// pa_idx, nra, ra_idx, tau, values, V, E, Pp, pairs; lo, hi and max_vol for the leaf decode).  The host
// half holds what every launcher does before it sizes its LDS: the net-shape test with the staged
// layout and the TM bucket, and the range checks of the query fields.
#pragma once
#include "launch.h"
#include "pointfwd.h"
#include "regfwd.h"

// the kernel instances, one per TM bucket (launch.h fa_tm_bucket)
#define FA_ROW_TMS(X) X(1) X(2) X(4) X(7) X(10)

// ---- device ------------------------------------------------------------------------------------
// per lane: the PA slot of input coordinate 16 t + 4 grp + i (-1: none) and the stride of its digit
// in the offset index (0: not an RA dim); fixed for the launch
template <int XT>
struct FaRowSlots {
  int8_t pslot[XT][4];
  int rstride[XT][4];
  int base;                 // 2 tau + 1
};

template <int XT, typename Args>
__device__ __forceinline__ void fa_row_slots(const Args& a, int grp, FaRowSlots<XT>& s) {
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

// all threads: the V x V pair-validity table valid[v * V + v'] from a.pairs (an index outside [0, V)
// names no pair); readable on return
template <typename Args>
__device__ __forceinline__ void fa_stage_pair_table(const Args& a, uint8_t* valid, int tid) {
  const int V = a.V;
  for (int i = tid; i < V * V; i += FA_THREADS) valid[i] = 0;
  __syncthreads();
  for (int q = tid; q < a.Pp; q += FA_THREADS) {
    const int64_t vi = a.pairs[2 * q], vj = a.pairs[2 * q + 1];
    if (vi >= 0 && vi < V && vj >= 0 && vj < V) valid[(int)vi * V + (int)vj] = 1;
  }
  __syncthreads();
}

// the query's coordinate rule: PA := values[v] when v >= 0 (-1: the base row's own), then the RA offset
// of vector e when e >= 0 (row-major over ra_idx, unclipped; -1: none)
template <int XT, typename Args>
struct FaQueryCoord {
  const Args& a;
  const FaRowSlots<XT>& sl;
  int v, e;
  __device__ __forceinline__ float operator()(int t, int i, float x) const {
    const int q = sl.pslot[t][i];
    if (v >= 0 && q >= 0) x = (float)a.values[v * a.npa + q];
    const int rs = sl.rstride[t][i];
    if (e >= 0 && rs > 0) x += (float)((e / rs) % sl.base - a.tau);
    return x;
  }
};

// rigorous forward of the 16 columns' rows into the slab row out = [lb x 16 | ub x 16]: coord(t, i, x)
// is the value of input coordinate 16 t + 4 grp + i given the base row's x = Xb[t][i]; g0 = net.g_fwd[0]
template <int TM, int XT, typename Coord>
__device__ __forceinline__ void fa_row_forward(const NetDesc& net, BoundArgs& ba, const PointCfg& cfg, const float* smem,
                                               int lane, const float (&Xb)[XT][4], float g0, const Coord coord,
                                               float* out, float (&HA)[TM][4], float (&EA)[TM][4],
                                               float (&HB)[TM][4], float (&EB)[TM][4]) {
#pragma unroll
  for (int t = 0; t < XT; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float x = coord(t, i, Xb[t][i]);
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

// ---- leaf enumeration (count.hip, gap.hip) -----------------------------------------------------
// The point s of a leaf is the mixed-radix decode over the non-PA dims in increasing dim order, last
// dim fastest (ops/count.lattice_points_at).
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

// ---- host --------------------------------------------------------------------------------------
// The net-shape test of the family (no layer over 160 wide, at most 32 inputs), the staged layout
// into rc and the TM bucket of the net; 0: the shape is not covered.
inline int fa_row_net(const NetDesc& net, RegNetCfg& rc) {
  for (int l = 0; l <= net.n_layers; ++l)
    if (net.dims[l] > 160) return 0;
  if (net.dims[0] > 32 || !fa_regnet_cfg(net, rc)) return 0;
  return fa_tm_bucket(fa_regnet_tm(net));
}

// Are the query fields of a launch inside what the kernels cover?  1..FA_MAX_PA PA dims and up to
// FA_MAX_RA RA dims inside the inputs, 1..32 PA assignments and offset vectors (one without RA dims).
template <typename Args>
inline bool fa_row_query_ok(const NetDesc& net, const Args& a) {
  if (a.npa < 1 || a.npa > FA_MAX_PA || a.nra < 0 || a.nra > FA_MAX_RA || a.tau < 0) return false;
  if (a.V < 1 || a.V > FA_RATE_MAX_V || a.E < 1 || a.E > FA_RATE_MAX_E || a.Pp < 0) return false;
  if (a.nra == 0 && a.E != 1) return false;
  for (int m = 0; m < a.npa; ++m)
    if (a.pa_idx[m] < 0 || a.pa_idx[m] >= net.dims[0]) return false;
  for (int m = 0; m < a.nra; ++m)
    if (a.ra_idx[m] < 0 || a.ra_idx[m] >= net.dims[0]) return false;
  return true;
}
