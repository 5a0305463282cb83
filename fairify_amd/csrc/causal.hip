// Causal-discrimination search over attribute sets: per (base row, attribute set) cert / poss bits
// from the rigorous point forward.  gfx950.
//
// Definitions: ops/causal.py, docs/DESIGN.md 5h.  Row s of x [S, n0] is one base row.  Set t =
// dims[t, 0..3] (strictly increasing feature indices, padded with -1) has A_t = prod |vals_k|
// assignments, enumerated row-major over the tuple, the last feature fastest; assignment a sets
// x[dims_j] := vals[voff[dims_j] + digit_j(a)].  An assignment is a candidate of a row when it differs
// from the row's own values in at least one component.  With [l, u] the rigorous logit bounds of the
// base row and [l', u'] those of an altered row, and label(x) = [N(x) > 0]:
//     cert (bit 1)   some candidate has  (l > 0 and u' <= 0) or (u <= 0 and l' > 0)   (=> poss)
//     poss (bit 0)   some candidate has  (u > 0 and l' <= 0) or (l <= 0 and u' > 0)
// code [S, T] holds one byte per (row, set): 0, 1 or 3.  The host decides the bytes equal to 1 exactly
// (engine/causal.py).
//
// Work shape: csrc/rowfwd.h, one slab row per wave and no query.  A work item is (64-row pass, set): items are
// strided over blockIdx.x, a set's passes side by side, so with the sets ordered by descending A_t the
// long items start first.  The base row is bounded once per item; the assignments are walked
// wave-uniformly with an odometer over the four digits (a padded slot has one value and always
// carries), so there is no division per assignment.  Each grp == 0 lane stores its row's byte once.
// No atomics.
#include <hip/hip_runtime.h>

#include "rowfwd.h"

// Waves per SIMD: the neighbours instances' values (docs/DESIGN.md 5h has the resource remarks).
template <int TM>
__global__ void __launch_bounds__(FA_THREADS) __attribute__((amdgpu_waves_per_eu(TM == 10 ? 1 : 2)))
fa_causal_kernel(NetDesc net, CausalArgs a, RegNetCfg rc) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int XT = TM < 2 ? TM : 2;     // input tiles kept per row: n0 <= 32 (the launch refuses wider)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, grp = lane >> 4;
  const int n0 = net.dims[0];
  float* slab = smem + rc.floats + wave * 32;
  fa_stage_wperm(net, rc, a.flat, smem, tid, FA_THREADS);
  __syncthreads();
  BoundArgs ba{};
  ba.R = 16;
  ba.out_lb = slab;
  ba.out_ub = slab + 16;
  const float g0 = net.g_fwd[0];
  float Xb[XT][4], HA[TM][4], EA[TM][4], HB[TM][4], EB[TM][4];
  const int passes = (a.S + 63) / 64;
  const long long items = (long long)passes * a.T;
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    const int t = (int)(it / passes), ps = (int)(it % passes);
    const int row = ps * 64 + wave * 16 + col;
    const bool rv = row < a.S;
    // the set's dims, the start of each one's value list and its length: wave-uniform addresses.  A
    // padded slot (-1) matches no coordinate and counts one value
    const int d0 = a.dims[4 * t], d1 = a.dims[4 * t + 1], d2 = a.dims[4 * t + 2], d3 = a.dims[4 * t + 3];
    const int o0 = d0 >= 0 ? a.voff[d0] : 0, c0 = d0 >= 0 ? a.voff[d0 + 1] - o0 : 1;
    const int o1 = d1 >= 0 ? a.voff[d1] : 0, c1 = d1 >= 0 ? a.voff[d1 + 1] - o1 : 1;
    const int o2 = d2 >= 0 ? a.voff[d2] : 0, c2 = d2 >= 0 ? a.voff[d2 + 1] - o2 : 1;
    const int o3 = d3 >= 0 ? a.voff[d3] : 0, c3 = d3 >= 0 ? a.voff[d3 + 1] - o3 : 1;
#pragma unroll
    for (int tt = 0; tt < XT; ++tt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k = 16 * tt + 4 * grp + i;
        Xb[tt][i] = (k < n0 && rv) ? a.x[(size_t)row * n0 + k] : 0.f;
      }
    // rigorous forward of the 16 columns' rows with the set's coordinates overwritten by v0 .. v3
    // (alter false: the base rows themselves), into the slab row
    // (fa_row_forward's body, kept in place like rate.hip's: called as a function the 4-tile instance
    // measured 5 % slower on AC-3, profiles/r22/rowfwd/README.md)
    auto run_row = [&](bool alter, float v0, float v1, float v2, float v3) {
#pragma unroll
      for (int tt = 0; tt < XT; ++tt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int k = 16 * tt + 4 * grp + i;
          float x = Xb[tt][i];
          if (alter) {
            if (k == d0) x = v0;
            if (k == d1) x = v1;
            if (k == d2) x = v2;
            if (k == d3) x = v3;
          }
          HA[tt][i] = x;
          EA[tt][i] = g0 * fabsf(x);      // inputs are exact: only the GEMM rounding term
        }
      for (int l = 0; l < net.n_layers; ++l) {
        if (l & 1) fa_point_layer<TM>(net, ba, rc, smem, l, 0, lane, HB, EB, HA, EA);
        else fa_point_layer<TM>(net, ba, rc, smem, l, 0, lane, HA, EA, HB, EB);
      }
    };
    run_row(false, 0.f, 0.f, 0.f, 0.f);
    // the base row's bounds and its own values on the set's dims, in the grp == 0 lane (the row's line
    // is in L1)
    const bool own = grp == 0 && rv;
    float lo_x = 0.f, up_x = 0.f;
    int x0 = 0, x1 = 0, x2 = 0, x3 = 0;
    if (own) {
      lo_x = slab[col];
      up_x = slab[16 + col];
      const float* xr = a.x + (size_t)row * n0;
      if (d0 >= 0) x0 = (int)xr[d0];
      if (d1 >= 0) x1 = (int)xr[d1];
      if (d2 >= 0) x2 = (int)xr[d2];
      if (d3 >= 0) x3 = (int)xr[d3];
    }
    bool cert = false, poss = false;
    const long long A = (long long)c0 * c1 * c2 * c3;
    int g0d = 0, g1d = 0, g2d = 0, g3d = 0;
    for (long long as = 0; as < A; ++as) {
      // wave-uniform stop that changes no output: every valid column has its cert bit (and with it poss)
      if (__ballot(own && !cert) == 0) break;
      const int v0 = d0 >= 0 ? a.vals[o0 + g0d] : 0, v1 = d1 >= 0 ? a.vals[o1 + g1d] : 0;
      const int v2 = d2 >= 0 ? a.vals[o2 + g2d] : 0, v3 = d3 >= 0 ? a.vals[o3 + g3d] : 0;
      // the odometer, last digit fastest
      if (++g3d >= c3) {
        g3d = 0;
        if (++g2d >= c2) {
          g2d = 0;
          if (++g1d >= c1) {
            g1d = 0;
            ++g0d;
          }
        }
      }
      // a candidate of this column: some component differs from the row's own (a padded slot never does)
      const bool cand = own && ((d0 >= 0 && v0 != x0) || (d1 >= 0 && v1 != x1) || (d2 >= 0 && v2 != x2) ||
                                (d3 >= 0 && v3 != x3));
      if (__ballot(cand && !cert) == 0) continue;
      run_row(true, (float)v0, (float)v1, (float)v2, (float)v3);
      if (cand) {
        const float lp = slab[col], up = slab[16 + col];
        if ((lo_x > 0.f && up <= 0.f) || (up_x <= 0.f && lp > 0.f)) cert = true;
        if ((up_x > 0.f && lp <= 0.f) || (lo_x <= 0.f && up > 0.f)) poss = true;
      }
    }
    if (own) a.code[(size_t)row * a.T + t] = (uint8_t)((cert ? 2 : 0) | (poss ? 1 : 0));
  }
}

// Dynamic LDS of one workgroup: the staged block and one slab row per wave.
static size_t causal_lds_bytes(const RegNetCfg& rc) {
  const size_t floats = (size_t)rc.floats + (size_t)(FA_THREADS / 64) * 32;
  return (floats * sizeof(float) + 15) & ~(size_t)15;
}

// Writes code [S, T].  Returns 0 if launched, -3 for shapes the kernel does not cover (the audit
// launcher's conditions: a layer over 160 wide, inputs over 32 wide or more than 64 KB of dynamic LDS --
// the instances are not in the raised-limit registry, docs/DESIGN.md 5h; and a set with more than 4
// dims, or whose dims are not strictly increasing inside the inputs with the padding last), -2 for a
// workgroup count outside 1 .. passes x T, > 0 a HIP error.
extern "C" int fa_causal_launch(const NetDesc& net, CausalArgs a, hipStream_t stream) {
  if (a.S <= 0 || a.T <= 0) return 0;
  if (a.D != 4 || !a.h_dims || !a.h_voff) return -3;
  RegNetCfg rc{};
  const int tmb = fa_row_net(net, rc);
  if (!tmb) return -3;
  const int n0 = net.dims[0];
  if (a.h_voff[0] != 0 || a.h_voff[n0] != a.nvals) return -3;
  for (int k = 0; k < n0; ++k)
    if (a.h_voff[k + 1] <= a.h_voff[k]) return -3;
  for (int t = 0; t < a.T; ++t) {
    int prev = -1;
    bool pad = false;
    for (int j = 0; j < 4; ++j) {
      const int d = a.h_dims[4 * t + j];
      if (d == -1) {
        pad = true;
        continue;
      }
      if (pad || d <= prev || d >= n0) return -3;
      prev = d;
    }
    if (prev < 0) return -3;
  }
  void (*k)(NetDesc, CausalArgs, RegNetCfg) = nullptr;
  switch (tmb) {
#define FA_CAUSAL_CASE(T) \
  case T: k = fa_causal_kernel<T>; break;
    FA_ROW_TMS(FA_CAUSAL_CASE)
#undef FA_CAUSAL_CASE
    default: return -3;
  }
  const size_t bytes = causal_lds_bytes(rc);
  if (bytes > 64 * 1024) return -3;
  const long long items = (long long)((a.S + 63) / 64) * a.T;
  if (a.blocks < 1 || a.blocks > items) return -2;
  hipLaunchKernelGGL(k, dim3((unsigned)a.blocks), dim3(FA_THREADS), bytes, stream, net, a, rc);
  return (int)hipGetLastError();
}
