// One layer of the rigorous point forward (logit + running fp32 error bound; the arithmetic is
// described in csrc/points.hip), shared by the point kernel and the discrimination-rate kernel
// (csrc/rate.hip).  The last layer writes [z - d, z + d] of point p to a.out_lb[p] / a.out_ub[p]:
// global memory in the point kernel, a wave-private LDS slab in the rate kernel.
#pragma once
#include "args.h"

struct PointCfg {
  int w_lds[FA_MAX_LAYERS];   // LDS float offset of W_l in MFMA operand order
  int b_lds[FA_MAX_LAYERS];
  int bp_lds[FA_MAX_LAYERS];  // the layer's biases again, zero padded to whole 16-neuron tiles (16-byte aligned)
};

template <int TM>
__device__ __forceinline__ void fa_point_layer(const NetDesc& net, const BoundArgs& a, const PointCfg& cfg,
                                               const float* smem, int l, int p0, int lane,
                                               const float (&H)[TM][4], const float (&E)[TM][4],
                                               float (&H2)[TM][4], float (&E2)[TM][4]) {
  const int col = lane & 15, grp = lane >> 4;
  const int n_in = net.dims[l], n_out = net.dims[l + 1];
  const int tin = (n_in + 15) >> 4, tout = (n_out + 15) >> 4;
  const float* sw = smem + cfg.w_lds[l];
  const float* sbp = smem + cfg.bp_lds[l];
  const bool last = l == net.n_layers - 1;
  const float gg = net.g_fwd[l];
  const float gi = net.g_one;
  const float gnext = last ? 0.f : net.g_fwd[l + 1];
  const int noff = net.neuron_off[l];
  const int p = p0 + col;
  const bool pv = p < a.R;
  // forced-zero flags of this point's hidden layer l (per point, or per the point's partition); which
  // of the two masks is in use is wave-uniform and decided here, not per accumulator register
  const bool masked = !last && (a.dead_in || a.dead_part);
  const uint8_t* drow = nullptr;
  if (masked && pv) {
    if (a.dead_in) drow = a.dead_in + (size_t)p * net.n_hidden + noff;
    else drow = a.dead_part + (size_t)a.node_part[a.part_mod ? p % a.part_mod : p] * net.n_hidden + noff;
  }
#pragma unroll
  for (int jt = 0; jt < TM; ++jt) {
    if (jt >= tout) break;
    // the lane's four biases of this tile, read ahead of the chains (their MFMAs cover the LDS wait)
    // with one unguarded 16-byte read of the zero-padded copy (a padded neuron's bias is 0)
    const float4 b4 = *reinterpret_cast<const float4*>(sbp + 16 * jt + 4 * grp);
    const float bl[4] = {b4.x, b4.y, b4.z, b4.w};
    bool forced[4] = {false, false, false, false};
    if (masked) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int j = 16 * jt + 4 * grp + i;
        forced[i] = drow && j < n_out && drow[j] != 0;
      }
    }
    f32x4 Z = {0.f, 0.f, 0.f, 0.f}, Q = {0.f, 0.f, 0.f, 0.f};
    const float4* wq = reinterpret_cast<const float4*>(sw) + (size_t)jt * tin * 64 + lane;
#pragma unroll
    for (int t = 0; t < TM; ++t) {
      if (t >= tin) break;
      const float4 w4 = wq[t * 64];
      const float wv[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        Z = fa_mfma4(wv[i], H[t][i], Z);
        Q = fa_mfma4(fabsf(wv[i]), E[t][i], Q);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = 16 * jt + 4 * grp + i;
      const bool jv = j < n_out;
      const float b = bl[i];
      const float z = Z[i] + b;
      // explicit fused steps (one rounding each), so that the bounds do not depend on which of the
      // products the compiler chooses to contract: Q (1 + 2g) + (g|b|), then + g1|z|
      const float d = fmaf(gi, fabsf(z), fmaf(Q[i], 1.f + 2.f * gg, gg * fabsf(b)));
      if (last) {
        if (j == 0 && pv) {
          a.out_lb[p] = z - d;
          a.out_ub[p] = z + d;
        }
        continue;
      }
      const bool zero = !jv || forced[i] || (z + d <= 0.f);
      const float h = zero ? 0.f : fmaxf(z, 0.f);
      const float e = zero ? 0.f : d;
      H2[jt][i] = h;
      E2[jt][i] = fmaf(gnext, h, e);   // next layer's error operand: e + g |h|  (h >= 0), fused
    }
  }
}
