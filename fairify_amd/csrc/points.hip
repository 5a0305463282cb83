// Rigorous point evaluation: logit + running fp32 error bound at integer points.  gfx950.
//
// Used by the branch-and-bound runtime to screen candidate counterexample pairs (every BFS
// level evaluates the LP-optimal vertex pair of every open node) and by the tensor BaB.  It
// replaces interval bound propagation on degenerate boxes (the reference replays candidate
// points with plain `net`, src/AC/Verify-AC.py:229-254; its soundness comes from Z3).
//
// Per layer, with h the fp32 inputs and e a bound on |h_exact - h|:
//     z = W^T h + b                                   (MFMA fma chain, one rounding per product)
//     d = (|W|^T (e + g|h|)) (1 + 2g) + g|b| + g1|z|  (g = gamma(K) of the GEMM, g1 = gamma(1))
// so |v_exact - z| <= d.  ReLU is 1-Lipschitz: h' = max(z, 0), e' = d — except that a neuron
// with z + d <= 0 (or forced dead) is exactly 0 with e' = 0, which keeps the exact zeros of
// sign-structured sums exact.  Output: [z - d, z + d].
//
// Layout (same as the symbolic kernel, csrc/symbolic.hip): one wave64 owns 16 points = the 16
// columns of v_mfma_f32_16x16x4_f32 tiles whose rows are neurons; the accumulator tile of layer
// l is the B operand of layer l+1 (reg i of tile t = neuron 16t + 4*(lane>>4) + i), W is staged
// once per workgroup in LDS in MFMA operand order.  Two products per K step: W.h and
// |W|.(e + g|h|); the epilogue is purely elementwise (no cross-lane traffic).
#include <hip/hip_runtime.h>

#include "launch.h"
#include "pointfwd.h"

// 7-tile nets: 260 -> 254 VGPRs (spill-free) doubles the waves per SIMD (1 -> 2)
template <int TM>
__global__ void __launch_bounds__(FA_THREADS) __attribute__((amdgpu_waves_per_eu(TM == 7 ? 2 : 1))) fa_point_kernel(NetDesc net, BoundArgs a, PointCfg cfg) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x;
  // BaB level: most nodes of a level are closed, and a workgroup none of whose tiles has an open
  // point would stage the whole weight block (63 KB for AC-4) to write nothing.  One pass over
  // row_open for the tiles of its grid-stride loop; the verdict is uniform over the workgroup.
  if (a.row_open) {
    const int nw = FA_THREADS / 64;
    const int ntile = (a.R + 15) >> 4;
    int any = 0;
    for (int tile = blockIdx.x * nw + (tid >> 6); tile < ntile; tile += gridDim.x * nw) {
      const int p = tile * 16 + (tid & 15);
      any |= p < a.R && a.row_open[p % a.open_mod];
    }
    if (!__syncthreads_or(any)) return;
  }
  // ---- stage the MFMA-operand-order weights + biases (pre-permuted in `flat`) into LDS
  {
    const float4* src = reinterpret_cast<const float4*>(a.flat + net.wperm_off);
    float4* dst = reinterpret_cast<float4*>(smem);
    for (int e = tid; e < (net.wperm_floats >> 2); e += FA_THREADS) dst[e] = src[e];
    for (int l = 0; l < net.n_layers; ++l) {
      const int n_out = net.dims[l + 1];
      const float* b = a.flat + net.wperm_off + cfg.b_lds[l];
      for (int j = tid; j < ((n_out + 15) & ~15); j += FA_THREADS) smem[cfg.bp_lds[l] + j] = j < n_out ? b[j] : 0.f;
    }
  }
  __syncthreads();
  const int lane = tid & 63, col = lane & 15, grp = lane >> 4;
  const int wave = tid >> 6, nw = FA_THREADS / 64;
  const int n0 = net.dims[0];
  const int tin0 = (n0 + 15) >> 4;
  const float g0 = net.g_fwd[0];
  const int ntile = (a.R + 15) >> 4;
  for (int tile = blockIdx.x * nw + wave; tile < ntile; tile += gridDim.x * nw) {
    const int p0 = tile * 16;
    const int p = p0 + col;
    if (a.row_open && !__any(p < a.R && a.row_open[p % a.open_mod])) continue;   // wave-uniform
    float HA[TM][4], EA[TM][4], HB[TM][4], EB[TM][4];
#pragma unroll
    for (int t = 0; t < TM; ++t) {
      if (t >= tin0) break;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k = 16 * t + 4 * grp + i;
        const float x = (k < n0 && p < a.R) ? a.lo[(size_t)p * n0 + k] : 0.f;
        HA[t][i] = x;
        EA[t][i] = g0 * fabsf(x);      // inputs are exact: only the GEMM rounding term
      }
    }
    for (int l = 0; l < net.n_layers; ++l) {
      if (l & 1) fa_point_layer<TM>(net, a, cfg, smem, l, p0, lane, HB, EB, HA, EA);
      else fa_point_layer<TM>(net, a, cfg, smem, l, p0, lane, HA, EA, HB, EB);
    }
  }
}

namespace {
typedef void (*PointKernel)(NetDesc, BoundArgs, PointCfg);

// the run-time-shape instances, one per TM bucket (launch.h fa_tm_bucket).  10 is BM-4's 150-wide
// layer: the unroller gives up on the 10x10-tile body and the operand arrays live in scratch
// (656 B/lane), still far cheaper than the IBP fallback, which stages each layer's W per box row
// (one 90 KB row per workgroup: G = 1)
#define FA_POINT_TMS(X) X(1) X(2) X(4) X(7) X(10)

PointKernel select_point(int TM) {
  switch (fa_tm_bucket(TM)) {
#define FA_POINT_CASE(T) \
  case T: return fa_point_kernel<T>;
    FA_POINT_TMS(FA_POINT_CASE)
#undef FA_POINT_CASE
    default: return nullptr;   // wider layers: the caller falls back to IBP
  }
}
}  // namespace

// Rigorous point forward over a.R points a.lo [R, n0] (a.hi ignored); writes a.out_lb/out_ub.
// Honours a.dead_in (per point) or a.dead_part + a.node_part (per point's partition).
// Returns 1 if launched, 0 if the shape is unsupported (caller falls back), <0 on error.
extern "C" int fa_point_try_launch(const NetDesc& net, BoundArgs a, hipStream_t stream) {
  if (a.R <= 0) return 1;
  PointKernel k = select_point(fa_widest_tiles(net, 0, net.n_layers));
  if (!k) return 0;
  PointCfg cfg{};
  int off = fa_lay_weights(net, net.n_layers, cfg.w_lds, 0);
  off = fa_lay_biases(net, net.n_layers, cfg.b_lds, off);
  if (((off + 3) & ~3) != net.wperm_floats) return -1;   // layout mismatch with the pre-permuted block
  if ((size_t)net.wperm_floats * sizeof(float) > 150 * 1024) return 0;
  off = net.wperm_floats;
  for (int l = 0; l < net.n_layers; ++l) {
    cfg.bp_lds[l] = off;
    off += fa_tiles(net.dims[l + 1]) * 16;
  }
  const size_t bytes = (size_t)off * sizeof(float);   // <= 150 KB + 16 layers x 10 tiles x 64 B
  const int per_cu = fa_blocks_per_cu((const void*)k, FA_THREADS, bytes);
  if (!per_cu) return -4;
  const long long tiles = (a.R + 15) / 16;
  long long blocks = (tiles + 3) / 4;
  const long long cap = (long long)fa_device_cus() * per_cu;
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(FA_THREADS), bytes, stream, net, a, cfg);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 1 : -(int)e;
}

#define FA_POINT_LDS(T) FA_LDS_K(fa_point_kernel<T>),
FA_LDS_REGISTER(FA_POINT_TMS(FA_POINT_LDS));
#undef FA_POINT_LDS
