// Discrimination-rate measurement: rigorous flip classification of sampled profiles.  gfx950.
//
// Per partition, n_samples profiles come from the simulation stage's counter-hash stream
// (fa_sample_coord, identical to ops/reference.py:sample_points) and never touch HBM.  A profile's
// x rows are the sample with its PA coordinates overwritten by each of the V PA assignments; its
// counterpart rows x' are the x rows themselves (PA-only query) or the x rows with the RA
// coordinates shifted by EVERY offset vector e in {-tau..tau}^nra (row-major over ra_idx,
// unclipped).  Every row goes through the rigorous point forward (csrc/pointfwd.h: fp32 logit +-
// the running Higham bound, exact zeros kept exact) and a profile is
//     certain   if some valid pair (v, v') and offset e have  u_x(v) < 0 < l_x'(v', e)  or
//               l_x(v) > 0 > u_x'(v', e);
//     possible  the same with  l_x(v) < 0 < u_x'(v', e)  or  u_x(v) > 0 > l_x'(v', e);
//     ambiguous = possible and not certain           (certain => exact flip => possible).
// Outputs per partition: the number of certain profiles, the number of ambiguous ones and up to
// FA_RATE_SLOTS of their sample indices (slots reserved with an integer atomic; the host decides
// those profiles exactly, engine/rate.py).  Integer atomics only: the counts are deterministic.
//
// Work shape: csrc/rowfwd.h, with a.split workgroups per partition.  Per pass the V x rows are
// forwarded first and their [l, u] kept in a wave-private LDS slab; then (relaxed) the E*V counterpart
// rows stream through the same forward into one more slab row and are tested on the spot against the
// stored x bounds -- nothing of size E*V is stored.  PA-only: the stored rows are tested against each
// other, one pass.
#include <hip/hip_runtime.h>

#include "rowfwd.h"

// 7-tile nets: two waves per SIMD like the point kernel (two AC-4 workgroups fit a CU's LDS), with
// 120 B/lane of scratch; one wave per SIMD measured slower (AC-4: 15.8 against 11.4 ms,
// profiles/r10/rate/README.md)
#ifndef FA_RATE_WPE7
#define FA_RATE_WPE7 2
#endif

template <int TM>
__global__ void __launch_bounds__(FA_THREADS) __attribute__((amdgpu_waves_per_eu(TM == 7 ? FA_RATE_WPE7 : 1)))
fa_rate_kernel(NetDesc net, RateArgs a, RegNetCfg rc) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int XT = TM < 2 ? TM : 2;     // input tiles kept per profile: n0 <= 32 (the launch refuses wider)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, grp = lane >> 4;
  const int n0 = net.dims[0];
  const int G = a.split;
  const int p = blockIdx.x / G;
  const int g = blockIdx.x - p * G;
  const int V = a.V, E = a.E;
  const bool rx = a.nra > 0;
  const int64_t pid = a.pids[p];
  // LDS after the staged block: per wave V + 1 slab rows of [lb x 16 | ub x 16] (row V: the
  // counterpart row in flight), the box, the certain counter, the pair table
  float* slab = smem + rc.floats + wave * (V + 1) * 32;
  float* s_lo = smem + rc.floats + (FA_THREADS / 64) * (V + 1) * 32;
  float* s_hi = s_lo + n0;
  int* cnt = (int*)(s_hi + n0);
  uint8_t* valid = (uint8_t*)(cnt + 1);       // [V][V]
  fa_stage_wperm(net, rc, a.flat, smem, tid, FA_THREADS);
  for (int i = tid; i < n0; i += FA_THREADS) {
    s_lo[i] = a.lo[(size_t)p * n0 + i];
    s_hi[i] = a.hi[(size_t)p * n0 + i];
  }
  if (tid == 0) cnt[0] = 0;
  fa_stage_pair_table(a, valid, tid);
  FaRowSlots<XT> slots;       // this lane's PA / RA slots, fixed for the launch
  fa_row_slots<XT>(a, grp, slots);
  // the layer function's view of one slab row: 16 points, lower bounds then upper bounds
  BoundArgs ba{};
  ba.R = 16;
  const float g0 = net.g_fwd[0];
  float Xb[XT][4], HA[TM][4], EA[TM][4], HB[TM][4], EB[TM][4];
  int ncert = 0;
  for (int s0 = g * 64; s0 < a.n_samples; s0 += G * 64) {
    const int s = s0 + wave * 16 + col;
    const bool sv = s < a.n_samples;
#pragma unroll
    for (int t = 0; t < XT; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k = 16 * t + 4 * grp + i;
        Xb[t][i] = (k < n0 && sv) ? fa_sample_coord(a.seed, pid, s, k, s_lo[k], s_hi[k]) : 0.f;
      }
    // rigorous forward of the 16 profiles' row (PA assignment v, offset vector e or -1) into slab row r
    // (fa_row_forward's body, kept in place: called as a function, the 1-tile instance took two more
    // VGPRs and lost its sixth wave per SIMD, profiles/r22/rowfwd/README.md)
    auto run_row = [&](int v, int e, int r) {
      const FaQueryCoord<XT, RateArgs> coord{a, slots, v, e};
#pragma unroll
      for (int t = 0; t < XT; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float x = coord(t, i, Xb[t][i]);
          HA[t][i] = x;
          EA[t][i] = g0 * fabsf(x);      // inputs are exact: only the GEMM rounding term
        }
      ba.out_lb = slab + r * 32;
      ba.out_ub = slab + r * 32 + 16;
      for (int l = 0; l < net.n_layers; ++l) {
        if (l & 1) fa_point_layer<TM>(net, ba, rc, smem, l, 0, lane, HB, EB, HA, EA);
        else fa_point_layer<TM>(net, ba, rc, smem, l, 0, lane, HA, EA, HB, EB);
      }
    };
    for (int v = 0; v < V; ++v) run_row(v, -1, v);
    // a slab row is written by lanes 0..15 and read back by the same lane only
    bool cert = false, poss = false;
    auto test_row = [&](int vp, int r) {
      const float lp = slab[r * 32 + col], up = slab[r * 32 + 16 + col];
      for (int v = 0; v < V; ++v) {
        if (!valid[v * V + vp]) continue;
        const float lv = slab[v * 32 + col], uv = slab[v * 32 + 16 + col];
        cert = cert || (uv < 0.f && lp > 0.f) || (lv > 0.f && up < 0.f);
        poss = poss || (lv < 0.f && up > 0.f) || (uv > 0.f && lp < 0.f);
      }
    };
    if (!rx) {
      if (grp == 0)
        for (int vp = 0; vp < V; ++vp) test_row(vp, vp);
    } else {
      for (int e = 0; e < E; ++e)
        for (int vp = 0; vp < V; ++vp) {
          run_row(vp, e, V);
          if (grp == 0) test_row(vp, V);
        }
    }
    if (grp == 0 && sv) {
      if (cert) {
        ++ncert;
      } else if (poss) {
        const int slot = atomicAdd(&a.amb[p], 1);
        if (slot < FA_RATE_SLOTS) a.amb_idx[(size_t)p * FA_RATE_SLOTS + slot] = s;
      }
    }
  }
  ncert += __shfl_xor(ncert, 1);
  ncert += __shfl_xor(ncert, 2);
  ncert += __shfl_xor(ncert, 4);
  ncert += __shfl_xor(ncert, 8);
  if (lane == 0 && ncert) atomicAdd(cnt, ncert);
  __syncthreads();
  if (tid == 0 && cnt[0]) atomicAdd(&a.flips[p], cnt[0]);
}

// Dynamic LDS of one workgroup, or 0 when the shape is not covered.
static size_t rate_lds_bytes(const NetDesc& net, const RateArgs& a, const RegNetCfg& rc) {
  const size_t floats = (size_t)rc.floats + (size_t)(FA_THREADS / 64) * (a.V + 1) * 32 + 2 * (size_t)net.dims[0];
  const size_t bytes = floats * sizeof(float) + sizeof(int) + (size_t)a.V * a.V;
  return (bytes + 15) & ~(size_t)15;
}

// Counts certain / ambiguous profiles of a.P partitions into a.flips / a.amb / a.amb_idx (the caller
// zero-initialises the two counters).  Returns 0 if launched, -3 for shapes the kernel does not
// cover (a layer over 160 wide, inputs over 32 wide, V or E over 32), -2 for a bad split, -4 when
// the dynamic-LDS limits were not prepared, > 0 a HIP error.
extern "C" int fa_rate_launch(const NetDesc& net, RateArgs a, hipStream_t stream) {
  if (a.P <= 0 || a.n_samples <= 0) return 0;
  if (!fa_row_query_ok(net, a)) return -3;
  RegNetCfg rc{};
  void (*k)(NetDesc, RateArgs, RegNetCfg) = nullptr;
  switch (fa_row_net(net, rc)) {
#define FA_RATE_CASE(T) \
  case T: k = fa_rate_kernel<T>; break;
    FA_ROW_TMS(FA_RATE_CASE)
#undef FA_RATE_CASE
    default: return -3;
  }
  const size_t bytes = rate_lds_bytes(net, a, rc);
  if (bytes > 160 * 1024) return -3;
  const int tiles = (a.n_samples + 63) / 64;
  if (a.split < 1 || a.split > tiles) return -2;
  if ((long long)a.P * a.split > 0x7FFFFFFFLL) return -2;
  if (!fa_lds_ok(bytes)) return -4;
  hipLaunchKernelGGL(k, dim3((unsigned)a.P * (unsigned)a.split), dim3(FA_THREADS), bytes, stream, net, a, rc);
  return (int)hipGetLastError();
}

#define FA_RATE_LDS(T) FA_LDS_K(fa_rate_kernel<T>),
FA_LDS_REGISTER(FA_ROW_TMS(FA_RATE_LDS));
#undef FA_RATE_LDS
