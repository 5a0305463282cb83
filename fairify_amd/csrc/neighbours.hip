// Single-attribute neighbourhood of real individuals: per (row, neighbour) discrimination bits from
// the rigorous point forward.  gfx950.
//
// Definitions: ops/neighbours.py, docs/DESIGN.md 5g.  Row i of x [N, n0] is one individual, own[i]
// its index in the PA-domain table (csrc/audit.hip).  Table entry j = (dim, off, abs) names the
// neighbour z of a row: z = x with z[dim] := c, c = off (abs) or x[dim] + off (relative).  The
// neighbour is valid when dom_lo[dim] <= c <= dom_hi[dim], c != x[dim] and |c - x[dim]| <=
// radius[dim].  With [l, u] the rigorous logit bounds of z and [l', u'] of a counterpart of z
// (PA := values[v'] for every v' the pair table allows after own[i], RA += every offset vector e):
//     cert bit j   valid, and some (v', e) has  u < 0 < l'  or  l > 0 > u'   (=> poss bit j)
//     poss bit j   valid, and some (v', e) has  l < 0 < u'  or  u > 0 > l'
// Bit j sits in word j / 32 at bit j % 32 of cert / poss [N, W].  The host decides poss & ~cert
// exactly (engine/neighbours.py).
//
// Work shape: csrc/rowfwd.h, one slab row per wave like the audit kernel.  A work item is (64-row pass, word):
// items are strided over blockIdx.x, so a short table of rows with a long neighbour table still
// fills the device.  The up to 32 neighbours of a word are walked wave-uniformly; each grp == 0 lane
// builds its row's two words in registers and stores them once.  No atomics.
#include <hip/hip_runtime.h>

#include "rowfwd.h"

// Waves per SIMD: the audit instances' values (docs/DESIGN.md 5g has the resource remarks of both).  No
// scratch up to four tiles; the 7-tile instance spills 328 B/lane at two waves and 12 B/lane at one, and
// measured 14 % faster at two (profiles/r19/neighbours/README.md).
template <int TM>
__global__ void __launch_bounds__(FA_THREADS) __attribute__((amdgpu_waves_per_eu(TM == 10 ? 1 : 2)))
fa_neighbour_kernel(NetDesc net, NeighbourArgs a, RegNetCfg rc) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int XT = TM < 2 ? TM : 2;     // input tiles kept per row: n0 <= 32 (the launch refuses wider)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, grp = lane >> 4;
  const int n0 = net.dims[0];
  const int V = a.V, E = a.E;
  float* slab = smem + rc.floats + wave * 32;
  uint8_t* valid = (uint8_t*)(smem + rc.floats + (FA_THREADS / 64) * 32);       // [V][V]
  fa_stage_wperm(net, rc, a.flat, smem, tid, FA_THREADS);
  fa_stage_pair_table(a, valid, tid);
  FaRowSlots<XT> slots;       // this lane's PA / RA slots, fixed for the launch
  fa_row_slots<XT>(a, grp, slots);
  BoundArgs ba{};
  ba.R = 16;
  const float g0 = net.g_fwd[0];
  float Xb[XT][4], HA[TM][4], EA[TM][4], HB[TM][4], EB[TM][4];
  const int passes = (a.N + 63) / 64;
  const long long items = (long long)passes * a.W;
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    const int ps = (int)(it / a.W), w = (int)(it % a.W);
    const int row = ps * 64 + wave * 16 + col;
    const bool rv = row < a.N;
    const int own = rv ? a.own[row] : -1;
    const bool ov = own >= 0 && own < V;
    const int oi = ov ? own : 0;
#pragma unroll
    for (int t = 0; t < XT; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k = 16 * t + 4 * grp + i;
        Xb[t][i] = (k < n0 && rv) ? a.x[(size_t)row * n0 + k] : 0.f;
      }
    // rigorous forward of the 16 columns' neighbour through coordinate kd (set to cf, or moved by cf
    // when relative), with PA assignment v (-1: the row's own) and offset vector e (-1: none), into
    // the slab row
    auto run_row = [&](int kd, float cf, bool isabs, int v, int e) {
      const FaQueryCoord<XT, NeighbourArgs> query{a, slots, v, e};
      auto coord = [&](int t, int i, float x) {
        if (16 * t + 4 * grp + i == kd) x = isabs ? cf : x + cf;
        return query(t, i, x);
      };
      fa_row_forward<TM>(net, ba, rc, smem, lane, Xb, g0, coord, slab, HA, EA, HB, EB);
    };
    unsigned cw = 0, pw = 0;
    const int j1 = min(a.M, 32 * w + 32);
    for (int j = 32 * w; j < j1; ++j) {
      // the table entry and its dimension's range and radius: wave-uniform addresses
      const int kd = a.nb_dim[j], off = a.nb_off[j];
      const bool isabs = a.nb_abs[j] != 0;
      if (kd < 0 || kd >= n0) continue;
      const int dlo = a.dom_lo[kd], dhi = a.dom_hi[kd], rad = a.radius[kd];
      // validity of this column's neighbour, in the grp == 0 lane (the row's line is in L1)
      bool nv = false;
      if (grp == 0 && ov) {
        const long long xk = (long long)a.x[(size_t)row * n0 + kd];
        const long long c = isabs ? (long long)off : xk + off;
        const long long d = c > xk ? c - xk : xk - c;
        nv = c >= dlo && c <= dhi && d != 0 && d <= (long long)rad;
      }
      const unsigned bit = 1u << (j & 31);
      // wave-uniform skips that change no output: no column has a valid neighbour here, or every
      // valid column already has its cert bit (which the same counterpart set in poss too)
      if (__ballot(nv) == 0) continue;
      const float cf = (float)off;
      run_row(kd, cf, isabs, -1, -1);
      float lo_z = 0.f, up_z = 0.f;
      if (grp == 0) {
        lo_z = slab[col];
        up_z = slab[16 + col];
      }
      for (int vp = 0; vp < V; ++vp) {
        if (__ballot(nv && !(cw & bit)) == 0) break;
        const bool vld = nv && valid[oi * V + vp] != 0;
        for (int e = 0; e < E; ++e) {
          if (__ballot(vld && !(cw & bit)) == 0) break;
          run_row(kd, cf, isabs, vp, e);
          if (vld) {
            const float lp = slab[col], up = slab[16 + col];
            if ((up_z < 0.f && lp > 0.f) || (lo_z > 0.f && up < 0.f)) cw |= bit;
            if ((lo_z < 0.f && up > 0.f) || (up_z > 0.f && lp < 0.f)) pw |= bit;
          }
        }
      }
    }
    if (grp == 0 && rv) {
      a.cert[(size_t)row * a.W + w] = (int)cw;
      a.poss[(size_t)row * a.W + w] = (int)pw;
    }
  }
}

// Dynamic LDS of one workgroup: the staged block, one slab row per wave, the pair table.
static size_t neighbour_lds_bytes(const NeighbourArgs& a, const RegNetCfg& rc) {
  const size_t floats = (size_t)rc.floats + (size_t)(FA_THREADS / 64) * 32;
  return (floats * sizeof(float) + (size_t)a.V * a.V + 15) & ~(size_t)15;
}

// Writes cert / poss [N, W].  Returns 0 if launched, -3 for shapes the kernel does not cover (the audit
// launcher's conditions: a layer over 160 wide, inputs over 32 wide, V or E over 32, or more than 64 KB
// of dynamic LDS -- the instances are not in the raised-limit registry, docs/DESIGN.md 5g), -2 for a
// workgroup count outside 1 .. passes x W, > 0 a HIP error.
extern "C" int fa_neighbour_launch(const NetDesc& net, NeighbourArgs a, hipStream_t stream) {
  if (a.N <= 0 || a.M <= 0) return 0;
  if (!fa_row_query_ok(net, a) || a.W != (a.M + 31) / 32) return -3;
  RegNetCfg rc{};
  void (*k)(NetDesc, NeighbourArgs, RegNetCfg) = nullptr;
  switch (fa_row_net(net, rc)) {
#define FA_NEIGHBOUR_CASE(T) \
  case T: k = fa_neighbour_kernel<T>; break;
    FA_ROW_TMS(FA_NEIGHBOUR_CASE)
#undef FA_NEIGHBOUR_CASE
    default: return -3;
  }
  const size_t bytes = neighbour_lds_bytes(a, rc);
  if (bytes > 64 * 1024) return -3;
  const long long items = (long long)((a.N + 63) / 64) * a.W;
  if (a.blocks < 1 || a.blocks > items) return -2;
  hipLaunchKernelGGL(k, dim3((unsigned)a.blocks), dim3(FA_THREADS), bytes, stream, net, a, rc);
  return (int)hipGetLastError();
}
