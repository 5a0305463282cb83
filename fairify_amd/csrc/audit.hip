// Audit of real individuals: per-row discrimination masks from the rigorous point forward.  gfx950.
//
// Definitions: ops/audit.py, docs/DESIGN.md 5f.  Row i of x [N, n0] (integral, from HBM) is one
// individual; own[i] is the index of its PA coordinates in the PA-domain table `values` (-1: outside
// the PA domain, all outputs 0).  Its counterparts are the row with PA := values[v'] for every v' the
// pair table allows after own[i], and RA += e for EVERY offset vector e in {-tau..tau}^nra (row-major
// over ra_idx, unclipped; E = 1 and no shift for a PA-only query).  With [l, u] the rigorous logit
// bounds of the own row and [l', u'] of a counterpart (csrc/pointfwd.h):
//     cert bit v'   some e has  u < 0 < l'  or  l > 0 > u'      (=> exact flip => poss bit v')
//     poss bit v'   some e has  l < 0 < u'  or  u > 0 > l'
//     own_sign      -1 if u < 0, +1 if l > 0, else 0.
// The host decides the bits poss & ~cert exactly (engine/audit.py).
//
// Work shape: csrc/rowfwd.h; a workgroup walks the 64-row passes blockIdx.x, blockIdx.x + gridDim.x, ...
// ONE x row per individual, forwarded once, its [l, u] kept in registers; every (v', e) counterpart
// streams through the same forward into the wave's single slab row and is tested on the spot through
// the V x V pair table in LDS, indexed by the column's own value.  Outputs are per row: no atomics.
#include <hip/hip_runtime.h>

#include "rowfwd.h"

// Waves per SIMD asked of the compiler, from its resource remarks (the table in docs/DESIGN.md 5f):
// with at most 64 KB of LDS two workgroups fit a CU, and up to 7 tiles two waves per SIMD cost no
// scratch (1 - 4 tiles) or 80 B/lane (7 tiles; the rate instance spills 120 B there).  The 10-tile
// instance spills 356 B/lane at two waves and 12 B/lane at one, like the rate instance: one wave.
template <int TM>
__global__ void __launch_bounds__(FA_THREADS) __attribute__((amdgpu_waves_per_eu(TM == 10 ? 1 : 2)))
fa_audit_kernel(NetDesc net, AuditArgs a, RegNetCfg rc) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int XT = TM < 2 ? TM : 2;     // input tiles kept per row: n0 <= 32 (the launch refuses wider)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, grp = lane >> 4;
  const int n0 = net.dims[0];
  const int V = a.V, E = a.E;
  // LDS after the staged block: one slab row [lb x 16 | ub x 16] per wave (the row in flight), the
  // pair table
  float* slab = smem + rc.floats + wave * 32;
  uint8_t* valid = (uint8_t*)(smem + rc.floats + (FA_THREADS / 64) * 32);       // [V][V]
  fa_stage_wperm(net, rc, a.flat, smem, tid, FA_THREADS);
  fa_stage_pair_table(a, valid, tid);
  FaRowSlots<XT> slots;       // this lane's PA / RA slots, fixed for the launch
  fa_row_slots<XT>(a, grp, slots);
  // the layer function's view of the slab row: 16 points, lower bounds then upper bounds
  BoundArgs ba{};
  ba.R = 16;
  const float g0 = net.g_fwd[0];
  float Xb[XT][4], HA[TM][4], EA[TM][4], HB[TM][4], EB[TM][4];
  const int passes = (a.N + 63) / 64;
  for (int ps = blockIdx.x; ps < passes; ps += gridDim.x) {
    const int row = ps * 64 + wave * 16 + col;
    const bool rv = row < a.N;
    const int own = rv ? a.own[row] : -1;
    const bool ov = own >= 0 && own < V;
    const int oi = ov ? own : 0;            // a row that is not audited reads table row 0, and ignores it
#pragma unroll
    for (int t = 0; t < XT; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k = 16 * t + 4 * grp + i;
        Xb[t][i] = (k < n0 && rv) ? a.x[(size_t)row * n0 + k] : 0.f;
      }
    // rigorous forward of the 16 rows (PA assignment v or -1: the row's own, offset vector e or -1)
    // into the slab row
    auto run_row = [&](int v, int e) {
      fa_row_forward<TM>(net, ba, rc, smem, lane, Xb, g0, FaQueryCoord<XT, AuditArgs>{a, slots, v, e}, slab, HA, EA, HB, EB);
    };
    run_row(-1, -1);
    // the slab row is written by lanes 0..15 and read back by the same lane only: the masks live in
    // the grp == 0 lanes (the other lanes keep 0)
    float lo_x = 0.f, up_x = 0.f;
    if (grp == 0) {
      lo_x = slab[col];
      up_x = slab[16 + col];
    }
    unsigned cert = 0, poss = 0;
    for (int vp = 0; vp < V; ++vp) {
      const bool vld = grp == 0 && ov && valid[oi * V + vp] != 0;
      for (int e = 0; e < E; ++e) {
        // wave-uniform skip that changes no output: no column has v' valid, or every valid column
        // already has its cert bit (which the same e set in poss too)
        if (__ballot(vld && !((cert >> vp) & 1u)) == 0) break;
        run_row(vp, e);
        if (vld) {
          const float lp = slab[col], up = slab[16 + col];
          if ((up_x < 0.f && lp > 0.f) || (lo_x > 0.f && up < 0.f)) cert |= 1u << vp;
          if ((lo_x < 0.f && up > 0.f) || (up_x > 0.f && lp < 0.f)) poss |= 1u << vp;
        }
      }
    }
    if (grp == 0 && rv) {
      a.cert[row] = ov ? (int)cert : 0;
      a.poss[row] = ov ? (int)poss : 0;
      a.own_sign[row] = (int8_t)(!ov ? 0 : up_x < 0.f ? -1 : lo_x > 0.f ? 1 : 0);
    }
  }
}

// Dynamic LDS of one workgroup: the staged block, one slab row per wave, the pair table.
static size_t audit_lds_bytes(const AuditArgs& a, const RegNetCfg& rc) {
  const size_t floats = (size_t)rc.floats + (size_t)(FA_THREADS / 64) * 32;
  return (floats * sizeof(float) + (size_t)a.V * a.V + 15) & ~(size_t)15;
}

// Writes cert / poss / own_sign of a.N rows.  Returns 0 if launched, -3 for shapes the kernel does not
// cover (a layer over 160 wide, inputs over 32 wide, V or E over 32, or more than 64 KB of dynamic LDS:
// the instances are not in the raised-limit registry, docs/DESIGN.md 5f), -2 for a bad workgroup count,
// > 0 a HIP error.
extern "C" int fa_audit_launch(const NetDesc& net, AuditArgs a, hipStream_t stream) {
  if (a.N <= 0) return 0;
  if (!fa_row_query_ok(net, a)) return -3;
  RegNetCfg rc{};
  void (*k)(NetDesc, AuditArgs, RegNetCfg) = nullptr;
  switch (fa_row_net(net, rc)) {
#define FA_AUDIT_CASE(T) \
  case T: k = fa_audit_kernel<T>; break;
    FA_ROW_TMS(FA_AUDIT_CASE)
#undef FA_AUDIT_CASE
    default: return -3;
  }
  const size_t bytes = audit_lds_bytes(a, rc);
  if (bytes > 64 * 1024) return -3;
  const int passes = (a.N + 63) / 64;
  if (a.blocks < 1 || a.blocks > passes) return -2;
  hipLaunchKernelGGL(k, dim3((unsigned)a.blocks), dim3(FA_THREADS), bytes, stream, net, a, rc);
  return (int)hipGetLastError();
}
