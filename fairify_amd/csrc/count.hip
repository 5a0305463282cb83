// Counting branch-and-bound over a partition's non-PA lattice (definitions: ops/count.py, DESIGN
// 5e).  gfx950.
//
// fa_count_enum_kernel   leaf enumeration, the hot path: every lattice point of a small box is
//                        classified like a discrimination-rate profile (csrc/rate.hip), the
//                        coordinates from the leaf's mixed-radix decode instead of the hash stream.
//                        Work shape: csrc/rowfwd.h.
// fa_count_rows_kernel   node boxes -> x rows (PA dims pinned) and widened counterpart rows.
// fa_count_level_kernel  one node per lane: box test over the pair list, int64 volume sums, leaf
//                        list and child pool slots reserved with one atomic per wave.
// The bound kernels (bounds.hip / symbolic.hip / crown.hip) run unchanged between the last two.
#include <hip/hip_runtime.h>

#include "rowfwd.h"
#include "wave.h"

// ---- leaf enumeration ------------------------------------------------------------------------
// A workgroup walks the leaves blockIdx.x, blockIdx.x + gridDim.x, ...: W is staged once for many
// small leaves.  Per leaf the widths and digit strides of its dims sit in LDS.  A leaf belongs to
// one workgroup, so its outputs do not depend on the grid size.
template <int TM>
__global__ void __launch_bounds__(FA_THREADS) __attribute__((amdgpu_waves_per_eu(TM == 7 ? 2 : 1)))
fa_count_enum_kernel(NetDesc net, EnumArgs a, RegNetCfg rc) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int XT = TM < 2 ? TM : 2;     // input tiles kept per point: n0 <= 32 (the launch refuses wider)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, grp = lane >> 4;
  const int n0 = net.dims[0];
  const int V = a.V, E = a.E;
  const bool rx = a.nra > 0;
  // LDS after the staged block: per wave V + 1 slab rows of [lb x 16 | ub x 16] (row V: the
  // counterpart row in flight), the leaf's lo / width / stride per dim, the certain counter and the
  // volume, the pair table
  float* slab = smem + rc.floats + wave * (V + 1) * 32;
  float* s_lo = smem + rc.floats + (FA_THREADS / 64) * (V + 1) * 32;
  int* s_w = (int*)(s_lo + n0);
  int* s_st = s_w + n0;
  int* cnt = s_st + n0;                       // [0] certain points, [1] the leaf's volume (0: skipped)
  uint8_t* valid = (uint8_t*)(cnt + 2);       // [V][V]
  fa_stage_wperm(net, rc, a.flat, smem, tid, FA_THREADS);
  fa_stage_pair_table(a, valid, tid);
  FaRowSlots<XT> slots;       // this lane's PA / RA slots, fixed for the launch
  fa_row_slots<XT>(a, grp, slots);
  BoundArgs ba{};
  ba.R = 16;
  const float g0 = net.g_fwd[0];
  float Xb[XT][4], HA[TM][4], EA[TM][4], HB[TM][4], EB[TM][4];
  for (int leaf = blockIdx.x; leaf < a.L; leaf += gridDim.x) {
    __syncthreads();     // the previous leaf's table and counter are no longer read
    if (tid == 0) {
      const int v = fa_enum_decode(a, leaf, n0, s_lo, s_w, s_st);
      cnt[0] = 0;
      cnt[1] = v;
      if (!v) a.cert[leaf] = -1;
    }
    __syncthreads();
    const int vol = cnt[1];
    int ncert = 0;
    for (int s0 = 0; s0 < vol; s0 += FA_THREADS / 4) {
      const int s = s0 + wave * 16 + col;
      const bool sv = s < vol;
      fa_enum_point<XT>(Xb, s, sv, grp, n0, s_lo, s_w, s_st);
      // rigorous forward of the 16 points' row (PA assignment v, offset vector e or -1) into slab row r
      auto run_row = [&](int v, int e, int r) {
        fa_row_forward<TM>(net, ba, rc, smem, lane, Xb, g0, FaQueryCoord<XT, EnumArgs>{a, slots, v, e}, slab + r * 32, HA,
                           EA, HB, EB);
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
          const int slot = atomicAdd(&a.amb[leaf], 1);
          if (slot < FA_RATE_SLOTS) a.amb_idx[(size_t)leaf * FA_RATE_SLOTS + slot] = s;
        }
      }
    }
    ncert += __shfl_xor(ncert, 1);
    ncert += __shfl_xor(ncert, 2);
    ncert += __shfl_xor(ncert, 4);
    ncert += __shfl_xor(ncert, 8);
    if (lane == 0 && ncert) atomicAdd(cnt, ncert);
    __syncthreads();
    if (tid == 0 && vol) a.cert[leaf] = cnt[0];
  }
}

static size_t enum_lds_bytes(const NetDesc& net, const EnumArgs& a, const RegNetCfg& rc) {
  const size_t words = (size_t)rc.floats + (size_t)(FA_THREADS / 64) * (a.V + 1) * 32 + 3 * (size_t)net.dims[0] + 2;
  const size_t bytes = words * sizeof(float) + (size_t)a.V * a.V;
  return (bytes + 15) & ~(size_t)15;
}

// Enumerates a.L leaves into a.cert / a.amb / a.amb_idx (the caller zero-initialises amb).  Returns 0
// if launched, -3 for shapes the kernel does not cover (a layer over 160 wide, inputs over 32 wide, V
// or E over 32, a leaf volume bound over 65 536), -2 for a bad workgroup count, -4 when the
// dynamic-LDS limits were not prepared, > 0 a HIP error.
extern "C" int fa_count_enum_launch(const NetDesc& net, EnumArgs a, hipStream_t stream) {
  if (a.L <= 0) return 0;
  if (!fa_row_query_ok(net, a)) return -3;
  if (a.max_vol < 1 || a.max_vol > FA_COUNT_MAX_VOL) return -3;
  RegNetCfg rc{};
  void (*k)(NetDesc, EnumArgs, RegNetCfg) = nullptr;
  switch (fa_row_net(net, rc)) {
#define FA_ENUM_CASE(T) \
  case T: k = fa_count_enum_kernel<T>; break;
    FA_ROW_TMS(FA_ENUM_CASE)
#undef FA_ENUM_CASE
    default: return -3;
  }
  const size_t bytes = enum_lds_bytes(net, a, rc);
  if (bytes > 160 * 1024) return -3;
  if (a.blocks < 1 || a.blocks > a.L) return -2;
  if (!fa_lds_ok(bytes)) return -4;
  hipLaunchKernelGGL(k, dim3((unsigned)a.blocks), dim3(FA_THREADS), bytes, stream, net, a, rc);
  return (int)hipGetLastError();
}

#define FA_ENUM_LDS(T) FA_LDS_K(fa_count_enum_kernel<T>),
FA_LDS_REGISTER(FA_ROW_TMS(FA_ENUM_LDS));
#undef FA_ENUM_LDS

// ---- row expansion ---------------------------------------------------------------------------
// One thread per row element: row r = node r / V with PA assignment r % V.
__global__ void __launch_bounds__(FA_THREADS) fa_count_rows_kernel(CountArgs a) {
  const long long total = (long long)a.N * a.V * a.n0;
  for (long long e = (long long)blockIdx.x * FA_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * FA_THREADS) {
    const int d = (int)(e % a.n0);
    const long long r = e / a.n0;
    const int v = (int)(r % a.V);
    const long long k = r / a.V;
    float l = a.lo[k * a.n0 + d], h = a.hi[k * a.n0 + d];
    for (int m = 0; m < a.npa; ++m)
      if (a.pa_idx[m] == d) l = h = a.values[v * a.npa + m];
    a.rlo[e] = l;
    a.rhi[e] = h;
    if (a.plo) {
      for (int m = 0; m < a.nra; ++m)
        if (a.ra_idx[m] == d) {
          l -= a.tau;
          h += a.tau;
        }
      a.plo[e] = l;
      a.phi[e] = h;
    }
  }
}

extern "C" int fa_count_rows_launch(CountArgs a, hipStream_t stream) {
  if (a.N <= 0) return 0;
  if (a.n0 < 1 || a.V < 1 || a.npa < 1 || a.npa > FA_MAX_PA || a.nra < 0 || a.nra > FA_MAX_RA) return -3;
  if ((a.plo == nullptr) != (a.phi == nullptr)) return -3;
  const long long total = (long long)a.N * a.V * a.n0;
  const long long blocks = (total + FA_THREADS - 1) / FA_THREADS;
  hipLaunchKernelGGL(fa_count_rows_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(FA_THREADS), 0,
                     stream, a);
  return (int)hipGetLastError();
}

// ---- level step ------------------------------------------------------------------------------
// One node per lane.  FAIR / UNFAIR nodes add their volume to their partition; an OPEN node of at
// most leaf_points points goes to the leaf list, any other OPEN node is halved along the dim with
// the largest (hi_d - lo_d) * s_d (fp32 product, lowest d on ties) into the child pool.
__global__ void __launch_bounds__(FA_THREADS) fa_count_level_kernel(CountArgs a) {
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * FA_THREADS + threadIdx.x;
  const bool nv = k < a.N;
  const int n0 = a.n0, V = a.V;
  int code = 0, nchild = 0, nleaf = 0, sd = -1, p = 0;
  if (nv) {
    p = a.part[k];
    const float* lx = a.lx + (size_t)k * V;
    const float* ux = a.ux + (size_t)k * V;
    const float* lxp = a.lxp + (size_t)k * V;
    const float* uxp = a.uxp + (size_t)k * V;
    bool unfair = false, poss = false;
    for (int q = 0; q < a.Pp; ++q) {
      const int vi = (int)a.pairs[2 * q], vj = (int)a.pairs[2 * q + 1];
      if (vi < 0 || vi >= V || vj < 0 || vj >= V) continue;
      const float li = lx[vi], ui = ux[vi], lj = lxp[vj], uj = uxp[vj];
      unfair = unfair || (ui < 0.f && lj > 0.f) || (li > 0.f && uj < 0.f);
      poss = poss || (li < 0.f && uj > 0.f) || (ui > 0.f && lj < 0.f);
    }
    code = unfair ? 2 : (poss ? 0 : 1);
    long long vol = 1;
    float best = -1.f;
    for (int d = 0; d < n0; ++d) {
      bool pa = false;
      for (int m = 0; m < a.npa; ++m) pa = pa || a.pa_idx[m] == d;
      if (pa) continue;
      const float w = a.hi[(size_t)k * n0 + d] - a.lo[(size_t)k * n0 + d];
      vol *= (long long)w + 1;
      const float sc = w * a.score[d];
      if (w > 0.f && sc > best) {
        best = sc;
        sd = d;
      }
    }
    a.code[k] = (uint8_t)code;
    if (code == 1) atomicAdd((unsigned long long*)&a.fair[p], (unsigned long long)vol);
    else if (code == 2) atomicAdd((unsigned long long*)&a.unfair[p], (unsigned long long)vol);
    else if (vol <= a.leaf_points || sd < 0) nleaf = 1;
    else nchild = 2;
  }
  // one atomic per wave and list
  const int ci = fa_wave_incl_scan(nchild, lane), li = fa_wave_incl_scan(nleaf, lane);
  int cb = 0, lb = 0;
  if (lane == 63) {
    if (ci) cb = atomicAdd(&a.counters[0], ci);
    if (li) lb = atomicAdd(&a.counters[1], li);
  }
  cb = __shfl(cb, 63) + ci - nchild;
  lb = __shfl(lb, 63) + li - nleaf;
  if (nleaf) {
    if (lb < a.leaf_cap) {
      for (int d = 0; d < n0; ++d) {
        a.leaf_lo[(size_t)lb * n0 + d] = a.lo[(size_t)k * n0 + d];
        a.leaf_hi[(size_t)lb * n0 + d] = a.hi[(size_t)k * n0 + d];
      }
      a.leaf_part[lb] = p;
    } else {
      atomicAdd(&a.counters[2], 1);
    }
  }
  if (nchild) {
    if (cb + 2 <= a.cap) {
      const float l = a.lo[(size_t)k * n0 + sd], h = a.hi[(size_t)k * n0 + sd];
      const float m = l + floorf((h - l) * 0.5f);
      for (int d = 0; d < n0; ++d) {
        const float dl = a.lo[(size_t)k * n0 + d], dh = a.hi[(size_t)k * n0 + d];
        a.olo[(size_t)cb * n0 + d] = dl;
        a.ohi[(size_t)cb * n0 + d] = d == sd ? m : dh;
        a.olo[(size_t)(cb + 1) * n0 + d] = d == sd ? m + 1.f : dl;
        a.ohi[(size_t)(cb + 1) * n0 + d] = dh;
      }
      a.opart[cb] = p;
      a.opart[cb + 1] = p;
      atomicAdd(&a.child_cnt[p], 2);
    } else {
      atomicAdd(&a.counters[2], 1);
    }
  }
}

extern "C" int fa_count_level_launch(CountArgs a, hipStream_t stream) {
  if (a.N <= 0) return 0;
  if (a.n0 < 1 || a.V < 1 || a.npa < 1 || a.npa > FA_MAX_PA || a.Pp < 0 || a.cap < 0 || a.leaf_cap < 0) return -3;
  if ((long long)a.N + FA_THREADS - 1 > 0x7FFFFFFFLL) return -2;
  hipLaunchKernelGGL(fa_count_level_kernel, dim3((unsigned)((a.N + FA_THREADS - 1) / FA_THREADS)), dim3(FA_THREADS), 0,
                     stream, a);
  return (int)hipGetLastError();
}
