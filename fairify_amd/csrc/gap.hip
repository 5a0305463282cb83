// Certified score gap between counterparts (definitions: ops/gap.py).  gfx950.
//
// fa_gap_enum_kernel   leaf enumeration, the hot path (work shape: csrc/rowfwd.h), over the leaves like
//                      fa_count_enum_kernel (csrc/count.hip); instead of counting flags every point
//                      reduces the certain / possible gap over pairs and offsets in registers, then an
//                      arg-max (lowest point, pair, offset on ties) runs over the wave and across the
//                      waves in LDS.  One lane stores the leaf's five outputs; no global atomics.
// fa_gap_level_kernel  level step: a 16-lane group per node concretises the coupled forms of every
//                      pair in fp64, picks the best pair, the code and the split dim, writes the
//                      candidate rows and reserves child / leaf slots with one atomic per wave.
#include <hip/hip_runtime.h>

#include <climits>

#include "rowfwd.h"
#include "wave.h"

// a - b in fp64, widened outward by g (|a| + |b|): the reference's separately rounded operations
// (no contraction into an fma)
__device__ __forceinline__ double fa_gap_lo(float a, float b, double g) {
  const double x = a, y = b;
  return __dsub_rn(__dsub_rn(x, y), __dmul_rn(g, __dadd_rn(fabs(x), fabs(y))));
}
__device__ __forceinline__ double fa_gap_hi(float a, float b, double g) {
  const double x = a, y = b;
  return __dadd_rn(__dsub_rn(x, y), __dmul_rn(g, __dadd_rn(fabs(x), fabs(y))));
}

template <int TM>
__global__ void __launch_bounds__(FA_THREADS) __attribute__((amdgpu_waves_per_eu(TM == 7 ? 2 : 1)))
fa_gap_enum_kernel(NetDesc net, GapEnumArgs a, RegNetCfg rc) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int XT = TM < 2 ? TM : 2;     // input tiles kept per point: n0 <= 32 (the launch refuses wider)
  constexpr int NW = FA_THREADS / 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, grp = lane >> 4;
  const int n0 = net.dims[0];
  const int V = a.V, E = a.E;
  const bool rx = a.nra > 0;
  const double g1 = a.g1;
  // LDS after the staged block: per wave V + 1 slab rows of [lb x 16 | ub x 16] (row V: the
  // counterpart row in flight), the leaf's lo / width / stride per dim, its volume, the waves'
  // winners (value, possible maximum, point, pair, offset) and the pair index of every (v, v')
  float* slab = smem + rc.floats + wave * (V + 1) * 32;
  float* s_lo = smem + rc.floats + NW * (V + 1) * 32;
  int* s_w = (int*)(s_lo + n0);
  int* s_st = s_w + n0;
  int* s_vol = s_st + n0;
  double* r_val = (double*)(((uintptr_t)(s_vol + 1) + 7) & ~(uintptr_t)7);      // [NW] certain, [NW] possible
  int* r_arg = (int*)(r_val + 2 * NW);        // [NW][3]
  int* pidx = r_arg + 3 * NW;                 // [V][V], -1: not a pair
  fa_stage_wperm(net, rc, a.flat, smem, tid, FA_THREADS);
  for (int i = tid; i < V * V; i += FA_THREADS) pidx[i] = INT_MAX;
  __syncthreads();
  for (int q = tid; q < a.Pp; q += FA_THREADS) {
    const int64_t vi = a.pairs[2 * q], vj = a.pairs[2 * q + 1];
    if (vi >= 0 && vi < V && vj >= 0 && vj < V) atomicMin(&pidx[(int)vi * V + (int)vj], q);
  }
  __syncthreads();
  for (int i = tid; i < V * V; i += FA_THREADS)
    if (pidx[i] == INT_MAX) pidx[i] = -1;
  FaRowSlots<XT> slots;       // this lane's PA / RA slots, fixed for the launch
  fa_row_slots<XT>(a, grp, slots);
  BoundArgs ba{};
  ba.R = 16;
  const float g0 = net.g_fwd[0];
  float Xb[XT][4], HA[TM][4], EA[TM][4], HB[TM][4], EB[TM][4];
  for (int leaf = blockIdx.x; leaf < a.L; leaf += gridDim.x) {
    __syncthreads();     // the previous leaf's table and winners are no longer read
    if (tid == 0) {
      s_vol[0] = fa_enum_decode(a, leaf, n0, s_lo, s_w, s_st);
    }
    __syncthreads();
    const int vol = s_vol[0];
    // this lane's winner so far: its points come in increasing order, so a strict improvement keeps
    // the lowest point
    double bc = -INFINITY, bp = -INFINITY;
    int bs = INT_MAX, bq = -1, be = -1;
    for (int s0 = 0; s0 < vol; s0 += FA_THREADS / 4) {
      const int s = s0 + wave * 16 + col;
      const bool sv = s < vol;
      fa_enum_point<XT>(Xb, s, sv, grp, n0, s_lo, s_w, s_st);
      // rigorous forward of the 16 points' row (PA assignment v, offset vector e or -1) into slab row r
      auto run_row = [&](int v, int e, int r) {
        fa_row_forward<TM>(net, ba, rc, smem, lane, Xb, g0, FaQueryCoord<XT, GapEnumArgs>{a, slots, v, e}, slab + r * 32,
                           HA, EA, HB, EB);
      };
      for (int v = 0; v < V; ++v) run_row(v, -1, v);
      // a slab row is written by lanes 0..15 and read back by the same lane only.  The point's own
      // winner over pairs and offsets: the larger cert, then the lower pair, then the lower offset
      double pc = -INFINITY, pp = -INFINITY;
      int pq = -1, pe = -1;
      auto test_row = [&](int vp, int r, int e) {
        const float lp = slab[r * 32 + col], up = slab[r * 32 + 16 + col];
        for (int v = 0; v < V; ++v) {
          const int q = pidx[v * V + vp];
          if (q < 0) continue;
          const float lv = slab[v * 32 + col], uv = slab[v * 32 + 16 + col];
          const double c1 = fa_gap_lo(lp, uv, g1), c2 = fa_gap_lo(lv, up, g1);
          const double p1 = fa_gap_hi(up, lv, g1), p2 = fa_gap_hi(uv, lp, g1);
          const double c = (c1 != c1 || c2 != c2) ? -INFINITY : fmax(c1, c2);     // a NaN certifies nothing
          const double p = (p1 != p1 || p2 != p2) ? INFINITY : fmax(p1, p2);      // and excludes nothing
          pp = fmax(pp, p);
          if (c > pc || (c == pc && (q < pq || (q == pq && e < pe)))) {
            pc = c;
            pq = q;
            pe = e;
          }
        }
      };
      if (!rx) {
        if (grp == 0)
          for (int vp = 0; vp < V; ++vp) test_row(vp, vp, 0);
      } else {
        for (int e = 0; e < E; ++e)
          for (int vp = 0; vp < V; ++vp) {
            run_row(vp, e, V);
            if (grp == 0) test_row(vp, V, e);
          }
      }
      if (grp == 0 && sv) {
        bp = fmax(bp, pp);
        if (pq >= 0 && pc > bc) {
          bc = pc;
          bs = s;
          bq = pq;
          be = pe;
        }
      }
    }
    // over the wave: the larger cert, the lower point on ties (a point lives in one lane, so its pair
    // and offset travel with it); lanes outside group 0 hold the neutral element
    {
      const double mine = bc;
      const int mys = bs;
      fa_group_argmax<64>(bc, bs);
      const int src = __ffsll((unsigned long long)__ballot(mine == bc && mys == bs)) - 1;
      bq = __shfl(bq, src, 64);
      be = __shfl(be, src, 64);
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) bp = fmax(bp, __shfl_xor(bp, off, 64));
    }
    if (lane == 0) {
      r_val[wave] = bc;
      r_val[NW + wave] = bp;
      r_arg[3 * wave] = bs;
      r_arg[3 * wave + 1] = bq;
      r_arg[3 * wave + 2] = be;
    }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < NW; ++w) {
        bp = fmax(bp, r_val[NW + w]);
        if (r_val[w] > bc || (r_val[w] == bc && r_arg[3 * w] < bs)) {
          bc = r_val[w];
          bs = r_arg[3 * w];
          bq = r_arg[3 * w + 1];
          be = r_arg[3 * w + 2];
        }
      }
      // no finite cert at all (every bound NaN): the reference's first key; a skipped leaf (empty box
      // or over max_vol) excludes nothing: leaf_hi = +inf, arg_s = -2
      if (vol && bq < 0) bs = bq = be = 0;
      a.leaf_lo[leaf] = bc;
      a.leaf_hi[leaf] = vol ? bp : (double)INFINITY;
      a.arg_s[leaf] = vol ? bs : -2;
      a.arg_pair[leaf] = bq;
      a.arg_e[leaf] = be;
    }
  }
}

static size_t gap_enum_lds_bytes(const NetDesc& net, const GapEnumArgs& a, const RegNetCfg& rc) {
  const int NW = FA_THREADS / 64;
  const size_t words = (size_t)rc.floats + (size_t)NW * (a.V + 1) * 32 + 3 * (size_t)net.dims[0] + 2 + 7 * (size_t)NW +
                       (size_t)a.V * a.V;
  return (words * sizeof(float) + 15) & ~(size_t)15;
}

// Enumerates a.L leaves into a.leaf_lo / leaf_hi / arg_*.  Returns 0 if launched, -3 for shapes the
// kernel does not cover (a layer over 160 wide, inputs over 32 wide, V or E over 32, a leaf volume
// bound over 65 536, more than 64 KB of LDS), -2 for a bad workgroup count, > 0 a HIP error.
extern "C" int fa_gap_enum_launch(const NetDesc& net, GapEnumArgs a, hipStream_t stream) {
  if (a.L <= 0) return 0;
  if (!fa_row_query_ok(net, a) || a.Pp < 1) return -3;
  if (a.max_vol < 1 || a.max_vol > FA_COUNT_MAX_VOL) return -3;
  RegNetCfg rc{};
  void (*k)(NetDesc, GapEnumArgs, RegNetCfg) = nullptr;
  switch (fa_row_net(net, rc)) {
#define FA_GAP_CASE(T) \
  case T: k = fa_gap_enum_kernel<T>; break;
    FA_ROW_TMS(FA_GAP_CASE)
#undef FA_GAP_CASE
    default: return -3;
  }
  const size_t bytes = gap_enum_lds_bytes(net, a, rc);
  if (bytes > 64 * 1024) return -3;
  const double ku = 3.0 * 0x1p-53;         // gamma(1, FP64_UNIT) as ops/reference.gamma rounds it
  a.g1 = ku / (1.0 - ku);
  if (a.blocks < 1 || a.blocks > a.L) return -2;
  hipLaunchKernelGGL(k, dim3((unsigned)a.blocks), dim3(FA_THREADS), bytes, stream, net, a, rc);
  return (int)hipGetLastError();
}

// ---- level step ------------------------------------------------------------------------------
// A 16-lane group per node, dims lane and lane + 16 (n0 <= 32).  Every pair and orientation is
// concretised in fp64 over the group (fa_group_sum<16>), the split dim comes from fa_group_argmax<16>,
// child and leaf slots are reserved with one atomic per wave as in fa_count_level_kernel.
__global__ void __launch_bounds__(FA_THREADS) fa_gap_level_kernel(GapLevelArgs a) {
  const int lane = threadIdx.x & 63, gl = lane & 15;
  const long long k = ((long long)blockIdx.x * FA_THREADS + threadIdx.x) >> 4;
  const bool nv = k < a.N;
  const int n0 = a.n0, V = a.V;
  float lo_[2], hi_[2];
  int ps[2];
  bool dv[2], ra[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int d = gl + 16 * j;
    dv[j] = nv && d < n0;
    lo_[j] = dv[j] ? a.lo[k * n0 + d] : 0.f;
    hi_[j] = dv[j] ? a.hi[k * n0 + d] : 0.f;
    ps[j] = -1;
    ra[j] = false;
    for (int m = 0; m < a.npa; ++m)
      if (a.pa_idx[m] == d) ps[j] = m;
    for (int m = 0; m < a.nra; ++m) ra[j] = ra[j] || a.ra_idx[m] == d;
  }
  const double tau = a.tau;
  double best = -INFINITY;
  int bk = -1;
  for (int q = 0; q < a.Pp; ++q) {
    const int vi = (int)a.pairs[2 * q], vj = (int)a.pairs[2 * q + 1];
    if (vi < 0 || vi >= V || vj < 0 || vj >= V) continue;
    const long long rx = k * V + vi, rp = k * V + vj;
    for (int o = 0; o < 2; ++o) {
      // A: U of the counterpart row minus L of the x row; B: U of the x row minus L of the counterpart
      const float* cU = o ? a.Uc : a.Ucp;
      const float* cL = o ? a.Lcp : a.Lc;
      const long long ru = o ? rx : rp, rl = o ? rp : rx;
      const int vu = o ? vi : vj, vl = o ? vj : vi;
      double val = 0.0, mag = 0.0;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if (!dv[j]) continue;
        const int d = gl + 16 * j;
        const double cu = cU[ru * n0 + d], cl = cL[rl * n0 + d];
        if (ps[j] >= 0) {
          const double pu = cu * (double)a.values[vu * a.npa + ps[j]], pl = cl * (double)a.values[vl * a.npa + ps[j]];
          val += pu - pl;
          mag += fabs(pu) + fabs(pl);
        } else {
          const double c = cu - cl, t1 = c * (double)lo_[j], t2 = c * (double)hi_[j];
          val += (t1 != t1 || t2 != t2) ? (double)NAN : fmax(t1, t2);
          mag += (fabs(cu) + fabs(cl)) * fmax(fabs((double)lo_[j]), fabs((double)hi_[j]));
          if (ra[j]) {
            const double r = tau * fabs(o ? cl : cu);      // the counterpart's coefficient
            val += r;
            mag += r;
          }
        }
      }
      val = fa_group_sum<16>(val);
      mag = fa_group_sum<16>(mag);
      double b = INFINITY;
      if (nv) {
        const double u0 = o ? a.U0[ru] : a.U0p[ru], ue = o ? a.Ue[ru] : a.Uep[ru];
        const double l0 = o ? a.L0p[rl] : a.L0[rl], le = o ? a.Lep[rl] : a.Le[rl];
        const double iu = o ? a.ub[ru] : a.ubp[ru], il = o ? a.lbp[rl] : a.lb[rl];
        double form = val + u0 + ue - l0 + le + a.gam * (mag + fabs(u0) + fabs(ue) + fabs(l0) + fabs(le));
        double iv = (iu - il) + a.g1 * (fabs(iu) + fabs(il));
        if (form != form) form = INFINITY;
        if (iv != iv) iv = INFINITY;
        b = fmin(form, iv);
      }
      if (b > best) {        // pair-major, A before B: a strict improvement keeps the first maximum
        best = b;
        bk = 2 * q + o;
      }
    }
  }
  // the best pair's fp32 coefficients, the candidate corner, the split score of this lane's dims
  const int bp = bk >> 1, bo = bk & 1;
  float c32[2] = {0.f, 0.f}, sc[2] = {-1.f, -1.f}, w[2] = {0.f, 0.f};
  bool anyp = false, can = false;
  long long vol = 1;
  if (nv && bk >= 0) {
    const int vi = (int)a.pairs[2 * bp], vj = (int)a.pairs[2 * bp + 1];
    const long long rx = k * V + vi, rp = k * V + vj;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (!dv[j]) continue;
      const int d = gl + 16 * j;
      float x, xp;
      if (ps[j] >= 0) {
        x = a.values[vi * a.npa + ps[j]];
        xp = a.values[vj * a.npa + ps[j]];
      } else {
        const float cu = bo ? a.Uc[rx * n0 + d] : a.Ucp[rp * n0 + d];
        const float cl = bo ? a.Lcp[rp * n0 + d] : a.Lc[rx * n0 + d];
        c32[j] = __fsub_rn(cu, cl);
        const bool up = bo ? cl <= 0.f : cu >= 0.f;
        x = c32[j] >= 0.f ? hi_[j] : lo_[j];
        xp = ra[j] ? x + (up ? a.tau : -a.tau) : x;
        w[j] = hi_[j] - lo_[j];
        vol *= (long long)w[j] + 1;
        float p = __fmul_rn(fabsf(c32[j]), w[j]);
        if (p != p) p = 0.f;
        sc[j] = w[j] > 0.f ? p : -1.f;
        anyp = anyp || sc[j] > 0.f;
        can = can || w[j] > 0.f;
      }
      a.coef[k * n0 + d] = c32[j];
      a.cand_x[k * n0 + d] = x;
      a.cand_xp[k * n0 + d] = xp;
    }
  }
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) {
    const int p2 = __shfl_xor((int)anyp, off, 64), c2 = __shfl_xor((int)can, off, 64);
    const long long v2 = __shfl_xor(vol, off, 64);
    anyp = anyp || p2;
    can = can || c2;
    vol *= v2;
  }
  if (!anyp) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
      if (sc[j] >= 0.f) sc[j] = __fmul_rn(w[j], a.score[gl + 16 * j]);
  }
  float s = sc[0];
  int sd = gl;
  if (sc[1] > s) {
    s = sc[1];
    sd = gl + 16;
  }
  fa_group_argmax<16>(s, sd);
  float ub = (float)best;
  if ((double)ub < best) ub = nextafterf(ub, INFINITY);
  int code = 0, nchild = 0, nleaf = 0, p = 0;
  if (nv) {
    p = a.part[k];
    const bool pruned = (double)ub <= a.thr[p];
    code = pruned ? 0 : ((vol <= a.leaf_points || !can) ? 1 : 2);
    if (gl == 0) {
      a.out_ub[k] = ub;
      a.code[k] = (uint8_t)code;
      a.best_pair[k] = bp;
      a.orient[k] = bo;
      a.sdim[k] = sd;
      nleaf = code == 1;
      nchild = code == 2 ? 2 : 0;
    }
  }
  // one atomic per wave and list; the group's leader holds the counts, its lanes read the base
  const int ci = fa_wave_incl_scan(nchild, lane), li = fa_wave_incl_scan(nleaf, lane);
  int cb = 0, lb = 0;
  if (lane == 63) {
    if (ci) cb = atomicAdd(&a.counters[0], ci);
    if (li) lb = atomicAdd(&a.counters[1], li);
  }
  cb = __shfl(cb, 63, 64) + ci - nchild;
  lb = __shfl(lb, 63, 64) + li - nleaf;
  cb = __shfl(cb, lane & ~15, 64);
  lb = __shfl(lb, lane & ~15, 64);
  if (code == 1) {
    if (lb < a.leaf_cap) {
#pragma unroll
      for (int j = 0; j < 2; ++j)
        if (dv[j]) {
          a.leaf_lo[(size_t)lb * n0 + gl + 16 * j] = lo_[j];
          a.leaf_hi[(size_t)lb * n0 + gl + 16 * j] = hi_[j];
        }
      if (gl == 0) {
        a.leaf_part[lb] = p;
        a.leaf_key[lb] = (int)k;
      }
    } else if (gl == 0) {
      atomicAdd(&a.counters[2], 1);
    }
  }
  if (code == 2) {
    if (cb + 2 <= a.cap) {
#pragma unroll
      for (int j = 0; j < 2; ++j)
        if (dv[j]) {
          const int d = gl + 16 * j;
          const float m = lo_[j] + floorf((hi_[j] - lo_[j]) * 0.5f);
          a.olo[(size_t)cb * n0 + d] = lo_[j];
          a.ohi[(size_t)cb * n0 + d] = d == sd ? m : hi_[j];
          a.olo[(size_t)(cb + 1) * n0 + d] = d == sd ? m + 1.f : lo_[j];
          a.ohi[(size_t)(cb + 1) * n0 + d] = hi_[j];
        }
      if (gl == 0) {
        a.opart[cb] = a.opart[cb + 1] = p;
        a.oub[cb] = a.oub[cb + 1] = ub;
        a.okey[cb] = 2 * (int)k;
        a.okey[cb + 1] = 2 * (int)k + 1;
      }
    } else if (gl == 0) {
      atomicAdd(&a.counters[2], 1);
    }
  }
}

// Level step over a.N nodes.  Returns 0 if launched, -3 for shapes the kernel does not cover (inputs
// over 32, V over 32, no pair), -2 for a node count whose keys do not fit an int, > 0 a HIP error.
extern "C" int fa_gap_level_launch(GapLevelArgs a, hipStream_t stream) {
  if (a.N <= 0) return 0;
  if (a.n0 < 1 || a.n0 > 32 || a.V < 1 || a.V > FA_RATE_MAX_V || a.Pp < 1) return -3;
  if (a.npa < 1 || a.npa > FA_MAX_PA || a.nra < 0 || a.nra > FA_MAX_RA || a.cap < 0 || a.leaf_cap < 0) return -3;
  for (int m = 0; m < a.npa; ++m)
    if (a.pa_idx[m] < 0 || a.pa_idx[m] >= a.n0) return -3;
  for (int m = 0; m < a.nra; ++m)
    if (a.ra_idx[m] < 0 || a.ra_idx[m] >= a.n0) return -3;
  if ((long long)a.N > 0x3FFFFFFFLL / 16) return -2;
  const double k1 = 3.0 * 0x1p-53, kn = (double)(2 * a.n0 + 8 + 2) * 0x1p-53;   // ops/reference.gamma
  a.g1 = k1 / (1.0 - k1);
  a.gam = kn / (1.0 - kn);
  const long long threads = (long long)a.N * 16;
  hipLaunchKernelGGL(fa_gap_level_kernel, dim3((unsigned)((threads + FA_THREADS - 1) / FA_THREADS)), dim3(FA_THREADS), 0,
                     stream, a);
  return (int)hipGetLastError();
}
