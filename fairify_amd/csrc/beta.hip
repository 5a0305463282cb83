// beta-CROWN bounding of ReLU-phase BaB nodes on gfx950 (stage "beta"; semantics:
// fairify_amd/ops/beta.py:level_ref, which the GPU tests compare this kernel against).
//
// The reference decides a partition with Z3, whose simplex case-splits each ReLU
// If(z >= 0, z, 0) (utils/verif_utils.py:525-528; src/AC/Verify-AC.py:146-158): inside a case
// split the phase is a linear constraint on the region.  Per node (box, ordered PA pair (va, vb),
// phases of both network copies) this kernel maximises the Lagrangian lower bound of
//     f_t(x) = t N(x, va) - (1 - t) N(x, vb)        (f_t >= 0 on the region: no violating pair)
// over the lower slopes alpha (unstable neurons), the split multipliers beta (fixed neurons) and t
// by projected Adam in fp32, then re-evaluates the bound at the best parameters in fp64 with
// rigorous rounding terms, picks the branching neuron by a filtered look-ahead and returns the
// concretising vertex (the host screens / confirms it as a candidate pair).
//
// Mapping: ONE wave64 per node, lanes over the neurons of a layer (widths <= 64 take one lane
// each; wider layers loop).  Per layer the backward step is lam_{l-1} = W_l mu_l: lane i of the
// previous layer sums over the w_l multipliers, read as LDS broadcasts, against the transposed
// weights (consecutive across lanes: no bank conflicts); the forward step of the linearised
// network reads W_l row-major the same way.  The weights are staged once per workgroup (the
// transposed copy too when it fits), the per-node bounds / records live in a per-wave LDS slab,
// the optimiser state (current parameters, Adam moments) in a global scratch row per node that
// stays L2-resident while the wave runs.  The network is a handful of KB and every node runs
// ~100 dependent passes through it, so the kernel is latency / issue bound.  The optimisation loop
// also exists batched on MFMA, 16 nodes of one network as the 16 columns (they share W; their
// multipliers are the B operand, the relaxation is elementwise on the accumulators):
// csrc/beta_opt16.hip, opt-in; this kernel then runs at iters = 0 as its second phase.  The
// infeasibility pass (a.feas) has the same two-phase form (BetaArgs::fpar / fgt: the proposed
// multipliers; this kernel at feas = 1, iters = 0 decides on its rigorous value at them).
#include <float.h>

#include <algorithm>

#include "args.h"

namespace {

constexpr double U64 = 1.1102230246251565e-16;   // 2^-53

// waves per SIMD the register allocation targets (the kernel is latency bound: one wave64 per node,
// dependent LDS / L2 round trips; at 186 VGPRs only 2 waves per SIMD fit)
#ifndef FA_BETA_WPE
#define FA_BETA_WPE 3
#endif

__device__ __forceinline__ double g64(int k) {    // Higham gamma_k in fp64, padded like ref.gamma
  const double ku = (k + 2) * U64;
  return ku / (1.0 - ku);
}

__device__ __forceinline__ void wsync() {
  // lanes of ONE wave exchange data through LDS: DS instructions of a wave execute in order, so a
  // compiler-level barrier with wave-scope fences is enough (no workgroup barrier: waves are independent)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <typename T>
__device__ __forceinline__ T tabs(T v) {
  return v < (T)0 ? -v : v;
}

template <typename T>
__device__ __forceinline__ T wsum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// wave arg-max (first index on ties); returns the winning value, index in *idx
__device__ __forceinline__ float wargmax(float v, int i, int* idx) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float v2 = __shfl_xor(v, o, 64);
    const int i2 = __shfl_xor(i, o, 64);
    if (v2 > v || (v2 == v && i2 < i)) {
      v = v2;
      i = i2;
    }
  }
  *idx = i;
  return v;
}

struct Slab {            // per-wave LDS workspace
  float* lb[2];          // phase-clamped pre-activation bounds [NH] per copy
  float* ub[2];
  float* lam[2];         // multiplier on h_j of the last backward pass [NH]
  float* z[2];           // linearised pre-activations at x* [NH]
  float* zb[2];          // pgap: sums of z / of the relaxation outputs h over the optimisation steps
  float* hb[2];          //   (the Lagrangian's primal iterates; their mean is the primal point) [NH]
  float* sc;             // branching scores [2 NH]
  int8_t* kd[2];         // relaxation kind of the last backward pass (0 off, 1 identity, 2 alpha, 3 chord)
  int8_t* ph[2];         // phases
  double* b0;            // broadcast buffers [mw] (fp32 passes use them as float arrays)
  double* b1;
  double* cf[2];         // input coefficients of the rigorous pass [n0]
  double* hm[2];         // |input| maxima per copy [n0]
  float* cft;            // input coefficients of a look-ahead pass [n0]
  float* xs;             // concretising vertex [n0]
  float* xps;            // copy B's vertex [n0] (relaxed: RA dims from x''s box; else = xs)
  float* gt[2];          // relaxed: current multipliers gP, gM of the tie |x_r - x'_r| <= tau [n0]
};

struct Node {            // per-node constants (wave-uniform)
  const float* lo;
  const float* hi;
  const float* plo;      // relaxed: x''s box on the RA dims (ramask), else nullptr
  const float* phi;
  unsigned long long ramask;
  float tau;             // relaxed: the tie's tolerance (its multipliers in Slab::gt; 0 / none: dropped)
  bool tie;
  float va[FA_MAX_PA];
  float vb[FA_MAX_PA];
  unsigned long long pamask;
};

// Backward pass of copy `c` (objective scale * logit).  T = float: an optimisation step (no
// rounding terms); T = double with RIG: the rigorous bound (every rounding charged to *err).
// REC: record lam / kind per neuron (the gradient and the scores read them).  ovr >= 0: look-ahead
// child -- neuron ovr of this copy gets phase ovs (its multiplier 0).  Leaves the input
// coefficients in `coef` (LDS, n0) and returns the constant.
template <typename T, bool RIG, bool REC, bool WTL>
__device__ T bwd(const NetDesc& nd, const float* Wf, const float* Wt, const Slab& S, int c, T scale,
                 const float* __restrict__ al, const float* __restrict__ be, int ovr, int ovs, T* coef, T* err,
                 int* infeas) {
  const int lane = threadIdx.x & 63;
  const int L = nd.n_layers;
  const int NH = nd.n_hidden;
  T* b0 = reinterpret_cast<T*>(S.b0);
  T* b1 = reinterpret_cast<T*>(S.b1);
  const float* lbv = S.lb[c];
  const float* ubv = S.ub[c];
  T cpart = 0, mpart = 0, epart = 0;
  int bad = 0;
  {
    const int w = nd.dims[L - 1];
    const float* wo = Wf + nd.w_off[L - 1];
    const int off = nd.neuron_off[L - 2];
    for (int j = lane; j < w; j += 64) {
      const T lam = scale * (T)wo[j];
      b0[j] = lam;
      if (RIG) epart += (T)U64 * tabs(lam) * (T)fmaxf(ubv[off + j], 0.f);
    }
    if (lane == 0) {
      const T c0 = scale * (T)Wf[nd.b_off[L - 1]];
      cpart += c0;
      if (RIG) mpart += tabs(c0);
    }
  }
  wsync();
  for (int l = L - 2; l >= 0; --l) {
    const int w = nd.dims[l + 1];
    const int win = nd.dims[l];
    const int off = nd.neuron_off[l];
    const float* bias = Wf + nd.b_off[l];
    for (int j = lane; j < w; j += 64) {
      const int k = off + j;
      const T lam = b0[j];
      float lbj = lbv[k], ubj = ubv[k];
      int p = S.ph[c][k];
      T bet = (T)be[k];
      if (k == ovr) {
        p = ovs;
        bet = 0;
        if (p > 0) lbj = fmaxf(lbj, 0.f);
        if (p < 0) ubj = fminf(ubj, 0.f);
        if (lbj > ubj) bad = 1;
      }
      if (p == 0) bet = 0;
      const bool dead = ubj <= 0.f || p < 0;
      const bool act = !dead && (lbj >= 0.f || p > 0);
      T base = 0, kap = 0;
      int kind = 0;
      if (act) {
        base = lam;
        kind = 1;
      } else if (!dead) {
        if (lam >= 0) {
          base = lam * (T)al[k];
          kind = 2;
        } else {
          T s = (T)ubj / ((T)ubj - (T)lbj);
          if (RIG) s *= (T)(1.0 + 4.0 * U64);         // rounded up: a steeper chord stays above relu
          base = lam * s;
          kap = -base * (T)lbj;
          kind = 3;
        }
      }
      const T mu = base - bet * (T)p;
      // a negative multiplier of a fixed neuron takes the interval side of its region
      const T kb = (p != 0 && bet < 0) ? bet * (T)p * (T)(p > 0 ? ubj : lbj) : (T)0;
      const T mb = mu * (T)bias[j];
      cpart += mb + kap + kb;
      if (RIG) {
        const T zmax = (T)fmaxf(fabsf(lbj), fabsf(ubj));
        T e = 0;
        if (kind == 2) e += (T)g64(1) * tabs(base) * zmax;
        if (kind == 3) e += (T)(3.0 * U64) * ((T)2 * tabs(base) * zmax + tabs(kap));
        if (p != 0) e += (T)g64(1) * (tabs(mu) * zmax + tabs(kb));
        epart += e;
        mpart += tabs(mb) + tabs(kap) + tabs(kb);
      }
      b1[j] = mu;
      if (REC) {
        S.lam[c][k] = (float)lam;
        S.kd[c][k] = (int8_t)kind;
      }
    }
    wsync();
    const float* wt = Wt + nd.w_off[l];
    for (int i = lane; i < win; i += 64) {
      // four independent partial sums: the LDS reads of a chunk issue together instead of one
      // dependent FMA (and its two LDS round trips) per multiplier (the rounding term covers any order)
      T a0 = 0, a1 = 0, a2 = 0, a3 = 0, aab = 0;
      int j = 0;
      for (; j + 4 <= w; j += 4) {
        const T w0 = (T)wt[j * win + i], w1 = (T)wt[(j + 1) * win + i];
        const T w2 = (T)wt[(j + 2) * win + i], w3 = (T)wt[(j + 3) * win + i];
        const T m0 = b1[j], m1 = b1[j + 1], m2 = b1[j + 2], m3 = b1[j + 3];
        a0 += w0 * m0;
        a1 += w1 * m1;
        a2 += w2 * m2;
        a3 += w3 * m3;
        if (RIG) aab += (tabs(w0) * tabs(m0) + tabs(w1) * tabs(m1)) + (tabs(w2) * tabs(m2) + tabs(w3) * tabs(m3));
      }
      for (; j < w; ++j) {
        const T wv = (T)wt[j * win + i];
        const T m = b1[j];
        a0 += wv * m;
        if (RIG) aab += tabs(wv) * tabs(m);
      }
      const T acc = (a0 + a1) + (a2 + a3);
      b0[i] = acc;
      if (RIG) {
        const T hmx = l > 0 ? (T)fmaxf(ubv[nd.neuron_off[l - 1] + i], 0.f) : (T)S.hm[c][i];
        epart += (T)g64(w) * aab * hmx;
      }
    }
    wsync();
  }
  for (int i = lane; i < nd.dims[0]; i += 64) coef[i] = b0[i];
  wsync();
  if (RIG) *err = wsum(epart) + (T)g64(2 * NH + 8) * wsum(mpart);
  if (infeas) *infeas = __any(bad) ? 1 : 0;
  return wsum(cpart);
}

// Concretisation of the coupled input form over the node box (PA dims: va / vb; relaxed RA dims:
// each copy over its own box, the tie |x_r - x'_r| <= tau dropped); WX: writes x* / x'* to S.xs /
// S.xps.  RIG: returns the bound less every rounding term (errA + errB passed in).
template <typename T, bool RIG, bool WX>
__device__ T conc(const NetDesc& nd, const Slab& S, const Node& N, const T* cA, const T* cB, T kA, T kB, T eAB) {
  const int lane = threadIdx.x & 63;
  const int n0 = nd.dims[0];
  T part = 0, mag = 0, emag = 0;
  for (int i = lane; i < n0; i += 64) {
    const float lo = N.lo[i], hi = N.hi[i];
    if ((N.pamask >> i) & 1ull) {
      // this PA dim's position in the value list
      const int q = __popcll(N.pamask & ((1ull << i) - 1ull));
      const T ta = cA[i] * (T)N.va[q];
      const T tb = cB[i] * (T)N.vb[q];
      part += ta + tb;
      if (RIG) mag += tabs(ta) + tabs(tb);
      if (WX) {
        S.xs[i] = lo;
        S.xps[i] = lo;
      }
    } else if ((N.ramask >> i) & 1ull) {
      // the tie's multipliers move coefficient between the copies: f >= f + gP (x_r - x'_r - tau)
      // + gM (x'_r - x_r - tau) on every admissible pair
      const float plo = N.plo[i], phi = N.phi[i];
      const T gp = N.tie ? (T)S.gt[0][i] : (T)0, gm = N.tie ? (T)S.gt[1][i] : (T)0;
      const T ca = cA[i] + (gp - gm);
      const T cb = cB[i] + (gm - gp);
      const float xa = ca >= 0 ? lo : hi;
      const float xb = cb >= 0 ? plo : phi;
      const T ta = ca * (T)xa;
      const T tb = cb * (T)xb;
      const T tt = -(T)N.tau * (gp + gm);
      part += ta + tb + tt;
      if (RIG) {
        mag += tabs(ta) + tabs(tb) + tabs(tt);
        // fl(gp - gm) is off by u (gp + gm): charged on both copies' magnitudes (ca may cancel it)
        const T mxa = (T)fmaxf(fabsf(lo), fabsf(hi)), mxb = (T)fmaxf(fabsf(plo), fabsf(phi));
        emag += (T)2 * (tabs(ca) * mxa + tabs(cb) * mxb + tabs(tt) + (gp + gm) * (mxa + mxb));
      }
      if (WX) {
        S.xs[i] = xa;
        S.xps[i] = xb;
      }
    } else {
      const T cf = cA[i] + cB[i];
      const float x = cf >= 0 ? lo : hi;
      const T tm = cf * (T)x;
      part += tm;
      if (RIG) {
        mag += tabs(tm);
        emag += tabs(cf) * (T)fmaxf(fabsf(lo), fabsf(hi));
      }
      if (WX) {
        S.xs[i] = x;
        S.xps[i] = x;
      }
    }
  }
  T B = wsum(part) + kA + kB;
  if (RIG) {
    const T m = wsum(mag) + tabs(kA) + tabs(kB);
    const T econ = (T)U64 * wsum(emag) + (T)g64(2 * n0 + 4) * m;
    B -= (eAB + econ) * (T)(1.0 + 1e-6);
  }
  wsync();
  return B;
}

// Linearised network of copy c at S.xs (PA dims = v): records z per neuron, returns the logit.
// zacc / hacc (pgap, optional): each neuron's z and relaxation output h are added to them (the
// primal iterate of this optimisation step; neuron k is always handled by the same lane).
template <typename T>
__device__ T fwd(const NetDesc& nd, const float* Wf, const Slab& S, const Node& N, int c, const float* v,
                 const float* __restrict__ al, float* zacc = nullptr, float* hacc = nullptr, float wacc = 1.f) {
  const int lane = threadIdx.x & 63;
  const int L = nd.n_layers;
  const int n0 = nd.dims[0];
  T* h0 = reinterpret_cast<T*>(S.b0);
  T* h1 = reinterpret_cast<T*>(S.b1);
  const float* xin = c == 0 ? S.xs : S.xps;
  for (int i = lane; i < n0; i += 64) {
    T x = (T)xin[i];
    if ((N.pamask >> i) & 1ull) x = (T)v[__popcll(N.pamask & ((1ull << i) - 1ull))];
    h0[i] = x;
  }
  wsync();
  for (int l = 0; l < L - 1; ++l) {
    const int w = nd.dims[l + 1];
    const int win = nd.dims[l];
    const int off = nd.neuron_off[l];
    const float* W = Wf + nd.w_off[l];
    const float* bias = Wf + nd.b_off[l];
    for (int j = lane; j < w; j += 64) {
      T z0 = (T)bias[j], z1 = 0, z2 = 0, z3 = 0;
      int i = 0;
      for (; i + 4 <= win; i += 4) {
        z0 += (T)W[i * w + j] * h0[i];
        z1 += (T)W[(i + 1) * w + j] * h0[i + 1];
        z2 += (T)W[(i + 2) * w + j] * h0[i + 2];
        z3 += (T)W[(i + 3) * w + j] * h0[i + 3];
      }
      for (; i < win; ++i) z0 += (T)W[i * w + j] * h0[i];
      const T z = (z0 + z1) + (z2 + z3);
      const int k = off + j;
      S.z[c][k] = (float)z;
      const int kind = S.kd[c][k];
      T h = 0;
      if (kind == 1) h = z;
      else if (kind == 2) h = (T)al[k] * z;
      else if (kind == 3) {
        const T lbj = (T)S.lb[c][k], ubj = (T)S.ub[c][k];
        h = ubj / (ubj - lbj) * (z - lbj);
      }
      h1[j] = h;
      if (zacc) {
        zacc[k] += wacc * (float)z;
        hacc[k] += wacc * (float)h;
      }
    }
    wsync();
    T* tmp = h0;
    h0 = h1;
    h1 = tmp;
  }
  const int w = nd.dims[L - 1];
  const float* wo = Wf + nd.w_off[L - 1];
  T part = 0;
  for (int j = lane; j < w; j += 64) part += (T)wo[j] * h0[j];
  const T out = wsum(part) + (T)Wf[nd.b_off[L - 1]];
  wsync();
  return out;
}

// WM: where the weights live -- 1: both copies (forward W_l and the transposed backward operand) staged
// in LDS; 0: the forward copy in LDS, the transposed one read from L2; 2: both from L2 (wide nets:
// BM-4's 91 KB of weights would leave LDS for one or two waves per CU, L2 reads leave it for the slabs)
template <int WM>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(FA_BETA_WPE))) void fa_beta_kernel(NetDesc nd,
                                                                                           BetaArgs a) {
  constexpr bool WTL = WM == 1;
  extern __shared__ float smem[];
  const int L = nd.n_layers;
  const int NH = nd.n_hidden;
  const int n0 = nd.dims[0];
  const int mw = nd.max_width;
  const int tot = nd.b_off[L - 1] + nd.dims[L];
  const int tot4 = WM == 2 ? 0 : (tot + 3) & ~3;
  float* Wl = smem;
  float* Wtl = smem + tot4;
  if (WM != 2)
    for (int k = threadIdx.x; k < tot; k += blockDim.x) {
      Wl[k] = a.flat[k];
      if (WTL) Wtl[k] = a.wt[k];
    }
  __syncthreads();
  const float* Wf = WM == 2 ? a.flat : (const float*)Wl;
  const float* Wt = WTL ? (const float*)Wtl : a.wt;
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * a.wpb + wave;
  if (r >= a.R) return;

  // ---- per-wave slab
  const int NHp = (NH + 3) & ~3;
  const int n0p = (n0 + 3) & ~3;
  const int mwp = (mw + 3) & ~3;
  const int slab = 15 * NHp + 4 * mwp + 13 * n0p + 32;
  float* base = smem + tot4 * (WTL ? 2 : 1) + wave * slab;
  Slab S;
  S.lb[0] = base; S.ub[0] = base + NHp; S.lb[1] = base + 2 * NHp; S.ub[1] = base + 3 * NHp;
  S.lam[0] = base + 4 * NHp; S.lam[1] = base + 5 * NHp;
  S.z[0] = base + 6 * NHp; S.z[1] = base + 7 * NHp;
  S.sc = base + 8 * NHp;                                  // 2 NHp
  int8_t* bytes = reinterpret_cast<int8_t*>(base + 10 * NHp);
  S.kd[0] = bytes; S.kd[1] = bytes + NHp; S.ph[0] = bytes + 2 * NHp; S.ph[1] = bytes + 3 * NHp;
  S.zb[0] = base + 11 * NHp; S.zb[1] = base + 12 * NHp; S.hb[0] = base + 13 * NHp; S.hb[1] = base + 14 * NHp;
  double* dbase = reinterpret_cast<double*>(base + 15 * NHp);  // 15 NHp is a multiple of 4: 16-B aligned
  S.b0 = dbase; S.b1 = dbase + mwp;
  S.cf[0] = dbase + 2 * mwp; S.cf[1] = S.cf[0] + n0p; S.hm[0] = S.cf[1] + n0p; S.hm[1] = S.hm[0] + n0p;
  S.cft = reinterpret_cast<float*>(S.hm[1] + n0p);
  S.xs = S.cft + n0p;
  S.xps = S.xs + n0p;
  S.gt[0] = S.xps + n0p;
  S.gt[1] = S.gt[0] + n0p;
  int* cand = reinterpret_cast<int*>(S.gt[1] + n0p);   // look-ahead candidates [32]

  Node N;
  N.lo = a.lo + (size_t)r * n0;
  N.hi = a.hi + (size_t)r * n0;
  N.ramask = a.plo ? a.ramask : 0ull;
  N.tie = N.ramask && a.gtie;
  N.tau = a.tau;
  N.plo = a.plo ? a.plo + (size_t)r * n0 : nullptr;
  N.phi = a.phi ? a.phi + (size_t)r * n0 : nullptr;
  N.pamask = 0;
  for (int q = 0; q < a.npa; ++q) {
    N.va[q] = a.va[(size_t)r * a.npa + q];
    N.vb[q] = a.vb[(size_t)r * a.npa + q];
    N.pamask |= 1ull << a.pa_idx[q];
  }
  // PA indices must be listed in increasing order for the popcount lookup (checked on the host)

  // ---- phase-clamped bounds, phases, |input| maxima
  int bad = 0, fixd = 0;
  {
    const float* LB[2] = {a.LBA + (size_t)r * NH, a.LBB + (size_t)r * NH};
    const float* UB[2] = {a.UBA + (size_t)r * NH, a.UBB + (size_t)r * NH};
    const size_t phs = a.ph_stride > 0 ? (size_t)a.ph_stride : (size_t)NH;
    const int8_t* PH[2] = {a.phA + (size_t)r * phs, a.phB + (size_t)r * phs};
    for (int c = 0; c < 2; ++c)
      for (int k = lane; k < NH; k += 64) {
        const int p = PH[c][k];
        float lb = LB[c][k], ub = UB[c][k];
        if (p > 0) lb = fmaxf(lb, 0.f);
        if (p < 0) ub = fminf(ub, 0.f);
        if (lb > ub) bad = 1;
        if (p != 0) fixd = 1;
        S.lb[c][k] = lb;
        S.ub[c][k] = ub;
        S.ph[c][k] = (int8_t)p;
      }
    for (int i = lane; i < n0; i += 64) {
      const double m = fmax(fabs((double)N.lo[i]), fabs((double)N.hi[i]));
      if ((N.pamask >> i) & 1ull) {
        const int q = __popcll(N.pamask & ((1ull << i) - 1ull));
        S.hm[0][i] = fabs((double)N.va[q]);
        S.hm[1][i] = fabs((double)N.vb[q]);
      } else if ((N.ramask >> i) & 1ull) {
        S.hm[0][i] = m;
        S.hm[1][i] = fmax(fabs((double)N.plo[i]), fabs((double)N.phi[i]));
      } else {
        S.hm[0][i] = m;
        S.hm[1][i] = m;
      }
    }
  }
  wsync();
  float* par = a.par + (size_t)r * 4 * NH;          // alpha_A, alpha_B, beta_A, beta_B (best)
  float* cur = a.scratch + (size_t)r * (a.feas ? 16 : 12) * NH;   // current
  float* mom = cur + 4 * NH;
  float* vel = cur + 8 * NH;
  // crossed bounds prove the region empty only through a fixed phase: with none fixed they are not
  // sound bounds of a non-empty box, so the node gets no bound (NaN: its partition stops, UNKNOWN)
  const bool corrupt = __any(bad) && !__any(fixd);
  if (a.skip && a.skip[r]) bad = 1;         // closed before bounding: same outputs as an empty region
  if (a.feas) {
    // infeasibility pass: only nodes the main pass left open and that fix some phase
    int fixed = 0;
    for (int c = 0; c < 2; ++c)
      for (int k = lane; k < NH; k += 64) fixed |= S.ph[c][k] != 0;
    if (__any(bad) || !__any(fixed) || !(a.bound[r] < 0.0)) return;
  }
  if (__any(bad)) {
    if (lane == 0) {
      a.bound[r] = (corrupt && !(a.skip && a.skip[r])) ? __builtin_nan("") : __builtin_inf();
      a.split[r] = -(2 * n0 + 1);
      a.binit[2 * r] = 0.f;
      a.binit[2 * r + 1] = 0.f;
    }
    for (int i = lane; i < n0; i += 64) {
      a.xstar[(size_t)r * n0 + i] = N.lo[i];
      if (a.xpstar) a.xpstar[(size_t)r * n0 + i] = N.ramask >> i & 1ull ? N.plo[i] : N.lo[i];
    }
    return;
  }
  // every neuron's state (par / cur / Adam moments, the pgap sums) is touched by the SAME lane
  // everywhere (lane j of its layer, j mod 64), so no lane reads a global word another lane of the
  // wave wrote (the scores and the split neuron's binit use that mapping too)
  const float* pg = (a.pgsum && a.pgn) ? a.pgsum + (size_t)r * 4 * NH : nullptr;
  // two-phase infeasibility pass: the batched optimiser's proposals instead of the pass's own start values
  const float* fpr = (a.feas && a.iters == 0 && a.fpar) ? a.fpar + (size_t)r * 4 * NH : nullptr;
  for (int l = 0; l < L - 1; ++l)
    for (int j = lane; j < nd.dims[l + 1]; j += 64)
      for (int q = 0; q < 4; ++q) {
        const int k = q * NH + nd.neuron_off[l] + j;
        // feas: the phase multipliers start at 0.5 on the fixed neurons (0 elsewhere), the slopes at the
        // main pass's best
        float c0 = a.feas && q >= 2 ? (S.ph[q - 2][k - q * NH] != 0 ? 0.5f : 0.f) : par[k];
        // (untrusted: a slope is clamped to [0, 1] here -- NaN gives 0 --; bwd zeroes an unfixed neuron's
        // multiplier and sends a negative one to the interval side; a NaN multiplier gives a NaN value,
        // which closes nothing)
        if (fpr) c0 = q < 2 ? fminf(fmaxf(fpr[k], 0.f), 1.f) : fpr[k];
        cur[k] = c0;
        if (a.feas) cur[12 * NH + k] = cur[k];          // best iterate of the pass
        mom[k] = 0.f;
        vel[k] = 0.f;
        // (q-invariant: the sums of neuron nd.neuron_off[l] + j; two-phase level: the optimiser's)
        const int kn = k - q * NH;
        S.zb[0][kn] = pg ? pg[kn] : 0.f;
        S.zb[1][kn] = pg ? pg[NH + kn] : 0.f;
        S.hb[0][kn] = pg ? pg[2 * NH + kn] : 0.f;
        S.hb[1][kn] = pg ? pg[3 * NH + kn] : 0.f;
      }
  float tc = a.t[r], tbest = tc, mt = 0.f, vt = 0.f;
  // orientation: the objective og (t N_A - (1 - t) N_B) rules out N_A < 0 < N_B (og = +1) or the reverse;
  // the infeasibility pass weighs it 0
  const float og = (a.osg ? (float)a.osg[r] : 1.f) * (a.feas ? 0.f : 1.f);
  float* fbest = cur + 12 * NH;                      // feas: the pass's best parameters (not par)
  float best = -FLT_MAX;
  // relaxed: the tie's multipliers of this lane's RA dim (lane = input dim; n0 <= 64)
  const bool my_ra = N.tie && lane < n0 && ((N.ramask >> lane) & 1ull);
  float* gio = N.tie ? a.gtie + (size_t)r * 2 * n0 : nullptr;
  float gbp = 0.f, gbm = 0.f, mgp = 0.f, vgp = 0.f, mgm = 0.f, vgm = 0.f;
  if (lane < n0) {
    S.gt[0][lane] = my_ra && !a.feas ? gio[lane] : 0.f;
    S.gt[1][lane] = my_ra && !a.feas ? gio[n0 + lane] : 0.f;
    if (fpr && a.fgt && my_ra) {       // the proposed tie multipliers, clamped to >= 0 (NaN gives 0)
      S.gt[0][lane] = fmaxf(a.fgt[(size_t)r * 2 * n0 + lane], 0.f);
      S.gt[1][lane] = fmaxf(a.fgt[(size_t)r * 2 * n0 + n0 + lane], 0.f);
    }
    gbp = S.gt[0][lane];
    gbm = S.gt[1][lane];
  }
  wsync();
  float* cA = reinterpret_cast<float*>(S.cf[0]);   // fp32 passes borrow the rigorous arrays
  float* cB = reinterpret_cast<float*>(S.cf[1]);
  const float b1c = 0.9f, b2c = 0.999f;
  float p1 = 1.f, p2 = 1.f, dk = 1.f;
  // primal iterates summed (pgap): weight 1 (mode 1), it + 1 (mode 2: later iterates count more), or
  // 1 on the second half of the steps only (mode 3)
  float nacc = pg ? a.pgn[r] : 0.f;
  for (int it = 0; it < a.iters; ++it) {
    const float kA = bwd<float, false, true, WTL>(nd, Wf, Wt, S, 0, og * tc, cur, cur + 2 * NH, -1, 0, cA, nullptr,
                                                  nullptr);
    const float kB = bwd<float, false, true, WTL>(nd, Wf, Wt, S, 1, -og * (1.f - tc), cur + NH, cur + 3 * NH, -1, 0, cB,
                                                  nullptr, nullptr);
    const float Bv = conc<float, false, true>(nd, S, N, cA, cB, kA, kB, 0.f);
    if (Bv > best) {
      best = Bv;
      tbest = tc;
      if (lane < n0) {
        gbp = S.gt[0][lane];
        gbm = S.gt[1][lane];
      }
      float* dst = a.feas ? fbest : par;
      for (int l = 0; l < L - 1; ++l)
        for (int j = lane; j < nd.dims[l + 1]; j += 64)
          for (int q = 0; q < 4; ++q) dst[q * NH + nd.neuron_off[l] + j] = cur[q * NH + nd.neuron_off[l] + j];
    }
    if (best > 0.f) break;
    const float wi = a.pgap == 2 ? (float)(it + 1) : (a.pgap == 3 ? (2 * it >= a.iters ? 1.f : 0.f) : 1.f);
    const bool acc = a.pgap && wi > 0.f;
    const float oA = fwd<float>(nd, Wf, S, N, 0, N.va, cur, acc ? S.zb[0] : nullptr, S.hb[0], wi);
    const float oB = fwd<float>(nd, Wf, S, N, 1, N.vb, cur + NH, acc ? S.zb[1] : nullptr, S.hb[1], wi);
    if (acc) nacc += wi;
    // Adam (bias-corrected), gradient ascent, projected
    p1 *= b1c;
    p2 *= b2c;
    const float c1 = 1.f - p1, c2 = 1.f - p2;
    for (int c = 0; c < 2; ++c)
      for (int l = 0; l < L - 1; ++l)
      for (int j = lane; j < nd.dims[l + 1]; j += 64) {
        const int k = nd.neuron_off[l] + j;
        const float z = S.z[c][k];
        const int kind = S.kd[c][k];
        const int p = S.ph[c][k];
        // all six words of this neuron's state first (L2 round trips in flight together), then the
        // updates: alpha (projected to [0, 1]) and beta (>= 0; the infeasibility pass boxes it in [0, 1])
        float* xa = cur + c * NH + k;
        float* ma = mom + c * NH + k;
        float* va_ = vel + c * NH + k;
        float* xb = cur + (2 + c) * NH + k;
        float* mb = mom + (2 + c) * NH + k;
        float* vb_ = vel + (2 + c) * NH + k;
        const float xa0 = *xa, ma0 = *ma, va0 = *va_, xb0 = *xb, mb0 = *mb, vb0 = *vb_;
        {
          const float g = kind == 2 ? S.lam[c][k] * z : 0.f;
          const float mm = b1c * ma0 + (1.f - b1c) * g;
          const float vv = b2c * va0 + (1.f - b2c) * g * g;
          *ma = mm;
          *va_ = vv;
          *xa = fminf(fmaxf(xa0 + a.lr_a * dk * (mm / c1) / (sqrtf(vv / c2) + 1e-8f), 0.f), 1.f);
        }
        {
          float g = 0.f;
          if (p != 0) {
            const float e = xb0 < 0.f ? (p > 0 ? S.ub[c][k] : S.lb[c][k]) : 0.f;
            g = -(float)p * (z - e);
          }
          const float mm = b1c * mb0 + (1.f - b1c) * g;
          const float vv = b2c * vb0 + (1.f - b2c) * g * g;
          *mb = mm;
          *vb_ = vv;
          float nx = xb0 + a.lr_b * dk * (mm / c1) / (sqrtf(vv / c2) + 1e-8f);
          if (a.beta_pos || a.feas) nx = fmaxf(nx, 0.f);
          if (a.feas) nx = fminf(nx, 1.f);              // homogeneous: a box keeps the scale fixed
          *xb = nx;
        }
      }
    if (!a.feas) {
      const float g = og * (oA + oB);
      mt = b1c * mt + (1.f - b1c) * g;
      vt = b2c * vt + (1.f - b2c) * g * g;
      tc = fminf(fmaxf(tc + a.lr_t * dk * (mt / c1) / (sqrtf(vt / c2) + 1e-8f), 0.f), 1.f);
    }
    if (my_ra) {      // tie multipliers: d/d gP = x_r* - x'_r* - tau, d/d gM = x'_r* - x_r* - tau
      const float d = S.xs[lane] - S.xps[lane];
      const float gp = d - N.tau, gm = -d - N.tau;
      mgp = b1c * mgp + (1.f - b1c) * gp;
      vgp = b2c * vgp + (1.f - b2c) * gp * gp;
      mgm = b1c * mgm + (1.f - b1c) * gm;
      vgm = b2c * vgm + (1.f - b2c) * gm * gm;
      const float gmax = a.feas ? 1.f : FLT_MAX;
      S.gt[0][lane] = fminf(fmaxf(S.gt[0][lane] + a.lr_t * dk * (mgp / c1) / (sqrtf(vgp / c2) + 1e-8f), 0.f), gmax);
      S.gt[1][lane] = fminf(fmaxf(S.gt[1][lane] + a.lr_t * dk * (mgm / c1) / (sqrtf(vgm / c2) + 1e-8f), 0.f), gmax);
    }
    dk *= a.decay;
    wsync();
  }
  if (lane == 0 && !a.feas) a.t[r] = a.iters > 0 ? tbest : tc;
  const float tf = a.iters > 0 ? tbest : tc;
  if (a.iters > 0 && lane < n0) {      // the kept (best) tie multipliers
    S.gt[0][lane] = gbp;
    S.gt[1][lane] = gbm;
    if (my_ra && !a.feas) {
      gio[lane] = gbp;
      gio[n0 + lane] = gbm;
    }
  }
  wsync();
  if (a.feas) {
    // rigorous value of the phase constraints' Lagrangian at the pass's best multipliers: > 0 proves
    // that no point of the (relaxed) region satisfies every fixed phase -- the node is closed
    const float* fp = a.iters > 0 ? fbest : cur;
    double eA = 0, eB = 0;
    const double kA = bwd<double, true, true, WTL>(nd, Wf, Wt, S, 0, 0.0, fp, fp + 2 * NH, -1, 0, S.cf[0], &eA,
                                                   nullptr);
    const double kB = bwd<double, true, true, WTL>(nd, Wf, Wt, S, 1, 0.0, fp + NH, fp + 3 * NH, -1, 0, S.cf[1], &eB,
                                                   nullptr);
    const double Bf = conc<double, true, false>(nd, S, N, S.cf[0], S.cf[1], kA, kB, eA + eB);
    if (lane == 0 && Bf > 0.0) a.bound[r] = __builtin_inf();
    if (lane == 0 && a.fval) a.fval[r] = Bf;
    return;
  }

  // ---- rigorous fp64 bound at the kept parameters
  double eA = 0, eB = 0;
  const double kA = bwd<double, true, true, WTL>(nd, Wf, Wt, S, 0, (double)og * (double)tf, par, par + 2 * NH, -1, 0, S.cf[0],
                                                 &eA, nullptr);
  const double kB = bwd<double, true, true, WTL>(nd, Wf, Wt, S, 1, -(double)og * (1.0 - (double)tf), par + NH, par + 3 * NH, -1,
                                                 0, S.cf[1], &eB, nullptr);
  const double Bd = conc<double, true, true>(nd, S, N, S.cf[0], S.cf[1], kA, kB, eA + eB);
  (void)fwd<double>(nd, Wf, S, N, 0, N.va, par);
  (void)fwd<double>(nd, Wf, S, N, 1, N.vb, par + NH);
  for (int i = lane; i < n0; i += 64) {
    a.xstar[(size_t)r * n0 + i] = S.xs[i];
    if (a.xpstar) a.xpstar[(size_t)r * n0 + i] = S.xps[i];
  }

  // a closed node is not branched: no scores, no look-ahead
  if (Bd >= 0.0) {
    if (lane == 0) {
      a.bound[r] = Bd;
      a.split[r] = -(2 * n0 + 1);
      a.binit[2 * r] = 0.f;
      a.binit[2 * r + 1] = 0.f;
    }
    return;
  }
  // ---- branching scores of unfixed unstable neurons: |lam| x relaxation gap at x*, or (pgap) the
  // primal gap mean(h) - relu(mean(z)) over the optimisation steps (the verified LP's rule,
  // smt/lpbab.py:_lp_bab, at the ergodic primal point).  Same lane mapping as the writers of par.
  const bool use_pg = a.pgap && nacc > 0.f;
  const float inv_n = 1.f / (nacc > 0.f ? nacc : 1.f);
  for (int c = 0; c < 2; ++c)
    for (int l = 0; l < L - 1; ++l)
      for (int j = lane; j < nd.dims[l + 1]; j += 64) {
        const int k = nd.neuron_off[l] + j;
        const int kind = S.kd[c][k];
        float s = 0.f;
        if (use_pg) {
          const float lbj = S.lb[c][k], ubj = S.ub[c][k];
          if (S.ph[c][k] == 0 && lbj < 0.f && ubj > 0.f) {
            const float zm = S.zb[c][k] * inv_n, hm = S.hb[c][k] * inv_n;
            s = fmaxf(hm - fmaxf(zm, 0.f), 0.f);
          }
        } else if (kind >= 2 && S.ph[c][k] == 0) {
          const float z = S.z[c][k];
          const float rz = fmaxf(z, 0.f);
          float gap;
          if (kind == 2) gap = rz - par[c * NH + k] * z;
          else {
            const float lbj = S.lb[c][k], ubj = S.ub[c][k];
            gap = ubj / (ubj - lbj) * (z - lbj) - rz;
          }
          s = fabsf(S.lam[c][k]) * fabsf(gap);
        }
        S.sc[c * NH + k] = s;
      }
  wsync();
  int j0;
  float mx;
  {
    float v = -1.f;
    int iv = 0x7fffffff;
    for (int k = lane; k < 2 * NH; k += 64)
      if (S.sc[k] > v) {
        v = S.sc[k];
        iv = k;
      }
    mx = wargmax(v, iv, &j0);
  }
  int jsel = j0;
  if (a.lookahead > 0 && mx > 0.f) {
    // filtered look-ahead: top-K by gap score, then top-K by chord intercept; each candidate's two
    // children are bounded at this node's parameters (new multiplier 0), the best worse child wins
    const int K = a.lookahead < 16 ? a.lookahead : 16;
    int nc = 0;
    for (int pass = 0; pass < 2; ++pass) {
      if (pass == 1) {
        for (int c = 0; c < 2; ++c)
          for (int k = lane; k < NH; k += 64) {
            float s = 0.f;
            if (S.kd[c][k] == 3 && S.ph[c][k] == 0) {
              const float lbj = S.lb[c][k], ubj = S.ub[c][k];
              s = fabsf(S.lam[c][k] * ubj / (ubj - lbj) * lbj);
            }
            S.sc[c * NH + k] = s;
          }
        wsync();
      }
      for (int q = 0; q < K; ++q) {
        float v = -1.f;
        int iv = 0x7fffffff;
        for (int k = lane; k < 2 * NH; k += 64)
          if (S.sc[k] > v) {
            v = S.sc[k];
            iv = k;
          }
        int jq;
        const float vq = wargmax(v, iv, &jq);
        if (!(vq > 0.f)) break;
        if (lane == 0) {
          cand[nc] = jq;
          S.sc[jq] = -1.f;
        }
        ++nc;
        wsync();
      }
    }
    float bw = -FLT_MAX;
    int bj = -1;
    float* cA32 = S.cft;
    for (int q = 0; q < nc; ++q) {
      const int jq = cand[q];
      const int c = jq >= NH ? 1 : 0;
      const int k = jq - c * NH;
      float worst = FLT_MAX;
      for (int sg = -1; sg <= 1; sg += 2) {
        int inf = 0;
        const float sc_c = c == 0 ? og * tf : -og * (1.f - tf);
        const float kc = bwd<float, false, false, WTL>(nd, Wf, Wt, S, c, sc_c, par + c * NH, par + (2 + c) * NH, k, sg,
                                                       cA32, nullptr, &inf);
        float* oth = reinterpret_cast<float*>(S.b1);       // the other copy's coefficients (fp32)
        for (int i = lane; i < n0; i += 64) oth[i] = (float)S.cf[1 - c][i];
        wsync();
        float Bc = c == 0 ? conc<float, false, false>(nd, S, N, cA32, oth, kc, (float)kB, 0.f)
                          : conc<float, false, false>(nd, S, N, oth, cA32, (float)kA, kc, 0.f);
        if (inf) Bc = FLT_MAX;
        worst = fminf(worst, Bc);
        wsync();
      }
      if (worst > bw) {
        bw = worst;
        bj = jq;
      }
    }
    if (bj >= 0) jsel = bj;
    // no candidate's children beat this node: the relaxations are not what keeps it open -- split
    // the input box instead (as the verified LP does)
    if (a.stall && (double)bw <= Bd) mx = 0.f;
  }
  // ---- outputs
  if (mx > 0.f) {
    // the split neuron's child multipliers, written by the lane that owns its par entries
    const int c = jsel >= NH ? 1 : 0;
    const int k = jsel - c * NH;
    int l = 0;
    while (l < L - 2 && k >= nd.neuron_off[l + 1]) ++l;
    if (lane == ((k - nd.neuron_off[l]) & 63)) {
      const float lam = S.lam[c][k];
      const int kind = S.kd[c][k];
      float slope = 0.f;
      if (kind == 2) slope = par[c * NH + k];
      else if (kind == 3) slope = S.ub[c][k] / (S.ub[c][k] - S.lb[c][k]);
      a.binit[2 * r] = lam * slope;
      a.binit[2 * r + 1] = lam * (1.f - slope);
    }
  }
  if (lane == 0) {
    a.bound[r] = Bd;
    int sp;
    if (mx > 0.f) {
      sp = jsel;
    } else {
      // input split: |coefficient| x width over x's non-PA dims (an RA dim: copy A's coefficient)
      // and, relaxed, x''s RA dims (copy B's, code n0 + d); none left: a lattice leaf
      float bv = -1.f;
      int bd = -1;
      for (int i = 0; i < n0; ++i) {
        if ((N.pamask >> i) & 1ull) continue;
        const bool ra = (N.ramask >> i) & 1ull;
        const float wd = N.hi[i] - N.lo[i];
        const double dg = ra && N.tie ? (double)S.gt[0][i] - (double)S.gt[1][i] : 0.0;
        if (wd > 0.f) {
          const float s = (float)fabs(ra ? S.cf[0][i] + dg : S.cf[0][i] + S.cf[1][i]) * wd + 1e-9f * wd;
          if (s > bv) {
            bv = s;
            bd = i;
          }
        }
        if (ra) {
          const float wp = N.phi[i] - N.plo[i];
          if (wp > 0.f) {
            const float s = (float)fabs(S.cf[1][i] - dg) * wp + 1e-9f * wp;
            if (s > bv) {
              bv = s;
              bd = n0 + i;
            }
          }
        }
      }
      sp = bd >= 0 ? -1 - bd : -(2 * n0 + 1);
    }
    a.split[r] = sp;
    if (!(mx > 0.f)) {
      a.binit[2 * r] = 0.f;
      a.binit[2 * r + 1] = 0.f;
    }
  }
}

FA_LDS_REGISTER(FA_LDS_K(fa_beta_kernel<1>), FA_LDS_K(fa_beta_kernel<0>), FA_LDS_K(fa_beta_kernel<2>));

}  // namespace

extern "C" size_t fa_beta_slab_floats(const NetDesc& nd) {
  const int NHp = (nd.n_hidden + 3) & ~3;
  const int n0p = (nd.dims[0] + 3) & ~3;
  const int mwp = (nd.max_width + 3) & ~3;
  return (size_t)(15 * NHp + 4 * mwp + 13 * n0p + 32);
}

// Launch configuration: waves per workgroup and whether the transposed weights fit in LDS next to
// the forward copy, chosen to maximise the waves resident per CU -- the kernel is latency bound, so
// resident waves are what hides its LDS / L2 round trips: min(workgroups per CU by LDS x waves per
// workgroup, FA_BETA_WPE x 4 SIMDs by registers); ties keep the LDS-staged transposed weights.
// Returns 0 on success, -1 when the network cannot run here (inputs > 64, no hidden layer, too many
// PA dims, the weights alone over the LDS budget).
extern "C" int fa_beta_config(const NetDesc& nd, int* wpb, int* wtl, size_t* bytes) {
  if (nd.dims[0] > 64 || nd.n_layers < 2 || nd.n_hidden <= 0) return -1;
  const int L = nd.n_layers;
  const size_t tot = (size_t)nd.b_off[L - 1] + nd.dims[L];
  const size_t tot4 = (tot + 3) & ~(size_t)3;
  const size_t slab = fa_beta_slab_floats(nd) * 4;
  const size_t lds_cu = 160 * 1024, cap = 160 * 1024 - 1024;
  const int reg_waves = 4 * FA_BETA_WPE;
  // FAIRIFY_BETA_WM=0/1/2 forces the weight placement (tests: every mode gives the same bounds)
  const char* fw = getenv("FAIRIFY_BETA_WM");
  const int force = (fw && *fw >= '0' && *fw <= '2') ? *fw - '0' : -1;
  int best = 0;
  for (int t : {1, 0, 2})             // (ties keep the earlier: more of the weights in LDS)
    for (int w : {8, 4, 2, 1}) {
      if (force >= 0 && t != force) continue;
      const size_t b = tot4 * 4 * (t == 1 ? 2 : (t == 0 ? 1 : 0)) + w * slab;
      if (b > cap) continue;
      const int per_cu = std::min((int)(lds_cu / b) * w, reg_waves);
      if (per_cu > best) {
        best = per_cu;
        *wpb = w;
        *wtl = t;
        *bytes = b;
      }
    }
  return best > 0 ? 0 : -1;
}

extern "C" int fa_beta_launch(const NetDesc& nd, BetaArgs a, hipStream_t stream) {
  if (a.R <= 0) return 0;
  int wpb = 0, wtl = 0;
  size_t bytes = 0;
  if (fa_beta_config(nd, &wpb, &wtl, &bytes) != 0) return -1;
  if (!fa_lds_ok(bytes)) return -2;
  a.wpb = wpb;
  a.wt_lds = wtl;
  const dim3 grid((a.R + wpb - 1) / wpb);
  const dim3 block(64 * wpb);
  if (wtl == 1)
    hipLaunchKernelGGL(fa_beta_kernel<1>, grid, block, bytes, stream, nd, a);
  else if (wtl == 2)
    hipLaunchKernelGGL(fa_beta_kernel<2>, grid, block, bytes, stream, nd, a);
  else
    hipLaunchKernelGGL(fa_beta_kernel<0>, grid, block, bytes, stream, nd, a);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}
