// Batched optimisation phase of the beta-CROWN level on gfx950 MFMA: 16 BaB nodes per wave64
// (opt-in, BetaConfig.batched; semantics: the `for (it < a.iters)` loop of fa_beta_kernel,
// csrc/beta.hip, whose fp64 rigorous pass still computes every bound -- this kernel only proposes
// the parameters (alpha, beta, t, tie multipliers) and the primal-gap sums).
//
// Mapping: node 16 g + (lane & 15) is MFMA column lane & 15 of wave-group g.  Nodes of one network
// share W; what differs per node is the multiplier vector, and that is the B operand.  A vector over
// a layer's neurons lives transposed in accumulator layout (reg i of tile t = neuron
// 16 t + 4 (lane >> 4) + i), so a backward step is lam_{l-1} = W_l . mu_l on v_mfma_f32_16x16x4_f32
// with mu formed elementwise in registers, a forward step of the linearised network the same with
// the forward operand order, and the accumulator tile of one layer is the operand of the next.
// Both operand orders of W (the blocks NetDesc::wperm_off / wback_off of `flat`) are staged once
// per workgroup in LDS.  Copy A and copy B are two independent accumulator chains per wave.
//
// Per-neuron state (clamped bounds, phases, the current parameter and its Adam moments -- beta of a
// fixed neuron, alpha of a free one; the other one never moves --, the recorded lam, the primal sums) lives in a per-group block of `scratch` in the layout [quantity][tile slot][lane][4]:
// every access is one 16-byte word per lane, 1 KB contiguous per wave, and a lane only ever reads
// words it wrote itself.  Per-node scalars (t, its moments, the best value, the frozen flag) are
// registers, replicated in the four lanes of a column.
//
// Neighbour independence: an MFMA column depends on its own B column only, the per-column sums go
// over the four lanes of the column in a fixed order, and nothing else crosses columns -- a node's
// outputs are bitwise the same whatever shares its wave and whatever R is.
//
// Feas mode (template parameter FEAS; opt-in, BetaConfig.batched_feas): the proposal phase of the
// infeasibility pass -- the `a.feas` branches of fa_beta_kernel, ops/beta.py:feasibility_ref.  Rows
// that run: bound < 0, some phase fixed in either copy, not skipped, bounds not crossed.  Objective
// weight 0 (the backward pass starts from a zero multiplier at the logit); a fixed neuron's multiplier
// starts at 0.5, a free neuron's slope at par, the tie multipliers at 0, all projected to [0, 1]; t is
// read, never updated (so the forward chain stops at the last hidden layer); no primal sums.  The best
// iterate goes to BetaArgs::fpar / fgt -- par, t and gtie are only read: the children inherit the
// main pass's best.  fa_beta_kernel at feas = 1, iters = 0 then decides on its rigorous fp64 value.
//
// Freeze rule: a column whose best value exceeds 0 stops updating (state, sums and parameters keep
// their values; its lanes still run the wave's MFMAs).  The wave ends when every column is frozen or
// after a.iters steps.  Skipped nodes, empty regions and crossed bounds are frozen from the start
// and get no output (the second phase treats them as before).
//
// Registers (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage), no scratch in
// any instance (main mode; the feas instances: profiles/r8/feas16/README.md): 1 tile 155 VGPRs, 2 tiles 219 (amdgpu_waves_per_eu 2: two waves per SIMD), 4 tiles
// 255 + 38 AGPRs, 7 tiles 256 + 74 AGPRs (hint 1: one wave per SIMD; at two waves per SIMD they
// spill some 200 / 480 B per lane).  Four waves per workgroup (__launch_bounds__(256): the 4- and 7-tile
// instances need more than 256 registers per lane); the staged weights allow 4 workgroups per CU
// on the 64-32-16-8-4 chains (34 KB) and one on AC-4 (127 KB).
#include <float.h>

#include <algorithm>

#include "args.h"

extern "C" int fa_beta_launch(const NetDesc& nd, BetaArgs a, hipStream_t stream);

namespace {

// per-copy quantities of the scratch block
// (Q_X: the neuron's one live parameter -- beta when its phase is fixed, else alpha: a fixed neuron is
// never relaxed with alpha and a free one has no split multiplier, so the other parameter's gradient is
// identically 0 and it keeps its start value in par; Q_M / Q_V: that parameter's Adam moments)
enum { Q_LB = 0, Q_UB, Q_PH, Q_X, Q_M, Q_V, Q_LAM, Q_ZS, Q_HS, Q_N };
// tie state (relaxed): gP, gM, their Adam moments, the best pair; two input tiles each
enum { G_P = 0, G_M, G_MP, G_VP, G_MM, G_VM, G_BP, G_BM, G_N };

struct Opt16Cfg {
  int wf[FA_MAX_LAYERS];     // LDS float offset of layer l's forward operand-order W
  int bl[FA_MAX_LAYERS];     // ... of its bias
  int wb[FA_MAX_LAYERS];     // ... of its backward operand-order W
  int slot[FA_MAX_LAYERS];   // first tile slot of hidden layer l
  int TS;                    // tile slots (16 neurons each) of all hidden layers
  int gfloats;               // scratch floats per wave-group
  int wpb;                   // waves per workgroup
  float* pgsum;              // [R, 4, NH] out: sums of zA, zB, hA, hB
  float* pgn;                // [R] out: sum of the weights
};

__device__ __forceinline__ float colsum(float v) {      // over the four lanes that hold a column
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

__device__ __forceinline__ float& f4(float4& v, int i) { return reinterpret_cast<float*>(&v)[i]; }

// The optimiser only proposes parameters (the fp64 rigorous pass bounds them whatever they are), so
// its steps use the hardware reciprocal and square root (1 ulp) instead of the IEEE sequences: the
// elementwise work, not the MFMAs, is most of this kernel's instructions.
__device__ __forceinline__ float fdiv(float a, float b) { return a * __builtin_amdgcn_rcpf(b); }

// one bias-corrected Adam step: m / c1 / (sqrt(v / c2) + eps) with ic1 = 1 / c1, ic2 = 1 / c2
__device__ __forceinline__ float adam_dir(float m, float v, float ic1, float ic2) {
  return fdiv(m * ic1, __builtin_amdgcn_sqrtf(v * ic2) + 1e-8f);
}

#ifndef FA_B16_WPE
#define FA_B16_WPE(TM) ((TM) <= 2 ? 2 : 1)
#endif

// FEAS: the proposal phase of the infeasibility pass (see the head of this file)
template <int TM, bool FEAS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(FA_B16_WPE(TM)))) void fa_beta_opt16_kernel(
    NetDesc nd, BetaArgs a, Opt16Cfg cfg) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int T0 = TM < 2 ? TM : 2;       // input tiles (n0 <= 32)
  const int tid = threadIdx.x;
  {
    const float4* s1 = reinterpret_cast<const float4*>(a.flat + nd.wperm_off);
    const float4* s2 = reinterpret_cast<const float4*>(a.flat + nd.wback_off);
    float4* d1 = reinterpret_cast<float4*>(smem);
    float4* d2 = reinterpret_cast<float4*>(smem + nd.wperm_floats);
    for (int e = tid; e < (nd.wperm_floats >> 2); e += blockDim.x) d1[e] = s1[e];
    for (int e = tid; e < (nd.wback_floats >> 2); e += blockDim.x) d2[e] = s2[e];
  }
  __syncthreads();
  const int lane = tid & 63, col = lane & 15, grp = lane >> 4, wave = tid >> 6;
  const int g = blockIdx.x * cfg.wpb + wave;
  if (g >= ((a.R + 15) >> 4)) return;
  const int L = nd.n_layers, NH = nd.n_hidden, n0 = nd.dims[0], TS = cfg.TS;
  const int r0 = 16 * g + col;
  const bool valid = r0 < a.R;
  const int r = valid ? r0 : a.R - 1;       // padding columns read the last node, write nothing
  float4* S = reinterpret_cast<float4*>(a.scratch + (size_t)g * cfg.gfloats);
  float4* ST = S + (size_t)2 * Q_N * TS * 64;
#define SQ(c, q, s) S[(size_t)((((c) * Q_N + (q)) * TS + (s)) * 64 + lane)]
#define SG(q, t) ST[((q) * 2 + (t)) * 64 + lane]

  const float* nlo = a.lo + (size_t)r * n0;
  const float* nhi = a.hi + (size_t)r * n0;
  const unsigned long long ramask = a.plo ? a.ramask : 0ull;
  const bool tie = ramask && a.gtie;
  const float* nplo = a.plo ? a.plo + (size_t)r * n0 : nullptr;
  const float* nphi = a.phi ? a.phi + (size_t)r * n0 : nullptr;
  const float* nva = a.va + (size_t)r * a.npa;
  const float* nvb = a.vb + (size_t)r * a.npa;
  unsigned long long pamask = 0;
  for (int q = 0; q < a.npa; ++q) pamask |= 1ull << a.pa_idx[q];
  float* par = a.par + (size_t)r * 4 * NH;
  float* gio = tie ? a.gtie + (size_t)r * 2 * n0 : nullptr;

  // ---- pack the node's phase-clamped bounds, phases and start parameters; clear moments and sums
  int bad = 0, fixd = 0;
  {
    const size_t phs = a.ph_stride > 0 ? (size_t)a.ph_stride : (size_t)NH;
    const float4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < 2; ++c) {
      const float* LB = (c ? a.LBB : a.LBA) + (size_t)r * NH;
      const float* UB = (c ? a.UBB : a.UBA) + (size_t)r * NH;
      const int8_t* PH = (c ? a.phB : a.phA) + (size_t)r * phs;
      for (int l = 0; l < L - 1; ++l) {
        const int w = nd.dims[l + 1], off = nd.neuron_off[l], tout = (w + 15) >> 4;
        for (int t = 0; t < tout; ++t) {
          float4 lb4 = zero, ub4 = zero, ph4 = zero, x4 = zero;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int j = 16 * t + 4 * grp + i;
            if (j < w) {
              const int k = off + j;
              const int p = PH[k];
              float lb = LB[k], ub = UB[k];
              if (p > 0) lb = fmaxf(lb, 0.f);
              if (p < 0) ub = fminf(ub, 0.f);
              if (lb > ub) bad = 1;
              f4(lb4, i) = lb;
              f4(ub4, i) = ub;
              f4(ph4, i) = (float)p;
              if (p != 0) fixd = 1;
              // (feas: a phase multiplier starts at 0.5, a slope at the main pass's best)
              f4(x4, i) = FEAS && p != 0 ? 0.5f : par[(p != 0 ? 2 + c : c) * NH + k];
            }
          }
          const int s = cfg.slot[l] + t;
          SQ(c, Q_LB, s) = lb4;
          SQ(c, Q_UB, s) = ub4;
          SQ(c, Q_PH, s) = ph4;
          SQ(c, Q_X, s) = x4;
          SQ(c, Q_M, s) = zero;
          SQ(c, Q_V, s) = zero;
          SQ(c, Q_ZS, s) = zero;
          SQ(c, Q_HS, s) = zero;
        }
      }
    }
    if (tie) {
#pragma unroll
      for (int t = 0; t < T0; ++t) {
        float4 gp4 = zero, gm4 = zero;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int d = 16 * t + 4 * grp + i;
          if (!FEAS && d < n0 && ((ramask >> d) & 1ull)) {      // (feas: the tie multipliers start at 0)
            f4(gp4, i) = gio[d];
            f4(gm4, i) = gio[n0 + d];
          }
        }
        SG(G_P, t) = gp4;
        SG(G_M, t) = gm4;
        SG(G_BP, t) = gp4;
        SG(G_BM, t) = gm4;
        SG(G_MP, t) = zero;
        SG(G_VP, t) = zero;
        SG(G_MM, t) = zero;
        SG(G_VM, t) = zero;
      }
    }
  }
  if (a.skip && a.skip[r]) bad = 1;
  if (FEAS) {     // only nodes the main pass left open and that fix some phase
    fixd |= __shfl_xor(fixd, 16, 64);
    fixd |= __shfl_xor(fixd, 32, 64);
    if (!fixd || !(a.bound[r] < 0.0)) bad = 1;
  }
  bad |= __shfl_xor(bad, 16, 64);
  bad |= __shfl_xor(bad, 32, 64);
  const bool live = valid && !bad;          // a column that is optimised and gets outputs
  bool frozen = !live;
  // feas: the best iterate goes to fpar / fgt (par, t and gtie stay the main pass's); every entry of
  // a live row is defined from the start (the pass's start values: iters = 0 proposes those)
  float* bpar = FEAS ? a.fpar + (size_t)r * 4 * NH : par;
  if (FEAS && live) {
    for (int c = 0; c < 2; ++c)
      for (int l = 0; l < L - 1; ++l) {
        const int w = nd.dims[l + 1], off = nd.neuron_off[l], tout = (w + 15) >> 4;
        for (int t = 0; t < tout; ++t) {
          const float4 ph4 = SQ(c, Q_PH, cfg.slot[l] + t), x4 = SQ(c, Q_X, cfg.slot[l] + t);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int j = 16 * t + 4 * grp + i;
            if (j < w) {
              const bool fx = (&ph4.x)[i] != 0.f;
              bpar[c * NH + off + j] = fx ? par[c * NH + off + j] : (&x4.x)[i];
              bpar[(2 + c) * NH + off + j] = fx ? (&x4.x)[i] : 0.f;
            }
          }
        }
      }
  }

  float tc = a.t[r], tbest = tc, mt = 0.f, vt = 0.f;
  // (feas: objective weight 0 -- the backward pass starts from a zero multiplier at the logit)
  const float og = FEAS ? 0.f : (a.osg ? (float)a.osg[r] : 1.f);
  float best = -FLT_MAX, nacc = 0.f;
  const float b1c = 0.9f, b2c = 0.999f;
  float p1 = 1.f, p2 = 1.f, dk = 1.f;
  const float bL = smem[cfg.bl[L - 1]];

  for (int it = 0; it < a.iters; ++it) {
    const float sc[2] = {og * tc, -og * (1.f - tc)};
    float lam[2][TM][4];
    float cp[2];
    // ---- backward chain of both copies
    {
      const int w = nd.dims[L - 1];
      const float* wl = smem + cfg.wb[L - 1];      // [ot][0][lane'][i']: W[j][0] at lane' = j & 15, i' = 0
#pragma unroll
      for (int t = 0; t < TM; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int j = 16 * t + 4 * grp + i;
          const float wv = j < w ? wl[(t * 64 + 4 * grp + i) * 4] : 0.f;
          lam[0][t][i] = sc[0] * wv;
          lam[1][t][i] = sc[1] * wv;
        }
      cp[0] = grp == 0 ? sc[0] * bL : 0.f;
      cp[1] = grp == 0 ? sc[1] * bL : 0.f;
    }
    for (int l = L - 2; l >= 0; --l) {
      const int w = nd.dims[l + 1], nin = nd.dims[l];
      const int tout = (w + 15) >> 4, tin = (nin + 15) >> 4;
      const float* b = smem + cfg.bl[l];
      float mu[2][TM][4];
#pragma unroll
      for (int t = 0; t < TM; ++t) {
        if (t < tout) {
          const int s = cfg.slot[l] + t;
#pragma unroll
          for (int c = 0; c < 2; ++c) {
            const float4 lb4 = SQ(c, Q_LB, s), ub4 = SQ(c, Q_UB, s), ph4 = SQ(c, Q_PH, s);
            const float4 x4 = SQ(c, Q_X, s);
            float4 lr4;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const int j = 16 * t + 4 * grp + i;
              const float lbj = (&lb4.x)[i], ubj = (&ub4.x)[i], pf = (&ph4.x)[i];
              const float lm = lam[c][t][i];
              const float bet = pf == 0.f ? 0.f : (&x4.x)[i];
              const bool dead = ubj <= 0.f || pf < 0.f;
              const bool act = !dead && (lbj >= 0.f || pf > 0.f);
              float base = 0.f, kap = 0.f;
              if (act) {
                base = lm;
              } else if (!dead) {
                if (lm >= 0.f) {
                  base = lm * (&x4.x)[i];       // (unstable and not fixed: the parameter is alpha)
                } else {
                  base = lm * fdiv(ubj, ubj - lbj);
                  kap = -base * lbj;
                }
              }
              const float m = base - bet * pf;
              // a negative multiplier of a fixed neuron takes the interval side of its region
              const float kb = (pf != 0.f && bet < 0.f) ? bet * pf * (pf > 0.f ? ubj : lbj) : 0.f;
              const bool jv = j < w;
              mu[c][t][i] = jv ? m : 0.f;
              if (jv) cp[c] += m * b[j] + kap + kb;
              f4(lr4, i) = lm;
            }
            SQ(c, Q_LAM, s) = lr4;
          }
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) mu[0][t][i] = mu[1][t][i] = 0.f;
        }
      }
      const float4* wb4 = reinterpret_cast<const float4*>(smem + cfg.wb[l]);
#pragma unroll
      for (int ot = 0; ot < TM; ++ot) {
        f32x4 ZA = {0.f, 0.f, 0.f, 0.f}, ZB = ZA;
        if (ot < tin) {
#pragma unroll
          for (int t = 0; t < TM; ++t) {
            if (t >= tout) break;
            const float4 w4 = wb4[(ot * tout + t) * 64 + lane];
            ZA = fa_mfma4(w4.x, mu[0][t][0], ZA);
            ZB = fa_mfma4(w4.x, mu[1][t][0], ZB);
            ZA = fa_mfma4(w4.y, mu[0][t][1], ZA);
            ZB = fa_mfma4(w4.y, mu[1][t][1], ZB);
            ZA = fa_mfma4(w4.z, mu[0][t][2], ZA);
            ZB = fa_mfma4(w4.z, mu[1][t][2], ZB);
            ZA = fa_mfma4(w4.w, mu[0][t][3], ZA);
            ZB = fa_mfma4(w4.w, mu[1][t][3], ZB);
          }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          lam[0][ot][i] = ZA[i];
          lam[1][ot][i] = ZB[i];
        }
      }
    }
    // ---- concretisation over the node box (coupled input form): x*, x'*, the step's value
    float xs[T0][4], xps[T0][4], gpv[T0][4], gmv[T0][4];
    float part = 0.f;
#pragma unroll
    for (int t = 0; t < T0; ++t) {
      float4 gp4 = {0.f, 0.f, 0.f, 0.f}, gm4 = gp4;
      if (tie) {
        gp4 = SG(G_P, t);
        gm4 = SG(G_M, t);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int d = 16 * t + 4 * grp + i;
        float xa = 0.f, xb = 0.f;
        gpv[t][i] = (&gp4.x)[i];
        gmv[t][i] = (&gm4.x)[i];
        if (d < n0) {
          const float lo = nlo[d], hi = nhi[d];
          const float cA = lam[0][t][i], cB = lam[1][t][i];
          if ((pamask >> d) & 1ull) {
            const int q = __popcll(pamask & ((1ull << d) - 1ull));
            part += cA * nva[q] + cB * nvb[q];
            xa = xb = lo;
          } else if ((ramask >> d) & 1ull) {
            // the tie's multipliers move coefficient between the copies
            const float gp = gpv[t][i], gm = gmv[t][i];
            const float ca = cA + (gp - gm), cb = cB + (gm - gp);
            xa = ca >= 0.f ? lo : hi;
            xb = cb >= 0.f ? nplo[d] : nphi[d];
            part += ca * xa + cb * xb + -a.tau * (gp + gm);
          } else {
            const float cf = cA + cB;
            xa = xb = cf >= 0.f ? lo : hi;
            part += cf * xa;
          }
        }
        xs[t][i] = xa;
        xps[t][i] = xb;
      }
    }
    const float kA = colsum(cp[0]), kB = colsum(cp[1]);
    const float Bv = colsum(part) + kA + kB;
    // ---- best iterate per column; a column whose best value exceeds 0 freezes
    const bool imp = !frozen && Bv > best;
    if (imp) {
      best = Bv;
      tbest = tc;
      if (tie) {
#pragma unroll
        for (int t = 0; t < T0; ++t) {
          SG(G_BP, t) = SG(G_P, t);
          SG(G_BM, t) = SG(G_M, t);
        }
      }
    }
    if (!frozen && best > 0.f) frozen = true;
    const bool upd = !frozen;
    if (!__any(upd || imp)) break;
    const float wi = a.pgap == 2 ? (float)(it + 1) : (a.pgap == 3 ? (2 * it >= a.iters ? 1.f : 0.f) : 1.f);
    const bool acc = !FEAS && a.pgap && wi > 0.f;       // (feas: no primal sums)
    p1 *= b1c;
    p2 *= b2c;
    const float ic1 = 1.f / (1.f - p1), ic2 = 1.f / (1.f - p2);
    // ---- forward chain of the linearised network at x* / x'*, the parameters' Adam step fused in
    float H[2][TM][4];
#pragma unroll
    for (int t = 0; t < TM; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float ha = 0.f, hb = 0.f;
        if (t < T0) {
          const int d = 16 * t + 4 * grp + i;
          if (d < n0) {
            ha = xs[t < T0 ? t : 0][i];
            hb = xps[t < T0 ? t : 0][i];
            if ((pamask >> d) & 1ull) {
              const int q = __popcll(pamask & ((1ull << d) - 1ull));
              ha = nva[q];
              hb = nvb[q];
            }
          }
        }
        H[0][t][i] = ha;
        H[1][t][i] = hb;
      }
    for (int l = 0; l < L - 1; ++l) {
      const int w = nd.dims[l + 1], nin = nd.dims[l], off = nd.neuron_off[l];
      const int tout = (w + 15) >> 4, tin = (nin + 15) >> 4;
      const float* b = smem + cfg.bl[l];
      const float4* wf4 = reinterpret_cast<const float4*>(smem + cfg.wf[l]);
      float H2[2][TM][4];
#pragma unroll
      for (int jt = 0; jt < TM; ++jt) {
        if (jt < tout) {
          f32x4 Z[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
          for (int t = 0; t < TM; ++t) {
            if (t >= tin) break;
            const float4 w4 = wf4[(jt * tin + t) * 64 + lane];
            Z[0] = fa_mfma4(w4.x, H[0][t][0], Z[0]);
            Z[1] = fa_mfma4(w4.x, H[1][t][0], Z[1]);
            Z[0] = fa_mfma4(w4.y, H[0][t][1], Z[0]);
            Z[1] = fa_mfma4(w4.y, H[1][t][1], Z[1]);
            Z[0] = fa_mfma4(w4.z, H[0][t][2], Z[0]);
            Z[1] = fa_mfma4(w4.z, H[1][t][2], Z[1]);
            Z[0] = fa_mfma4(w4.w, H[0][t][3], Z[0]);
            Z[1] = fa_mfma4(w4.w, H[1][t][3], Z[1]);
          }
          const int s = cfg.slot[l] + jt;
#pragma unroll
          for (int c = 0; c < 2; ++c) {
            const float4 lb4 = SQ(c, Q_LB, s), ub4 = SQ(c, Q_UB, s), ph4 = SQ(c, Q_PH, s);
            const float4 lr4 = SQ(c, Q_LAM, s);
            float4 x4 = SQ(c, Q_X, s), m4 = SQ(c, Q_M, s), v4 = SQ(c, Q_V, s);
            float4 zs4 = {0.f, 0.f, 0.f, 0.f}, hs4 = zs4;
            if (acc) {
              zs4 = SQ(c, Q_ZS, s);
              hs4 = SQ(c, Q_HS, s);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const int j = 16 * jt + 4 * grp + i;
              const bool jv = j < w;
              const float lbj = (&lb4.x)[i], ubj = (&ub4.x)[i], pf = (&ph4.x)[i], lm = (&lr4.x)[i];
              const float x0 = (&x4.x)[i];
              const float z = jv ? Z[c][i] + b[j] : 0.f;
              const bool dead = ubj <= 0.f || pf < 0.f;
              const bool act = !dead && (lbj >= 0.f || pf > 0.f);
              const int kind = act ? 1 : (dead ? 0 : (lm >= 0.f ? 2 : 3));
              float h = 0.f;
              if (kind == 1) h = z;
              else if (kind == 2) h = x0 * z;
              else if (kind == 3) h = fdiv(ubj, ubj - lbj) * (z - lbj);
              H2[c][jt][i] = jv ? h : 0.f;
              if (imp && jv) bpar[(pf != 0.f ? 2 + c : c) * NH + off + j] = x0;   // the best iterate
              if (upd && jv) {
                if (acc) {
                  f4(zs4, i) += wi * z;
                  f4(hs4, i) += wi * h;
                }
                // the live parameter's gradient: beta of a fixed neuron, alpha of an unstable free one
                float gr = kind == 2 ? lm * z : 0.f;
                if (pf != 0.f) {
                  const float e = x0 < 0.f ? (pf > 0.f ? ubj : lbj) : 0.f;
                  gr = -pf * (z - e);
                }
                const float mm = b1c * (&m4.x)[i] + (1.f - b1c) * gr;
                const float vv = b2c * (&v4.x)[i] + (1.f - b2c) * gr * gr;
                f4(m4, i) = mm;
                f4(v4, i) = vv;
                const float nx = x0 + (pf != 0.f ? a.lr_b : a.lr_a) * dk * adam_dir(mm, vv, ic1, ic2);
                // alpha projected to [0, 1]; beta >= 0 when beta_pos (feas: to [0, 1] -- the value is
                // homogeneous in the multipliers, a box keeps the scale fixed)
                f4(x4, i) = (pf != 0.f && !FEAS) ? (a.beta_pos ? fmaxf(nx, 0.f) : nx) : fminf(fmaxf(nx, 0.f), 1.f);
              }
            }
            SQ(c, Q_X, s) = x4;
            SQ(c, Q_M, s) = m4;
            SQ(c, Q_V, s) = v4;
            if (acc) {
              SQ(c, Q_ZS, s) = zs4;
              SQ(c, Q_HS, s) = hs4;
            }
          }
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) H2[0][jt][i] = H2[1][jt][i] = 0.f;
        }
      }
#pragma unroll
      for (int t = 0; t < TM; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          H[0][t][i] = H2[0][t][i];
          H[1][t][i] = H2[1][t][i];
        }
    }
    float oA = 0.f, oB = 0.f;
    if (!FEAS) {      // (feas: t is read, never updated -- no logit needed)
      const int tin = (nd.dims[L - 1] + 15) >> 4;
      const float4* wf4 = reinterpret_cast<const float4*>(smem + cfg.wf[L - 1]);
      f32x4 ZA = {0.f, 0.f, 0.f, 0.f}, ZB = ZA;
#pragma unroll
      for (int t = 0; t < TM; ++t) {
        if (t >= tin) break;
        const float4 w4 = wf4[t * 64 + lane];
        ZA = fa_mfma4(w4.x, H[0][t][0], ZA);
        ZB = fa_mfma4(w4.x, H[1][t][0], ZB);
        ZA = fa_mfma4(w4.y, H[0][t][1], ZA);
        ZB = fa_mfma4(w4.y, H[1][t][1], ZB);
        ZA = fa_mfma4(w4.z, H[0][t][2], ZA);
        ZB = fa_mfma4(w4.z, H[1][t][2], ZB);
        ZA = fa_mfma4(w4.w, H[0][t][3], ZA);
        ZB = fa_mfma4(w4.w, H[1][t][3], ZB);
      }
      // the logit is row 0 of the tile: reg 0 of the column's first lane
      oA = __shfl(ZA[0] + bL, col, 64);
      oB = __shfl(ZB[0] + bL, col, 64);
    }
    if (!FEAS && upd) {
      if (acc) nacc += wi;
      const float gr = og * (oA + oB);
      mt = b1c * mt + (1.f - b1c) * gr;
      vt = b2c * vt + (1.f - b2c) * gr * gr;
      tc = fminf(fmaxf(tc + a.lr_t * dk * adam_dir(mt, vt, ic1, ic2), 0.f), 1.f);
    }
    if (tie) {      // tie multipliers: d/d gP = x_r* - x'_r* - tau, d/d gM = x'_r* - x_r* - tau
#pragma unroll
      for (int t = 0; t < T0; ++t) {
        float4 gp4 = SG(G_P, t), gm4 = SG(G_M, t);
        float4 mp4 = SG(G_MP, t), vp4 = SG(G_VP, t), mm4 = SG(G_MM, t), vm4 = SG(G_VM, t);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int d = 16 * t + 4 * grp + i;
          if (upd && d < n0 && ((ramask >> d) & 1ull)) {
            const float df = xs[t][i] - xps[t][i];
            const float gp = df - a.tau, gm = -df - a.tau;
            const float mgp = b1c * (&mp4.x)[i] + (1.f - b1c) * gp;
            const float vgp = b2c * (&vp4.x)[i] + (1.f - b2c) * gp * gp;
            const float mgm = b1c * (&mm4.x)[i] + (1.f - b1c) * gm;
            const float vgm = b2c * (&vm4.x)[i] + (1.f - b2c) * gm * gm;
            f4(mp4, i) = mgp;
            f4(vp4, i) = vgp;
            f4(mm4, i) = mgm;
            f4(vm4, i) = vgm;
            const float gmax = FEAS ? 1.f : FLT_MAX;
            f4(gp4, i) = fminf(fmaxf((&gp4.x)[i] + a.lr_t * dk * adam_dir(mgp, vgp, ic1, ic2), 0.f), gmax);
            f4(gm4, i) = fminf(fmaxf((&gm4.x)[i] + a.lr_t * dk * adam_dir(mgm, vgm, ic1, ic2), 0.f), gmax);
          }
        }
        SG(G_P, t) = gp4;
        SG(G_M, t) = gm4;
        SG(G_MP, t) = mp4;
        SG(G_VP, t) = vp4;
        SG(G_MM, t) = mm4;
        SG(G_VM, t) = vm4;
      }
    }
    dk *= a.decay;
  }

  // ---- outputs: t and the tie multipliers of the best iterate (par was written when it improved),
  // the primal sums of every node (zero for the nodes left to the second phase)
  if (!valid) return;
  if (live && (FEAS || a.iters > 0)) {
    if (!FEAS && grp == 0) a.t[r] = tbest;
    if (FEAS && tie) gio = a.fgt + (size_t)r * 2 * n0;
    if (tie) {
#pragma unroll
      for (int t = 0; t < T0; ++t) {
        const float4 gp4 = SG(G_BP, t), gm4 = SG(G_BM, t);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int d = 16 * t + 4 * grp + i;
          if (d < n0 && ((ramask >> d) & 1ull)) {
            gio[d] = (&gp4.x)[i];
            gio[n0 + d] = (&gm4.x)[i];
          }
        }
      }
    }
  }
  if (FEAS) return;
  if (grp == 0) cfg.pgn[r] = nacc;
  float* pg = cfg.pgsum + (size_t)r * 4 * NH;
  for (int c = 0; c < 2; ++c)
    for (int l = 0; l < L - 1; ++l) {
      const int w = nd.dims[l + 1], off = nd.neuron_off[l], tout = (w + 15) >> 4;
      for (int t = 0; t < tout; ++t) {
        const float4 zs4 = SQ(c, Q_ZS, cfg.slot[l] + t), hs4 = SQ(c, Q_HS, cfg.slot[l] + t);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int j = 16 * t + 4 * grp + i;
          if (j < w) {
            pg[c * NH + off + j] = (&zs4.x)[i];
            pg[(2 + c) * NH + off + j] = (&hs4.x)[i];
          }
        }
      }
    }
#undef SQ
#undef SG
}

FA_LDS_REGISTER(FA_LDS_K((fa_beta_opt16_kernel<1, false>)), FA_LDS_K((fa_beta_opt16_kernel<2, false>)),
                FA_LDS_K((fa_beta_opt16_kernel<4, false>)), FA_LDS_K((fa_beta_opt16_kernel<7, false>)),
                FA_LDS_K((fa_beta_opt16_kernel<1, true>)), FA_LDS_K((fa_beta_opt16_kernel<2, true>)),
                FA_LDS_K((fa_beta_opt16_kernel<4, true>)), FA_LDS_K((fa_beta_opt16_kernel<7, true>)));

// Tile depth, LDS offsets and scratch layout; false when the network is outside the kernel's limits.
bool opt16_cfg(const NetDesc& nd, Opt16Cfg& cfg, int* tm, size_t* bytes) {
  const int L = nd.n_layers;
  if (L < 2 || L > FA_MAX_LAYERS || nd.n_hidden <= 0 || nd.dims[0] > 32 || nd.dims[L] != 1) return false;
  int tmax = (nd.dims[0] + 15) / 16, off = 0, wb = nd.wperm_floats, ts = 0;
  for (int l = 0; l < L; ++l) {
    const int tin = (nd.dims[l] + 15) / 16, tout = (nd.dims[l + 1] + 15) / 16;
    if (l < L - 1) {
      if (nd.dims[l + 1] > 112) return false;
      tmax = std::max(tmax, tout);
      cfg.slot[l] = ts;
      ts += tout;
    }
    cfg.wf[l] = off;
    off += tin * tout * 256;
    cfg.wb[l] = wb;
    wb += tin * tout * 256;
  }
  for (int l = 0; l < L; ++l) {
    cfg.bl[l] = off;
    off += nd.dims[l + 1];
  }
  if (((off + 3) & ~3) != nd.wperm_floats || wb - nd.wperm_floats != nd.wback_floats) return false;
  cfg.TS = ts;
  cfg.gfloats = (2 * Q_N * ts + G_N * 2) * 256;
  *bytes = (size_t)(nd.wperm_floats + nd.wback_floats) * sizeof(float);
  if (*bytes > 160 * 1024 - 1024) return false;
  cfg.wpb = 4;
  *tm = tmax <= 1 ? 1 : (tmax <= 2 ? 2 : (tmax <= 4 ? 4 : 7));
  return true;
}

// launches the instance of tile depth tm in the main (FEAS = false) or the feas mode
template <bool FEAS>
int opt16_run(const NetDesc& nd, const BetaArgs& a, const Opt16Cfg& cfg, int tm, size_t bytes, hipStream_t stream) {
  const int ng = (a.R + 15) / 16;
  const dim3 grid((ng + cfg.wpb - 1) / cfg.wpb), block(64 * cfg.wpb);
  if (tm == 1)
    hipLaunchKernelGGL((fa_beta_opt16_kernel<1, FEAS>), grid, block, bytes, stream, nd, a, cfg);
  else if (tm == 2)
    hipLaunchKernelGGL((fa_beta_opt16_kernel<2, FEAS>), grid, block, bytes, stream, nd, a, cfg);
  else if (tm == 4)
    hipLaunchKernelGGL((fa_beta_opt16_kernel<4, FEAS>), grid, block, bytes, stream, nd, a, cfg);
  else
    hipLaunchKernelGGL((fa_beta_opt16_kernel<7, FEAS>), grid, block, bytes, stream, nd, a, cfg);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace

extern "C" int fa_beta_opt16_fits(const NetDesc& nd) {
  Opt16Cfg cfg;
  int tm = 0;
  size_t bytes = 0;
  return opt16_cfg(nd, cfg, &tm, &bytes) ? 1 : 0;
}

// floats of BetaArgs::scratch the batched optimiser needs for R nodes (0: the network does not fit)
extern "C" size_t fa_beta_opt16_scratch_floats(const NetDesc& nd, int R) {
  Opt16Cfg cfg;
  int tm = 0;
  size_t bytes = 0;
  if (!opt16_cfg(nd, cfg, &tm, &bytes)) return 0;
  return (size_t)((R + 15) / 16) * (size_t)cfg.gfloats;
}

// Phase 1 alone: optimises par / t / gtie of the R nodes in place (best iterate) and writes the
// primal sums pgsum [R, 4, NH] and their weights pgn [R].  0 on success, -1 when the network does
// not fit, -2 LDS limit not raised, -3 launch error, -4 missing buffers.
extern "C" int fa_beta_opt16_launch(const NetDesc& nd, BetaArgs a, float* pgsum, float* pgn, hipStream_t stream) {
  Opt16Cfg cfg;
  int tm = 0;
  size_t bytes = 0;
  if (!opt16_cfg(nd, cfg, &tm, &bytes) || a.npa > FA_MAX_PA || a.feas) return -1;
  if (!pgsum || !pgn || !a.scratch) return -4;
  if (a.R <= 0) return 0;
  if (!fa_lds_ok(bytes)) return -2;
  cfg.pgsum = pgsum;
  cfg.pgn = pgn;
  return opt16_run<false>(nd, a, cfg, tm, bytes, stream);
}

// The proposal phase of the infeasibility pass alone: a.iters steps on the phase constraints'
// Lagrangian of the rows the main pass left open with a fixed phase (a.bound < 0), best iterate to
// a.fpar [R, 4, NH] / a.fgt [R, 2, n0]; par / t / gtie / bound are only read.  Return codes as above.
extern "C" int fa_beta_opt16_feas_launch(const NetDesc& nd, BetaArgs a, hipStream_t stream) {
  Opt16Cfg cfg;
  int tm = 0;
  size_t bytes = 0;
  if (!opt16_cfg(nd, cfg, &tm, &bytes) || a.npa > FA_MAX_PA) return -1;
  const bool tie = a.plo && a.ramask && a.gtie;
  if (!a.fpar || !a.bound || !a.scratch || (tie && !a.fgt)) return -4;
  if (a.R <= 0) return 0;
  if (!fa_lds_ok(bytes)) return -2;
  cfg.pgsum = nullptr;
  cfg.pgn = nullptr;
  return opt16_run<true>(nd, a, cfg, tm, bytes, stream);
}

// The two-phase infeasibility pass: the proposal kernel, then fa_beta_kernel at feas = 1, iters = 0
// on the same stream, which evaluates the rigorous fp64 value at the proposals and closes the row
// (bound := +inf) when it is > 0.  a.scratch must hold max(R * 16 * NH, fa_beta_opt16_scratch_floats).
extern "C" int fa_beta_feas16_launch(const NetDesc& nd, BetaArgs a, hipStream_t stream) {
  a.feas = 1;
  a.pgsum = nullptr;
  a.pgn = nullptr;
  const int rc = fa_beta_opt16_feas_launch(nd, a, stream);
  if (rc != 0) return rc;
  a.iters = 0;
  const int r2 = fa_beta_launch(nd, a, stream);
  return r2 == 0 ? 0 : r2 - 10;
}

// The two-phase level: the batched optimiser, then fa_beta_kernel at iters = 0 on the same stream
// (rigorous fp64 bound at the proposed parameters, scores seeded with the optimiser's primal sums,
// look-ahead, vertices).  a.pgsum / a.pgn are the level's primal-sum buffers.
extern "C" int fa_beta_level16_launch(const NetDesc& nd, BetaArgs a, hipStream_t stream) {
  const int rc = fa_beta_opt16_launch(nd, a, const_cast<float*>(a.pgsum), const_cast<float*>(a.pgn), stream);
  if (rc != 0) return rc;
  a.iters = 0;
  const int r2 = fa_beta_launch(nd, a, stream);
  return r2 == 0 ? 0 : r2 - 10;
}
