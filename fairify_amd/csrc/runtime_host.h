// Host layer shared by the three native BaB runtimes (bab_runtime.cpp, relu_runtime.cpp,
// beta_runtime.cpp): error helpers, the exact checker's set-up, geometric buffer growth, the level
// counters, the forward-form buffers, the candidate-point screen and the candidate sink
// (pinned candidate records -> confirmed witnesses -> SAT flags on the device).  What differs per
// runtime -- root staging, the level bodies, the settle calls, the result assembly -- stays there.
//
// Buffer-lifetime rule (checked on this header and on the runtimes by tests/test_stream_lifetime.py):
// the host side of EVERY hipMemcpyAsync is a runtime-owned pinned fa_mem::HostBuf, never a pageable
// std::vector / numpy temporary, and nothing writes, releases or regrows it before the
// hipStreamSynchronize that retires the copy (so a released block is idle when the cache hands it
// to another runtime).
#pragma once

#include <hip/hip_runtime.h>
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "args.h"
#include "devmem.h"
#include "exact_host.h"

extern "C" int fa_bounds_launch(const NetDesc& net, BoundArgs args, hipStream_t stream);
extern "C" int fa_point_try_launch(const NetDesc& net, BoundArgs a, hipStream_t stream);
extern "C" int fa_set_status_launch(const int* idx, int n, int8_t* status, int8_t v, hipStream_t stream);

namespace fa_rt {

namespace py = pybind11;

inline void ck(hipError_t e, const char* what) {
  if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}
inline void ckl(int rc, const char* what) {
  if (rc != 0) throw std::runtime_error(std::string(what) + " launch failed, code " + std::to_string(rc));
}

// gamma_{k+2} of the fp32 error model with unit roundoff `unit`, rounded up
inline float gamma_up(int k, double unit) {
  const double ku = (k + 2) * unit;
  return std::nextafter((float)(ku / (1.0 - ku)), INFINITY);
}

// geometric growth of a pool of `cur` entries to at least `want` (<= cap): doubling from `floor`
inline int grow_to(int cur, int want, int floor, int cap) {
  int n = std::max(cur, floor);
  while (n < want) n = (n > cap / 2) ? cap : n * 2;
  return std::min(n, cap);
}

// fp64 host copy of the network [W_0|b_0|W_1|b_1|...] behind device pointer `flat` plus the
// query's PA / RA masks, for the native exact confirmation
inline fa_exact::ExactChecker make_exact(const NetDesc& net, const float* flat, const std::vector<int>& pa,
                                         const std::vector<int>& ra, float tau) {
  int np = 0;
  for (int l = 0; l < net.n_layers; ++l) np = std::max(np, net.b_off[l] + net.dims[l + 1]);
  std::vector<float> hf(np);
  ck(hipMemcpy(hf.data(), flat, np * sizeof(float), hipMemcpyDeviceToHost), "cp weights");
  fa_exact::ExactChecker e;
  e.n0 = net.dims[0];
  e.n_layers = net.n_layers;
  e.dims.assign(net.dims, net.dims + net.n_layers + 1);
  e.w_off.assign(net.w_off, net.w_off + net.n_layers);
  e.b_off.assign(net.b_off, net.b_off + net.n_layers);
  e.w.assign(hf.begin(), hf.end());
  e.is_pa.assign(e.n0, 0);
  e.is_ra.assign(e.n0, 0);
  for (int k : pa) e.is_pa[k] = 1;
  for (int k : ra) e.is_ra[k] = 1;
  e.tau = tau;
  return e;
}

// The level-end counters (children, candidates) the settle kernels write into fine-grained
// (coherent) pinned words; read after the level-end synchronisation.
struct LevelCounters {
  fa_mem::HostBuf hcount_buf_{true};
  LevelCounters() { hcount_buf_.ensure(4 * sizeof(int)); }
  void reset() { std::memset(hcount_buf_.p, 0, 4 * sizeof(int)); }   // solve start: nothing in flight
  int* host_ptr() { return reinterpret_cast<int*>(hcount_buf_.p); }
  int children() const { return reinterpret_cast<volatile const int*>(hcount_buf_.p)[0]; }
  int candidates() const { return reinterpret_cast<volatile const int*>(hcount_buf_.p)[1]; }
};

// Forward linear forms of `rows` bound rows (lower / upper: coefficients, constant, error), their
// output bounds and, with_layers, every neuron's bounds.
struct FormBufs {
  fa_mem::DevBuf<float> Lc, L0, Le, Uc, U0, Ue, olb, oub, lay_lb, lay_ub;
  void ensure(size_t rows, int n0, int n_neurons, bool with_layers) {
    Lc.ensure(rows * n0); Uc.ensure(rows * n0);
    L0.ensure(rows); Le.ensure(rows); U0.ensure(rows); Ue.ensure(rows);
    olb.ensure(rows); oub.ensure(rows);
    if (with_layers) { lay_lb.ensure(rows * n_neurons); lay_ub.ensure(rows * n_neurons); }
  }
  // forms and output bounds; the layer bounds are the caller's choice per launch
  void fill(BoundArgs& b) const {
    b.out_lb = olb.p; b.out_ub = oub.p;
    b.Lc = Lc.p; b.L0 = L0.p; b.Le = Le.p; b.Uc = Uc.p; b.U0 = U0.p; b.Ue = Ue.p;
  }
  void fill(CrownPhaseArgs& c) const {
    c.out_lb = olb.p; c.out_ub = oub.p;
    c.Lc = Lc.p; c.L0 = L0.p; c.Le = Le.p; c.Uc = Uc.p; c.U0 = U0.p; c.Ue = Ue.p;
    c.layer_lb = lay_lb.p; c.layer_ub = lay_ub.p;
  }
};

// Rigorous bounds of the network at `rows` candidate points: the point kernel where it holds the
// network, else interval bounds of the degenerate boxes.  node_part / dead_part: per-partition
// masked networks (point r reads node_part[r % part_mod]); row_open: skip points of closed nodes
// (point r belongs to node r % open_mod).
inline void screen_points(const NetDesc& net, const float* flat, const float* pts, int rows, float* lb, float* ub,
                          hipStream_t st, const int* node_part = nullptr, int part_mod = 0,
                          const uint8_t* dead_part = nullptr, const uint8_t* row_open = nullptr, int open_mod = 0) {
  BoundArgs b{};
  b.flat = flat; b.lo = pts; b.hi = pts; b.R = rows; b.symbolic = 0;
  b.out_lb = lb; b.out_ub = ub;
  if (dead_part) { b.node_part = node_part; b.part_mod = part_mod; b.dead_part = dead_part; }
  if (row_open) { b.row_open = row_open; b.open_mod = open_mod; }
  const int prc = fa_point_try_launch(net, b, st);
  if (prc < 0) ckl(-prc, "points");
  if (prc == 0) ckl(fa_bounds_launch(net, b, st), "bounds(points)");
}

// Candidate records of one level and what becomes of them.  The split kernels append records
// [cand_alloc_][2 n0 + 1] (x, x', partition id) straight into coherent pinned host memory; the
// level-end synchronisation retires them, confirm_candidates reads them, and the next level's
// split (launched after the confirmation returns) is the next writer.
struct CandSink {
  static constexpr int kMax = 1 << 24;   // candidates confirmable per BFS level
  fa_mem::HostBuf cand_host_{true};
  fa_mem::HostBuf hidx_;                 // confirmed-SAT partition ids before fa_set_status
  fa_mem::DevBuf<int> idx_;
  int cand_alloc_ = 0;
  const int n0_;
  explicit CandSink(int n0) : n0_(n0) {}

  float* records() { return reinterpret_cast<float*>(cand_host_.p); }

  // room for `need` records (doubling from `floor`, at most kMax); called at a level start
  void ensure_cand(long long need, int floor) {
    if (need <= cand_alloc_) return;
    const int n = grow_to(cand_alloc_, (int)std::min<long long>(need, kMax), floor, kMax);
    cand_host_.ensure((size_t)n * (2 * n0_ + 1) * sizeof(float));
    cand_alloc_ = n;
  }

  // Called once per level, right after the level-end synchronisation, WITHOUT the GIL (taken only
  // around the Python callback).  Native exact check (chk; null: off, as for per-partition masked
  // networks): pair constraints + fp64 logits with a rigorous rounding bound; only pairs whose
  // sign the bound cannot settle go to `confirm` (exact rational arithmetic).  Newly SAT
  // partitions get status 1 on the device: their nodes are skipped from the next level on.
  void confirm_candidates(int n_cand, fa_exact::Witnesses& w, const fa_exact::ExactChecker* chk, py::object& confirm,
                          int8_t* status, hipStream_t st) {
    const size_t w2 = (size_t)2 * n0_;
    const std::vector<float> rec(records(), records() + (size_t)n_cand * (w2 + 1));
    const std::vector<int> newly = fa_exact::select_witnesses(
        rec.data(), n_cand, w, chk,
        [&](const std::vector<int>& slots, const std::vector<float>& pairs, const std::vector<int>& parts) {
          py::gil_scoped_acquire gil;
          const int na = (int)slots.size();
          py::array_t<float> abuf({na, 2 * n0_});
          py::array_t<int> aparts(na);
          std::memcpy(abuf.mutable_data(), pairs.data(), sizeof(float) * pairs.size());
          std::memcpy(aparts.mutable_data(), parts.data(), sizeof(int) * parts.size());
          py::array_t<bool> res = confirm(aparts, abuf).cast<py::array_t<bool>>();
          if (res.size() != na) throw std::runtime_error("candidate confirmation: answer count mismatch");
          return std::vector<char>(res.data(), res.data() + na);
        });
    if (newly.empty()) return;
    idx_.ensure(newly.size());
    hidx_.ensure(newly.size() * sizeof(int));
    std::memcpy(hidx_.p, newly.data(), newly.size() * sizeof(int));
    ck(hipMemcpyAsync(idx_.p, hidx_.p, newly.size() * sizeof(int), hipMemcpyHostToDevice, st), "cp idx");
    ckl(fa_set_status_launch(idx_.p, (int)newly.size(), status, 1, st), "set_status");
    // no sync: the next level's kernels are stream-ordered after set_status, and hidx_.p / idx_
    // are only rewritten by the next call, which runs after the next level-end sync (the sync
    // that retires this copy -- the buffer-lifetime rule above)
  }
};

}  // namespace fa_rt
