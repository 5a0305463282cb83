// Native ReLU-phase branch-and-bound driver (stage "relu", engine/relu_bab.py: the torch path is
// the reference semantics).  Host loop over BFS levels of device-resident node pools; per level
// and sub-batch of nodes:
//   rows (PA values per row) -> forward symbolic bounds with the rows' ReLU phases (symbolic.hip)
//   -> every-layer backward bounds (relu.hip: fa_crown_phase) -> node certificate + vertex pair +
//   branching decision -> rigorous point bounds of the vertex pairs -> candidates / children
// then one settle kernel and ONE host synchronisation; candidate pairs are confirmed exactly on
// the host (fp64 with a rigorous bound, exact_host.h; undecided signs -> Python rational check).
#include <hip/hip_runtime.h>
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "runtime_host.h"

namespace py = pybind11;

extern "C" int fa_crown_phase_launch(const NetDesc& net, CrownPhaseArgs a, hipStream_t stream);
extern "C" int fa_refine_launch(const NetDesc& net, BoundArgs a, hipStream_t stream);
extern "C" int fa_relu_rows_launch(ReluLevelArgs a, hipStream_t stream);
extern "C" int fa_relu_cert_launch(ReluLevelArgs a, hipStream_t stream);
extern "C" int fa_relu_split_launch(ReluLevelArgs a, hipStream_t stream);
extern "C" int fa_relu_settle_launch(int P, int8_t* status, const int* part_nodes, int* nodes_start, int* counters,
                                     int* host_counts, hipStream_t stream);
extern "C" int fa_relu_reset_launch(int* counters, hipStream_t stream);

const NetDesc& fa_net_desc(py::handle net);

namespace {

using fa_rt::ck;
using fa_rt::ckl;

template <typename T>
using RBuf = fa_mem::DevBuf<T>;

}  // namespace

class ReluRuntime {
 public:
  ReluRuntime(py::handle net, uintptr_t flat, std::vector<int> pa, std::vector<float> values_f,
              std::vector<int64_t> pairs, int capacity, int batch_nodes, double unit, int refine,
              std::vector<int> ra, double tau, int norient, py::object keep)
      : net_(fa_net_desc(net)), flat_((const float*)flat), keep_(std::move(keep)), pa_(std::move(pa)),
        cap_(capacity), batch_(batch_nodes), unit_(unit), refine_(refine), ra_(std::move(ra)), tau_((float)tau),
        sink_(net_.dims[0]) {
    n0_ = net_.dims[0];
    nh_ = net_.n_hidden;
    npa_ = (int)pa_.size();
    if (npa_ == 0 || npa_ > FA_CMAX_PA) throw std::invalid_argument("bad PA");
    // relaxed queries (x' RA box per node): at most FA_MAX_RA dims, none of them a PA dim
    relaxed_ = !ra_.empty() && tau_ > 0.f;
    if (!relaxed_) ra_.clear();
    if ((int)ra_.size() > FA_MAX_RA) throw std::invalid_argument("bad RA");
    for (int d : ra_) {
      if (d < 0 || d >= n0_) throw std::invalid_argument("RA dim out of range");
      for (int k : pa_)
        if (k == d) throw std::invalid_argument("RA dim is a PA dim");
    }
    V_ = (int)(values_f.size() / npa_);
    // relaxed queries, norient = 2: both orientations are roots of the same search -- every ordered
    // pair appears twice in the table, the second copy (index >= neg_from_) ruling out the reverse
    // orientation N(x, va) > 0 > N(x', vb) (relu.hip reads the negated logit's forms)
    if (norient == 2 && relaxed_ && !pairs.empty()) {
      neg_from_ = (int)(pairs.size() / 2);
      std::vector<int64_t> twice(pairs);
      twice.insert(twice.end(), pairs.begin(), pairs.end());
      pairs.swap(twice);
    }
    Pp_ = (int)(pairs.size() / 2);
    vals_.ensure(values_f.size());
    pairs_.ensure(std::max<size_t>(pairs.size(), 2));
    ck(hipMemcpy(vals_.p, values_f.data(), values_f.size() * sizeof(float), hipMemcpyHostToDevice), "cp");
    if (!pairs.empty())
      ck(hipMemcpy(pairs_.p, pairs.data(), pairs.size() * sizeof(int64_t), hipMemcpyHostToDevice), "cp");
    const size_t R = 2 * (size_t)batch_;
    rlo_.ensure(R * n0_); rhi_.ensure(R * n0_); rpart_.ensure(R);
    infeas_.ensure(R);
    form_.ensure(R, n0_, net_.n_neurons, true);
    split_.ensure(2 * R); score_.ensure(2 * R);
    open_.ensure(batch_); choice_.ensure(batch_); idim_.ensure(batch_);
    cpts_.ensure(R * n0_); pe_lb_.ensure(R); pe_ub_.ensure(R);
    counters_.ensure(2);
    exact_ = fa_rt::make_exact(net_, flat_, pa_, ra_, tau_);   // ra_ is empty unless relaxed
  }

  py::tuple solve(py::array_t<float, py::array::c_style | py::array::forcecast> lo,
                  py::array_t<float, py::array::c_style | py::array::forcecast> hi,
                  py::array_t<int8_t, py::array::c_style | py::array::forcecast> status0, int budget,
                  double time_budget, py::object confirm, uintptr_t stream_i) {
    hipStream_t st = (hipStream_t)stream_i;
    const auto t0 = std::chrono::steady_clock::now();
    const int P = (int)lo.shape(0);
    if (lo.ndim() != 2 || lo.shape(1) != n0_ || hi.shape(0) != P || status0.shape(0) != P)
      throw std::invalid_argument("relu solve: shape mismatch");
    status_.ensure(P);
    nodes_.ensure(P);
    nodes_start_.ensure(P);
    std::vector<int> run;
    for (int p = 0; p < P; ++p)
      if (status0.data()[p] == 3) run.push_back(p);
    const long long n_root = (long long)run.size() * Pp_;
    if (n_root > cap_) throw std::invalid_argument("more root nodes than pool capacity");
    ensure_pool(0, std::max<long long>(n_root, 1));
    // staged host block: status | part | pair | lo | hi (one H2D copy), then device memsets
    const int nbox = relaxed_ ? 4 : 2;     // lo, hi (+ relaxed: x' lo, hi)
    const size_t sb = (size_t)((P + 3) & ~3) + (size_t)n_root * (2 * sizeof(int) + nbox * n0_ * sizeof(float));
    hstage_.ensure(sb);
    {
      unsigned char* h = hstage_.p;
      std::memcpy(h, status0.data(), P);
      int* hp = reinterpret_cast<int*>(h + ((P + 3) & ~3));
      int* hq = hp + n_root;
      float* hl = reinterpret_cast<float*>(hq + n_root);
      float* hh = hl + n_root * n0_;
      float* hpl = hh + n_root * n0_;        // relaxed only
      float* hph = hpl + n_root * n0_;
      long long k = 0;
      for (int p : run)
        for (int q = 0; q < Pp_; ++q, ++k) {
          hp[k] = p;
          hq[k] = q;
          for (int d = 0; d < n0_; ++d) {
            hl[k * n0_ + d] = lo.data()[(size_t)p * n0_ + d];
            hh[k * n0_ + d] = hi.data()[(size_t)p * n0_ + d];
          }
          if (relaxed_) {                    // x': the RA dims widened by tau, unclipped
            for (int d = 0; d < n0_; ++d) {
              hpl[k * n0_ + d] = hl[k * n0_ + d];
              hph[k * n0_ + d] = hh[k * n0_ + d];
            }
            for (int d : ra_) {
              hpl[k * n0_ + d] -= tau_;
              hph[k * n0_ + d] += tau_;
            }
          }
        }
      stage_.ensure(sb);
      ck(hipMemcpyAsync(stage_.p, hstage_.p, sb, hipMemcpyHostToDevice, st), "cp stage");
      const unsigned char* d = stage_.p;
      ck(hipMemcpyAsync(status_.p, d, P, hipMemcpyDeviceToDevice, st), "cp status");
      d += (P + 3) & ~3;
      ck(hipMemcpyAsync(part_[0].p, d, n_root * sizeof(int), hipMemcpyDeviceToDevice, st), "cp part");
      d += n_root * sizeof(int);
      ck(hipMemcpyAsync(pair_[0].p, d, n_root * sizeof(int), hipMemcpyDeviceToDevice, st), "cp pair");
      d += n_root * sizeof(int);
      ck(hipMemcpyAsync(lo_[0].p, d, n_root * n0_ * sizeof(float), hipMemcpyDeviceToDevice, st), "cp lo");
      d += n_root * n0_ * sizeof(float);
      ck(hipMemcpyAsync(hi_[0].p, d, n_root * n0_ * sizeof(float), hipMemcpyDeviceToDevice, st), "cp hi");
      d += n_root * n0_ * sizeof(float);
      if (relaxed_) {
        ck(hipMemcpyAsync(plo_[0].p, d, n_root * n0_ * sizeof(float), hipMemcpyDeviceToDevice, st), "cp plo");
        d += n_root * n0_ * sizeof(float);
        ck(hipMemcpyAsync(phi_[0].p, d, n_root * n0_ * sizeof(float), hipMemcpyDeviceToDevice, st), "cp phi");
      }
      ck(hipMemsetAsync(phase_[0].p, 0, (size_t)n_root * 2 * nh_, st), "memset phase");
      ck(hipMemsetAsync(nodes_.p, 0, P * sizeof(int), st), "memset nodes");
      ck(hipMemsetAsync(nodes_start_.p, 0, P * sizeof(int), st), "memset nodes_start");
    }
    fa_exact::Witnesses wit(P, n0_, lo.data(), hi.data());
    hcount_.reset();
    int cur = 0;
    long long n_in = n_root;
    int levels = 0;
    bool timed_out = false;
    long long total = 0;
    {
      py::gil_scoped_release nogil;
      while (n_in > 0) {
        const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (el > time_budget) {
          timed_out = true;
          break;
        }
        const int nxt = cur ^ 1;
        ensure_pool(nxt, 2 * n_in);
        sink_.ensure_cand(n_in, 1 << 14);
        ckl(fa_relu_reset_launch(counters_.p, st), "reset");
        for (long long s = 0; s < n_in; s += batch_) {
          const int nb = (int)std::min<long long>(batch_, n_in - s);
          level(cur, nxt, s, nb, P, budget, st);
        }
        ckl(fa_relu_settle_launch(P, status_.p, nodes_.p, nodes_start_.p, counters_.p, hcount_.host_ptr(), st),
            "settle");
        ck(hipStreamSynchronize(st), "sync");
        total += n_in;
        ++levels;
        const int n_out = std::min(hcount_.children(), pool_[nxt]);
        const int n_cand = std::min(hcount_.candidates(), sink_.cand_alloc_);
        if (n_cand > 0) sink_.confirm_candidates(n_cand, wit, &exact_, confirm, status_.p, st);
        cur = nxt;
        n_in = n_out;
      }
    }
    // results
    const size_t hn_off = ((size_t)P + 15) & ~size_t(15);
    hout_.ensure(hn_off + (size_t)P * sizeof(int));
    ck(hipMemcpyAsync(hout_.p, status_.p, P, hipMemcpyDeviceToHost, st), "cp status out");
    ck(hipMemcpyAsync(hout_.p + hn_off, nodes_.p, P * sizeof(int), hipMemcpyDeviceToHost, st), "cp nodes out");
    ck(hipStreamSynchronize(st), "sync");
    const int8_t* hs = reinterpret_cast<const int8_t*>(hout_.p);
    const int* hn = reinterpret_cast<const int*>(hout_.p + hn_off);
    // partitions with nodes left after a time-out
    std::vector<char> left(P, 0);
    if (timed_out && n_in > 0) {
      std::vector<int> lp((size_t)n_in);
      ck(hipMemcpy(lp.data(), part_[cur].p, n_in * sizeof(int), hipMemcpyDeviceToHost), "cp left");
      for (int p : lp) left[p] = 1;
    }
    py::array_t<int8_t> status_out(P);
    py::array_t<int64_t> nodes_out(P);
    for (int p = 0; p < P; ++p) {
      int8_t v = hs[p];
      if (wit.got[p]) v = 1;
      else if (v == 3 || v == 4) v = left[p] ? 0 : 2;     // every node closed => UNSAT
      status_out.mutable_data()[p] = v;
      nodes_out.mutable_data()[p] = hn[p];
    }
    py::array_t<int64_t> ax({P, n0_}), axp({P, n0_});
    std::memcpy(ax.mutable_data(), wit.cex_x.data(), sizeof(int64_t) * wit.cex_x.size());
    std::memcpy(axp.mutable_data(), wit.cex_xp.data(), sizeof(int64_t) * wit.cex_xp.size());
    py::dict stats;
    stats["levels"] = levels;
    stats["nodes"] = total;
    stats["timed_out"] = timed_out;
    stats["time"] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return py::make_tuple(status_out, ax, axp, nodes_out, stats);
  }

 private:
  void level(int cur, int nxt, long long s, int nb, int P, int budget, hipStream_t st) {
    ReluLevelArgs a{};
    a.Nn = nb; a.n0 = n0_; a.nh = nh_; a.npa = npa_;
    for (int k = 0; k < npa_; ++k) a.pa_idx[k] = pa_[k];
    a.pairs = pairs_.p; a.values = vals_.p; a.neg_from = neg_from_;
    a.part = part_[cur].p + s; a.pair = pair_[cur].p + s;
    a.xlo = lo_[cur].p + s * n0_; a.xhi = hi_[cur].p + s * n0_;
    a.phase = phase_[cur].p + s * 2 * nh_;
    a.rlo = rlo_.p; a.rhi = rhi_.p; a.rpart = rpart_.p;
    a.olb = form_.olb.p; a.oub = form_.oub.p; a.infeas = infeas_.p;
    a.Lc = form_.Lc.p; a.L0 = form_.L0.p; a.Le = form_.Le.p;
    a.Uc = form_.Uc.p; a.U0 = form_.U0.p; a.Ue = form_.Ue.p;
    a.split = split_.p;
    a.open = open_.p; a.choice = choice_.p; a.idim = idim_.p; a.cpts = cpts_.p;
    a.pe_lb = pe_lb_.p; a.pe_ub = pe_ub_.p;
    a.status = status_.p; a.part_nodes = nodes_.p; a.nodes_start = nodes_start_.p; a.budget = budget;
    a.opart = part_[nxt].p; a.opair = pair_[nxt].p; a.oxlo = lo_[nxt].p; a.oxhi = hi_[nxt].p;
    a.ophase = phase_[nxt].p; a.count_out = counters_.p; a.cap = pool_[nxt];
    a.cand_buf = sink_.records(); a.cand_count = counters_.p + 1; a.cand_cap = sink_.cand_alloc_;
    a.unit = (float)unit_;
    a.gmarg = fa_rt::gamma_up(2 * n0_ + 4, unit_);
    if (relaxed_) {
      a.nra = (int)ra_.size();
      for (int k = 0; k < a.nra; ++k) a.ra_idx[k] = ra_[k];
      a.tau = tau_;
      a.xplo = plo_[cur].p + s * n0_; a.xphi = phi_[cur].p + s * n0_;
      a.oxplo = plo_[nxt].p; a.oxphi = phi_[nxt].p;
    }
    ckl(fa_relu_rows_launch(a, st), "relu rows");
    const int R = 2 * nb;
    ck(hipMemsetAsync(infeas_.p, 0, R, st), "memset infeas");
    BoundArgs b{};
    b.flat = flat_; b.lo = rlo_.p; b.hi = rhi_.p; b.R = R; b.symbolic = 1;
    form_.fill(b);
    b.layer_lb = form_.lay_lb.p; b.layer_ub = form_.lay_ub.p;
    b.V = 0;
    for (int k = 0; k < npa_; ++k) b.fold |= 1ull << pa_[k];
    b.skip_status = status_.p; b.skip_part = rpart_.p;
    b.phase_in = a.phase;           // node-major [n][2][nh] = row-major [2n + side][nh]
    b.infeas = infeas_.p;
    ckl(fa_bounds_launch(net_, b, st), "relu bounds");
    // hidden-layer bounds by back-substitution with the rows' fixed phases (refine.hip): tighter
    // relaxation intervals for the backward pass, and empty regions detected (infeas)
    if (refine_) {
      const int rc = fa_refine_launch(net_, b, st);
      if (rc == -1) refine_ = 0;
      else ckl(rc, "relu refine");
    }
    CrownPhaseArgs c{};
    c.flat = flat_; c.lo = rlo_.p; c.hi = rhi_.p; c.R = R; c.phase = a.phase;
    c.infeas = infeas_.p;
    form_.fill(c);
    c.split = split_.p; c.score = score_.p; c.low = nullptr;
    c.skip_status = status_.p; c.skip_part = rpart_.p;
    const int rc = fa_crown_phase_launch(net_, c, st);
    if (rc != 0) throw std::runtime_error("crown_phase launch failed, code " + std::to_string(rc));
    ckl(fa_relu_cert_launch(a, st), "relu cert");
    // points 2n / 2n+1 belong to node n, not to node r % open_mod: no closed-node skip, every pair
    // is evaluated
    fa_rt::screen_points(net_, flat_, cpts_.p, R, pe_lb_.p, pe_ub_.p, st);
    ckl(fa_relu_split_launch(a, st), "relu split");
  }

  void ensure_pool(int i, long long need) {
    const int want = (int)std::min<long long>(std::max<long long>(need, 1), cap_);
    if (want <= pool_[i]) return;
    const int n = fa_rt::grow_to(pool_[i], want, 1 << 14, cap_);
    part_[i].ensure(n); pair_[i].ensure(n);
    lo_[i].ensure((size_t)n * n0_); hi_[i].ensure((size_t)n * n0_);
    if (relaxed_) { plo_[i].ensure((size_t)n * n0_); phi_[i].ensure((size_t)n * n0_); }
    phase_[i].ensure((size_t)n * 2 * nh_);
    pool_[i] = n;
  }

  NetDesc net_;
  const float* flat_;
  py::object keep_;         // owner of the memory behind flat_, held for the runtime's lifetime
  std::vector<int> pa_;
  int cap_, batch_;
  double unit_;
  int refine_ = 0;          // phase-aware back-substituted hidden-layer bounds (ReluConfig.refine)
  std::vector<int> ra_;     // relaxed queries: RA dims and tolerance (x' box per node)
  float tau_ = 0.f;
  bool relaxed_ = false;
  int n0_ = 0, nh_ = 0, npa_ = 0, V_ = 0, Pp_ = 0;
  int neg_from_ = 0;        // > 0: pairs [neg_from_, Pp_) are the reverse orientation
  int pool_[2] = {0, 0};
  fa_exact::ExactChecker exact_;
  RBuf<float> vals_;
  RBuf<int64_t> pairs_;
  RBuf<int> part_[2], pair_[2];
  RBuf<float> lo_[2], hi_[2], plo_[2], phi_[2];
  RBuf<int8_t> phase_[2];
  RBuf<float> rlo_, rhi_, score_, cpts_, pe_lb_, pe_ub_;
  fa_rt::FormBufs form_;
  RBuf<int> rpart_, split_, choice_, idim_, counters_, nodes_, nodes_start_;
  RBuf<uint8_t> infeas_, open_;
  RBuf<int8_t> status_;
  RBuf<unsigned char> stage_;
  fa_rt::LevelCounters hcount_;
  // pinned staging under the buffer-lifetime rule of runtime_host.h (released / regrown only after
  // the stream synchronisation that retires its last copy)
  fa_mem::HostBuf hstage_, hout_;
  fa_rt::CandSink sink_;
};

void register_relu(py::module& m) {
  py::class_<ReluRuntime>(m, "ReluRuntime")
      .def(py::init<py::handle, uintptr_t, std::vector<int>, std::vector<float>, std::vector<int64_t>, int, int,
                    double, int, std::vector<int>, double, int, py::object>(),
           py::arg("net"), py::arg("flat"), py::arg("pa"), py::arg("values_f"), py::arg("pairs"),
           py::arg("capacity"), py::arg("batch_nodes"), py::arg("unit"), py::arg("refine") = 0,
           py::arg("ra") = std::vector<int>(), py::arg("tau") = 0.0, py::arg("norient") = 1,
           py::arg("keep") = py::none())
      .def("solve", &ReluRuntime::solve, py::arg("lo"), py::arg("hi"), py::arg("status"), py::arg("budget"),
           py::arg("time_budget"), py::arg("confirm"), py::arg("stream"));
}
