// pybind11 bindings of the fairify_amd HIP kernels (module fairify_amd._C).
//
// Tensors cross the boundary as raw device pointers (Python ints from Tensor.data_ptr()) plus
// the caller's HIP stream (torch.cuda.current_stream().cuda_stream), so the extension has no
// dependency on the torch C++ headers and launches onto whatever stream torch is using.
//
// A binding that fills one of the larger args.h structs takes (net, **keywords): every key is the
// struct field's name (plus `stream`), read through Kw (kwargs.h) by the family's filler below, so a
// field is named once here and once in ops/hip.py and a missing or unknown key raises TypeError before
// any launch.  Bindings that pass up to 14 scalars straight to a launcher or into a small struct of
// their own (forward, decode, pack_masks, knn, actdiff, prune_masks, heuristic, agree, trace_marker)
// stay positional: nothing there is repeated.
#include <hip/hip_runtime.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <cstdint>
#include <stdexcept>
#include <vector>

#include "kwargs.h"
#include "runtime_host.h"

extern "C" int fa_bounds_launch(const NetDesc& net, BoundArgs args, hipStream_t stream);
extern "C" int fa_crown_phase_launch(const NetDesc& net, CrownPhaseArgs a, hipStream_t stream);
extern "C" size_t fa_crown_phase_bytes(const NetDesc& net);
extern "C" int fa_point_try_launch(const NetDesc& net, BoundArgs a, hipStream_t stream);
extern "C" int fa_forward_launch(const NetDesc& net, FwdArgs a, hipStream_t stream);
extern "C" int fa_sim_launch(const NetDesc& net, SimArgs a, hipStream_t stream);
extern "C" int fa_sim_shaped(const NetDesc& net);
extern "C" int fa_sym_shaped(const NetDesc& net, unsigned long long fold_mask);
extern "C" int fa_sym_geometry(const NetDesc& net, unsigned long long fold_mask, int* out);
extern "C" int fa_crown_shaped(const NetDesc& net, int mask);
extern "C" int fa_refine_shaped(const NetDesc& net, int logit);
extern "C" int fa_rate_launch(const NetDesc& net, RateArgs a, hipStream_t stream);
extern "C" int fa_audit_launch(const NetDesc& net, AuditArgs a, hipStream_t stream);
extern "C" int fa_neighbour_launch(const NetDesc& net, NeighbourArgs a, hipStream_t stream);
extern "C" int fa_causal_launch(const NetDesc& net, CausalArgs a, hipStream_t stream);
extern "C" int fa_count_enum_launch(const NetDesc& net, EnumArgs a, hipStream_t stream);
extern "C" int fa_gap_enum_launch(const NetDesc& net, GapEnumArgs a, hipStream_t stream);
extern "C" int fa_gap_level_launch(GapLevelArgs a, hipStream_t stream);
extern "C" int fa_count_rows_launch(CountArgs a, hipStream_t stream);
extern "C" int fa_count_level_launch(CountArgs a, hipStream_t stream);
extern "C" int fa_ascent_launch(const NetDesc& net, AscentArgs a, hipStream_t stream);
extern "C" int fa_certify_launch(CertArgs a, hipStream_t stream);
extern "C" int fa_falsify_launch(const NetDesc& net, FalsifyArgs a, hipStream_t stream);
extern "C" int fa_prune_masks_launch(const NetDesc& net, int P, const int* counts, const float* ub, int ub_stride,
                                     const uint8_t* sym_dead, uint8_t* code, int* cnt, hipStream_t stream);
extern "C" int fa_heuristic_launch(const NetDesc& net, int Pu, const int64_t* rows, const float* lb, const float* ub,
                                   int stride, const uint8_t* code, double q50, double qlo, double qhi, uint8_t* hnew,
                                   uint8_t* hmerged, int* hcnt, hipStream_t stream);
extern "C" int fa_agree_launch(const NetDesc& net, const float* flat, int Pm, const int64_t* rows, const float* lo,
                               const float* hi, const int64_t* pids, const uint8_t* dead, int S, uint32_t seed,
                               int* agree, hipStream_t stream);

extern "C" int fa_decode_launch(const DecodeDesc& d, const int64_t* ids, int P, const float* chunk_lo,
                                const float* chunk_hi, float* lo, float* hi, hipStream_t stream);
extern "C" int fa_trace_marker_launch(int tag, int* sink, hipStream_t stream);
extern "C" int fa_beta_launch(const NetDesc& nd, BetaArgs a, hipStream_t stream);
extern "C" int fa_beta_config(const NetDesc& nd, int* wpb, int* wtl, size_t* bytes);
extern "C" int fa_beta_opt16_fits(const NetDesc& nd);
extern "C" size_t fa_beta_opt16_scratch_floats(const NetDesc& nd, int R);
extern "C" int fa_beta_opt16_launch(const NetDesc& nd, BetaArgs a, float* pgsum, float* pgn, hipStream_t stream);
extern "C" int fa_beta_level16_launch(const NetDesc& nd, BetaArgs a, hipStream_t stream);
extern "C" int fa_beta_opt16_feas_launch(const NetDesc& nd, BetaArgs a, hipStream_t stream);
extern "C" int fa_beta_feas16_launch(const NetDesc& nd, BetaArgs a, hipStream_t stream);
extern "C" int fa_knn_launch(const float* X, int n, int d, int k, int* idx, float* dist, hipStream_t stream);
extern "C" int fa_actdiff_launch(const NetDesc& net, const float* flat, const float* x, const float* xp, int npairs,
                                 float* sum_out, hipStream_t stream);
extern "C" int fa_pack_masks_launch(const uint8_t* src, int P, int N, int stride, int sel, uint8_t* out, int NB,
                                    unsigned long long* hash, hipStream_t stream);

// BaB level kernels (bab.hip), bound one launch at a time for the level tests
extern "C" int fa_split_launch(SplitArgs a, hipStream_t stream);
extern "C" int fa_settle_launch(SettleArgs s, hipStream_t stream);
extern "C" int fa_bab_init_launch(BabInitArgs a, hipStream_t stream);
extern "C" int fa_bab_finish_launch(int P, const int8_t* status, const int* nodes, const int* open_left, int* out,
                                    hipStream_t stream);
extern "C" int fa_mark_unknown_launch(const int* part, int n, int8_t* status, hipStream_t stream);

template <typename T>
static T* P(uintptr_t p) { return reinterpret_cast<T*>(p); }

using fa_rt::gamma_up;

struct Net {
  NetDesc d;
  explicit Net(const std::vector<int>& dims, double unit) {
    if (dims.size() < 2 || dims.size() > FA_MAX_LAYERS + 1) throw std::invalid_argument("bad layer count");
    std::memset(&d, 0, sizeof(d));
    d.n_layers = (int)dims.size() - 1;
    int off = 0, noff = 0, mw = 0, mws = 0;
    for (size_t i = 0; i < dims.size(); ++i) {
      d.dims[i] = dims[i];
      mw = std::max(mw, dims[i]);
    }
    for (int l = 0; l < d.n_layers; ++l) {
      d.w_off[l] = off;
      off += dims[l] * dims[l + 1];
      d.b_off[l] = off;
      off += dims[l + 1];
      d.neuron_off[l] = noff;
      noff += dims[l + 1];
      mws = std::max(mws, dims[l] * dims[l + 1]);
      d.g_gemm[l] = gamma_up(2 * dims[l] + 1, unit);
      d.g_fwd[l] = gamma_up(dims[l] + 1, unit);
    }
    d.n_neurons = noff;
    d.n_hidden = noff - dims.back();
    d.max_width = mw;
    d.max_wsize = mws;
    d.unit = (float)unit;
    d.g_conc = gamma_up(dims[0] + 1, unit);
    d.g_one = gamma_up(1, unit);
    n_params = off;
    d.wperm_off = (off + 3) & ~3;
    int wp = 0;
    for (int l = 0; l < d.n_layers; ++l) wp += ((dims[l] + 15) / 16) * ((dims[l + 1] + 15) / 16) * 256;
    for (int l = 0; l < d.n_layers; ++l) wp += dims[l + 1];
    d.wperm_floats = (wp + 3) & ~3;
    total_floats = d.wperm_off + d.wperm_floats;
    // packed narrow-network block (ops/backend.py: pack_groups / mfma_packed_block)
    d.pack_g = 1;
    if (d.n_layers >= 2 && dims[0] <= 16 && mw <= 16) {
      int mh = 0;
      for (int l = 1; l < d.n_layers; ++l) mh = std::max(mh, dims[l]);
      d.pack_g = mh <= 4 ? 4 : (mh <= 8 ? 2 : 1);   // box stride 16 / pack_g: a multiple of 4
    }
    d.pack_off = total_floats;
    d.pack_floats = 0;
    if (d.pack_g > 1) {
      d.pack_floats = d.pack_g * 256 + (d.n_layers - 1) * 256 + d.n_layers * 16;
      total_floats += d.pack_floats;
    }
    // backward operand order block (ops/backend.py: mfma_back_block)
    d.wback_off = total_floats;
    int wb = 0;
    for (int l = 0; l < d.n_layers; ++l) wb += ((dims[l] + 15) / 16) * ((dims[l + 1] + 15) / 16) * 256;
    d.wback_floats = wb;
    total_floats += wb;
  }
  int n_params;
  int total_floats;
};

const NetDesc& fa_net_desc(py::handle h) { return h.cast<const Net&>().d; }
void register_bab(py::module& m);
void register_relu(py::module& m);
void register_beta(py::module& m);
extern "C" int fa_crown_launch(const NetDesc& net, BoundArgs a, hipStream_t stream);
extern "C" int fa_refine_launch(const NetDesc& net, BoundArgs a, hipStream_t stream);
extern "C" int fa_backward_launch(const NetDesc& net, BoundArgs a, hipStream_t stream);
extern "C" int fa_refine_crown_launch(const NetDesc& net, BoundArgs a, hipStream_t stream);
void register_csv(py::module& m);

using fa_rt::ckl;

// ---- fillers: one per struct family, the keys are the args.h field names ---------------------------
// the stream key, read last: every key the caller passed must have been read by then
static hipStream_t finish(Kw& k) {
  const hipStream_t s = reinterpret_cast<hipStream_t>(k.u64("stream"));
  k.done();
  return s;
}

// an index list (pa -> npa / pa_idx, ra -> nra / ra_idx, free -> nfree / free_idx); returns its length
static int dims(Kw& k, const char* key, int* idx, size_t cap, const char* too_many) {
  const std::vector<int> v = k.ints(key);
  if (v.size() > cap) throw std::invalid_argument(too_many);
  std::copy(v.begin(), v.end(), idx);
  return (int)v.size();
}

// The block BoundArgs and CrownPhaseArgs share.  `req`: the pointer groups the entry cannot run without
// (the others may be left out: nullptr); lo / hi: the keys of the row boxes.
enum { OUT = 1, FORMS = 2, LAYERS = 4 };
template <typename A>
static A row_args(Kw& k, int req, const char* lo = "lo", const char* hi = "hi") {
  auto p = [&](const char* key, int group) { return (req & group) ? k.need<float>(key) : k.ptr<float>(key); };
  A a{};
  a.flat = k.need<const float>("flat");
  a.lo = k.need<const float>(lo);
  a.hi = k.need<const float>(hi);
  a.R = k.i("R");
  a.out_lb = p("out_lb", OUT);
  a.out_ub = p("out_ub", OUT);
  a.Lc = p("Lc", FORMS); a.L0 = p("L0", FORMS); a.Le = p("Le", FORMS);
  a.Uc = p("Uc", FORMS); a.U0 = p("U0", FORMS); a.Ue = p("Ue", FORMS);
  a.layer_lb = p("layer_lb", LAYERS);
  a.layer_ub = p("layer_ub", LAYERS);
  return a;
}
static BoundArgs bound_args(Kw& k, int req, const char* lo = "lo", const char* hi = "hi") {
  BoundArgs a = row_args<BoundArgs>(k, req, lo, hi);
  a.dead_in = k.ptr<const uint8_t>("dead_in");
  return a;
}

// The query block SimArgs, RateArgs, FalsifyArgs and AscentArgs share ...
template <typename A>
static void fill_query(A& a, Kw& k, const char* too_many) {
  a.flat = k.need<const float>("flat");
  a.lo = k.need<const float>("lo");
  a.hi = k.need<const float>("hi");
  a.P = k.i("P");
  a.V = k.i("V");
  a.npa = dims(k, "pa", a.pa_idx, FA_MAX_PA, too_many);
  a.values = k.ptr<const int64_t>("values");
  a.Pp = k.i("Pp");
  a.pairs = k.ptr<const int64_t>("pairs");
}
// ... the sample stream and the RA offsets of the three that draw their points (not AscentArgs) ...
template <typename A>
static void fill_samples(A& a, Kw& k, const char* too_many) {
  a.pids = k.need<const int64_t>("pids");
  a.n_samples = k.i("n_samples");
  a.seed = (uint32_t)k.u64("seed");
  a.nra = dims(k, "ra", a.ra_idx, FA_MAX_RA, too_many);
  a.tau = k.i("tau");
}
// ... and the witness outputs with the free dims of the two that run the lattice ascent
template <typename A>
static void fill_ascent(A& a, Kw& k, const char* too_many) {
  a.K = k.i("K");
  a.iters = k.i("iters");
  a.nfree = dims(k, "free", a.free_idx, 64, too_many);
  a.found = k.need<uint8_t>("found");
  a.wit_x = k.need<float>("wit_x");
  a.wit_xp = k.need<float>("wit_xp");
}

// The query block of the row-forward kernels that take their rows or leaves from the caller (AuditArgs,
// NeighbourArgs, EnumArgs, GapEnumArgs; csrc/rowfwd.h).  `pairs` may be absent when there is no pair,
// unless `need_pairs`.
template <typename A>
static void fill_pairs(A& a, Kw& k, bool need_pairs = false) {
  a.flat = k.need<const float>("flat");
  a.V = k.i("V");
  a.npa = dims(k, "pa", a.pa_idx, FA_MAX_PA, "too many PA/RA dims");
  a.values = k.need<const int64_t>("values");
  a.Pp = k.i("Pp");
  a.pairs = (need_pairs || a.Pp > 0) ? k.need<const int64_t>("pairs") : k.ptr<const int64_t>("pairs");
  a.nra = dims(k, "ra", a.ra_idx, FA_MAX_RA, "too many PA/RA dims");
  a.tau = k.i("tau");
  a.E = k.i("E");
}
// the PA / RA dims of a query lie inside the n0 inputs, or std::invalid_argument
template <typename A>
static void dims_inside(const char* fn, const A& a, int n0) {
  for (int q = 0; q < a.npa; ++q)
    if (a.pa_idx[q] < 0 || a.pa_idx[q] >= n0) throw std::invalid_argument(std::string(fn) + ": PA dim outside the inputs");
  for (int q = 0; q < a.nra; ++q)
    if (a.ra_idx[q] < 0 || a.ra_idx[q] >= n0) throw std::invalid_argument(std::string(fn) + ": RA dim outside the inputs");
}

// One beta level (BetaArgs; beta_level and the batched entry points share it).  `flags`: bit 0 stall,
// bits 1-2 the primal-gap weights, bit 3 the infeasibility pass (ops/hip.py:beta_flags).
static BetaArgs beta_args(const Net& net, Kw& k) {
  BetaArgs a;
  std::memset(&a, 0, sizeof(a));
  a.flat = k.need<const float>("flat");
  a.wt = k.ptr<const float>("wt");
  a.R = k.i("R");
  a.npa = dims(k, "pa", a.pa_idx, FA_MAX_PA, "beta_level: too many PA dims");
  for (int q = 0; q < a.npa; ++q)
    if (a.pa_idx[q] < 0 || a.pa_idx[q] >= net.d.dims[0] || (q && a.pa_idx[q] <= a.pa_idx[q - 1]))
      throw std::invalid_argument("beta_level: PA dims must be increasing input indices");
  a.lo = k.need<const float>("lo");
  a.hi = k.need<const float>("hi");
  a.va = k.need<const float>("va");
  a.vb = k.need<const float>("vb");
  a.LBA = k.need<const float>("LBA");
  a.UBA = k.need<const float>("UBA");
  a.LBB = k.need<const float>("LBB");
  a.UBB = k.need<const float>("UBB");
  a.phA = k.need<const int8_t>("phA");
  a.phB = k.need<const int8_t>("phB");
  a.par = k.need<float>("par");
  a.t = k.need<float>("t");
  a.scratch = k.need<float>("scratch");
  a.iters = k.i("iters");
  a.lr_a = k.f("lr_a");
  a.lr_b = k.f("lr_b");
  a.lr_t = k.f("lr_t");
  a.decay = k.f("decay");
  a.lookahead = k.i("lookahead", 0);
  a.beta_pos = k.i("beta_pos", 1);
  const int flags = k.i("flags", 0);
  a.stall = flags & 1;
  a.pgap = (flags >> 1) & 3;
  a.feas = (flags >> 3) & 1;      // scratch [R, 16, NH]
  a.bound = k.ptr<double>("bound");
  a.split = k.ptr<int>("split");
  a.xstar = k.ptr<float>("xstar");
  a.binit = k.ptr<float>("binit");
  a.ramask = k.u64("ramask", 0);
  a.plo = k.ptr<const float>("plo");
  a.phi = k.ptr<const float>("phi");
  a.xpstar = k.ptr<float>("xpstar");
  a.gtie = k.ptr<float>("gtie");
  a.tau = k.f("tau", 0.f);
  a.osg = k.ptr<const int8_t>("osg");
  a.pgsum = k.ptr<const float>("pgsum");
  a.pgn = k.ptr<const float>("pgn");
  a.fpar = k.ptr<float>("fpar");
  a.fgt = k.ptr<float>("fgt");
  a.fval = k.ptr<double>("fval");
  if ((net.d.dims[0] < 64 && (a.ramask >> net.d.dims[0])) || (a.ramask && (!a.plo || !a.phi)))
    throw std::invalid_argument("beta_level: RA mask beyond the inputs or no x' box");
  return a;
}

// Level end (SettleArgs): the keys are the field names behind `pre` ("" for the settle binding,
// "settle_" for the block fused into a split launch); esc goes as the two lists esc_budget / esc_open
// (esc.n = their length).  `fused`: the workgroup counter `done` is needed too.
static SettleArgs settle_args(Kw& k, const std::string& fn, const std::string& pre, bool fused) {
  // Kw keeps the key's characters only for the call: the composed names live here
  std::vector<std::string> names;
  names.reserve(20);
  auto key = [&](const char* f) { names.push_back(pre + f); return names.back().c_str(); };
  SettleArgs s{};
  s.P = k.i(key("P"));
  if (s.P <= 0) throw std::invalid_argument(fn + ": " + pre + "P must be positive");
  s.status = k.need<int8_t>(key("status"));
  s.lvl_open = k.need<int>(key("lvl_open"));
  s.part_open = k.ptr<int>(key("part_open"));
  s.part_nodes = k.need<const int>(key("part_nodes"));
  s.nodes_start = k.need<int>(key("nodes_start"));
  s.prev_start = k.need<int>(key("prev_start"));
  s.counters_cur = k.need<const int>(key("counters_cur"));
  s.counters_next = k.need<int>(key("counters_next"));
  s.host_counts = k.need<int>(key("host_counts"));
  s.pbudget = k.ptr<int>(key("pbudget"));
  s.prob = k.ptr<uint8_t>(key("prob"));
  s.budget2 = k.i(key("budget2"));
  s.max_open = k.i(key("max_open"));
  const std::vector<int> eb = k.ints(key("esc_budget")), eo = k.ints(key("esc_open"));
  if (eb.size() != eo.size() || eb.size() > FA_MAX_ESC)
    throw std::invalid_argument(fn + ": esc_budget / esc_open hold the same number of steps, at most 4");
  s.esc.n = (int)eb.size();
  std::copy(eb.begin(), eb.end(), s.esc.budget);
  std::copy(eo.begin(), eo.end(), s.esc.open);
  s.done = fused ? k.need<int>(key("done")) : k.ptr<int>(key("done"));
  if (s.prob && !s.pbudget) throw std::invalid_argument(fn + ": prob without pbudget");
  return s;
}

PYBIND11_MODULE(_C, m) {
  m.doc() = "fairify_amd CDNA4 (gfx950) kernels";
  py::class_<Net>(m, "Net")
      .def(py::init<const std::vector<int>&, double>())
      .def_readonly("n_params", &Net::n_params)
      .def_readonly("total_floats", &Net::total_floats)
      .def_property_readonly("wperm_off", [](const Net& n) { return n.d.wperm_off; })
      .def_property_readonly("pack_g", [](const Net& n) { return n.d.pack_g; })
      .def_property_readonly("pack_off", [](const Net& n) { return n.d.pack_off; })
      .def_property_readonly("n_hidden", [](const Net& n) { return n.d.n_hidden; })
      .def_property_readonly("n_neurons", [](const Net& n) { return n.d.n_neurons; });

  m.def("bounds", [](const Net& net, py::kwargs kw) {
    Kw k("bounds", kw);
    const int symbolic = k.i("symbolic");
    BoundArgs a = bound_args(k, symbolic ? OUT | FORMS : OUT);
    a.symbolic = symbolic;
    a.G = k.i("G", 0);
    a.dead_out = k.ptr<uint8_t>("dead_out");
    a.fold = k.u64("fold", 0);
    a.phase_in = k.ptr<const int8_t>("phase_in");
    a.infeas = k.ptr<uint8_t>("infeas");
    // the BaB runtimes' launch form, for tests: node-row expansion (row r = node r / V with its PA
    // dims set to values[r % V]) and the status filter
    a.V = k.i("V", 0);
    if (a.V > 0) {
      a.npa = dims(k, "pa", a.pa_idx, FA_MAX_PA, "bounds: too many protected attributes");
      a.values = k.need<const float>("values");
    }
    a.skip_status = k.ptr<const int8_t>("skip_status");
    a.skip_part = k.ptr<const int>("skip_part");
    if (a.skip_status && !a.skip_part) throw std::invalid_argument("bounds: skip_status without skip_part");
    ckl(fa_bounds_launch(net.d, a, finish(k)), "bounds");
  });

  // ReLU-phase backward bounds (relu.hip), refining a preceding phase-aware `bounds` call in place
  m.def("crown_phase", [](const Net& net, py::kwargs kw) {
    Kw k("crown_phase", kw);
    CrownPhaseArgs a = row_args<CrownPhaseArgs>(k, OUT | FORMS | LAYERS);
    a.phase = k.ptr<const int8_t>("phase");
    a.infeas = k.ptr<const uint8_t>("infeas");
    a.split = k.need<int>("split");
    a.score = k.need<float>("score");
    a.low = k.ptr<float>("low");
    const int rc = fa_crown_phase_launch(net.d, a, finish(k));
    if (rc != 0) throw std::runtime_error("crown_phase launch failed, code " + std::to_string(rc));
  });

  // does the ReLU-phase backward kernel hold this network (layers <= 256 wide, LDS <= 160 KB)?
  m.def("relu_fits", [](const Net& net) { return fa_crown_phase_bytes(net.d) > 0; });

  // backward output bounds refining forms/out bounds written by a preceding `bounds` call
  m.def("crown", [](const Net& net, py::kwargs kw) {
    Kw k("crown", kw);
    const BoundArgs a = bound_args(k, OUT | FORMS | LAYERS);
    ckl(fa_crown_launch(net.d, a, finish(k)), "crown");
  });

  // The three refine.hip entries return the launch code (0 done, -1 shape not supported).
  // refine: back-substituted hidden-layer bounds, tightening layer_lb / layer_ub of a preceding symbolic
  // `bounds` call in place
  m.def("refine", [](const Net& net, py::kwargs kw) {
    Kw k("refine", kw);
    BoundArgs a = bound_args(k, LAYERS);
    a.phase_in = k.ptr<const int8_t>("phase_in");   // ReLU-phase rows [R, n_hidden] (+1 / -1 fixed, 0 free)
    a.infeas = k.ptr<uint8_t>("infeas");            // [R] set to 1 where a refined bound contradicts a phase
    const int rc = fa_refine_launch(net.d, a, finish(k));
    if (rc < -1) throw std::runtime_error("refine launch failed, code " + std::to_string(rc));
    return rc;
  });
  // refined hidden-layer bounds + the logit's backward pass in one launch (what the BaB runtime runs
  // for BaBConfig.refine level 1), tightening a preceding symbolic `bounds` call in place
  m.def("refine_crown", [](const Net& net, py::kwargs kw) {
    Kw k("refine_crown", kw);
    const BoundArgs a = bound_args(k, OUT | FORMS | LAYERS);
    const int rc = fa_refine_crown_launch(net.d, a, finish(k));
    if (rc < -1) throw std::runtime_error("refine_crown launch failed, code " + std::to_string(rc));
    return rc;
  });
  // every neuron's bounds and the logit's forms by back-substitution alone (mode FULL); layer_lb /
  // layer_ub may be left out
  m.def("backward_bounds", [](const Net& net, py::kwargs kw) {
    Kw k("backward_bounds", kw);
    const BoundArgs a = bound_args(k, OUT | FORMS);
    const int rc = fa_backward_launch(net.d, a, finish(k));
    if (rc < -1) throw std::runtime_error("backward_bounds launch failed, code " + std::to_string(rc));
    return rc;
  });

  // rows that are points: lo = hi = x; the point kernel, or the interval pass where it does not fit
  m.def("point_bounds", [](const Net& net, py::kwargs kw) {
    Kw k("point_bounds", kw);
    BoundArgs a = bound_args(k, OUT, "x", "x");
    // optional closed-node skip of the BaB level (args.h): point r belongs to node r % open_mod
    a.row_open = k.ptr<const uint8_t>("row_open");
    a.open_mod = k.i("open_mod", 0);
    if (a.row_open && a.open_mod <= 0) throw std::invalid_argument("point_bounds: row_open needs open_mod > 0");
    const hipStream_t stream = finish(k);
    const int rc = fa_point_try_launch(net.d, a, stream);
    if (rc < 0) ckl(-rc, "point_bounds");
    if (rc == 0) ckl(fa_bounds_launch(net.d, a, stream), "point_bounds(ibp)");
  });

  m.def("forward", [](const Net& net, uintptr_t flat, uintptr_t x, int B, uintptr_t dead, uintptr_t out,
                      uintptr_t stream) {
    FwdArgs a{};
    a.flat = P<const float>(flat);
    a.x = P<const float>(x);
    a.B = B;
    a.dead = P<const uint8_t>(dead);
    a.out = P<float>(out);
    ckl(fa_forward_launch(net.d, a, (hipStream_t)stream), "forward");
  });

  m.def("sim", [](const Net& net, py::kwargs kw) {
    Kw k("sim", kw);
    SimArgs a{};
    fill_query(a, k, "too many PA/RA dims");
    fill_samples(a, k, "too many PA/RA dims");
    a.counts = k.need<int>("counts");
    a.found = k.need<uint8_t>("found");
    a.wit_x = k.need<float>("wit_x");
    a.wit_xp = k.need<float>("wit_xp");
    a.z0 = k.ptr<float>("z0");
    a.keys = k.ptr<int>("keys");
    a.split = k.i("split");
    a.regcount = k.i("regcount");
    if (a.split < 1 || (a.split > 1 && !a.keys)) throw std::invalid_argument("sim: split > 1 needs a keys buffer");
    ckl(fa_sim_launch(net.d, a, finish(k)), "sim");
  });
  m.def("sim_shaped", [](const Net& net) { return fa_sim_shaped(net.d) != 0; });
  // would a launch run a compile-time-shape instance?  The launch's own selection (the *_SHAPED
  // switches included): symbolic by fold mask, crown with / without a forced-dead mask, refine
  // without / with the logit's backward pass (refine / refine_crown and backward_bounds)
  m.def("sym_shaped", [](const Net& net, unsigned long long fold) { return fa_sym_shaped(net.d, fold) != 0; });
  // launch geometry of the register-resident symbolic kernel for this network and fold mask (needs a
  // device: the occupancy query); None when the launch would take the LDS-tiled kernel
  m.def("sym_geometry", [](const Net& net, unsigned long long fold) -> py::object {
    int g[8] = {0};
    if (fa_sym_geometry(net.d, fold, g) != 1) return py::none();
    py::dict d;
    d["threads"] = g[0];
    d["lds_bytes"] = g[1];
    d["blocks_per_cu"] = g[2];
    d["cus"] = g[3];
    d["rows_per_block"] = g[4];
    d["waves_per_simd"] = g[5];
    d["shaped"] = g[6] != 0;
    d["regs"] = g[7];
    return d;
  });
  m.def("crown_shaped", [](const Net& net, bool mask) { return fa_crown_shaped(net.d, mask) != 0; });
  m.def("refine_shaped", [](const Net& net, bool logit) { return fa_refine_shaped(net.d, logit) != 0; });

  // discrimination-rate counts (csrc/rate.hip); flips / amb zero-initialised by the caller
  m.def("rate", [](const Net& net, py::kwargs kw) {
    Kw k("rate", kw);
    RateArgs a{};
    fill_query(a, k, "too many PA/RA dims");
    fill_samples(a, k, "too many PA/RA dims");
    a.E = k.i("E");
    a.flips = k.need<int>("flips");
    a.amb = k.need<int>("amb");
    a.amb_idx = k.need<int>("amb_idx");
    a.split = k.i("split");
    const int rc = fa_rate_launch(net.d, a, finish(k));
    if (rc == -3) throw std::invalid_argument("rate: shape not covered (layer > 160, inputs > 32, V > 32 or E > 32)");
    ckl(rc, "rate");
  });

  // audit of real rows (csrc/audit.hip): per-row cert / poss masks and the own sign.  Returns false when
  // the kernel does not cover the shape (the caller takes the composed path), true when launched
  m.def("audit", [](const Net& net, py::kwargs kw) {
    Kw k("audit", kw);
    AuditArgs a{};
    fill_pairs(a, k);
    a.x = k.need<const float>("x");
    a.own = k.need<const int>("own");
    a.N = k.i("N");
    a.cert = k.need<int>("cert");
    a.poss = k.need<int>("poss");
    a.own_sign = k.need<int8_t>("own_sign");
    a.blocks = k.i("blocks");
    if (a.N < 0) throw std::invalid_argument("audit: negative row count");
    dims_inside("audit", a, net.d.dims[0]);
    const int rc = fa_audit_launch(net.d, a, finish(k));
    if (rc == -3) return false;
    if (rc == -2) throw std::invalid_argument("audit: workgroup count outside 1..number of 64-row passes");
    ckl(rc, "audit");
    return true;
  });

  // single-attribute neighbourhood of real rows (csrc/neighbours.hip): cert / poss words [N, W].  Returns
  // false when the kernel does not cover the shape (the caller takes the composed path)
  m.def("neighbours", [](const Net& net, py::kwargs kw) {
    Kw k("neighbours", kw);
    NeighbourArgs a{};
    fill_pairs(a, k);
    a.x = k.need<const float>("x");
    a.own = k.need<const int>("own");
    a.N = k.i("N");
    a.M = k.i("M");
    a.W = k.i("W");
    a.nb_dim = k.need<const int>("nb_dim");
    a.nb_off = k.need<const int>("nb_off");
    a.nb_abs = k.need<const int>("nb_abs");
    a.dom_lo = k.need<const int>("dom_lo");
    a.dom_hi = k.need<const int>("dom_hi");
    a.radius = k.need<const int>("radius");
    a.cert = k.need<int>("cert");
    a.poss = k.need<int>("poss");
    a.blocks = k.i("blocks");
    if (a.N < 0 || a.M < 0) throw std::invalid_argument("neighbours: negative row or neighbour count");
    if (a.W != (a.M + 31) / 32) throw std::invalid_argument("neighbours: W is not ceil(M / 32)");
    dims_inside("neighbours", a, net.d.dims[0]);
    const int rc = fa_neighbour_launch(net.d, a, finish(k));
    if (rc == -3) return false;
    if (rc == -2) throw std::invalid_argument("neighbours: workgroup count outside 1..passes x words");
    ckl(rc, "neighbours");
    return true;
  });

  // causal-discrimination search over attribute sets (csrc/causal.hip): one byte per (row, set), bit 0
  // poss, bit 1 cert.  set_dims / value_off: the host copies of dims [T, D] and voff [n0 + 1], which the
  // checks here and in the launcher read.  Returns false when the kernel does not cover the shape (the
  // caller takes the composed path)
  m.def("causal", [](const Net& net, py::kwargs kw) {
    Kw k("causal", kw);
    CausalArgs a{};
    a.flat = k.need<const float>("flat");
    a.x = k.need<const float>("x");
    a.S = k.i("S");
    a.T = k.i("T");
    a.D = k.i("D");
    a.dims = k.need<const int>("dims");
    a.vals = k.need<const int>("vals");
    a.voff = k.need<const int>("voff");
    a.nvals = k.i("nvals");
    const std::vector<int> set_dims = k.ints("set_dims");
    const std::vector<int> value_off = k.ints("value_off");
    a.h_dims = set_dims.data();
    a.h_voff = value_off.data();
    a.code = k.need<uint8_t>("code");
    a.blocks = k.i("blocks");
    if (a.S < 0 || a.T < 0) throw std::invalid_argument("causal: negative row or set count");
    if (a.D < 1) throw std::invalid_argument("causal: a set needs at least one dim");
    if (set_dims.size() != (size_t)a.T * (size_t)a.D) throw std::invalid_argument("causal: set_dims is not [T, D]");
    if (value_off.size() != (size_t)net.d.dims[0] + 1)
      throw std::invalid_argument("causal: value_off is not one offset per input plus the end");
    if (value_off.front() != 0 || value_off.back() != a.nvals)
      throw std::invalid_argument("causal: value_off does not span vals");
    for (size_t i = 1; i < value_off.size(); ++i)
      if (value_off[i] <= value_off[i - 1]) throw std::invalid_argument("causal: a feature without values");
    const int rc = fa_causal_launch(net.d, a, finish(k));
    if (rc == -3) return false;
    if (rc == -2) throw std::invalid_argument("causal: workgroup count outside 1..passes x sets");
    ckl(rc, "causal");
    return true;
  });

  // counting branch-and-bound (csrc/count.hip).  count_enum: leaf enumeration; amb zero-initialised by
  // the caller
  m.def("count_enum", [](const Net& net, py::kwargs kw) {
    Kw k("count_enum", kw);
    EnumArgs a{};
    fill_pairs(a, k);
    a.lo = k.need<const float>("lo");
    a.hi = k.need<const float>("hi");
    a.L = k.i("L");
    a.max_vol = k.i("max_vol");
    a.cert = k.need<int>("cert");
    a.amb = k.need<int>("amb");
    a.amb_idx = k.need<int>("amb_idx");
    a.blocks = k.i("blocks");
    const int rc = fa_count_enum_launch(net.d, a, finish(k));
    if (rc == -3)
      throw std::invalid_argument(
          "count_enum: shape not covered (layer > 160, inputs > 32, V > 32, E > 32 or leaf volume > 65536)");
    ckl(rc, "count_enum");
  });
  // score-gap leaf enumeration (csrc/gap.hip): false when the kernel does not cover the shape
  m.def("gap_enum", [](const Net& net, py::kwargs kw) {
    Kw k("gap_enum", kw);
    GapEnumArgs a{};
    fill_pairs(a, k, true);
    a.lo = k.need<const float>("lo");
    a.hi = k.need<const float>("hi");
    a.L = k.i("L");
    a.max_vol = k.i("max_vol");
    a.leaf_lo = k.need<double>("leaf_lo");
    a.leaf_hi = k.need<double>("leaf_hi");
    a.arg_s = k.need<int>("arg_s");
    a.arg_pair = k.need<int>("arg_pair");
    a.arg_e = k.need<int>("arg_e");
    a.blocks = k.i("blocks");
    const int rc = fa_gap_enum_launch(net.d, a, finish(k));
    if (rc == -3) return false;
    if (rc == -2) throw std::invalid_argument("gap_enum: workgroup count outside 1..leaves");
    ckl(rc, "gap_enum");
    return true;
  });
  // score-gap level step (csrc/gap.hip): false when the kernel does not cover the shape
  m.def("gap_level", [](py::kwargs kw) {
    Kw k("gap_level", kw);
    GapLevelArgs a{};
    a.N = k.i("N");
    a.n0 = k.i("n0");
    a.V = k.i("V");
    a.npa = dims(k, "pa", a.pa_idx, FA_MAX_PA, "too many PA/RA dims");
    a.nra = dims(k, "ra", a.ra_idx, FA_MAX_RA, "too many PA/RA dims");
    a.tau = k.f("tau");
    a.lo = k.need<const float>("lo");
    a.hi = k.need<const float>("hi");
    a.part = k.need<const int>("part");
    a.values = k.need<const float>("values");
    a.Pp = k.i("Pp");
    a.pairs = k.need<const int64_t>("pairs");
    a.Lc = k.need<const float>("Lc");
    a.L0 = k.need<const float>("L0");
    a.Le = k.need<const float>("Le");
    a.Uc = k.need<const float>("Uc");
    a.U0 = k.need<const float>("U0");
    a.Ue = k.need<const float>("Ue");
    a.lb = k.need<const float>("lb");
    a.ub = k.need<const float>("ub");
    a.Lcp = k.need<const float>("Lcp");
    a.L0p = k.need<const float>("L0p");
    a.Lep = k.need<const float>("Lep");
    a.Ucp = k.need<const float>("Ucp");
    a.U0p = k.need<const float>("U0p");
    a.Uep = k.need<const float>("Uep");
    a.lbp = k.need<const float>("lbp");
    a.ubp = k.need<const float>("ubp");
    a.thr = k.need<const double>("thr");
    a.score = k.need<const float>("score");
    a.leaf_points = (long long)k.u64("leaf_points");
    a.out_ub = k.need<float>("out_ub");
    a.code = k.need<uint8_t>("code");
    a.best_pair = k.need<int>("best_pair");
    a.orient = k.need<int>("orient");
    a.sdim = k.need<int>("sdim");
    a.coef = k.need<float>("coef");
    a.cand_x = k.need<float>("cand_x");
    a.cand_xp = k.need<float>("cand_xp");
    a.olo = k.need<float>("olo");
    a.ohi = k.need<float>("ohi");
    a.opart = k.need<int>("opart");
    a.oub = k.need<float>("oub");
    a.okey = k.need<int>("okey");
    a.cap = k.i("cap");
    a.leaf_lo = k.need<float>("leaf_lo");
    a.leaf_hi = k.need<float>("leaf_hi");
    a.leaf_part = k.need<int>("leaf_part");
    a.leaf_key = k.need<int>("leaf_key");
    a.leaf_cap = k.i("leaf_cap");
    a.counters = k.need<int>("counters");
    const int rc = fa_gap_level_launch(a, finish(k));
    if (rc == -3) return false;
    if (rc == -2) throw std::invalid_argument("gap_level: too many nodes in one launch");
    ckl(rc, "gap_level");
    return true;
  });
  // the block the row expansion and the level step share
  auto count_args = [](Kw& k) {
    CountArgs a{};
    a.N = k.i("N");
    a.n0 = k.i("n0");
    a.V = k.i("V");
    a.npa = dims(k, "pa", a.pa_idx, FA_MAX_PA, "too many PA/RA dims");
    a.lo = k.need<const float>("lo");
    a.hi = k.need<const float>("hi");
    return a;
  };
  m.def("count_rows", [count_args](py::kwargs kw) {
    Kw k("count_rows", kw);
    CountArgs a = count_args(k);
    a.nra = dims(k, "ra", a.ra_idx, FA_MAX_RA, "too many PA/RA dims");
    a.tau = k.f("tau");
    a.values = k.need<const float>("values");
    a.rlo = k.need<float>("rlo");
    a.rhi = k.need<float>("rhi");
    a.plo = k.ptr<float>("plo");
    a.phi = k.ptr<float>("phi");
    ckl(fa_count_rows_launch(a, finish(k)), "count_rows");
  });
  m.def("count_level", [count_args](py::kwargs kw) {
    Kw k("count_level", kw);
    CountArgs a = count_args(k);
    a.part = k.need<const int>("part");
    a.lx = k.need<const float>("lx");
    a.ux = k.need<const float>("ux");
    a.lxp = k.need<const float>("lxp");
    a.uxp = k.need<const float>("uxp");
    a.Pp = k.i("Pp");
    a.pairs = k.ptr<const int64_t>("pairs");
    a.score = k.need<const float>("score");
    a.leaf_points = (long long)k.u64("leaf_points");
    a.code = k.need<uint8_t>("code");
    a.fair = k.need<long long>("fair");
    a.unfair = k.need<long long>("unfair");
    a.child_cnt = k.need<int>("child_cnt");
    a.olo = k.need<float>("olo");
    a.ohi = k.need<float>("ohi");
    a.opart = k.need<int>("opart");
    a.cap = k.i("cap");
    a.leaf_lo = k.need<float>("leaf_lo");
    a.leaf_hi = k.need<float>("leaf_hi");
    a.leaf_part = k.need<int>("leaf_part");
    a.leaf_cap = k.i("leaf_cap");
    a.counters = k.need<int>("counters");
    if (a.Pp > 0 && !a.pairs) throw py::type_error("count_level() missing required keyword argument 'pairs'");
    ckl(fa_count_level_launch(a, finish(k)), "count_level");
  });

  // returns false if the partition's candidate rows do not fit in LDS (caller keeps PyTorch)
  m.def("ascent", [](const Net& net, py::kwargs kw) {
    Kw k("ascent", kw);
    AscentArgs a{};
    fill_query(a, k, "too many PA/free dims");
    fill_ascent(a, k, "too many PA/free dims");
    a.x0 = k.need<const float>("x0");
    a.f0 = k.need<const float>("f0");
    a.q0 = k.need<const int>("q0");
    const int rc = fa_ascent_launch(net.d, a, finish(k));
    if (rc == -1) return false;
    ckl(rc, "ascent");
    return true;
  });

  // fused residual falsifier; returns false when the network shape is not supported (caller
  // keeps the PyTorch path)
  m.def("falsify", [](const Net& net, py::kwargs kw) {
    Kw k("falsify", kw);
    FalsifyArgs a{};
    fill_query(a, k, "too many PA/RA/free dims");
    fill_samples(a, k, "too many PA/RA/free dims");
    fill_ascent(a, k, "too many PA/RA/free dims");
    if (a.tau <= 0) {                       // not relaxed: no RA offsets
      a.nra = 0;
      std::fill_n(a.ra_idx, FA_MAX_RA, 0);
    }
    a.n_local = k.i("n_local");
    a.walk_k = k.i("walk_k");
    a.walk_steps = k.i("walk_steps");
    a.how = k.need<int8_t>("how");
    a.dseed = (uint32_t)k.u64("dseed");
    const int rc = fa_falsify_launch(net.d, a, finish(k));
    if (rc == 0) return false;
    if (rc < 0) ckl(-rc, "falsify");
    return true;
  });


  m.def("prune_masks", [](const Net& net, int Pn, uintptr_t counts, uintptr_t ub, int ub_stride, uintptr_t sym_dead,
                          uintptr_t code, uintptr_t cnt, uintptr_t stream) {
    ckl(fa_prune_masks_launch(net.d, Pn, P<const int>(counts), P<const float>(ub), ub_stride,
                                P<const uint8_t>(sym_dead), P<uint8_t>(code), P<int>(cnt), (hipStream_t)stream),
          "prune_masks");
  });

  m.def("heuristic", [](const Net& net, int Pu, uintptr_t rows, uintptr_t lb, uintptr_t ub, int stride, uintptr_t code,
                        double q50, double qlo, double qhi, uintptr_t hnew, uintptr_t hmerged, uintptr_t hcnt,
                        uintptr_t stream) {
    ckl(fa_heuristic_launch(net.d, Pu, P<const int64_t>(rows), P<const float>(lb), P<const float>(ub), stride,
                              P<const uint8_t>(code), q50, qlo, qhi, P<uint8_t>(hnew), P<uint8_t>(hmerged),
                              P<int>(hcnt), (hipStream_t)stream),
          "heuristic");
  });

  // returns false when the network shape is not supported (caller keeps the PyTorch path)
  m.def("agree", [](const Net& net, uintptr_t flat, int Pm, uintptr_t rows, uintptr_t lo, uintptr_t hi, uintptr_t pids,
                    uintptr_t dead, int S, uint32_t seed, uintptr_t agree, uintptr_t stream) {
    const int rc = fa_agree_launch(net.d, P<const float>(flat), Pm, P<const int64_t>(rows), P<const float>(lo),
                                   P<const float>(hi), P<const int64_t>(pids), P<const uint8_t>(dead), S, seed,
                                   P<int>(agree), (hipStream_t)stream);
    if (rc == 0) return false;
    if (rc < 0) ckl(-rc, "agree");
    return true;
  });

  m.def("certify", [](py::kwargs kw) {
    Kw k("certify", kw);
    auto in = [&](const char* key) { return k.need<const float>(key); };
    CertArgs a{};
    a.Nn = k.i("Nn"); a.n0 = k.i("n0"); a.V = k.i("V"); a.Pp = k.i("Pp"); a.norient = k.i("norient");
    a.Lc = in("Lc"); a.L0 = in("L0"); a.Le = in("Le"); a.Uc = in("Uc"); a.U0 = in("U0"); a.Ue = in("Ue");
    a.olb = in("olb"); a.oub = in("oub");
    a.Lcp = in("Lcp"); a.L0p = in("L0p"); a.Lep = in("Lep"); a.Ucp = in("Ucp"); a.U0p = in("U0p"); a.Uep = in("Uep");
    a.olbp = in("olbp"); a.oubp = in("oubp");
    a.xlo = in("xlo"); a.xhi = in("xhi"); a.xplo = in("xplo"); a.xphi = in("xphi");
    a.pairs = k.ptr<const int64_t>("pairs");
    a.values = k.ptr<const int64_t>("values");
    a.npa = dims(k, "pa", a.pa_idx, FA_CMAX_PA, "too many PA/RA dims");
    a.nra = dims(k, "ra", a.ra_idx, FA_MAX_RA, "too many PA/RA dims");
    a.tau = k.f("tau");
    a.shared = k.need<const uint8_t>("shared");
    a.unit = k.f("unit");
    a.gmarg = std::nextafter(k.f("gmarg"), INFINITY);
    a.gmin = k.ptr<float>("gmin"); a.tstar = k.ptr<float>("tstar");     // [Nn, Q]: empty without pairs
    a.open = k.need<uint8_t>("open"); a.score = k.need<float>("score"); a.split_dim = k.need<int64_t>("split_dim");
    a.cand_x = k.need<float>("cand_x"); a.cand_xp = k.need<float>("cand_xp");
    a.cand_v = k.need<int64_t>("cand_v"); a.cand_o = k.need<int64_t>("cand_o");
    a.scores = k.ptr<float>("scores"); a.leaf = k.ptr<uint8_t>("leaf");
    // the fields the native BaB runtime sets (absent: 0 / nullptr)
    a.skip_closed = k.i("skip_closed", 0);
    a.status = k.ptr<const int8_t>("status"); a.part = k.ptr<const int>("part");
    a.smear = k.i("smear", 0);
    a.lay_lb = k.ptr<const float>("lay_lb"); a.lay_ub = k.ptr<const float>("lay_ub"); a.lay_N = k.i("lay_N", 0);
    a.W0T = k.ptr<const float>("W0T"); a.n1 = k.i("n1", 0);
    if ((a.status == nullptr) != (a.part == nullptr)) throw std::invalid_argument("certify: status and part go together");
    if (a.smear && (!a.lay_lb || !a.lay_ub || !a.W0T || a.n1 <= 0 || a.lay_N < a.n1))
      throw std::invalid_argument("certify: smear needs lay_lb, lay_ub, W0T and 0 < n1 <= lay_N");
    ckl(fa_certify_launch(a, finish(k)), "certify");
  });

  // ---- BaB level kernels (bab.hip), one launch each: what tests/test_split_level_gpu.py compares with
  // the plain oracle of tests/split_cases.py.  The native runtime (bab_runtime.cpp) fills the same
  // structs itself.
  // split_level: one sub-batch of a level.  The settle_* keys (the SettleArgs fields) fuse the level
  // end into this launch; without settle_P there is none (settle.P = 0).  host_counts may be device
  // memory.
  m.def("split_level", [](py::kwargs kw) {
    Kw k("split_level", kw);
    SplitArgs a{};
    a.Nn = k.i("Nn"); a.n0 = k.i("n0"); a.relaxed = k.i("relaxed");
    a.V = k.i("V"); a.Pp = k.i("Pp"); a.norient = k.i("norient");
    a.nra = dims(k, "ra", a.ra_idx, FA_MAX_RA, "too many PA/RA dims");
    a.tau = k.f("tau");
    auto opt_if = [&](const char* key, bool req) { return req ? k.need<float>(key) : k.ptr<float>(key); };
    a.xlo = k.need<const float>("xlo"); a.xhi = k.need<const float>("xhi");
    a.xplo = opt_if("xplo", a.relaxed); a.xphi = opt_if("xphi", a.relaxed);
    a.part = k.need<const int>("part");
    a.open = k.need<const uint8_t>("open");
    a.leaf = k.need<const uint8_t>("leaf");
    a.scores = k.need<const float>("scores");
    a.cand_x = k.need<const float>("cand_x"); a.cand_xp = k.need<const float>("cand_xp");
    a.pe_lb = k.need<const float>("pe_lb"); a.pe_ub = k.need<const float>("pe_ub");
    a.olb = k.need<const float>("olb"); a.oub = k.need<const float>("oub");
    a.olbp = k.need<const float>("olbp"); a.oubp = k.need<const float>("oubp");
    a.pairs = k.ptr<const int64_t>("pairs");
    a.values = k.ptr<const int64_t>("values");
    a.npa = dims(k, "pa", a.pa_idx, FA_CMAX_PA, "too many PA/RA dims");
    a.shared = a.relaxed ? k.need<const uint8_t>("shared") : k.ptr<const uint8_t>("shared");
    a.status = k.need<int8_t>("status");
    a.part_nodes = k.need<int>("part_nodes");
    a.part_open = k.ptr<int>("part_open");
    a.lvl_open = k.ptr<int>("lvl_open");
    a.nodes_start = k.need<const int>("nodes_start");
    a.prev_start = k.need<const int>("prev_start");
    a.budget = k.i("budget");
    a.pbudget = k.ptr<const int>("pbudget");
    a.prob = k.ptr<uint8_t>("prob");
    a.budget2 = k.i("budget2");
    a.m = k.i("m");
    a.target = k.i("target");
    a.oxlo = k.need<float>("oxlo"); a.oxhi = k.need<float>("oxhi");
    a.oxplo = opt_if("oxplo", a.relaxed); a.oxphi = opt_if("oxphi", a.relaxed);
    a.opart = k.need<int>("opart");
    a.count_out = k.need<int>("count_out");
    a.cap = k.i("cap");
    a.cand_buf = k.need<float>("cand_buf");
    a.cand_count = k.need<int>("cand_count");
    a.cand_cap = k.i("cand_cap");
    if (kw.contains("settle_P")) a.settle = settle_args(k, "split_level", "settle_", true);
    if (a.Nn < 0 || a.n0 < 1 || a.V < 1 || a.norient < 1 || a.norient > 2 || a.Pp < 0 || a.cap < 0 || a.cand_cap < 0)
      throw std::invalid_argument("split_level: sizes out of range");
    if ((a.Pp > 0 && !a.pairs) || (a.npa > 0 && !a.values))
      throw py::type_error("split_level() missing required keyword argument 'pairs' / 'values'");
    for (int q = 0; q < a.npa; ++q)
      if (a.pa_idx[q] < 0 || a.pa_idx[q] >= a.n0) throw std::invalid_argument("split_level: PA dim outside the inputs");
    for (int q = 0; q < a.nra; ++q)
      if (a.ra_idx[q] < 0 || a.ra_idx[q] >= a.n0) throw std::invalid_argument("split_level: RA dim outside the inputs");
    const int rc = fa_split_launch(a, finish(k));
    if (rc == -3) throw std::invalid_argument("split_level: shape not covered (n0 > 64, more than 8 PA or RA dims)");
    ckl(rc, "split_level");
  });
  m.def("settle", [](py::kwargs kw) {
    Kw k("settle", kw);
    const SettleArgs s = settle_args(k, "settle", "", false);
    ckl(fa_settle_launch(s, finish(k)), "settle");
  });
  // stage: the device copy of the staged block [status int8 x P, padded to 4 B | running partition
  // ids x n_run | lo x n_run*n0 | hi x n_run*n0] (uint8)
  m.def("bab_init", [](py::kwargs kw) {
    Kw k("bab_init", kw);
    BabInitArgs a{};
    a.P = k.i("P"); a.n_run = k.i("n_run"); a.n0 = k.i("n0");
    a.stage = k.need<const unsigned char>("stage");
    a.status = k.need<int8_t>("status");
    a.nodes = k.need<int>("nodes"); a.open_left = k.need<int>("open_left"); a.lvl_open = k.need<int>("lvl_open");
    a.nodes_start = k.need<int>("nodes_start"); a.prev_start = k.need<int>("prev_start");
    a.part = k.need<int>("part");
    a.xlo = k.need<float>("xlo"); a.xhi = k.need<float>("xhi");
    a.xplo = k.ptr<float>("xplo"); a.xphi = k.ptr<float>("xphi");
    a.nra = dims(k, "ra", a.ra_idx, FA_MAX_RA, "too many PA/RA dims");
    a.tau = k.f("tau");
    a.counters = k.need<int>("counters");
    a.pbudget = k.ptr<int>("pbudget");
    a.prob = k.ptr<uint8_t>("prob");
    a.budget = k.i("budget");
    if (a.P < 0 || a.n_run < 0 || a.n0 < 1) throw std::invalid_argument("bab_init: sizes out of range");
    if ((a.xplo == nullptr) != (a.xphi == nullptr)) throw std::invalid_argument("bab_init: xplo and xphi go together");
    const int rc = fa_bab_init_launch(a, finish(k));
    if (rc == -3) throw std::invalid_argument("bab_init: more than 8 RA dims");
    ckl(rc, "bab_init");
  });
  m.def("bab_finish", [](py::kwargs kw) {
    Kw k("bab_finish", kw);
    const int Pn = k.i("P");
    const int8_t* status = k.need<const int8_t>("status");
    const int* nodes = k.need<const int>("nodes");
    const int* open_left = k.need<const int>("open_left");
    int* out = k.need<int>("out");
    ckl(fa_bab_finish_launch(Pn, status, nodes, open_left, out, finish(k)), "bab_finish");
  });
  m.def("mark_unknown", [](py::kwargs kw) {
    Kw k("mark_unknown", kw);
    const int* part = k.need<const int>("part");
    const int n = k.i("n");
    int8_t* status = k.need<int8_t>("status");
    ckl(fa_mark_unknown_launch(part, n, status, finish(k)), "mark_unknown");
  });
  m.def("set_status", [](py::kwargs kw) {
    Kw k("set_status", kw);
    const int* idx = k.need<const int>("idx");
    const int n = k.i("n");
    int8_t* status = k.need<int8_t>("status");
    const int v = k.i("v");
    ckl(fa_set_status_launch(idx, n, status, (int8_t)v, finish(k)), "set_status");
  });

  m.def("decode", [](std::vector<int> radix, std::vector<long long> div, std::vector<int> chunk_off,
                     std::vector<float> base_lo, std::vector<float> base_hi, uintptr_t ids, int Pn,
                     uintptr_t chunk_lo, uintptr_t chunk_hi, uintptr_t lo, uintptr_t hi, uintptr_t stream) {
    const size_t n0 = radix.size();
    if (n0 == 0 || n0 > FA_DECODE_MAX_DIMS || div.size() != n0 || chunk_off.size() != n0 || base_lo.size() != n0 ||
        base_hi.size() != n0)
      throw std::invalid_argument("decode: descriptor sizes");
    DecodeDesc d{};
    d.n0 = (int)n0;
    for (size_t k = 0; k < n0; ++k) {
      if (radix[k] < 0 || (radix[k] > 0 && div[k] <= 0)) throw std::invalid_argument("decode: radix/div");
      d.radix[k] = radix[k];
      d.div[k] = div[k];
      d.chunk_off[k] = chunk_off[k];
      d.base_lo[k] = base_lo[k];
      d.base_hi[k] = base_hi[k];
    }
    ckl(fa_decode_launch(d, P<const int64_t>(ids), Pn, P<const float>(chunk_lo), P<const float>(chunk_hi),
                           P<float>(lo), P<float>(hi), (hipStream_t)stream),
          "decode");
  });
  m.def("pack_masks", [](uintptr_t src, int Pn, int N, int stride, int sel, uintptr_t out, int NB, uintptr_t hash,
                         uintptr_t stream) {
    ckl(fa_pack_masks_launch(P<const uint8_t>(src), Pn, N, stride, sel, P<uint8_t>(out), NB,
                               P<unsigned long long>(hash), (hipStream_t)stream),
          "pack_masks");
  });
  m.def("knn", [](uintptr_t X, int n, int d, int k, uintptr_t idx, uintptr_t dist, uintptr_t stream) {
    ckl(fa_knn_launch(P<const float>(X), n, d, k, P<int>(idx), P<float>(dist), (hipStream_t)stream), "knn");
  });
  m.def("actdiff", [](const Net& net, uintptr_t flat, uintptr_t x, uintptr_t xp, int npairs, uintptr_t sum_out,
                      uintptr_t stream) {
    ckl(fa_actdiff_launch(net.d, P<const float>(flat), P<const float>(x), P<const float>(xp), npairs,
                            P<float>(sum_out), (hipStream_t)stream),
          "actdiff");
  });
  m.def("trace_marker", [](int tag, uintptr_t sink, uintptr_t stream) {
    ckl(fa_trace_marker_launch(tag, P<int>(sink), (hipStream_t)stream), "trace_marker");
  });
  // The beta entries return the launch code (0 done).
  m.def("beta_level", [](const Net& net, py::kwargs kw) {
    Kw k("beta_level", kw);
    const BetaArgs a = beta_args(net, k);
    return fa_beta_launch(net.d, a, finish(k));
  });
  // two-phase level (csrc/beta_opt16.hip): the batched MFMA optimiser, then fa_beta_kernel at iters = 0
  // seeded with its primal sums pgsum [R, 4, NH] / pgn [R]; scratch must hold
  // max(R * 12 * NH, beta_opt16_scratch(R)) floats
  m.def("beta_level16", [](const Net& net, py::kwargs kw) {
    Kw k("beta_level16", kw);
    const BetaArgs a = beta_args(net, k);
    return fa_beta_level16_launch(net.d, a, finish(k));
  });
  // phase 1 alone: par / t / gtie optimised in place (best iterate), pgsum / pgn written; no wt
  m.def("beta_opt16", [](const Net& net, py::kwargs kw) {
    Kw k("beta_opt16", kw);
    BetaArgs a = beta_args(net, k);
    float* pgsum = const_cast<float*>(a.pgsum);
    float* pgn = const_cast<float*>(a.pgn);
    a.wt = a.pgsum = a.pgn = nullptr;
    return fa_beta_opt16_launch(net.d, a, pgsum, pgn, finish(k));
  });
  // the infeasibility pass alone on rows whose main-pass outputs (par, t, gtie, bound) are given.  mode 0:
  // the per-node pass (fa_beta_kernel, feas = 1, `iters` steps; scratch [R, 16, NH]); 1: the two-phase
  // pass (proposals to fpar [R, 4, NH] / fgt [R, 2, n0] by the batched optimiser's feas mode, then the
  // per-node kernel at iters = 0 on them; scratch max(R * 16 * NH, beta_opt16_scratch(R))); 2: the
  // proposal phase alone; 3: the rigorous phase alone on the fpar / fgt given.  fval [R] (optional):
  // the rigorous value of the rows that ran.  bound: +inf written on the rows the pass closes.  Takes a
  // level's keywords: its branching keys (lookahead, beta_pos, flags, split, xstar, binit, xpstar) are
  // read and overridden
  m.def("beta_feas", [](const Net& net, py::kwargs kw) {
    Kw k("beta_feas", kw);
    BetaArgs a = beta_args(net, k);
    const int mode = k.i("mode");
    const hipStream_t st = finish(k);
    if (mode < 0 || mode > 3) throw std::invalid_argument("beta_feas: mode must be 0..3");
    if (mode != 0 && !a.fpar) throw std::invalid_argument("beta_feas: fpar required");
    a.lookahead = a.stall = a.pgap = 0;
    a.beta_pos = a.feas = 1;
    a.split = nullptr;
    a.xstar = a.binit = a.xpstar = nullptr;
    if (mode == 0) {
      a.fpar = a.fgt = nullptr;
      return fa_beta_launch(net.d, a, st);
    }
    if (mode == 1) return fa_beta_feas16_launch(net.d, a, st);
    if (mode == 2) return fa_beta_opt16_feas_launch(net.d, a, st);
    a.iters = 0;
    return fa_beta_launch(net.d, a, st);
  });
  m.def("beta_batched_fits", [](const Net& net) { return fa_beta_opt16_fits(net.d) != 0; });
  m.def("beta_opt16_scratch", [](const Net& net, int R) { return fa_beta_opt16_scratch_floats(net.d, R); });
  m.def("beta_config", [](const Net& net) {
    int w = 0, t = 0;
    size_t b = 0;
    const int rc = fa_beta_config(net.d, &w, &t, &b);
    return py::make_tuple(rc, w, t, b);
  });
  m.def("beta_fits", [](const Net& net) {
    int w = 0, t = 0;
    size_t b = 0;
    return fa_beta_config(net.d, &w, &t, &b) == 0;
  });
  m.def("arch", []() { return std::string("gfx950"); });
  // raise the dynamic-LDS limit of every registered kernel once (common.h); Backend construction
  // calls it before any host thread launches.  0 on success.
  m.def("prepare_lds", [] { return fa_lds_prepare(); });
  m.def("lds_registered", [] { return (int)fa_lds_registry().size(); });
  register_bab(m);
  register_relu(m);
  register_beta(m);
  // caching allocator of the native runtimes (devmem.h): hipFree / hipHostFree calls reaching the
  // driver stay 0 in steady state
  m.def("mem_stats", [] {
    const fa_mem::Stats s = fa_mem::stats();
    py::dict d;
    d["dev_cached_bytes"] = s.dev_cached_bytes;
    d["dev_live_bytes"] = s.dev_live_bytes;
    d["host_cached_bytes"] = s.host_cached_bytes;
    d["host_live_bytes"] = s.host_live_bytes;
    d["dev_mallocs"] = s.dev_mallocs;
    d["dev_hits"] = s.dev_hits;
    d["host_mallocs"] = s.host_mallocs;
    d["host_hits"] = s.host_hits;
    d["driver_frees"] = s.driver_frees;
    return d;
  });
  m.def("mem_release_cached", [] { fa_mem::release_cached(); });
  register_csv(m);
}
