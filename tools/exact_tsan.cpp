// Host sanitizer harness for the multi-threaded native paths ("thread-sanitizer for
// the host solver pool").  In a bench or CLI run, 8 host threads drive the BaB runtime without
// the GIL and each confirms its candidate pairs with fa_exact::ExactChecker
// (csrc/exact_host.h); rank 0's CSV formatting core (csrc/csv_format.h) runs on a background
// thread next to them.  This harness runs both from T threads that share ONE checker (read
// only) and writes results into per-thread buffers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=thread -pthread -Ifairify_amd/csrc tools/exact_tsan.cpp
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -pthread -Ifairify_amd/csrc tools/exact_tsan.cpp
//
// Checks: no data race / memory error reported by the sanitizer; every thread's verdicts equal
// the single-threaded ones; the fp64 sign with its rounding bound never contradicts a long-double
// evaluation of the same network (ambiguous points are allowed to answer "ask").
//
// The witness selection behind the runtimes' confirm_candidates (fa_exact::select_witnesses) runs
// on the main thread and on every one of the T threads, each on its own state: its result equals
// a naive reference (per partition the lexicographically smallest confirmed pair) and does not
// change under 20 shuffles of the record order; partitions already decided are never asked about
// and keep their witness; without a checker every remaining candidate is asked about; no records
// or only rejected ones give nothing; a partition id outside [0, P) throws.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "csv_format.h"
#include "exact_host.h"

static int ref_sign(const fa_exact::ExactChecker& c, const double* x) {
  std::vector<long double> h(x, x + c.n0), hn;
  for (int l = 0; l < c.n_layers; ++l) {
    const int nin = c.dims[l], nout = c.dims[l + 1];
    hn.assign(nout, 0.0L);
    for (int j = 0; j < nout; ++j) {
      long double z = c.w[c.b_off[l] + j];
      for (int i = 0; i < nin; ++i) z += h[i] * (long double)c.w[c.w_off[l] + (size_t)i * nout + j];
      hn[j] = (l < c.n_layers - 1 && z < 0) ? 0.0L : z;
    }
    h.swap(hn);
  }
  return h[0] > 0 ? 1 : (h[0] < 0 ? -1 : 0);
}

// ---- witness selection ---------------------------------------------------------------------------
namespace wsel {

using fa_exact::ExactChecker;
using fa_exact::Witnesses;

constexpr int P = 3;

// what the "exact rational check" answers in this harness: a fixed function of the pair and partition
static bool oracle(const float* pair, int n0, int part) {
  long s = part;
  for (int d = 0; d < 2 * n0; ++d) s += (long)std::llround(pair[d]) * (d + 1);
  return s % 3 != 0;
}

static int part_of(const float* rec, int n0, int i) {
  int p;
  std::memcpy(&p, rec + (size_t)i * (2 * n0 + 1) + 2 * n0, sizeof(int));
  return p;
}

static void set_part(std::vector<float>& rec, int n0, int i, int p) {
  std::memcpy(rec.data() + (size_t)i * (2 * n0 + 1) + 2 * n0, &p, sizeof(int));
}

struct Result {
  std::vector<char> got;
  std::vector<int64_t> cx, cxp;
  std::set<int> newly;
  bool operator==(const Result& o) const { return got == o.got && cx == o.cx && cxp == o.cxp && newly == o.newly; }
};

struct Case {
  int n0, n;
  std::vector<float> rec, lo, hi;   // n records; boxes [P][n0]
  bool preset;                      // partition 1 decided before, witness 77...
};

static Witnesses fresh(const Case& c) {
  Witnesses w(P, c.n0, c.lo.data(), c.hi.data());
  if (c.preset) {
    w.got[1] = 1;
    for (int d = 0; d < c.n0; ++d) w.cex_x[c.n0 + d] = w.cex_xp[c.n0 + d] = 77;
  }
  return w;
}

// naive reference: per undecided partition, the lexicographically smallest confirmed pair
static Result reference(const Case& c, const ExactChecker* chk) {
  Witnesses w = fresh(c);
  Result r;
  const int n0 = c.n0;
  const size_t rw = 2 * n0 + 1;
  for (int p = 0; p < P; ++p) {
    if (w.got[p]) continue;
    int best = -1;
    for (int i = 0; i < c.n; ++i) {
      const float* pr = c.rec.data() + i * rw;
      if (part_of(c.rec.data(), n0, i) != p) continue;
      int v = chk ? chk->check(pr, c.lo.data() + (size_t)p * n0, c.hi.data() + (size_t)p * n0) : -1;
      if (v < 0) v = oracle(pr, n0, p) ? 1 : 0;
      if (!v) continue;
      if (best < 0 || std::lexicographical_compare(pr, pr + 2 * n0, c.rec.data() + best * rw,
                                                    c.rec.data() + best * rw + 2 * n0))
        best = i;
    }
    if (best < 0) continue;
    w.got[p] = 1;
    r.newly.insert(p);
    for (int d = 0; d < n0; ++d) {
      w.cex_x[(size_t)p * n0 + d] = (int64_t)std::llround(c.rec[best * rw + d]);
      w.cex_xp[(size_t)p * n0 + d] = (int64_t)std::llround(c.rec[best * rw + n0 + d]);
    }
  }
  r.got = w.got; r.cx = w.cex_x; r.cxp = w.cex_xp;
  return r;
}

// runs the selection; *asked: how many candidates reached ask; *bad: ask saw a decided partition
// or inconsistent arguments
static Result select(const Case& c, const std::vector<float>& rec, const ExactChecker* chk, int* asked, int* bad) {
  Witnesses w = fresh(c);
  const std::vector<char> before = w.got;
  const size_t w2 = 2 * c.n0;
  const std::vector<int> newly = fa_exact::select_witnesses(
      rec.data(), c.n, w, chk,
      [&](const std::vector<int>& slots, const std::vector<float>& pairs, const std::vector<int>& parts) {
        std::vector<char> out(slots.size());
        *asked += (int)slots.size();
        if (pairs.size() != slots.size() * w2 || parts.size() != slots.size()) ++*bad;
        for (size_t k = 0; k < slots.size(); ++k) {
          if (before[parts[k]] || parts[k] != part_of(rec.data(), c.n0, slots[k]) ||
              std::memcmp(pairs.data() + k * w2, rec.data() + (size_t)slots[k] * (w2 + 1), w2 * sizeof(float)))
            ++*bad;
          out[k] = oracle(pairs.data() + k * w2, c.n0, parts[k]);
        }
        return out;
      });
  Result r;
  r.got = w.got; r.cx = w.cex_x; r.cxp = w.cex_xp;
  r.newly.insert(newly.begin(), newly.end());
  if (r.newly.size() != newly.size()) ++*bad;   // a partition reported twice
  return r;
}

// n records over P partitions: distinct pairs that meet the pair constraints of `chk` (PA dims
// differ, RA dim within tau, the rest shared) and duplicates of them in other slots
static Case make_case(const ExactChecker& chk, int n, unsigned seed, bool preset) {
  std::mt19937 g(seed);
  std::uniform_int_distribution<int> ui(0, 9);
  Case c;
  c.n0 = chk.n0; c.n = n; c.preset = preset;
  const int n0 = c.n0;
  const size_t rw = 2 * n0 + 1;
  c.lo.assign((size_t)P * n0, 0.f);
  c.hi.assign((size_t)P * n0, 9.f);
  c.rec.assign((size_t)n * rw, 0.f);
  const int distinct = std::max(1, (2 * n) / 3);
  for (int i = 0; i < n; ++i) {
    if (i >= distinct) {   // duplicate of an earlier record (pair and partition) in another slot
      const int j = ui(g) % distinct;
      std::copy(c.rec.begin() + j * rw, c.rec.begin() + (j + 1) * rw, c.rec.begin() + i * rw);
      continue;
    }
    for (int d = 0; d < n0; ++d) {
      const int x = ui(g);
      int xp = x;
      if (chk.is_pa[d]) xp = (x + 1 + ui(g) % 9) % 10;
      else if (chk.is_ra[d]) xp = std::min(9, x + ui(g) % 3);
      c.rec[i * rw + d] = (float)x;
      c.rec[i * rw + n0 + d] = (float)xp;
    }
    set_part(c.rec, n0, i, ui(g) % P);
  }
  return c;
}

static int fail(const char* what, int n0, unsigned seed) {
  std::printf("FAIL: witness selection, %s (n0 %d, seed %u)\n", what, n0, seed);
  return 1;
}

// every check of one (checker, seed); chk_or_null: the checker passed to the selection
static int run(const ExactChecker& chk, bool with_chk, unsigned seed) {
  int fails = 0;
  const int n0 = chk.n0;
  const ExactChecker* cp = with_chk ? &chk : nullptr;
  for (int preset = 0; preset < 2; ++preset) {
    const Case c = make_case(chk, 64, seed + preset, preset != 0);
    const Result ref = reference(c, cp);
    int asked = 0, bad = 0;
    const Result first = select(c, c.rec, cp, &asked, &bad);
    if (!(first == ref)) fails += fail("result differs from the naive reference", n0, seed);
    if (bad) fails += fail("ask saw a decided partition or wrong arguments", n0, seed);
    if (preset) {
      if (first.newly.count(1)) fails += fail("decided partition reported again", n0, seed);
      for (int d = 0; d < n0; ++d)
        if (first.cx[n0 + d] != 77 || first.cxp[n0 + d] != 77) fails += fail("decided witness overwritten", n0, seed);
    }
    int remaining = 0;
    for (int i = 0; i < c.n; ++i) remaining += !(preset && part_of(c.rec.data(), n0, i) == 1);
    if (!with_chk && asked != remaining) fails += fail("null checker: not every remaining candidate asked", n0, seed);
    if (!with_chk && !preset) {
      // the generated data must hold a partition with two distinct confirmed pairs
      bool two = false;
      for (int p = 0; p < P && !two; ++p) {
        std::set<std::vector<float>> conf;
        for (int i = 0; i < c.n; ++i) {
          const float* pr = c.rec.data() + (size_t)i * (2 * n0 + 1);
          if (part_of(c.rec.data(), n0, i) == p && oracle(pr, n0, p)) conf.insert(std::vector<float>(pr, pr + 2 * n0));
        }
        two = conf.size() >= 2;
      }
      if (!two) fails += fail("test data lacks two confirmed pairs in one partition", n0, seed);
    }
    // 20 shuffles of the record order
    std::mt19937 g(seed * 31 + 5);
    std::vector<int> perm(c.n);
    for (int i = 0; i < c.n; ++i) perm[i] = i;
    const size_t rw = 2 * n0 + 1;
    for (int it = 0; it < 20; ++it) {
      std::shuffle(perm.begin(), perm.end(), g);
      std::vector<float> rec(c.rec.size());
      for (int i = 0; i < c.n; ++i)
        std::copy(c.rec.begin() + perm[i] * rw, c.rec.begin() + (perm[i] + 1) * rw, rec.begin() + i * rw);
      int a2 = 0, b2 = 0;
      if (!(select(c, rec, cp, &a2, &b2) == ref) || b2) fails += fail("result changes with the record order", n0, seed);
    }
    // no records; only rejected records (no checker, ask says no to all)
    {
      Case e = c;
      e.n = 0;
      int a = 0, b = 0;
      const Result r = select(e, e.rec, cp, &a, &b);
      if (!r.newly.empty() || a != 0 || !(r.got == fresh(c).got)) fails += fail("zero records give a result", n0, seed);
      Witnesses w = fresh(c);
      const std::vector<int> none = fa_exact::select_witnesses(
          c.rec.data(), c.n, w, nullptr,
          [](const std::vector<int>& s, const std::vector<float>&, const std::vector<int>&) {
            return std::vector<char>(s.size(), 0);
          });
      if (!none.empty() || !(w.got == fresh(c).got) || !(w.cex_x == fresh(c).cex_x))
        fails += fail("rejected records give a result", n0, seed);
    }
    // a partition id outside [0, P) throws and nothing is indexed with it
    for (int badp : {-1, P}) {
      Case e = c;
      set_part(e.rec, n0, c.n / 2, badp);
      bool threw = false;
      int a = 0, b = 0;
      try {
        select(e, e.rec, cp, &a, &b);
      } catch (const std::runtime_error& ex) {
        threw = std::string(ex.what()).find("slot " + std::to_string(c.n / 2)) != std::string::npos;
      }
      if (!threw) fails += fail("partition id out of range not reported", n0, seed);
    }
  }
  return fails;
}

// a small checker of its own for n0 = 2 (PA dim 1); the harness's 13-input checker is the other shape
static ExactChecker small_checker() {
  ExactChecker c;
  c.n0 = 2;
  c.dims = {2, 3, 1};
  c.n_layers = 2;
  c.w_off = {0, 9};
  c.b_off = {6, 12};
  std::mt19937 g(11);
  std::normal_distribution<float> nd(0.f, 0.6f);
  for (int i = 0; i < 13; ++i) c.w.push_back((double)nd(g));
  c.is_pa = {0, 1};
  c.is_ra = {0, 0};
  return c;
}

static int run_all(const ExactChecker& big, const ExactChecker& small, unsigned seed) {
  int fails = 0;
  for (const ExactChecker* c : {&small, &big})
    for (int with_chk = 0; with_chk < 2; ++with_chk) fails += run(*c, with_chk != 0, seed);
  return fails;
}

}  // namespace wsel

int main(int argc, char** argv) {
  const int T = argc > 1 ? std::atoi(argv[1]) : 8;
  const int N = argc > 2 ? std::atoi(argv[2]) : 4000;
  std::mt19937 g(7);
  std::normal_distribution<float> nd(0.f, 0.4f);
  fa_exact::ExactChecker c;
  c.n0 = 13;
  c.dims = {13, 16, 8, 1};
  c.n_layers = 3;
  int off = 0;
  for (int l = 0; l < c.n_layers; ++l) {
    c.w_off.push_back(off);
    off += c.dims[l] * c.dims[l + 1];
    c.b_off.push_back(off);
    off += c.dims[l + 1];
  }
  for (int i = 0; i < off; ++i) c.w.push_back((double)nd(g));   // fp32 values, as the runtime's copy
  c.is_pa.assign(c.n0, 0);
  c.is_ra.assign(c.n0, 0);
  c.is_pa[8] = 1;   // Adult sex
  c.is_ra[0] = 1;   // age, tau 2 (relaxed query)
  c.tau = 2.f;
  // candidate pairs inside per-pair boxes; about half satisfy the pair constraints
  std::uniform_int_distribution<int> ui(0, 9);
  std::vector<float> pairs((size_t)N * 2 * c.n0), lo((size_t)N * c.n0), hi((size_t)N * c.n0);
  for (int k = 0; k < N; ++k) {
    for (int d = 0; d < c.n0; ++d) {
      lo[(size_t)k * c.n0 + d] = 0.f;
      hi[(size_t)k * c.n0 + d] = 9.f;
      const float x = (float)ui(g);
      float xp = x;
      if (d == 8) xp = (float)(1 - (int)x % 2);
      else if (d == 0) xp = std::fmin(9.f, x + (float)(ui(g) % 3));
      else if (ui(g) == 0 && k % 2) xp = (float)ui(g);   // breaks the shared-feature constraint
      pairs[(size_t)k * 2 * c.n0 + d] = x;
      pairs[(size_t)k * 2 * c.n0 + c.n0 + d] = xp;
    }
  }
  std::vector<int> serial(N);
  for (int k = 0; k < N; ++k)
    serial[k] = c.check(pairs.data() + (size_t)k * 2 * c.n0, lo.data() + (size_t)k * c.n0, hi.data() + (size_t)k * c.n0);
  int fails = 0, ask = 0, viol = 0;
  for (int k = 0; k < N; ++k) {
    ask += serial[k] < 0;
    viol += serial[k] == 1;
    std::vector<double> x(c.n0);
    for (int d = 0; d < c.n0; ++d) x[d] = pairs[(size_t)k * 2 * c.n0 + d];
    const int s = c.sign(x.data());
    if (s != 2 && s != ref_sign(c, x.data())) {
      if (++fails < 10) std::printf("FAIL: sign mismatch at pair %d\n", k);
    }
  }
  // witness selection: single-threaded, then (below) from every thread on its own state
  const fa_exact::ExactChecker small = wsel::small_checker();
  fails += wsel::run_all(c, small, 100);
  std::vector<int> wfails(T, 0);
  // T threads share the checker (const) and format CSV fields into their own strings
  std::vector<std::vector<int>> res(T, std::vector<int>(N));
  std::vector<std::string> text(T);
  std::vector<std::thread> th;
  for (int t = 0; t < T; ++t)
    th.emplace_back([&, t] {
      wfails[t] = wsel::run_all(c, small, 200 + 7 * t);
      for (int k = t; k < N + t; ++k) {
        const int i = k % N;   // every thread walks all pairs from a different start
        res[t][i] = c.check(pairs.data() + (size_t)i * 2 * c.n0, lo.data() + (size_t)i * c.n0,
                            hi.data() + (size_t)i * c.n0);
        fa_csv::append_repr(text[t], 0.001 * i + t);
        fa_csv::append_round4(text[t], 1.0 / (i + 1));
        std::vector<double> v(c.n0);
        for (int d = 0; d < c.n0; ++d) v[d] = pairs[(size_t)i * 2 * c.n0 + d];
        fa_csv::append_np_vector(text[t], v.data(), c.n0);
      }
    });
#ifdef FA_TSAN_SELFTEST
  // negative control: an unsynchronised shared counter, which the thread sanitizer must report
  static int shared_hits = 0;
  for (int t = 0; t < T; ++t) th.emplace_back([] { for (int i = 0; i < 1000; ++i) ++shared_hits; });
#endif
  for (auto& x : th) x.join();
  for (int t = 0; t < T; ++t) fails += wfails[t];
  for (int t = 0; t < T; ++t)
    for (int k = 0; k < N; ++k)
      if (res[t][k] != serial[k] && ++fails < 20) std::printf("FAIL: thread %d pair %d\n", t, k);
  std::printf("exact_tsan: %d threads x %d pairs, %d violations, %d ambiguous, %s\n", T, N, viol, ask,
              fails ? "FAILED" : "ok");
  return fails ? 1 : 0;
}
