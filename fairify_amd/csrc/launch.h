// Host launch support shared by the kernel families with occupancy-capped grids and
// compile-time-shape instances (symbolic.hip, crown.hip, refine.hip, points.hip, forward.hip):
// the CU count, the cached occupancy query, the 16-neuron tile arithmetic of the MFMA operand
// layouts, and the table of shaped instances.  Host code only; no kernel lives here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>

#include "common.h"

// compute units of the current device (256 when the query fails), asked once
inline int fa_device_cus() {
  static int cus = 0;
  static std::once_flag once;
  std::call_once(once, [] {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
      cus = 256;
  });
  return cus;
}

// Resident workgroups per CU of `kernel` at `threads` per workgroup and `bytes` of dynamic LDS,
// cached per (kernel, threads, bytes); at least 1.  0: the LDS limit of the registered kernels is
// not raised yet (fa_lds_ok, common.h) -- the caller returns its "not ready" code and launches nothing.
inline int fa_blocks_per_cu(const void* kernel, int threads, size_t bytes) {
  if (!fa_lds_ok(bytes)) return 0;
  static std::mutex mu;
  static std::map<std::tuple<const void*, int, size_t>, int> occ;
  std::lock_guard<std::mutex> g(mu);
  const auto key = std::make_tuple(kernel, threads, bytes);
  auto it = occ.find(key);
  if (it != occ.end()) return it->second;
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, bytes) != hipSuccess || per_cu <= 0)
    per_cu = 1;
  occ[key] = per_cu;
  return per_cu;
}

// ---- 16-neuron tiles ----------------------------------------------------------------------------
inline int fa_tiles(int n) { return (n + 15) / 16; }

// widest of dims[lo..hi] in tiles (at least 1)
inline int fa_widest_tiles(const NetDesc& net, int lo, int hi) {
  int tm = 1;
  for (int l = lo; l <= hi; ++l) tm = std::max(tm, fa_tiles(net.dims[l]));
  return tm;
}

// the TM template bucket (1 / 2 / 4 / 7 / 10) that holds a layer of `tm` tiles; 0: wider than any
inline int fa_tm_bucket(int tm) { return tm <= 1 ? 1 : tm <= 2 ? 2 : tm <= 4 ? 4 : tm <= 7 ? 7 : tm <= 10 ? 10 : 0; }

// MFMA-operand-order layout: layer l's weight tiles at w_lds[l] for the first `nl` layers, starting
// at float offset `off`; returns the offset behind them
inline int fa_lay_weights(const NetDesc& net, int nl, int* w_lds, int off) {
  for (int l = 0; l < nl; ++l) {
    w_lds[l] = off;
    off += fa_tiles(net.dims[l]) * fa_tiles(net.dims[l + 1]) * 256;
  }
  return off;
}
// ... and the same layers' biases, unpadded, at b_lds[l]
inline int fa_lay_biases(const NetDesc& net, int nl, int* b_lds, int off) {
  for (int l = 0; l < nl; ++l) {
    b_lds[l] = off;
    off += net.dims[l + 1];
  }
  return off;
}

// is the environment switch `name` set to 0?  (read per call: the bitwise-equality tests toggle the
// *_SHAPED switches between launches)
inline bool fa_env_off(const char* name) {
  const char* e = getenv(name);
  return e && *e == '0';
}

// ---- compile-time-shape instances ---------------------------------------------------------------
// One entry per instance: `key` is whatever else the file's selection distinguishes (its TM bucket,
// paired / packed, mask; 0 when nothing), dims the layer widths dims[0..L] the instance was compiled for.
template <class K>
struct FaShaped {
  int key;
  std::vector<int> dims;
  K k;
};
// the instance compiled for this key and exactly net.dims[0..L], or nullptr
template <class K>
K fa_find_shaped(const std::vector<FaShaped<K>>& table, const NetDesc& net, int key) {
  for (const auto& s : table)
    if (s.key == key && (int)s.dims.size() == net.n_layers + 1 && std::equal(s.dims.begin(), s.dims.end(), net.dims))
      return s.k;
  return nullptr;
}
