// Keyword reader of the bindings that fill an args.h struct (bindings.cpp): every struct field crosses
// the Python/C++ boundary under its own name.  A key that is missing raises TypeError, and so does a
// key that nothing read (done()): a misspelt optional pointer must not turn into a null pointer.
#pragma once
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstdint>
#include <set>
#include <string>
#include <vector>

namespace py = pybind11;

class Kw {
 public:
  Kw(const char* fn, const py::kwargs& kw) : fn_(fn), kw_(kw) {}
  // device pointer (Tensor.data_ptr()): absent or 0 is nullptr / raises
  template <typename T> T* ptr(const char* k) { return reinterpret_cast<T*>(u64(k, 0)); }
  template <typename T> T* need(const char* k) {
    T* p = ptr<T>(k);
    if (!p) throw py::type_error(fn_ + "() missing required keyword argument '" + k + "'");
    return p;
  }
  int i(const char* k) { return as<int>(k, nullptr); }
  int i(const char* k, int dflt) { return as<int>(k, &dflt); }
  float f(const char* k) { return as<float>(k, nullptr); }
  float f(const char* k, float dflt) { return as<float>(k, &dflt); }
  uint64_t u64(const char* k) { return as<uint64_t>(k, nullptr); }
  uint64_t u64(const char* k, uint64_t dflt) { return as<uint64_t>(k, &dflt); }
  std::vector<int> ints(const char* k) { return as<std::vector<int>>(k, nullptr); }
  // every key passed must have been read by now
  void done() const {
    for (auto item : kw_) {
      const std::string k = py::str(item.first);
      if (!seen_.count(k)) throw py::type_error(fn_ + "() got an unexpected keyword argument '" + k + "'");
    }
  }

 private:
  template <typename V> V as(const char* k, const V* dflt) {
    seen_.insert(k);
    const py::handle h(PyDict_GetItemString(kw_.ptr(), k));
    if (!h && dflt) return *dflt;
    if (!h) throw py::type_error(fn_ + "() missing required keyword argument '" + k + "'");
    try {
      return h.cast<V>();
    } catch (const py::cast_error&) {
      throw py::type_error(fn_ + "(): keyword argument '" + k + "' has the wrong type");
    }
  }
  std::string fn_;
  const py::kwargs& kw_;
  std::set<std::string> seen_;
};
