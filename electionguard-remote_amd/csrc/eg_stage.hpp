// eg_stage.hpp — the chunked staging driver of the entry points that come in a host-pointer and
// a device-pointer variant (eg_capi_codes / contestdata / range / preencrypt.inc).  An entry point
// registers its buffers as COLUMNS, each with its bytes per item written once, and hands run() a
// callable that enqueues one chunk of m items on device pointers:
//
//   Stage st(ops, host, n, chunk);
//   st.once(dcon, nc * 32);            // read once per call, the same for every chunk
//   st.in(ids, 32);                    // per item, read by the chunk
//   st.out(sorted, nsel * 32);         // per item, written by the chunk; a null pointer is no column
//   return st.run([&](size_t m) { return chunk_locked(c, m, dcon, ids, sorted); });
//
// The columns are the entry point's own pointer variables: before each call of the callable the
// driver REBINDS them to that chunk's device pointers, so the callable reads them by reference.
//   device mode  per-item columns are the caller's pointer + i0 * stride, once columns are left as
//                they are; nothing is copied or synchronised.
//   host mode    every column is carved out of ONE device buffer (ops.alloc) at 256-byte offsets,
//                per-item columns sized for min(chunk, n) items.  Once columns are uploaded before
//                the loop; per chunk the inputs are uploaded, the callable runs, the outputs are
//                downloaded, then one sync.
// A non-zero status of the callable or of an operation ends run() with that status at once.
//
// No HIP here: the device work goes through Ops (eg_capi.hip binds it to the context's stream and
// workspace; tests/cpp/stage_test.cpp to memcpy):
//   int alloc(size_t bytes, void** out);  int h2d(void* dst, const void* src, size_t bytes);
//   int d2h(void* dst, const void* src, size_t bytes);  int sync();
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <vector>

namespace egstage {

constexpr size_t kAlign = 256;

template <class Ops>
class Stage {
 public:
  Stage(Ops ops, bool host, size_t n, size_t chunk) : ops_(ops), host_(host), n_(n), chunk_(std::max<size_t>(chunk, 1)) {}

  template <class T>
  void in(const T*& p, size_t stride) { add(&p, p, stride, kIn); }
  template <class T>
  void out(T*& p, size_t stride) {
    if (p) add(&p, p, stride, kOut);
  }
  template <class T>
  void once(const T*& p, size_t bytes) { add(&p, p, bytes, kOnce); }

  // offset of column i (in registration order) in the staging buffer; valid after a host-mode run()
  size_t offset(size_t i) const { return cols_[i].off; }

  template <class F>
  int run(F&& chunk_fn) {
    int rc;
    if (!n_) return 0;
    if (host_) {
      const size_t first = std::min(chunk_, n_);
      size_t total = 0;
      for (Col& c : cols_) {
        c.off = total;
        total += (c.stride * (c.kind == kOnce ? 1 : first) + kAlign - 1) / kAlign * kAlign;
      }
      void* buf = nullptr;
      if ((rc = ops_.alloc(total, &buf))) return rc;
      for (Col& c : cols_) {
        c.dev = (char*)buf + c.off;
        bind(c, c.dev);
        if (c.kind == kOnce && (rc = ops_.h2d(c.dev, c.user, c.stride))) return rc;
      }
    }
    for (size_t i0 = 0; i0 < n_; i0 += chunk_) {
      const size_t m = std::min(chunk_, n_ - i0);
      for (const Col& c : cols_) {
        if (c.kind == kOnce) continue;
        if (!host_) bind(c, c.user + i0 * c.stride);
        else if (c.kind == kIn && (rc = ops_.h2d(c.dev, c.user + i0 * c.stride, m * c.stride))) return rc;
      }
      if ((rc = chunk_fn(m))) return rc;
      if (!host_) continue;
      for (const Col& c : cols_)
        if (c.kind == kOut && (rc = ops_.d2h(c.user + i0 * c.stride, c.dev, m * c.stride))) return rc;
      if ((rc = ops_.sync())) return rc;
    }
    return 0;
  }

 private:
  enum Kind { kIn, kOut, kOnce };
  struct Col {
    void* var;     // the entry point's pointer variable
    char* user;    // the pointer the caller passed
    size_t stride; // bytes per item (kOnce: bytes)
    Kind kind;
    size_t off = 0;
    char* dev = nullptr;
  };
  void add(void* var, const void* user, size_t stride, Kind kind) {
    cols_.push_back(Col{var, (char*)user, stride, kind});
  }
  // object pointers share one representation: the variable is written as bytes, whatever it points to
  static void bind(const Col& c, const char* p) { std::memcpy(c.var, &p, sizeof p); }

  Ops ops_;
  bool host_;
  size_t n_, chunk_;
  std::vector<Col> cols_;
};

}  // namespace egstage
