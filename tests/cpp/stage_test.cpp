// CPU test of the chunked staging driver (electionguard-remote_amd/csrc/eg_stage.hpp), the code
// every host / _dev pair of libeg_hip.so's codes, contest-data, range and pre-encryption entry
// points runs its chunks through.  The operations are memcpy on a fake device arena and count their
// calls; the chunk callable checks what it is handed and computes its outputs from its inputs.
// Prints one JSON line; exit 0 when every case holds.
//
//   g++ -std=c++17 -O2 -I electionguard-remote_amd/csrc tests/cpp/stage_test.cpp
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "eg_stage.hpp"

static int g_failures = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      ++g_failures;                                                          \
      fprintf(stderr, "line %d: %s (%s)\n", __LINE__, #cond, g_case);        \
    }                                                                        \
  } while (0)
static char g_case[64] = "";

constexpr size_t kChunk = 4, kGuard = 64, kOnceBytes = 48;
constexpr size_t SA = 1, SB = 32, SX = 1024, SY = 32, SZ = 1;  // bytes per item of the columns

struct Arena {
  std::vector<uint8_t> mem;
  int allocs = 0, h2d = 0, d2h = 0, syncs = 0;
  int fail_h2d_at = 0;  // the k-th upload fails with status 9
  std::vector<size_t> h2d_bytes;
  bool holds(const void* p, size_t n) const {
    const uint8_t* q = (const uint8_t*)p;
    return !mem.empty() && q >= mem.data() && q + n <= mem.data() + mem.size();
  }
};

struct FakeOps {
  Arena* a;
  int alloc(size_t bytes, void** out) const {
    ++a->allocs;
    a->mem.assign(bytes, 0xEE);
    *out = a->mem.data();
    return 0;
  }
  int h2d(void* dst, const void* src, size_t n) const {
    ++a->h2d;
    if (a->fail_h2d_at && a->h2d == a->fail_h2d_at) return 9;
    a->h2d_bytes.push_back(n);
    if (!a->holds(dst, n) || a->holds(src, 1)) return 100;
    std::memcpy(dst, src, n);
    return 0;
  }
  int d2h(void* dst, const void* src, size_t n) const {
    ++a->d2h;
    if (!a->holds(src, n) || a->holds(dst, 1)) return 101;
    std::memcpy(dst, src, n);
    return 0;
  }
  int sync() const {
    ++a->syncs;
    return 0;
  }
};

// a caller's buffer of n * stride bytes between two guards
struct Guarded {
  std::vector<uint8_t> v;
  size_t bytes;
  Guarded(size_t n, size_t stride, uint8_t fill) : v(n * stride + 2 * kGuard, 0xA5), bytes(n * stride) {
    std::memset(data(), fill, bytes);
  }
  uint8_t* data() { return v.data() + kGuard; }
  bool guards_ok() const {
    for (size_t i = 0; i < kGuard; ++i)
      if (v[i] != 0xA5 || v[kGuard + bytes + i] != 0xA5) return false;
    return true;
  }
};

static uint8_t in_byte(int col, size_t item, size_t t) { return (uint8_t)(col * 67 + item * 13 + t * 7 + 1); }
// every output byte depends on both inputs and the once column of its own item
static uint8_t out_byte(int col, size_t item, size_t t) {
  return (uint8_t)(in_byte(0, item, 0) + in_byte(1, item, t % SB) * 3 + (uint8_t)(t % kOnceBytes) + col * 29 + t);
}

// One run of n items.  fail_chunk >= 0: the callable returns 7 in that chunk.
static void run_case(bool host, size_t n, int fail_chunk, int fail_h2d_at) {
  snprintf(g_case, sizeof g_case, "%s n=%zu fail_chunk=%d fail_h2d=%d", host ? "host" : "device", n, fail_chunk,
           fail_h2d_at);
  Arena ar;
  ar.fail_h2d_at = fail_h2d_at;
  Guarded A(n, SA, 0), B(n, SB, 0), X(n, SX, 0x5C), Y(n, SY, 0x5C), Z(n, SZ, 0x5C), K(1, kOnceBytes, 0);
  for (size_t i = 0; i < n; ++i) {
    A.data()[i] = in_byte(0, i, 0);
    for (size_t t = 0; t < SB; ++t) B.data()[i * SB + t] = in_byte(1, i, t);
  }
  for (size_t t = 0; t < kOnceBytes; ++t) K.data()[t] = (uint8_t)t;
  const uint8_t *a = A.data(), *k = K.data();
  const uint32_t* b = (const uint32_t*)B.data();  // a typed column: the stride is still in bytes
  uint8_t *x = X.data(), *y = Y.data(), *z = Z.data(), *w = nullptr;
  egstage::Stage<FakeOps> st(FakeOps{&ar}, host, n, kChunk);
  st.once(k, kOnceBytes);
  st.in(a, SA);
  st.in(b, SB);
  st.out(x, SX);
  st.out(w, 16);  // an optional output nobody asked for: no column
  st.out(y, SY);
  st.out(z, SZ);
  size_t i0 = 0, chunks = 0;
  int ops_at_failure = -1;
  const auto ops = [&] { return ar.allocs + ar.h2d + ar.d2h + ar.syncs; };
  const int rc = st.run([&](size_t m) -> int {
    CHECK(m == std::min(kChunk, n - i0));
    CHECK(w == nullptr);
    if (host) {
      CHECK(ar.holds(a, m * SA) && ar.holds(b, m * SB) && ar.holds(k, kOnceBytes));
      CHECK(ar.holds(x, m * SX) && ar.holds(y, m * SY) && ar.holds(z, m * SZ));
      for (const void* p : {(const void*)a, (const void*)b, (const void*)k, (const void*)x, (const void*)y, (const void*)z})
        CHECK(((const uint8_t*)p - ar.mem.data()) % 256 == 0);
    } else {  // the caller's own pointers, advanced by the items done
      CHECK(a == A.data() + i0 * SA && (const uint8_t*)b == B.data() + i0 * SB && k == K.data());
      CHECK(x == X.data() + i0 * SX && y == Y.data() + i0 * SY && z == Z.data() + i0 * SZ);
    }
    // exactly the caller's bytes of this chunk's items
    CHECK(std::memcmp(a, A.data() + i0 * SA, m * SA) == 0);
    CHECK(std::memcmp(b, B.data() + i0 * SB, m * SB) == 0);
    CHECK(std::memcmp(k, K.data(), kOnceBytes) == 0);
    if ((int)chunks == fail_chunk) {
      ops_at_failure = ops();
      return 7;
    }
    for (size_t j = 0; j < m; ++j) {
      CHECK(a[j] == in_byte(0, i0 + j, 0));
      for (size_t t = 0; t < SX; ++t) x[j * SX + t] = out_byte(0, i0 + j, t);
      for (size_t t = 0; t < SY; ++t) y[j * SY + t] = out_byte(1, i0 + j, t);
      z[j] = out_byte(2, i0 + j, 0);
    }
    i0 += m;
    ++chunks;
    return 0;
  });
  const size_t nchunks = (n + kChunk - 1) / kChunk;
  size_t done = n;  // items whose outputs must have landed
  if (fail_chunk >= 0) {
    CHECK(rc == 7 && (int)chunks == fail_chunk && ops() == ops_at_failure);
    done = (size_t)fail_chunk * kChunk;
  } else if (fail_h2d_at) {
    CHECK(rc == 9 && ar.h2d == fail_h2d_at && ar.d2h == 3 * (int)chunks && ar.syncs == (int)chunks);
    done = chunks * kChunk;
  } else {
    CHECK(rc == 0 && chunks == nchunks);
    if (host) {
      CHECK(ar.allocs == 1 && ar.syncs == (int)nchunks);
      CHECK(ar.h2d == 1 + 2 * (int)nchunks && ar.d2h == 3 * (int)nchunks);
      size_t once_uploads = 0;
      for (size_t bts : ar.h2d_bytes) once_uploads += bts == kOnceBytes;
      CHECK(once_uploads == 1 && ar.h2d_bytes.front() == kOnceBytes);
      for (size_t c = 0; c < 6; ++c) CHECK(st.offset(c) % 256 == 0);
      const size_t first = std::min(kChunk, n);
      CHECK(ar.mem.size() == 256 + 256 + 256 + first * SX + 256 + 256);  // every column at most one 256-byte row but x
    }
  }
  if (!host) CHECK(ops() == 0);
  // outputs at i0 * stride and nowhere else
  for (size_t i = 0; i < n; ++i) {
    bool ok = true;
    for (size_t t = 0; t < SX; ++t) ok &= X.data()[i * SX + t] == (i < done ? out_byte(0, i, t) : 0x5C);
    for (size_t t = 0; t < SY; ++t) ok &= Y.data()[i * SY + t] == (i < done ? out_byte(1, i, t) : 0x5C);
    ok &= Z.data()[i] == (i < done ? out_byte(2, i, 0) : 0x5C);
    CHECK(ok);
  }
  CHECK(A.guards_ok() && B.guards_ok() && X.guards_ok() && Y.guards_ok() && Z.guards_ok() && K.guards_ok());
  // the inputs are read only
  for (size_t i = 0; i < n; ++i) CHECK(A.data()[i] == in_byte(0, i, 0) && B.data()[i * SB + 5] == in_byte(1, i, 5));
}

int main() {
  int cases = 0;
  for (int host = 0; host < 2; ++host) {
    for (size_t n : {(size_t)1, kChunk - 1, kChunk, kChunk + 1, 2 * kChunk + 3}) {
      run_case(host != 0, n, -1, 0);
      ++cases;
    }
    run_case(host != 0, 2 * kChunk + 3, 1, 0);  // the callable fails in the second of three chunks
    ++cases;
  }
  run_case(true, 2 * kChunk + 3, -1, 1);  // the once column's upload fails: the callable never runs
  run_case(true, 2 * kChunk + 3, -1, 4);  // an input upload of the second chunk fails
  cases += 2;
  // no items: nothing is called
  {
    snprintf(g_case, sizeof g_case, "n=0");
    Arena ar;
    const uint8_t* a = nullptr;
    egstage::Stage<FakeOps> st(FakeOps{&ar}, true, 0, kChunk);
    st.in(a, 1);
    int calls = 0;
    CHECK(st.run([&](size_t) { return ++calls; }) == 0 && !calls && !ar.allocs && !ar.h2d && !ar.syncs);
    ++cases;
  }
  printf("{\"cases\": %d, \"failures\": %d}\n", cases, g_failures);
  return g_failures ? 1 : 0;
}
