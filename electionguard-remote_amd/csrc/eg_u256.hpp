// eg_u256.hpp — the 256-bit scalars of the proofs and their arithmetic mod q: one thread per
// scalar, scalars in memory are 32 bytes big-endian.  Plain integer code with no HIP in it beyond
// the function qualifiers: the device headers include it under hipcc, and tests/cpp/u256_test.cpp
// compiles the same bodies with a plain host compiler (as eg_powjob.hpp's test does).
//
// What is branch-free in its operands is said at each function; trustee secrets, nonces and votes
// only ever go through those.  mulsmall_mod is the one function that loops on its data.
#pragma once
#include <stdint.h>

// EG_U256_FN(inl): the qualifiers of every function here.  Under hipcc a device function with the
// inlining it names (mulmod256 is __noinline__: one copy per kernel, not one per call); on the host
// a plain inline function.
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define EG_U256_FN(inl) __device__ inl
#else
#define EG_U256_FN(inl) inline
#endif

namespace eg {

struct U256 {
  uint32_t w[8];  // little-endian words
};
EG_U256_FN(__forceinline__) U256 ld256(const uint8_t* __restrict__ be) {
  U256 r;
  const uint32_t* s = reinterpret_cast<const uint32_t*>(be);
#pragma unroll
  for (int i = 0; i < 8; ++i) r.w[i] = __builtin_bswap32(s[7 - i]);
  return r;
}
EG_U256_FN(__forceinline__) void st256(uint8_t* __restrict__ be, const U256& a) {
  uint32_t* d = reinterpret_cast<uint32_t*>(be);
#pragma unroll
  for (int i = 0; i < 8; ++i) d[7 - i] = __builtin_bswap32(a.w[i]);
}
// the scalar of a value below 2^32, and zero
EG_U256_FN(__forceinline__) U256 u256_small(uint32_t v) {
  U256 r;
  r.w[0] = v;
#pragma unroll
  for (int i = 1; i < 8; ++i) r.w[i] = 0;
  return r;
}
EG_U256_FN(__forceinline__) U256 u256_zero() { return u256_small(0); }
// a == b, every word compared whatever the others gave
EG_U256_FN(__forceinline__) bool eq256(const U256& a, const U256& b) {
  uint32_t d = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) d |= a.w[i] ^ b.w[i];
  return d == 0;
}
// The mod-q helpers below are branch-free in their operands (trustee responses v = u - c s and
// the encryption's R c_fake touch secrets): a < b is the borrow of a - b, selections are masks.
EG_U256_FN(__forceinline__) bool lt256(const U256& a, const U256& b) {
  int64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    c += (int64_t)a.w[i] - (int64_t)b.w[i];
    c >>= 32;
  }
  return c != 0;
}
EG_U256_FN(__forceinline__) U256 sel256(uint32_t mask, const U256& a, const U256& b) {  // mask ? a : b
  U256 r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.w[i] = (a.w[i] & mask) | (b.w[i] & ~mask);
  return r;
}
EG_U256_FN(__forceinline__) uint32_t add256(U256& a, const U256& b) {
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    c += (uint64_t)a.w[i] + b.w[i];
    a.w[i] = (uint32_t)c;
    c >>= 32;
  }
  return (uint32_t)c;
}
EG_U256_FN(__forceinline__) uint32_t sub256(U256& a, const U256& b) {
  int64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    c += (int64_t)a.w[i] - (int64_t)b.w[i];
    a.w[i] = (uint32_t)c;
    c >>= 32;
  }
  return (uint32_t)(c & 1);
}
// (a + b) mod q for a, b < q
EG_U256_FN(__forceinline__) U256 addmod256(U256 a, const U256& b, const U256& q) {
  const uint32_t carry = add256(a, b);
  U256 t = a;
  const uint32_t borrow = sub256(t, q);
  return sel256(0u - (carry | (borrow ^ 1u)), t, a);  // subtract q iff a + b >= q
}
// (L * a) mod q for a < q, L < 2^32  (schoolbook + repeated subtraction-free fold).
// NOT branch-free: the subtraction loop runs floor(L a / q) < L times, so its trip count follows
// the data.  For PUBLIC values only: the verifier's challenges and the selection limits.
EG_U256_FN(__forceinline__) U256 mulsmall_mod(const U256& a, uint32_t L, const U256& q) {
  // r = L*a as 288-bit, then reduce by long division on the top word
  uint32_t r[9];
  uint64_t c = 0;
  for (int i = 0; i < 8; ++i) {
    c += (uint64_t)a.w[i] * L;
    r[i] = (uint32_t)c;
    c >>= 32;
  }
  r[8] = (uint32_t)c;
  U256 x;
  for (int i = 0; i < 8; ++i) x.w[i] = r[i];
  // subtract hi * q repeatedly: value = r8*2^256 + x; x < 2^256, r8 < L
  // reduce via q's structure-free approach: while (r8 || x >= q) x -= q (with borrow into r8)
  uint32_t hi = r[8];
  while (hi != 0 || !lt256(x, q)) {
    const uint32_t borrow = sub256(x, q);
    hi -= borrow;
  }
  return x;
}
EG_U256_FN(__forceinline__) U256 negmod(const U256& a, const U256& q) {  // (q - a) mod q, branch-free
  uint32_t nz = 0;
  for (int i = 0; i < 8; ++i) nz |= a.w[i];
  U256 r = q;
  sub256(r, a);
  return sel256(0u - (uint32_t)(nz != 0), r, a);
}

// (a - b) mod q for a, b < q
EG_U256_FN(__forceinline__) U256 submod256(U256 a, const U256& b, const U256& q) {
  const uint32_t borrow = sub256(a, b);
  U256 t = a;
  add256(t, q);
  return sel256(0u - borrow, t, a);
}
// (a * b) mod q for a, b < q: left-to-right double-and-always-add with a masked select (one
// thread; per proof, not per limb), so neither operand's bits steer the control flow.  r is
// zeroed in place, not through u256_zero(): with the call the same 231 instructions come out on
// other register numbers (profiles/u256_hash_codegen.txt has both listings), and the code that
// trustee secrets pass through is kept instruction for instruction.
EG_U256_FN(__noinline__) U256 mulmod256(const U256& a, const U256& b, const U256& q) {
  U256 r;
  for (int k = 0; k < 8; ++k) r.w[k] = 0;
  for (int bit = 255; bit >= 0; --bit) {
    r = addmod256(r, r, q);
    const U256 t = addmod256(r, b, q);
    r = sel256(0u - ((a.w[bit >> 5] >> (bit & 31)) & 1u), t, r);
  }
  return r;
}
// (k * a) mod q for a < q and k < 256, on a fixed schedule of eight doublings and eight masked
// additions: neither k (the prover's value m) nor a steers a branch.
EG_U256_FN(__forceinline__) U256 mulbyte_mod(const U256& a, uint32_t k, const U256& q) {
  U256 r = u256_zero();
  for (int bit = 7; bit >= 0; --bit) {
    r = addmod256(r, r, q);
    const U256 t = addmod256(r, a, q);
    r = sel256(0u - ((k >> bit) & 1u), t, r);
  }
  return r;
}
// x mod q for ANY 256-bit x and any q > 1, branch-free in x: the double-and-add ladder of
// mulmod256 over x's bits with the addend 1 (the trustee's secret and nonces pass through here).
// mulmod256 asks b < q only of its addend, and 1 < q.
EG_U256_FN(__forceinline__) U256 mod256_any(const U256& x, const U256& q) { return mulmod256(x, u256_small(1), q); }

}  // namespace eg
