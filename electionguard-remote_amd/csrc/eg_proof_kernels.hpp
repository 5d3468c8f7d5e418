// eg_proof_kernels.hpp — the scalar and hash kernels around k_pow that every proof family shares:
// the encryption's scalars (k_enc_*), the generic response (k_response), the verifier's scalar
// derivation (k_scalar_prep*), the reduction mod q (k_reduce_q) and the Fiat-Shamir hash + compare
// (k_hash_check).  One thread per item; the arithmetic is eg_u256.hpp's, the pre-image writer
// eg_hash_elems.hpp's.  Only eg_capi.hip includes this: the 16-lane unit (eg_pow16.hip) takes
// eg_kernels.hpp alone and compiles none of it.
#pragma once
#include "eg_hash_elems.hpp"
#include "eg_kernels.hpp"
#include "eg_u256.hpp"

namespace eg {

// Encryption scalars, one thread per selection (nonces n = (R, u, c_fake, v_fake)):
//   s_fake = v_fake + R*c_fake, s_gneg = m ? c_fake : -c_fake, mscal = m   (mod q)
// (known-nonce simulation of the fake branch: a_f = g^s_fake, b_f = K^s_fake g^(+-c_fake)).
// plus (eg_ctx_set_proof_format EG_RESPONSE_PLUS: a = g^v X^-c): s_fake = v_fake - R*c_fake and
// s_gneg = m ? -c_fake : c_fake.  The response convention is public; the vote stays masked.
__global__ void k_enc_prep(const uint8_t* __restrict__ q_be, const uint8_t* __restrict__ votes,
                           const uint8_t* __restrict__ nonces, uint32_t n, uint8_t* __restrict__ derived,
                           uint32_t plus) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const U256 q = ld256(q_be);
  const U256 R = ld256(nonces + ((size_t)i * 4 + 0) * 32);
  const U256 cf = ld256(nonces + ((size_t)i * 4 + 2) * 32);
  const U256 vf = ld256(nonces + ((size_t)i * 4 + 3) * 32);
  const uint32_t m = votes[i] ? 1u : 0u;
  const U256 Rc = mulmod256(R, cf, q);
  const U256 sf = plus ? submod256(vf, Rc, q) : addmod256(vf, Rc, q);
  // (m xor plus) ? c_fake : -c_fake, branch-free in the (secret) vote
  const U256 sg = sel256((0u - m) ^ (0u - (plus & 1u)), cf, negmod(cf, q));
  st256(derived + ((size_t)i * 3 + 0) * 32, u256_small(m));
  st256(derived + ((size_t)i * 3 + 1) * 32, sf);
  st256(derived + ((size_t)i * 3 + 2) * 32, sg);
}

// R_sum per contest (one thread per contest): sum of the spc selection nonces R
__global__ void k_enc_rsum(const uint8_t* __restrict__ q_be, const uint8_t* __restrict__ nonces, uint32_t ncon,
                           uint32_t spc, uint8_t* __restrict__ rsum) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= ncon) return;
  const U256 q = ld256(q_be);
  U256 r = u256_zero();
  for (uint32_t s = 0; s < spc; ++s) r = addmod256(r, ld256(nonces + (((size_t)j * spc + s) * 4) * 32), q);
  st256(rsum + (size_t)j * 32, r);
}

// k_enc_rsum for a manifest of unequal contests: contest j = b * nc + k sums the len[k] selection
// nonces R from selection b * nsel + first[k] on
__global__ void k_enc_rsum_seg(const uint8_t* __restrict__ q_be, const uint8_t* __restrict__ nonces, uint32_t ncon,
                               uint32_t nc, uint32_t nsel, const uint32_t* __restrict__ first,
                               const uint32_t* __restrict__ len, uint8_t* __restrict__ rsum) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= ncon) return;
  const U256 q = ld256(q_be);
  const uint32_t b = j / nc, k = j % nc, n = len[k];
  const size_t s0 = (size_t)b * nsel + first[k];
  U256 r = u256_zero();
  for (uint32_t s = 0; s < n; ++s) r = addmod256(r, ld256(nonces + ((s0 + s) * 4) * 32), q);
  st256(rsum + (size_t)j * 32, r);
}

// Finish the range proofs: c_real = c - c_fake, v_real = u - c_real*R (plus: u + c_real*R); arrange by m.
__global__ void k_enc_finish(const uint8_t* __restrict__ q_be, const uint8_t* __restrict__ votes,
                             const uint8_t* __restrict__ nonces, const uint8_t* __restrict__ chal, uint32_t n,
                             uint8_t* __restrict__ rproof, uint32_t plus) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const U256 q = ld256(q_be);
  const U256 R = ld256(nonces + ((size_t)i * 4 + 0) * 32);
  const U256 u = ld256(nonces + ((size_t)i * 4 + 1) * 32);
  const U256 cf = ld256(nonces + ((size_t)i * 4 + 2) * 32);
  const U256 vf = ld256(nonces + ((size_t)i * 4 + 3) * 32);
  const U256 c = ld256(chal + (size_t)i * 32);
  const U256 cr = submod256(c, cf, q);
  const U256 cR = mulmod256(cr, R, q);
  const U256 vr = plus ? addmod256(u, cR, q) : submod256(u, cR, q);
  uint8_t* o = rproof + (size_t)i * 4 * 32;
  const uint32_t mk = 0u - (uint32_t)(votes[i] != 0);  // the branch order follows the vote: masked
  st256(o + 0, sel256(mk, cf, cr));
  st256(o + 32, sel256(mk, vf, vr));
  st256(o + 64, sel256(mk, cr, cf));
  st256(o + 96, sel256(mk, vr, vf));
}

// Encryption commitments are computed vote-independently, real branch (a, b) in slots 0-1 and
// the simulated branch in slots 2-3 of each selection's 4 commitment elements; this puts them in
// proof order (branch 0 first), i.e. swaps the pairs where the vote is 1, with masks (the vote
// is secret).  One thread per 4-word column of a selection's pair.
__global__ void k_enc_order(uint32_t* __restrict__ comm, const uint8_t* __restrict__ votes, uint32_t n) {
  constexpr uint32_t kQuads = 2 * kW / 4;  // a pair of elements, in uint4
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)n * kQuads) return;
  const uint32_t i = (uint32_t)(t / kQuads), k = (uint32_t)(t % kQuads);
  const uint32_t mk = 0u - (uint32_t)(votes[i] != 0);
  uint4* lo = reinterpret_cast<uint4*>(comm + (size_t)i * 4 * kW) + k;
  uint4* hi = lo + kQuads;
  const uint4 a = *lo, b = *hi;
  *lo = make_uint4((a.x & ~mk) | (b.x & mk), (a.y & ~mk) | (b.y & mk), (a.z & ~mk) | (b.z & mk),
                   (a.w & ~mk) | (b.w & mk));
  *hi = make_uint4((b.x & ~mk) | (a.x & mk), (b.y & ~mk) | (a.y & mk), (b.z & ~mk) | (a.z & mk),
                   (b.w & ~mk) | (a.w & mk));
}

// Generic response v = u - c*x mod q (plus: u + c*x; x per item or shared when x_stride == 0);
// writes proof (c, v) as 2 x 32 B.
__global__ void k_response(const uint8_t* __restrict__ q_be, const uint8_t* __restrict__ u_be,
                           const uint8_t* __restrict__ chal, const uint8_t* __restrict__ x_be, uint32_t x_stride,
                           uint32_t n, uint8_t* __restrict__ proof, uint32_t plus) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const U256 q = ld256(q_be);
  const U256 u = ld256(u_be + (size_t)i * 32);
  const U256 c = ld256(chal + (size_t)i * 32);
  const U256 x = ld256(x_be + (size_t)i * x_stride);
  const U256 cx = mulmod256(c, x, q);
  const U256 v = plus ? addmod256(u, cx, q) : submod256(u, cx, q);
  st256(proof + (size_t)i * 64, c);
  st256(proof + (size_t)i * 64 + 32, v);
}

// out[i] = in[i] mod q for any 256-bit in[i], branch-free in it (a trustee's secret, nonces and
// challenges; the mix's nonces).  out may be in: a thread reads its scalar before it writes it.
__global__ void __launch_bounds__(kBlock) k_reduce_q(const uint8_t* __restrict__ q_be, const uint8_t* in, uint64_t n,
                                                     uint8_t* out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const U256 q = ld256(q_be);
  st256(out + i * 32, mod256_any(ld256(in + i * 32), q));
}

// scalar derivation for the verifier (one thread per selection / contest)
//   sel: out[i] = (q - c1_i) mod q  ; ok[i] = all of c0,v0,c1,v1 < q
//   con: out[i] = (q - L*c_i mod q) ; ok[i] = c,v < q
// plus (EG_RESPONSE_PLUS, a = g^v X^-c): out[i] = L*c_i mod q, and the proof words in neg_mask
// (the challenges the variable bases are raised to) are negated in place, so the same job tables
// compute X^-c; the Fiat-Shamir check then reads the caller's unmodified proofs.
__device__ __forceinline__ void scalar_prep_item(const uint8_t* __restrict__ q_be, uint8_t* __restrict__ proofs,
                                                 uint32_t i, uint32_t words_per, uint32_t neg_idx, uint32_t L,
                                                 uint8_t* __restrict__ out, uint8_t* __restrict__ ok, uint32_t plus,
                                                 uint32_t neg_mask) {
  const U256 q = ld256(q_be);
  bool good = true;
  for (uint32_t k = 0; k < words_per; ++k) good &= lt256(ld256(proofs + ((size_t)i * words_per + k) * 32), q);
  U256 c = ld256(proofs + ((size_t)i * words_per + neg_idx) * 32);
  if (good) {
    if (L != 1) c = mulsmall_mod(c, L, q);
    if (!plus) c = negmod(c, q);
    if (plus)
      for (uint32_t k = 0; k < words_per; ++k)
        if ((neg_mask >> k) & 1u) {
          uint8_t* w = proofs + ((size_t)i * words_per + k) * 32;
          st256(w, negmod(ld256(w), q));
        }
  } else {
    c = u256_zero();
  }
  st256(out + (size_t)i * 32, c);
  ok[i] = good ? 1 : 0;
}

__global__ void k_scalar_prep(const uint8_t* __restrict__ q_be, uint8_t* __restrict__ proofs,
                              uint32_t n, uint32_t words_per, uint32_t neg_idx, uint32_t L,
                              uint8_t* __restrict__ out, uint8_t* __restrict__ ok, uint32_t plus,
                              uint32_t neg_mask) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  scalar_prep_item(q_be, proofs, i, words_per, neg_idx, L, out, ok, plus, neg_mask);
}

// the contest form for a manifest of unequal contests: item i (contest i % period of its ballot)
// takes its selection limit L from Ltab[i % period]
__global__ void k_scalar_prep_tab(const uint8_t* __restrict__ q_be, uint8_t* __restrict__ proofs,
                                  uint32_t n, uint32_t words_per, uint32_t neg_idx,
                                  const uint32_t* __restrict__ Ltab, uint32_t period,
                                  uint8_t* __restrict__ out, uint8_t* __restrict__ ok, uint32_t plus,
                                  uint32_t neg_mask) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  scalar_prep_item(q_be, proofs, i, words_per, neg_idx, Ltab[i % period], out, ok, plus, neg_mask);
}

// ---------------------------------------------------------------------------------
// Fiat-Shamir hash + compare (one thread per proof).
//   H = hash_elems(qbar, e_0, ...) mod q (eg_hash_elems.hpp; q >= 2^255)
//   selection: elements (qbar, alpha, beta, a0, b0, a1, b1), expect (c0 + c1) mod q
//   contest  : elements (qbar, A, B, a, b),                   expect c
// (the elements after qbar in the ctx's pre-image order, eg_ctx_set_proof_format; up to 8 sources;
// a source of stride 0 is one element shared by every proof, e.g. the election key K)
// ---------------------------------------------------------------------------------
struct HashSrc {
  const uint8_t* ptr;  // base pointer
  uint32_t bytes;      // element width (32 or 512)
  uint32_t stride;     // bytes between consecutive proofs' elements
};

__global__ void __launch_bounds__(kBlock) k_hash_check(const uint8_t* __restrict__ q_be,
                                                       const uint8_t* __restrict__ qbar_be, uint32_t n,
                                                       uint32_t nsrc, HashSrc s0, HashSrc s1, HashSrc s2,
                                                       HashSrc s3, HashSrc s4, HashSrc s5, HashSrc s6, HashSrc s7,
                                                       const uint8_t* __restrict__ proofs,
                                                       uint32_t proof_words, uint32_t cidx0, uint32_t cidx1,
                                                       const uint8_t* __restrict__ pre_ok,
                                                       const uint8_t* __restrict__ pre_ok2, uint32_t pre2_div,
                                                       uint8_t* __restrict__ ok, uint8_t* __restrict__ out_h,
                                                       uint32_t hash_minimal) {
  __shared__ uint32_t s_buf[kBlock * kHashBufStride];
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  HashElems H(s_buf, hash_minimal);
  H.q(qbar_be);
  const HashSrc src[8] = {s0, s1, s2, s3, s4, s5, s6, s7};
  for (uint32_t k = 0; k < nsrc; ++k) H.elem(src[k].ptr + (size_t)i * src[k].stride, src[k].bytes);
  const U256 q = ld256(q_be);
  const U256 h = H.mod_q_top(q);
  if (out_h) st256(out_h + (size_t)i * 32, h);
  if (!ok) return;
  U256 c = ld256(proofs + ((size_t)i * proof_words + cidx0) * 32);
  if (cidx1 != kNone) c = addmod256(c, ld256(proofs + ((size_t)i * proof_words + cidx1) * 32), q);
  bool good = eq256(c, h);
  if (pre_ok) good &= pre_ok[i] != 0;
  if (pre_ok2) {
    // pre_ok2 indexed per element pair: both pad/data of selection i must be < p
    good &= pre_ok2[(size_t)i * pre2_div] != 0 && pre_ok2[(size_t)i * pre2_div + 1] != 0;
  }
  ok[i] = good ? 1 : 0;
}

}  // namespace eg
