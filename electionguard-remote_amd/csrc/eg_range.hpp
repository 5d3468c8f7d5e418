// eg_range.hpp — the scalar, hash and ordering kernels of the 0..L range proof
// (include/eg_hip_range.h).  The exponentiations are k_pow jobs (eg_kernels.hpp);
// these kernels run one thread per item with 256-thread workgroups, 64-bit item indices and no
// barrier, like the scalar kernels of eg_proof_kernels.hpp; scalars are eg_u256.hpp's,
// the pre-image writer eg_hash_elems.hpp's.
//
// An item's proof is B = L + 1 branches (c_j, v_j), 2 B scalars of 32 bytes; its commitments are
// 2 B consecutive elements (a_0, b_0, ..., a_L, b_L).
#pragma once
#include "eg_hash_elems.hpp"
#include "eg_kernels.hpp"
#include "eg_u256.hpp"

namespace eg {

// Verifier scalars of item i from its proof row (a working copy: the hash reads the caller's).
//   e_j = c_j, or -c_j in place under EG_RESPONSE_PLUS (the comb exponents of alpha and beta);
//   gneg[i B + j] = -j e_j mod q (the g term of b_j; zero for branch 0);
//   ok[i] = every c_j, v_j < q.  A row that fails keeps its words and gets zero g terms.
__global__ void __launch_bounds__(kBlock) k_range_scalars(const uint8_t* __restrict__ q_be,
                                                          uint8_t* __restrict__ proofs, uint64_t n, uint32_t L,
                                                          uint8_t* __restrict__ gneg, uint8_t* __restrict__ ok,
                                                          uint32_t plus) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t B = L + 1;
  const U256 q = ld256(q_be);
  uint8_t* row = proofs + i * B * 64;
  bool good = true;
  for (uint32_t k = 0; k < 2 * B; ++k) good &= lt256(ld256(row + (size_t)k * 32), q);
  for (uint32_t j = 0; j < B; ++j) {
    U256 g = u256_zero();
    if (good) {
      U256 e = ld256(row + (size_t)j * 64);
      if (plus) {
        e = negmod(e, q);
        st256(row + (size_t)j * 64, e);
      }
      g = negmod(mulsmall_mod(e, j, q), q);
    }
    st256(gneg + (i * B + j) * 32, g);
  }
  ok[i] = good ? 1 : 0;
}

// Prover scalars of item i: nonces (u, c_0, v_0, ..., c_L, v_L), encryption nonce R, value m.
//   s[i B + j] = v_j + R e_j,  t[i B + j] = (m - j) e_j   (mod q),  e_j = c_j or -c_j (plus)
// for EVERY j, the real branch included (its pair is computed and then replaced, k_range_order),
// so the work does not depend on m; m enters through mulbyte_mod's masks only.
__global__ void __launch_bounds__(kBlock) k_range_prep(const uint8_t* __restrict__ q_be,
                                                       const uint8_t* __restrict__ values,
                                                       const uint8_t* __restrict__ nonces,
                                                       const uint8_t* __restrict__ Rs, uint64_t n, uint32_t L,
                                                       uint8_t* __restrict__ s, uint8_t* __restrict__ t,
                                                       uint32_t plus) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t B = L + 1;
  const U256 q = ld256(q_be);
  const U256 R = ld256(Rs + i * 32);
  const uint32_t m = values[i];
  const uint8_t* row = nonces + i * (2 * B + 1) * 32 + 32;
  for (uint32_t j = 0; j < B; ++j) {
    const U256 c = ld256(row + (size_t)j * 64);
    const U256 v = ld256(row + (size_t)j * 64 + 32);
    const U256 e = sel256(0u - (plus & 1u), negmod(c, q), c);
    st256(s + (i * B + j) * 32, addmod256(v, mulmod256(R, e, q), q));
    st256(t + (i * B + j) * 32, submod256(mulbyte_mod(e, m, q), mulbyte_mod(e, j, q), q));
  }
}

// The prover computes every branch as a simulated one into the item's 2 B commitment elements
// and the real pair (g^u, K^u) apart; this moves the real pair into branch m with masks: every
// branch is read and written whatever m is, so no address depends on the value.  A value above
// L matches no branch.  One thread per 4-word column of a pair.
__global__ void __launch_bounds__(kBlock) k_range_order(uint32_t* __restrict__ comm,
                                                        const uint32_t* __restrict__ real,
                                                        const uint8_t* __restrict__ values, uint64_t n,
                                                        uint32_t L) {
  constexpr uint32_t kQuads = 2 * kW / 4;  // a pair of elements, in uint4
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * kQuads) return;
  const uint64_t i = t / kQuads;
  const uint32_t k = (uint32_t)(t % kQuads), B = L + 1, m = values[i];
  const uint4 r = reinterpret_cast<const uint4*>(real + i * 2 * kW)[k];
  uint4* p = reinterpret_cast<uint4*>(comm + i * B * 2 * kW) + k;
  for (uint32_t j = 0; j < B; ++j, p += kQuads) {
    const uint32_t mk = 0u - (uint32_t)(j == m);
    const uint4 a = *p;
    *p = make_uint4((a.x & ~mk) | (r.x & mk), (a.y & ~mk) | (r.y & mk), (a.z & ~mk) | (r.z & mk),
                    (a.w & ~mk) | (r.w & mk));
  }
}

// Close the proofs: c_m = c - sum_{j != m} c_j, v_m = u - c_m R (plus: u + c_m R), the other
// branches as supplied; the supplied (c_m, v_m) is ignored.  Every branch is read and written and
// the real one picked by masks; an item whose value exceeds L gets an all-zero row.
__global__ void __launch_bounds__(kBlock) k_range_finish(const uint8_t* __restrict__ q_be,
                                                         const uint8_t* __restrict__ values,
                                                         const uint8_t* __restrict__ nonces,
                                                         const uint8_t* __restrict__ Rs,
                                                         const uint8_t* __restrict__ chal, uint64_t n, uint32_t L,
                                                         uint8_t* __restrict__ proofs, uint32_t plus) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t B = L + 1;
  const U256 q = ld256(q_be);
  const uint32_t m = values[i];
  const uint8_t* nrow = nonces + i * (2 * B + 1) * 32;
  const U256 zero = u256_zero();
  U256 sum = zero;
  for (uint32_t j = 0; j < B; ++j) {
    const U256 c = ld256(nrow + 32 + (size_t)j * 64);
    sum = addmod256(sum, sel256(0u - (uint32_t)(j == m), zero, c), q);
  }
  const U256 cm = submod256(ld256(chal + i * 32), sum, q);
  const U256 cR = mulmod256(cm, ld256(Rs + i * 32), q);
  const U256 u = ld256(nrow);
  const U256 vm = plus ? addmod256(u, cR, q) : submod256(u, cR, q);
  const uint32_t valid = 0u - (uint32_t)(m <= L);
  uint8_t* o = proofs + i * B * 64;
  for (uint32_t j = 0; j < B; ++j) {
    const uint32_t mk = 0u - (uint32_t)(j == m);
    const U256 c = sel256(mk, cm, ld256(nrow + 32 + (size_t)j * 64));
    const U256 v = sel256(mk, vm, ld256(nrow + 64 + (size_t)j * 64));
    st256(o + (size_t)j * 64, sel256(valid, c, zero));
    st256(o + (size_t)j * 64 + 32, sel256(valid, v, zero));
  }
}

// Fiat-Shamir hash of item i: Q-bar, then in the context's pre-image order the message (alpha,
// beta: 1024 bytes per item in cts), the 2 B commitments (consecutive 512-byte elements in comm)
// and, for EG_PREIMAGE_WITH_KEY, the shared key first.  k_hash_check's eight sources cannot hold
// the up to 35 elements, so the element's address is computed from its position.
//   ok != null (verify): ok[i] = (sum_j c_j mod q == H) & sc_ok[i] & ltp[2 i] & ltp[2 i + 1]
//                        (the scalar flag of k_range_scalars; the range and residue flags of
//                        alpha and beta, k_import / k_resid_check); proofs are the caller's rows
//   out_h != null (prove): out_h[i] = H
// The digest is closed as k_hash_check's: mod_q_top, the production q.
__global__ void __launch_bounds__(kBlock) k_range_hash(const uint8_t* __restrict__ q_be,
                                                       const uint8_t* __restrict__ qbar_be, uint64_t n, uint32_t L,
                                                       const uint8_t* __restrict__ cts,
                                                       const uint8_t* __restrict__ comm,
                                                       const uint8_t* __restrict__ key, uint32_t order,
                                                       const uint8_t* __restrict__ proofs,
                                                       const uint8_t* __restrict__ sc_ok,
                                                       const uint8_t* __restrict__ ltp, uint8_t* __restrict__ ok,
                                                       uint8_t* __restrict__ out_h, uint32_t hash_minimal) {
  __shared__ uint32_t s_buf[kBlock * kHashBufStride];
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t B = L + 1, ncomm = 2 * B;
  const uint8_t* msg = cts + i * 1024;
  const uint8_t* cm = comm + i * ncomm * 512;
  HashElems H(s_buf, hash_minimal);
  H.q(qbar_be);
  const uint32_t lead = order == 2u ? 1u : 0u;  // EG_PREIMAGE_WITH_KEY
  const uint32_t nel = lead + 2 + ncomm;
  for (uint32_t k = 0; k < nel; ++k) {
    const uint8_t* src;
    if (k < lead) {
      src = key;
    } else {
      const uint32_t e = k - lead;
      if (order == 1u) src = e < ncomm ? cm + (size_t)e * 512 : msg + (size_t)(e - ncomm) * 512;  // commitments first
      else src = e < 2 ? msg + (size_t)e * 512 : cm + (size_t)(e - 2) * 512;
    }
    H.p(src);
  }
  const U256 q = ld256(q_be);
  const U256 h = H.mod_q_top(q);
  if (out_h) st256(out_h + i * 32, h);
  if (!ok) return;
  U256 c = ld256(proofs + i * B * 64);
  for (uint32_t j = 1; j < B; ++j) c = addmod256(c, ld256(proofs + i * B * 64 + (size_t)j * 64), q);
  bool good = eq256(c, h);
  good &= sc_ok[i] != 0 && ltp[i * 2] != 0 && ltp[i * 2 + 1] != 0;
  ok[i] = good ? 1 : 0;
}

}  // namespace eg
