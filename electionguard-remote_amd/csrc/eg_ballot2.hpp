// eg_ballot2.hpp — the kernels that map a placeholder-free ballot (include/eg_hip_ballot2.h;
// DESIGN.md §15) onto the range proof's contiguous items.  A ballot's rows are ragged (every
// contest has its own selection count and limits); the range chunk functions take one limit and
// contiguous items.  These kernels move rows between the two through per-manifest device tables,
// sum each contest's nonces and votes, and fold the verdicts.  The group arithmetic is k_pow,
// k_prod_tab, k_prod, k_import and k_export, unchanged.
//
// Conventions of DESIGN §11: one thread per item (the row movers: per 16-byte quad of an item's
// row, as k_range_order does per column), 256-thread workgroups, 64-bit indices, no barrier.
//
// A LIMIT CLASS holds a ballot's `per` items of one limit (its selections, or its contests); item
// j of ballot b is the class's packed item b * per + j, and tab[j] says where its row sits in the
// ballot's ragged array, in units the caller scales (mul) and shifts (shift).
#pragma once
#include "eg_range.hpp"
#include "eg_u256.hpp"

namespace eg {

// Rows of `quads` uint4 between a ballot-major ragged array and a class's packed items:
//   ragged quad = b * ballot_quads + tab[j] * mul + shift + k,  packed quad = (b * per + j) * quads + k
// scatter == 0 copies ragged -> packed (ciphertexts, proof rows, R, nonce rows in), else packed ->
// ragged (proofs out).  One thread per quad.
__global__ void __launch_bounds__(kBlock) k_b2_rows(uint4* __restrict__ ragged, uint4* __restrict__ packed,
                                                    const uint32_t* __restrict__ tab, uint32_t per, uint32_t quads,
                                                    uint64_t nitems, uint64_t ballot_quads, uint32_t mul,
                                                    uint32_t shift, uint32_t scatter) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nitems * quads) return;
  const uint64_t i = t / quads, b = i / per;
  const uint32_t k = (uint32_t)(t % quads), j = (uint32_t)(i % per);
  const uint64_t r = b * ballot_quads + (uint64_t)tab[j] * mul + shift + k;
  if (scatter) ragged[r] = packed[t];
  else packed[t] = ragged[r];
}

// k_b2_rows for one byte per item (votes and contest values in, verdict bytes out):
//   ragged byte = b * ballot_bytes + tab[j]
__global__ void __launch_bounds__(kBlock) k_b2_bytes(uint8_t* __restrict__ ragged, uint8_t* __restrict__ packed,
                                                     const uint32_t* __restrict__ tab, uint32_t per, uint64_t nitems,
                                                     uint64_t ballot_bytes, uint32_t scatter) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nitems) return;
  const uint64_t r = (i / per) * ballot_bytes + tab[i % per];
  if (scatter) ragged[r] = packed[i];
  else packed[i] = ragged[r];
}

// The ciphertext jobs' scalars of selection i = b * NS + s: its nonce R (the first of its nonce
// rows, row sn_row[s] of the ballot) and its vote byte as a 32-byte scalar -> sc[2 i], sc[2 i + 1].
// The vote is data only: no address depends on it.
__global__ void __launch_bounds__(kBlock) k_b2_ctscal(const uint8_t* __restrict__ votes,
                                                      const uint8_t* __restrict__ sel_nonces,
                                                      const uint32_t* __restrict__ sn_row, uint32_t NS, uint64_t SN,
                                                      uint64_t ns, uint8_t* __restrict__ sc) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ns) return;
  const uint64_t b = i / NS;
  const uint32_t s = (uint32_t)(i % NS);
  st256(sc + i * 64, ld256(sel_nonces + (b * SN + sn_row[s]) * 32));
  st256(sc + i * 64 + 32, u256_small(votes[i]));
}

// Per (ballot, contest) j = b * nc + k: rsum[j] = sum of its selections' R mod q, and value[j],
// the byte the contest's range prover takes: M = sum of its votes, or 255 (above every limit, so
// the prover writes an all-zero row) when M exceeds climit[k].  The selections' own over-limit
// rows are the range prover's (k_range_finish).  Written with masks: the votes are added and
// compared, never branched on or used in an address.
__global__ void __launch_bounds__(kBlock) k_b2_sums(const uint8_t* __restrict__ q_be,
                                                    const uint8_t* __restrict__ votes,
                                                    const uint8_t* __restrict__ sel_nonces,
                                                    const uint32_t* __restrict__ first,
                                                    const uint32_t* __restrict__ nsel,
                                                    const uint32_t* __restrict__ sn_off,
                                                    const uint32_t* __restrict__ olimit,
                                                    const uint32_t* __restrict__ climit, uint32_t nc, uint32_t NS,
                                                    uint64_t SN, uint64_t ncn, uint8_t* __restrict__ rsum,
                                                    uint8_t* __restrict__ value) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= ncn) return;
  const uint64_t b = j / nc;
  const uint32_t k = (uint32_t)(j % nc), n = nsel[k], rows = 2 * olimit[k] + 4;
  const U256 q = ld256(q_be);
  const uint8_t* v = votes + b * NS + first[k];
  const uint8_t* R = sel_nonces + (b * SN + sn_off[k]) * 32;
  U256 r = u256_zero();
  uint32_t M = 0;
  for (uint32_t s = 0; s < n; ++s) {
    r = addmod256(r, ld256(R + (uint64_t)s * rows * 32), q);
    M += v[s];
  }
  st256(rsum + j * 32, r);
  const uint32_t over = 0u - (uint32_t)(M > climit[k]);
  value[j] = (uint8_t)((M & ~over) | (255u & over));
}

// The range + residue flag of each selection of one limit class, from the flags the range
// verifier leaves per packed item (ltp[2 i], ltp[2 i + 1]: alpha, beta) into the ballot-major
// fl[b * NS + s].
__global__ void __launch_bounds__(kBlock) k_b2_flags(const uint8_t* __restrict__ ltp,
                                                     const uint32_t* __restrict__ tab, uint32_t per, uint64_t nitems,
                                                     uint32_t NS, uint8_t* __restrict__ fl) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nitems) return;
  fl[(i / per) * NS + tab[i % per]] = (ltp[i * 2] != 0 && ltp[i * 2 + 1] != 0) ? 1 : 0;
}

// ok_contest[j] of contest j = b * nc + k: the range verdict of its aggregate (okc[j]) AND the
// flags of its nsel[k] selections from first[k] on (k_contest_flags_seg's rule: the aggregate is a
// valid residue when every factor is, and a contest holding an invalid selection falls with it).
__global__ void __launch_bounds__(kBlock) k_b2_verdict(const uint8_t* __restrict__ okc, const uint8_t* __restrict__ fl,
                                                       const uint32_t* __restrict__ first,
                                                       const uint32_t* __restrict__ nsel, uint32_t nc, uint32_t NS,
                                                       uint64_t ncn, uint8_t* __restrict__ ok_contest) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= ncn) return;
  const uint32_t k = (uint32_t)(j % nc), n = nsel[k];
  const uint8_t* f = fl + (j / nc) * NS + first[k];
  uint8_t ok = okc[j] != 0 ? 1 : 0;
  for (uint32_t s = 0; s < n; ++s) ok &= f[s];
  ok_contest[j] = ok;
}

}  // namespace eg
