// eg_preencrypt.hpp — pre-encrypted ballots (include/eg_hip_preencrypt.h): component nonces and
// hashes, the sorted lists and short codes, recording and the pre-encryption check.
//
// Contest k owns spc_k slots from off_k, so it has spc_k selection vectors of spc_k components;
// per ballot V = sum spc_k^2 components (voff_k the contest's first) and nsel vectors:
//   w(k,i,j)   = voff_k + i spc_k + j
//   rho[b,w]   = H(xi_b, 4, w)
//   e[b,w]     = H(P alpha, P beta)              alpha = g^rho, beta = K^rho g^[i = j]
//   psi[b,k,i] = H(dcon[k], e[b,w(k,i,0)] .. e[b,w(k,i,spc_k-1)])      (k_seg_hash)
//   Omega(psi) = the last code_bytes bytes of psi
// A recorded ballot keeps, per contest, limit_k chosen vectors: S = sum limit_k spc_k component
// ciphertexts per ballot (soff_k the contest's first) and T = sum limit_k vectors (toff_k).
//
// Conventions are eg_codes.hpp's: one thread per item, 256 threads per block, 64-bit indices, no
// barrier, hashes through eg_hash_elems.hpp's HashElems (closed by mod_q_top), scalars through
// eg_u256.hpp, byte rows through eg_kernels.hpp's row helpers.  Every loop reads its operands from
// memory: there is no local array, so nothing goes to scratch.
#pragma once
#include "eg_hash_elems.hpp"
#include "eg_kernels.hpp"
#include "eg_u256.hpp"

namespace eg {

// mask of a short code: the low code_bytes bytes of psi's last word
__device__ __forceinline__ uint32_t code_mask(uint32_t code_bytes) {
  return code_bytes >= 4 ? 0xFFFFFFFFu : ((1u << (8 * code_bytes)) - 1u);
}

// rho = H(xi, 4, w), on the block's buffer s_buf
__device__ __forceinline__ U256 pre_rho(uint32_t* s_buf, const uint8_t* __restrict__ xi, uint32_t w,
                                        uint32_t hash_minimal, const uint8_t* __restrict__ q_be) {
  HashElems H(s_buf, hash_minimal);
  H.q(xi);
  H.small(4u);
  H.small(w);
  return H.mod_q_top(ld256(q_be));
}

// One thread per (b, w): rho[b,w] and the diagonal scalar [i = j] (diag: V flags, one per
// component of a ballot), the two exponents of the component's fixed-base job.
__global__ void __launch_bounds__(256) k_pre_nonces(const uint8_t* __restrict__ q_be,
                                                    const uint8_t* __restrict__ ballot_nonces, uint64_t nb, uint32_t V,
                                                    const uint32_t* __restrict__ diag, uint8_t* __restrict__ rho,
                                                    uint8_t* __restrict__ unit, uint32_t hash_minimal) {
  __shared__ uint32_t s_buf[256 * kHashBufStride];
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nb * V) return;
  const uint64_t b = i / V;
  const uint32_t w = (uint32_t)(i - b * V);
  st256(rho + i * 32, pre_rho(s_buf, ballot_nonces + b * 32, w, hash_minimal, q_be));
  st256(unit + i * 32, u256_small(diag[w]));
}

// One thread per ciphertext: e = H(P alpha, P beta); cts (n, 2, 512).
__global__ void __launch_bounds__(256) k_pre_comp_hash(const uint8_t* __restrict__ q_be,
                                                       const uint8_t* __restrict__ cts, uint64_t n,
                                                       uint8_t* __restrict__ out, uint32_t hash_minimal) {
  __shared__ uint32_t s_buf[256 * kHashBufStride];
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  HashElems H(s_buf, hash_minimal);
  H.p(cts + i * 1024);
  H.p(cts + i * 1024 + 512);
  st256(out + i * 32, H.mod_q_top(ld256(q_be)));
}

// One thread per row: dst[i] = src[idx[i]], 32-byte rows (dcon expanded to one row per vector,
// the leading element k_seg_hash reads by position).
__global__ void __launch_bounds__(256) k_pre_expand(const uint8_t* __restrict__ src, const uint32_t* __restrict__ idx,
                                                    uint64_t n, uint8_t* __restrict__ dst) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint4* s = reinterpret_cast<const uint4*>(src + (uint64_t)idx[i] * 32);
  uint4* d = reinterpret_cast<uint4*>(dst + i * 32);
  d[0] = s[0];
  d[1] = s[1];
}

// One thread per (b, k): ranks the contest's spc_k vector hashes by counting (ascending as
// 256-bit integers, ties to the lower i) and writes sorted / perm at the rank, the short code at
// the vector's own position.  Two vectors of one contest with the same short code clear the
// ballot's flag: a byte store of 0 into a flag the host set to 1 (every writer stores 0).
__global__ void __launch_bounds__(256) k_pre_sort(const uint8_t* __restrict__ psi, uint64_t nb, uint32_t nc,
                                                  uint32_t nsel, const uint32_t* __restrict__ off,
                                                  const uint32_t* __restrict__ spc, uint32_t code_bytes,
                                                  uint8_t* __restrict__ sorted, uint32_t* __restrict__ perm,
                                                  uint32_t* __restrict__ codes, uint8_t* __restrict__ unique) {
  const uint64_t it = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (it >= nb * nc) return;
  const uint64_t b = it / nc;
  const uint32_t k = (uint32_t)(it - b * nc);
  const uint32_t m = spc[k];
  const uint64_t row = b * nsel + off[k];
  const uint32_t cm = code_mask(code_bytes);
  bool coll = false;
  for (uint32_t i = 0; i < m; ++i) {
    const U256 a = ld256(psi + (row + i) * 32);
    uint32_t rank = 0;
    for (uint32_t x = 0; x < m; ++x) {
      const U256 c = ld256(psi + (row + x) * 32);
      rank += (lt256(c, a) || (x < i && eq256(c, a))) ? 1u : 0u;
      coll |= x < i && ((c.w[0] ^ a.w[0]) & cm) == 0;
    }
    st256(sorted + (row + rank) * 32, a);
    perm[row + rank] = i;
    codes[row + i] = a.w[0] & cm;
  }
  if (coll) unique[b] = 0;
}

// One thread per chosen component (b, u), u < S: chosen slot t of contest k is the (t+1)-th set
// vote of the contest, found by a masked scan of all spc_k votes (slot 0's vector when the votes
// hold fewer: the contest is then flagged by k_pre_place).  Writes rho[b, w(k,i,j)] and [i = j].
__global__ void __launch_bounds__(256) k_pre_rec_nonces(const uint8_t* __restrict__ q_be,
                                                        const uint8_t* __restrict__ ballot_nonces,
                                                        const uint8_t* __restrict__ votes, uint64_t nb, uint32_t S,
                                                        uint32_t nsel, const uint32_t* __restrict__ uk,
                                                        const uint32_t* __restrict__ ul,
                                                        const uint32_t* __restrict__ off,
                                                        const uint32_t* __restrict__ spc,
                                                        const uint32_t* __restrict__ voff, uint8_t* __restrict__ rho,
                                                        uint8_t* __restrict__ unit, uint32_t hash_minimal) {
  __shared__ uint32_t s_buf[256 * kHashBufStride];
  const uint64_t it = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (it >= nb * S) return;
  const uint64_t b = it / S;
  const uint32_t u = (uint32_t)(it - b * S);
  const uint32_t k = uk[u], m = spc[k];
  const uint32_t t = ul[u] / m, j = ul[u] - t * m;
  const uint8_t* v = votes + b * nsel + off[k];
  uint32_t seen = 0, i = 0;
  for (uint32_t x = 0; x < m; ++x) {
    const uint32_t set = v[x] != 0 ? 1u : 0u;
    const uint32_t hit = 0u - (set & (seen == t ? 1u : 0u));
    i = (x & hit) | (i & ~hit);
    seen += set;
  }
  const uint32_t w = voff[k] + i * m + j;
  st256(rho + it * 32, pre_rho(s_buf, ballot_nonces + b * 32, w, hash_minimal, q_be));
  st256(unit + it * 32, u256_small(i == j ? 1u : 0u));
}

// One thread per (b, slot s): the recorded ballot's encryption nonce of slot off_k + j,
// R' = sum over the contest's limit_k chosen vectors of rho[b, w(k,i,j)] mod q, from the chosen
// components' nonces (rho, (nb, S, 32), vote order), into the R position of sel_nonces
// (nb, nsel, 4, 32).  No address depends on a vote.
__global__ void __launch_bounds__(256) k_pre_rec_sums(const uint8_t* __restrict__ q_be, const uint8_t* __restrict__ rho,
                                                      uint64_t nb, uint32_t nsel, uint32_t S,
                                                      const uint32_t* __restrict__ kof,
                                                      const uint32_t* __restrict__ off,
                                                      const uint32_t* __restrict__ spc,
                                                      const uint32_t* __restrict__ soff,
                                                      const uint32_t* __restrict__ limit,
                                                      uint8_t* __restrict__ sel_nonces) {
  const uint64_t it = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (it >= nb * nsel) return;
  const uint64_t b = it / nsel;
  const uint32_t s = (uint32_t)(it - b * nsel);
  const uint32_t k = kof[s], m = spc[k], j = s - off[k];
  const U256 q = ld256(q_be);
  U256 r = u256_zero();
  for (uint32_t t = 0; t < limit[k]; ++t) r = addmod256(r, ld256(rho + (b * S + soff[k] + t * m + j) * 32), q);
  st256(sel_nonces + it * 128, r);
}

// One thread per (b, k): looks each chosen vector's psi up in the contest's sorted list, orders
// the chosen vectors by rank (counting, over the ranks kept in rk) and writes sel_rank / sel_codes
// in that order and place[b, toff_k + t], the position vector t moves to.  ok = 0: a vote above 1,
// votes that do not sum to limit_k, or a psi that is not in the list (its rank reads spc_k).
__global__ void __launch_bounds__(256) k_pre_place(const uint8_t* __restrict__ votes, const uint8_t* __restrict__ psic,
                                                   const uint8_t* __restrict__ sorted, uint64_t nb, uint32_t nc,
                                                   uint32_t nsel, uint32_t T, const uint32_t* __restrict__ off,
                                                   const uint32_t* __restrict__ spc,
                                                   const uint32_t* __restrict__ toff,
                                                   const uint32_t* __restrict__ limit, uint32_t code_bytes,
                                                   uint32_t* rk, uint32_t* __restrict__ sel_rank,
                                                   uint32_t* __restrict__ sel_codes, uint32_t* __restrict__ place,
                                                   uint8_t* __restrict__ ok) {
  const uint64_t it = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (it >= nb * nc) return;
  const uint64_t b = it / nc;
  const uint32_t k = (uint32_t)(it - b * nc);
  const uint32_t m = spc[k], L = limit[k];
  const uint64_t row = b * nsel + off[k], trow = b * T + toff[k];
  const uint32_t cm = code_mask(code_bytes);
  bool good = true;
  uint32_t cnt = 0;
  for (uint32_t x = 0; x < m; ++x) {
    const uint32_t v = votes[row + x];
    good &= v <= 1;
    cnt += v;
  }
  good &= cnt == L;
  for (uint32_t t = 0; t < L; ++t) {
    const U256 a = ld256(psic + (trow + t) * 32);
    uint32_t r = m;
    for (uint32_t x = 0; x < m; ++x)
      if (r == m && eq256(ld256(sorted + (row + x) * 32), a)) r = x;
    rk[trow + t] = r;
    good &= r < m;
  }
  for (uint32_t t = 0; t < L; ++t) {
    const uint32_t r = rk[trow + t];
    uint32_t pos = 0;
    for (uint32_t x = 0; x < L; ++x) {
      const uint32_t rx = rk[trow + x];
      pos += (rx < r || (rx == r && x < t)) ? 1u : 0u;
    }
    sel_rank[trow + pos] = r;
    sel_codes[trow + pos] = ld256(psic + (trow + t) * 32).w[0] & cm;
    place[trow + t] = pos;
  }
  ok[it] = good ? 1 : 0;
}

// One thread per 16 bytes of a chosen component's 1 KiB row: src (nb, S, 2, 512) in vote order
// -> out in rank order (vector t of its contest moves to position place[b, toff_k + t]).
__global__ void __launch_bounds__(256) k_pre_copy_rows(const uint8_t* __restrict__ src,
                                                       const uint32_t* __restrict__ place, uint64_t nb, uint32_t S,
                                                       uint32_t T, const uint32_t* __restrict__ uk,
                                                       const uint32_t* __restrict__ ul,
                                                       const uint32_t* __restrict__ spc,
                                                       const uint32_t* __restrict__ soff,
                                                       const uint32_t* __restrict__ toff, uint8_t* __restrict__ out) {
  const uint64_t it = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (it >= nb * S * 64) return;
  const uint64_t c = it / 64, piece = it - c * 64;
  const uint64_t b = c / S;
  const uint32_t u = (uint32_t)(c - b * S);
  const uint32_t k = uk[u], m = spc[k];
  const uint32_t t = ul[u] / m, j = ul[u] - t * m;
  const uint32_t pos = place[b * T + toff[k] + t];
  const uint64_t d = b * S + soff[k] + pos * m + j;
  reinterpret_cast<uint4*>(out + d * 1024)[piece] = reinterpret_cast<const uint4*>(src + c * 1024)[piece];
}

// One thread per 512-byte element: flags[e] &= (element != 0), on top of k_import's element < p.
__global__ void __launch_bounds__(256) k_pre_nonzero(const uint8_t* __restrict__ be, uint64_t n,
                                                     uint8_t* __restrict__ flags) {
  const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  if (row512_or(be + e * 512, ~0u, 0u) == 0) flags[e] = 0;
}

// One thread per (b, k), the verdict of the pre-encryption check:
//   every element of the chosen vectors in [1, p)            (flags, (nb, S, 2))
//   ranks < spc_k and strictly ascending, the sorted list strictly ascending
//   psi of chosen vector t == sorted[rank_t], its recorded code == Omega(psi)
//   the chosen vectors' slot-wise products (prod, (nb, nsel, 2, 512)) == the ballot's ciphertexts
__global__ void __launch_bounds__(256) k_pre_verify(const uint8_t* __restrict__ flags,
                                                    const uint32_t* __restrict__ sel_rank,
                                                    const uint32_t* __restrict__ sel_codes,
                                                    const uint8_t* __restrict__ psic,
                                                    const uint8_t* __restrict__ sorted,
                                                    const uint8_t* __restrict__ prod, const uint8_t* __restrict__ cts,
                                                    uint64_t nb, uint32_t nc, uint32_t nsel, uint32_t S, uint32_t T,
                                                    const uint32_t* __restrict__ off,
                                                    const uint32_t* __restrict__ spc,
                                                    const uint32_t* __restrict__ soff,
                                                    const uint32_t* __restrict__ toff,
                                                    const uint32_t* __restrict__ limit, uint32_t code_bytes,
                                                    uint8_t* __restrict__ ok) {
  const uint64_t it = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (it >= nb * nc) return;
  const uint64_t b = it / nc;
  const uint32_t k = (uint32_t)(it - b * nc);
  const uint32_t m = spc[k], L = limit[k];
  const uint64_t row = b * nsel + off[k], trow = b * T + toff[k], srow = b * S + soff[k];
  const uint32_t cm = code_mask(code_bytes);
  bool good = true;
  for (uint32_t x = 0; x < L * m * 2; ++x) good &= flags[srow * 2 + x] != 0;
  for (uint32_t x = 1; x < m; ++x) good &= lt256(ld256(sorted + (row + x - 1) * 32), ld256(sorted + (row + x) * 32));
  for (uint32_t t = 0; t < L; ++t) {
    const uint32_t r = sel_rank[trow + t];
    good &= r < m;
    if (t) good &= sel_rank[trow + t - 1] < r;
    const U256 a = ld256(psic + (trow + t) * 32);
    // a rank outside the list compares against its first entry; the verdict is already 0
    good &= eq256(a, ld256(sorted + (row + (r < m ? r : 0u)) * 32));
    good &= sel_codes[trow + t] == (a.w[0] & cm);
  }
  good &= quads_diff(reinterpret_cast<const uint4*>(prod + row * 1024),
                     reinterpret_cast<const uint4*>(cts + row * 1024), (uint64_t)m * 64) == 0;
  ok[it] = good ? 1 : 0;
}

// One thread per ballot: ok[b] = (conf[b] == the confirmation hash recomputed from the sorted lists).
__global__ void __launch_bounds__(256) k_pre_conf_check(const uint8_t* __restrict__ calc,
                                                        const uint8_t* __restrict__ conf, uint64_t nb,
                                                        uint8_t* __restrict__ ok) {
  const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= nb) return;
  ok[b] = eq256(ld256(calc + b * 32), ld256(conf + b * 32)) ? 1 : 0;
}

}  // namespace eg
