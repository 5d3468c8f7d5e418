// eg_shuffle.hpp — the hash, scalar, scan and gather kernels of the verifiable shuffle: generators,
// mix, prover and verifier (include/eg_hip_shuffle.h).  DESIGN §11's conventions: one
// thread per item (one 8-lane group per element in the Montgomery kernel), 256 threads per block,
// 64-bit indices; only the scan and the dot use a block barrier.  The powers and the products are
// k_pow, k_prod, k_mul and k_pp_* (eg_kernels.hpp, eg_prodpow.hpp); the mix's nonces are reduced
// mod q by k_reduce_q and the generator seed is hashed by k_hash_check (eg_proof_kernels.hpp).
// Scalars are eg_u256.hpp's, the pre-image writer eg_hash_elems.hpp's.
#pragma once

#include "eg_hash_elems.hpp"
#include "eg_kernels.hpp"
#include "eg_u256.hpp"

namespace eg {

// X[k] = D[k,0] || ... || D[k,15], D[k,t] = SHA-256("|gseed|43|k|t|") raw: item i = 16 k + t
// writes its 32 bytes at X + 32 i (gseed: 32 bytes in HBM, 16-byte aligned)
__global__ void __launch_bounds__(kBlock) k_sh_expand(const uint8_t* __restrict__ gseed, uint32_t tag, uint64_t items,
                                                      uint32_t hash_minimal, uint8_t* __restrict__ X) {
  __shared__ uint32_t s_buf[kBlock * kHashBufStride];
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= items) return;
  HashElems H(s_buf, hash_minimal);
  H.q(gseed);
  H.small(tag);
  H.small((uint32_t)(i >> 4));
  H.small((uint32_t)(i & 15u));
  uint32_t dig[8];
  H.digest(dig);
  uint32_t* out = reinterpret_cast<uint32_t*>(X + i * 32);
#pragma unroll
  for (int k = 0; k < 8; ++k) out[k] = __builtin_bswap32(dig[k]);
}

// flag |= 1 if a canonical 512-byte row is 0 or 1 (a generator that generates nothing)
__global__ void __launch_bounds__(kBlock) k_sh_trivial(const uint8_t* __restrict__ rows, uint64_t n,
                                                       uint32_t* __restrict__ flag) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (row512_or(rows + i * 512, ~0x01000000u, 0u) == 0) atomicOr(flag, 1u);  // the last byte may be 0 or 1
}

// out[i] = in[min(psi[i / per], rows - 1) * per + i % per] * x[i]  (Montgomery form; per elements
// per row, items = rows * per; 8-lane groups like k_mul).  The clamp keeps a psi that is no
// permutation inside the array.  out may be x: a group reads x[i] before it writes out[i], and no
// other group touches either.
template <bool F>
__global__ void __launch_bounds__(kBlock) k_sh_gather_mul(const MontConsts* __restrict__ C,
                                                          const uint32_t* __restrict__ in,
                                                          const uint32_t* __restrict__ psi, uint32_t rows, uint32_t per,
                                                          const uint32_t* x, uint64_t items, uint32_t* out) {
  const uint64_t gid = (uint64_t)blockIdx.x * kGroupsPerBlock + threadIdx.x / kT;
  const uint64_t e = gid < items ? gid : items - 1;
  const uint32_t row = (uint32_t)(e / per), col = (uint32_t)(e % per);
  const uint32_t src = min(psi[row], rows - 1u);
  uint32_t* slot = group_slot();
  Mont<F> M;
  M.load(C);
  uint32_t v[kL];
  load_elem(v, in + ((size_t)src * per + col) * kW);
  mmul_g(M, v, slot, x + (size_t)e * kW);
  if (gid < items) store_elem(out + (size_t)gid * kW, v);
}

// ---------------------------------------------------------------------------------
// the proof's hashes: hash_elems in the context's format, closed by mod_q_any (a test group's q
// may be far below 2^256)
// ---------------------------------------------------------------------------------
// leaf[i] = H(Q 0x40, P x_0, ..., P x_{m-1}) of row i's m elements (512-byte rows, 16-byte aligned)
__global__ void __launch_bounds__(kBlock) k_sh_leaf(const uint8_t* __restrict__ q_be, const uint8_t* __restrict__ rows,
                                                    uint64_t m, uint64_t n, uint32_t hash_minimal,
                                                    uint8_t* __restrict__ out) {
  __shared__ uint32_t s_buf[kBlock * kHashBufStride];
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  HashElems H(s_buf, hash_minimal);
  H.small(0x40u);
  for (uint64_t k = 0; k < m; ++k) H.p(rows + (i * m + k) * 512);
  st256(out + i * 32, H.mod_q_any(ld256(q_be)));
}

// one level of T: out[c] = H(Q 0x41, Q len, Q v_0, ...) of chunk c's len <= 256 values of in (n in all)
__global__ void __launch_bounds__(kBlock) k_sh_tree(const uint8_t* __restrict__ q_be, const uint8_t* __restrict__ in,
                                                    uint64_t n, uint32_t hash_minimal, uint8_t* __restrict__ out) {
  __shared__ uint32_t s_buf[kBlock * kHashBufStride];
  const uint64_t ch = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (ch * 256 >= n) return;
  const uint32_t len = (uint32_t)(n - ch * 256 < 256 ? n - ch * 256 : 256);
  HashElems H(s_buf, hash_minimal);
  H.small(0x41u);
  H.small(len);
  for (uint32_t k = 0; k < len; ++k) H.q(in + (ch * 256 + k) * 32);
  st256(out + ch * 32, H.mod_q_any(ld256(q_be)));
}

// H(Q y, Q 0x44, Q j), on the block's buffer s_buf
__device__ __forceinline__ U256 sh_challenge(uint32_t* s_buf, const uint8_t* __restrict__ y, uint32_t j,
                                             uint32_t hash_minimal, const U256& q) {
  HashElems H(s_buf, hash_minimal);
  H.q(y);
  H.small(0x44u);
  H.small(j);
  return H.mod_q_any(q);
}

// u[j] = H(Q y, Q 0x44, Q j); with psi also up[i] = u[psi(i)], hashed again instead of gathered
// (an entry >= n reads as n - 1)
__global__ void __launch_bounds__(kBlock) k_sh_challenges(const uint8_t* __restrict__ q_be, const uint8_t* __restrict__ y,
                                                          const uint32_t* __restrict__ psi, uint64_t n,
                                                          uint32_t hash_minimal, uint8_t* __restrict__ u,
                                                          uint8_t* __restrict__ up) {
  __shared__ uint32_t s_buf[kBlock * kHashBufStride];
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const U256 q = ld256(q_be);
  st256(u + i * 32, sh_challenge(s_buf, y, (uint32_t)i, hash_minimal, q));
  if (psi != nullptr) st256(up + i * 32, sh_challenge(s_buf, y, min(psi[i], (uint32_t)(n - 1)), hash_minimal, q));
}

// inv[psi(i)] = i  (inv zeroed before; an entry >= n counts as n - 1)
__global__ void __launch_bounds__(kBlock) k_sh_invert(const uint32_t* __restrict__ psi, uint64_t n,
                                                      uint32_t* __restrict__ inv) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  inv[min(psi[i], (uint32_t)(n - 1))] = (uint32_t)i;
}

// ---------------------------------------------------------------------------------
// the proof's scalars
// ---------------------------------------------------------------------------------
// One level of the scan of the affine maps x -> A x + B mod q (composition is associative): every
// block replaces its 256 maps by their inclusive compositions (Hillis-Steele in LDS, 8 steps) and
// writes the block's total to tot[block].  In place: A, B hold the maps in and the prefixes out.
__global__ void __launch_bounds__(kBlock) k_sh_scan(const uint8_t* __restrict__ q_be, uint8_t* A, uint8_t* B,
                                                    uint64_t n, uint8_t* __restrict__ totA,
                                                    uint8_t* __restrict__ totB) {
  __shared__ U256 sa[kBlock], sb[kBlock];
  const uint32_t t = threadIdx.x;
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + t;
  const U256 q = ld256(q_be);
  U256 a = u256_small(1), b = u256_zero();
  if (i < n) a = ld256(A + i * 32), b = ld256(B + i * 32);
  for (uint32_t d = 1; d < kBlock; d <<= 1) {
    sa[t] = a;
    sb[t] = b;
    __syncthreads();
    if (t >= d) {  // mine after the earlier run: (a, b) o (ea, eb) = (a ea, a eb + b)
      const U256 ea = sa[t - d], eb = sb[t - d];
      b = addmod256(mulmod256(a, eb, q), b, q);
      a = mulmod256(a, ea, q);
    }
    __syncthreads();
  }
  if (i < n) st256(A + i * 32, a), st256(B + i * 32, b);
  if (t == kBlock - 1) st256(totA + (uint64_t)blockIdx.x * 32, a), st256(totB + (uint64_t)blockIdx.x * 32, b);
}

// ... and the way down: the maps of block k > 0 are composed after the prefix of blocks 0 .. k-1
__global__ void __launch_bounds__(kBlock) k_sh_scan_apply(const uint8_t* __restrict__ q_be, uint8_t* A, uint8_t* B,
                                                          uint64_t n, const uint8_t* __restrict__ preA,
                                                          const uint8_t* __restrict__ preB) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || blockIdx.x == 0) return;
  const U256 q = ld256(q_be);
  const U256 pa = ld256(preA + (uint64_t)(blockIdx.x - 1) * 32), pb = ld256(preB + (uint64_t)(blockIdx.x - 1) * 32);
  const U256 a = ld256(A + i * 32), b = ld256(B + i * 32);
  st256(B + i * 32, addmod256(mulmod256(a, pb, q), b, q));
  st256(A + i * 32, mulmod256(a, pa, q));
}

// Block-reduced SUM_i a_i b_i mod q (b == nullptr: SUM a_i), or with PROD the product PROD_i a_i:
// column blockIdx.x, block blockIdx.y of 256 items; a_i at a + 32 (col cs + i is), b_i at b + 32 i;
// the block's result goes to out + 32 (col gridDim.y + block).  Operands < q.
template <bool PROD>
__global__ void __launch_bounds__(kBlock) k_sh_dot(const uint8_t* __restrict__ q_be, const uint8_t* __restrict__ a,
                                                   uint64_t cs, uint64_t is, const uint8_t* __restrict__ b, uint64_t n,
                                                   uint8_t* __restrict__ out) {
  __shared__ U256 s[kBlock];
  const uint32_t t = threadIdx.x;
  const uint64_t col = blockIdx.x, i = (uint64_t)blockIdx.y * blockDim.x + t;
  const U256 q = ld256(q_be);
  U256 v = u256_small(PROD ? 1u : 0u);
  if (i < n) {
    v = ld256(a + (col * cs + i * is) * 32);
    if (b != nullptr) v = mulmod256(v, ld256(b + i * 32), q);
  }
  s[t] = v;
  __syncthreads();
  for (uint32_t d = kBlock / 2; d > 0; d >>= 1) {
    if (t < d) {
      const U256 x = s[t], y = s[t + d];
      s[t] = PROD ? mulmod256(x, y, q) : addmod256(x, y, q);
    }
    __syncthreads();
  }
  if (t == 0) st256(out + (col * gridDim.y + blockIdx.y) * 32, s[0]);
}

// out[i] = om[i] + c x[i] mod q  (operands < q)
__global__ void __launch_bounds__(kBlock) k_sh_respond(const uint8_t* __restrict__ q_be, const uint8_t* __restrict__ c_be,
                                                       const uint8_t* __restrict__ om, const uint8_t* __restrict__ x,
                                                       uint64_t n, uint8_t* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const U256 q = ld256(q_be);
  st256(out + i * 32, addmod256(ld256(om + i * 32), mulmod256(ld256(c_be), ld256(x + i * 32), q), q));
}

// out[i] = (q - in[i] mod q) mod q
__global__ void __launch_bounds__(kBlock) k_sh_neg(const uint8_t* __restrict__ q_be, const uint8_t* __restrict__ in,
                                                   uint64_t n, uint8_t* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const U256 q = ld256(q_be);
  st256(out + i * 32, negmod(mod256_any(ld256(in + i * 32), q), q));
}

// ---------------------------------------------------------------------------------
// the verifier's flags (bits of the failed mask: 1 range, 2 residue, 4 challenge)
// ---------------------------------------------------------------------------------
// flag |= 1 if a scalar is >= q
__global__ void __launch_bounds__(kBlock) k_sh_range(const uint8_t* __restrict__ q_be, const uint8_t* __restrict__ x,
                                                     uint64_t n, uint32_t* __restrict__ flag) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (!lt256(ld256(x + i * 32), ld256(q_be))) atomicOr(flag, 1u);
}

// flag |= 2 unless the element given was below p (lt_p) and its canonical q-th power is 1
__global__ void __launch_bounds__(kBlock) k_sh_resid(const uint8_t* __restrict__ pw, const uint8_t* __restrict__ lt_p,
                                                     uint64_t n, uint32_t* __restrict__ flag) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (row512_or(pw + i * 512, ~0u, 0x01000000u) != 0 || lt_p[i] == 0) atomicOr(flag, 2u);  // big-endian 1
}

// mask = flag | (4 unless c' == c); ok = mask == 0
__global__ void k_sh_verdict(const uint8_t* __restrict__ c_given, const uint8_t* __restrict__ c_made,
                             const uint32_t* __restrict__ flag, uint8_t* __restrict__ ok,
                             uint32_t* __restrict__ mask) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const uint32_t m = *flag | (eq256(ld256(c_given), ld256(c_made)) ? 0u : 4u);
  *mask = m;
  *ok = m == 0 ? 1 : 0;
}

}  // namespace eg
