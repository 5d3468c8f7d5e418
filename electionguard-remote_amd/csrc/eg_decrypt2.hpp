// eg_decrypt2.hpp — the scalar and compare kernels of the threshold decryption with one combined
// proof per text (include/eg_hip_decrypt2.h).  DESIGN §11's conventions: one thread
// per item, 256 threads per block, 64-bit indices, no barrier.  The exponentiations, products and
// hashes of the family are k_pow, k_prod, k_pp_* and k_hash_check (eg_kernels.hpp, eg_prodpow.hpp,
// eg_proof_kernels.hpp); the reduction of the secret, the nonces and the challenges of
// eg_decrypt2_respond mod q is eg_proof_kernels.hpp's k_reduce_q, in place.
#pragma once

#include "eg_kernels.hpp"
#include "eg_u256.hpp"

namespace eg {

// ci[t, i] = c[t] * (w[i] mod q) mod q  (item j = t * k + i; c < q comes from the device hash)
__global__ void __launch_bounds__(kBlock) k_d2_ci(const uint8_t* __restrict__ q_be, const uint8_t* __restrict__ c_be,
                                                   const uint8_t* __restrict__ w_be, uint64_t items, uint32_t k,
                                                   uint8_t* __restrict__ ci) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= items) return;
  const U256 q = ld256(q_be);
  const U256 w = mod256_any(ld256(w_be + (j % k) * 32), q);
  st256(ci + j * 32, mulmod256(ld256(c_be + (j / k) * 32), w, q));
}

// ok[j] = a[j] < q and b[j] < q  (a, b: 32-byte scalars `stride` bytes apart)
__global__ void __launch_bounds__(kBlock) k_d2_range(const uint8_t* __restrict__ q_be, const uint8_t* __restrict__ a,
                                                      const uint8_t* __restrict__ b, uint32_t stride, uint64_t n,
                                                      uint8_t* __restrict__ ok) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const U256 q = ld256(q_be);
  const bool good = lt256(ld256(a + j * stride), q) & lt256(ld256(b + j * stride), q);
  ok[j] = good ? 1 : 0;
}

// ok[j] = pre[j] and the recomputed canonical pair got[j] (a, b: 1024 bytes) equals the given
// bytes: a given element >= p never matches.  Both rows are 16-byte aligned (the entry points check).
__global__ void __launch_bounds__(kBlock) k_d2_match(const uint8_t* __restrict__ got, const uint8_t* __restrict__ given,
                                                      const uint8_t* __restrict__ pre, uint64_t n,
                                                      uint8_t* __restrict__ ok) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint32_t diff = quads_diff(reinterpret_cast<const uint4*>(got + j * 1024),
                                   reinterpret_cast<const uint4*>(given + j * 1024), 64);
  ok[j] = (diff == 0 && pre[j] != 0) ? 1 : 0;
}

// v[t] = SUM_i (vi[t, i] mod q) mod q
__global__ void __launch_bounds__(kBlock) k_d2_vsum(const uint8_t* __restrict__ q_be, const uint8_t* __restrict__ vi,
                                                     uint64_t n, uint32_t k, uint8_t* __restrict__ v) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const U256 q = ld256(q_be);
  U256 r = u256_zero();
  for (uint32_t i = 0; i < k; ++i) r = addmod256(r, mod256_any(ld256(vi + (t * k + i) * 32), q), q);
  st256(v + t * 32, r);
}

}  // namespace eg
