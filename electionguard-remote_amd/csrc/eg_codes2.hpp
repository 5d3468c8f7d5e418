// eg_codes2.hpp — ballot nonces from one per-ballot seed and the opening of challenged ballots for
// the placeholder-free ballot (include/eg_hip_codes2.h).  The hashes are
// eg_hash_elems.hpp's hash_elems, closed as eg_codes.hpp's are; the ragged row layouts are
// include/eg_hip_ballot2.h's.
//
//   sel_nonces[b, r]     = H(xi_b, 5, r)      0 <= r < SN
//   contest_nonces[b, r] = H(xi_b, 6, r)      0 <= r < CN
//   selection i of contest k: R = sel_nonces[b, sn_off[k] + i (2 olimit[k] + 4)]
//   open: ok = (alpha == g^R) and (beta == K^R g^m for one m in 0..olimit[k]); votes = m, else 0
//
// The hash kernels follow DESIGN §11: one thread per hash, 256-thread workgroups, 64-bit indices,
// no barrier, the SHA block buffer in LDS at kHashBufStride.  The match kernel is eg_kernels.hpp's
// shape: one selection per group of kT lanes, tail groups recompute a clamped selection.
#pragma once
#include "eg_hash_elems.hpp"
#include "eg_kernels.hpp"

namespace eg {

// One thread per output row: threads [0, nb SN) write sel_nonces (nb, SN, 32), the next nb CN
// write contest_nonces (nb, CN, 32) -- eg_encrypt_ballots_v2's input layout.
__global__ void __launch_bounds__(256) k_b2_derive_nonces(const uint8_t* __restrict__ q_be,
                                                          const uint8_t* __restrict__ ballot_nonces, uint64_t nb,
                                                          uint32_t SN, uint32_t CN, uint8_t* __restrict__ sel_nonces,
                                                          uint8_t* __restrict__ contest_nonces,
                                                          uint32_t hash_minimal) {
  __shared__ uint32_t s_buf[256 * kHashBufStride];
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint64_t nsn = nb * SN;
  if (i >= nsn + nb * CN) return;
  const bool is_sel = i < nsn;
  const uint64_t j = is_sel ? i : i - nsn;
  const uint64_t per = is_sel ? (uint64_t)SN : (uint64_t)CN;
  const uint64_t b = j / per;
  const uint32_t r = (uint32_t)(j - b * per);
  HashElems H(s_buf, hash_minimal);
  H.q(ballot_nonces + b * 32);
  H.small(is_sel ? 5u : 6u);
  H.small(r);
  st256((is_sel ? sel_nonces : contest_nonces) + j * 32, H.mod_q_top(ld256(q_be)));
}

// One thread per selection i = b * NS + s: only its R, row sn_row[s] of the ballot's selection
// nonces, into the packed R[i] (the exponent rows of the two fixed-base batches).
__global__ void __launch_bounds__(256) k_b2_derive_r(const uint8_t* __restrict__ q_be,
                                                     const uint8_t* __restrict__ ballot_nonces,
                                                     const uint32_t* __restrict__ sn_row, uint32_t NS, uint64_t n,
                                                     uint8_t* __restrict__ R, uint32_t hash_minimal) {
  __shared__ uint32_t s_buf[256 * kHashBufStride];
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint64_t b = i / NS;
  HashElems H(s_buf, hash_minimal);
  H.q(ballot_nonces + b * 32);
  H.small(5u);
  H.small(sn_row[i - b * NS]);
  st256(R + i * 32, H.mod_q_top(ld256(q_be)));
}

// This lane's limbs of the 512 big-endian bytes at be (any value below 2^4096), through the slot.
__device__ __forceinline__ void be_to_regs(uint32_t* slot, const uint8_t* __restrict__ be, uint32_t (&x)[kL]) {
  stage_be(slot, be);
  wave_sync();
#pragma unroll
  for (int j = 0; j < kL; ++j) x[j] = bits_limb(slot, kLimbBits * (glane() * kL + j));
  wave_sync();
}

// One selection i = b * NS + s per group: the vote m in 0..olim[s] with beta == K^R g^m, and
// alpha == g^R.  gR and KR are the canonical bytes of g^R and K^R (n x 512), g_mont is g in
// Montgomery form.  T starts as the PLAIN value K^R and each step is mont_mul(T, g R) = T g, so T
// stays plain: no import, no inverse, one multiply per candidate.  T is compared reduced to [0, p)
// with beta's limbs as given; a beta of 0 or of p or more equals no T, and alpha is compared with
// the canonical bytes of g^R, so an alpha of 0 or of p or more fails too.  The loop runs to the
// largest limit of the wave's selections whatever matches (a wave-uniform exit; at most
// EG_RANGE_MAX_LIMIT multiplies), and a match past the selection's own limit does not count.
template <bool F>
__global__ void __launch_bounds__(kBlock) k_b2_match(const MontConsts* __restrict__ C,
                                                     const uint32_t* __restrict__ g_mont,
                                                     const uint8_t* __restrict__ gR, const uint8_t* __restrict__ KR,
                                                     const uint8_t* __restrict__ cts,
                                                     const uint32_t* __restrict__ olim, uint32_t NS, uint32_t n,
                                                     uint8_t* __restrict__ votes, uint8_t* __restrict__ ok) {
  const uint32_t gid = group_id();
  const uint32_t e = gid < n ? gid : n - 1;
  uint32_t* slot = group_slot();
  Mont<F> M;
  M.load(C);
  const uint32_t L = olim[e % NS];
  const uint64_t gmask = (uint64_t)((1u << kT) - 1u) << (gslot() * kT);
  // alpha == g^R on bytes: each lane its 64
  bool aeq = true;
  {
    constexpr int kPer = 32 / kT;
    const uint4* a = reinterpret_cast<const uint4*>(cts + (size_t)e * 1024) + glane() * kPer;
    const uint4* w = reinterpret_cast<const uint4*>(gR + (size_t)e * 512) + glane() * kPer;
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      const uint4 u = a[k], v = w[k];
      aeq &= u.x == v.x && u.y == v.y && u.z == v.z && u.w == v.w;
    }
  }
  const bool alpha_ok = (__ballot(!aeq) & gmask) == 0;
  uint32_t beta[kL], x[kL];
  be_to_regs(slot, cts + (size_t)e * 1024 + 512, beta);
  be_to_regs(slot, KR + (size_t)e * 512, x);
  elem_to_lds(slot, g_mont);  // the multiplier of every step
  wave_sync();
  uint32_t vote = 0;
  bool found = false;
  for (uint32_t m = 0;; ++m) {
    uint32_t t[kL];
#pragma unroll
    for (int j = 0; j < kL; ++j) t[j] = x[j];
    regs_reduce_lazy(M, t);
    bool eq = true;
#pragma unroll
    for (int j = 0; j < kL; ++j) eq &= t[j] == beta[j];
    if ((__ballot(!eq) & gmask) == 0 && m <= L) {
      found = true;
      vote = m;
    }
    if (__ballot(m < L) == 0) break;
    M.mul(x, slot);
  }
  if (glane() == 0 && gid < n) {
    const bool good = found && alpha_ok;
    votes[gid] = good ? (uint8_t)vote : 0;
    ok[gid] = good ? 1 : 0;
  }
}

}  // namespace eg
