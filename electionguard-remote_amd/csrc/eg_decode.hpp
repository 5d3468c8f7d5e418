// eg_decode.hpp — kernels of the device-side decode (include/eg_hip_decode.h; entry
// points: eg_capi_decode.inc): the two sweeps of the segmented batch inverse, and the table build
// and giant steps of the discrete logarithm to the base g.  The element layout, the Montgomery
// multiply and the wave-uniform rule are eg_kernels.hpp's: one element per group of kT lanes, tail
// groups run on the Montgomery one and store nothing, and every multiply, reduction and ballot is
// reached by all 64 lanes of a wave.  Everything here is PUBLIC data: values decide branches.
#pragma once
#include "eg_kernels.hpp"

namespace eg {

constexpr uint32_t kDcEmpty = 0xFFFFFFFFu;  // a free slot of the table (no baby step has this index)

__device__ __forceinline__ uint64_t group_mask() { return (uint64_t)((1u << kT) - 1u) << (gslot() * kT); }

// x = 0 mod p for a lazy value x in [0, 2p): its canonical residue has no limb set (group-uniform)
template <bool F>
__device__ __forceinline__ bool dc_is_zero(const Mont<F>& M, const uint32_t (&x)[kL]) {
  uint32_t t[kL];
#pragma unroll
  for (int j = 0; j < kL; ++j) t[j] = x[j];
  regs_reduce_lazy(M, t);
  bool nz = false;
#pragma unroll
  for (int j = 0; j < kL; ++j) nz |= t[j] != 0;
  return (__ballot(nz) & group_mask()) == 0;
}

// ---------------------------------------------------------------------------------
// Batch inverse, one level.  The n elements of X are cut into segments of S; group s owns segment
// s = elements s S .. min(n, (s + 1) S) - 1 and no other group touches them.
//   forward   P[i] = X[s S] * ... * X[i] (P[s S] = X[s S]), T[s] = the segment's total
//   backward  given Tinv[s] = T[s]^-1:  X[i] <- X[i]^-1, from the segment's end:
//             X[i]^-1 = acc * P[i - 1], acc <- acc * X[i]  (acc = Tinv[s] at the start, X[s S]^-1 at the end)
// zero != nullptr (level 0, the caller's elements): the forward sweep replaces an element that is
// 0 mod p by the Montgomery one and sets zero[i]; the backward sweep writes 0 there.
// The k loops run S times in every group (the trip count is the launch's); a step past a segment's
// end is skipped when the whole wave is past it, else it multiplies by the Montgomery one.
// ---------------------------------------------------------------------------------
template <bool F>
__global__ void __launch_bounds__(kBlock) k_dc_fwd(const MontConsts* __restrict__ C, uint32_t* X, uint32_t n,
                                                   uint32_t S, uint8_t* zero, uint32_t* __restrict__ P,
                                                   uint32_t* __restrict__ T) {
  const uint32_t nseg = (n + S - 1) / S;
  const uint32_t gid = group_id();
  const bool live = gid < nseg;
  const uint32_t s = live ? gid : nseg - 1;
  const uint32_t start = s * S;
  const uint32_t len = n - start < S ? n - start : S;
  uint32_t* slot = group_slot();
  Mont<F> M;
  M.load(C);
  uint32_t acc[kL], y[kL];
#pragma unroll 1
  for (uint32_t k = 0; k < S; ++k) {
    const bool in = live && k < len;
    if (__ballot(in) == 0) break;
    const size_t i = (size_t)start + (in ? k : 0u);
    load_elem(y, in ? X + i * kW : C->one);
    if (zero != nullptr) {
      const bool z = dc_is_zero(M, y);
      if (z) load_elem(y, C->one);
      if (in) {
        if (z) store_elem(X + i * kW, y);
        if (glane() == 0) zero[i] = z ? 1 : 0;
      }
    }
    if (k == 0) {
#pragma unroll
      for (int j = 0; j < kL; ++j) acc[j] = y[j];
    } else {
      regs_to_lds(slot, y);
      wave_sync();
      M.mul(acc, slot);
      wave_sync();
    }
    if (in) store_elem(P + i * kW, acc);
  }
  if (live) store_elem(T + (size_t)s * kW, acc);
}

template <bool F>
__global__ void __launch_bounds__(kBlock) k_dc_bwd(const MontConsts* __restrict__ C, uint32_t* X, uint32_t n,
                                                   uint32_t S, const uint8_t* __restrict__ zero,
                                                   const uint32_t* __restrict__ P,
                                                   const uint32_t* __restrict__ Tinv) {
  const uint32_t nseg = (n + S - 1) / S;
  const uint32_t gid = group_id();
  const bool live = gid < nseg;
  const uint32_t s = live ? gid : nseg - 1;
  const uint32_t start = s * S;
  const uint32_t len = n - start < S ? n - start : S;
  uint32_t* slot = group_slot();
  Mont<F> M;
  M.load(C);
  uint32_t acc[kL], inv[kL];
  load_elem(acc, live ? Tinv + (size_t)s * kW : C->one);
#pragma unroll 1
  for (uint32_t k = S - 1; k >= 1; --k) {
    const bool in = live && k < len;
    if (__ballot(in) == 0) continue;
    const size_t i = (size_t)start + (in ? k : 1u);
#pragma unroll
    for (int j = 0; j < kL; ++j) inv[j] = acc[j];
    mmul_g(M, inv, slot, in ? P + (i - 1) * kW : C->one);
    mmul_g(M, acc, slot, in ? X + i * kW : C->one);
    if (in) {
      if (zero != nullptr && zero[i]) {
#pragma unroll
        for (int j = 0; j < kL; ++j) inv[j] = 0;
      }
      store_elem(X + i * kW, inv);
    }
  }
  if (live) {
    if (zero != nullptr && zero[start]) {
#pragma unroll
      for (int j = 0; j < kL; ++j) acc[j] = 0;
    }
    store_elem(X + (size_t)start * kW, acc);
  }
}

// ---------------------------------------------------------------------------------
// The table of the discrete logarithm.
// ---------------------------------------------------------------------------------
// E[i] <- the canonical residue in [0, p) of the lazy Montgomery value E[i]: the form the baby steps
// are stored, fingerprinted and compared in.  x -> x R mod p is a bijection of [0, p), so two
// elements are equal iff these residues are.
template <bool F>
__global__ void __launch_bounds__(kBlock) k_dc_canon(const MontConsts* __restrict__ C, uint32_t* E, uint32_t n) {
  const uint32_t gid = group_id();
  const uint32_t e = gid < n ? gid : n - 1;
  Mont<F> M;
  M.load(C);
  uint32_t x[kL];
  load_elem(x, E + (size_t)e * kW);
  regs_reduce_lazy(M, x);
  if (gid < n) store_elem(E + (size_t)gid * kW, x);
}

// The fp_bits-bit fingerprint of a canonical residue from its three lowest limbs (its low 64 bits,
// mixed by splitmix64's finalizer, the top fp_bits kept), and the home slot the fingerprint fixes.
__host__ __device__ inline uint64_t dc_fingerprint(uint32_t l0, uint32_t l1, uint32_t l2, uint32_t fp_bits) {
  uint64_t h = (uint64_t)l0 | ((uint64_t)l1 << kLimbBits) | ((uint64_t)l2 << (2 * kLimbBits));
  h ^= h >> 30;
  h *= 0xBF58476D1CE4E5B9ull;
  h ^= h >> 27;
  h *= 0x94D049BB133111EBull;
  h ^= h >> 31;
  return h >> (64 - fp_bits);
}
__host__ __device__ inline uint32_t dc_home(uint64_t fp, uint32_t slot_mask) {
  return (uint32_t)((fp * 0x9E3779B97F4A7C15ull) >> 32) & slot_mask;
}

// One thread per baby step j < m: claim the first free slot from the fingerprint's home on by
// compare-and-swap on the index array, then write the fingerprint beside it (the lookups are later
// launches, so a claimed slot's fingerprint is never read before it is written).  slots >= 2 m: a
// free slot always exists.
__global__ void __launch_bounds__(256) k_dc_insert(const uint32_t* __restrict__ baby, uint32_t m, uint32_t fp_bits,
                                                   uint32_t slot_mask, uint32_t* ht_j, uint64_t* ht_fp) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= m) return;
  const uint32_t* e = baby + (size_t)j * kW;  // lane 0's block: limbs 0, 1, 2
  const uint64_t fp = dc_fingerprint(e[0], e[1], e[2], fp_bits);
  uint32_t pos = dc_home(fp, slot_mask);
  for (uint32_t probe = 0; probe <= slot_mask; ++probe) {
    if (atomicCAS(&ht_j[pos], kDcEmpty, j) == kDcEmpty) {
      ht_fp[pos] = fp;
      return;
    }
    pos = (pos + 1) & slot_mask;
  }
}

// Giant steps, one group per text: counts[i] = the t in [0, max_count] with g^t = Y[i], else -1.
// baby holds the canonical baby steps g^0 .. g^(m-1) and, at index m, the step g^(-m), which stays in
// the group's LDS slot as the multiplier of every step.  Per giant step i = 0 .. m: the working value
// (lazy, < 2p) is reduced to its canonical residue c, the fingerprint is taken from c, and the probe
// loop runs wave-uniformly while any group still probes: a slot whose fingerprint matches is a hit
// only if all kN limbs of c equal the stored baby step's, and only for t = i m + j <= max_count;
// anything else moves on to the next slot, and a text without a hit to the next giant step.  A group
// past n starts as done; the wave leaves when all its groups are.
template <bool F>
__global__ void __launch_bounds__(kBlock) k_dc_giant(const MontConsts* __restrict__ C,
                                                     const uint32_t* __restrict__ Y, uint32_t n,
                                                     const uint32_t* __restrict__ baby, uint32_t m,
                                                     uint64_t max_count, uint32_t fp_bits, uint32_t slot_mask,
                                                     const uint32_t* __restrict__ ht_j,
                                                     const uint64_t* __restrict__ ht_fp,
                                                     long long* __restrict__ counts) {
  const uint32_t gid = group_id();
  const bool live = gid < n;
  const uint32_t e = live ? gid : n - 1;
  uint32_t* slot = group_slot();
  Mont<F> M;
  M.load(C);
  uint32_t acc[kL], c[kL];
  load_elem(acc, Y + (size_t)e * kW);
  elem_to_lds(slot, baby + (size_t)m * kW);
  wave_sync();
  const uint64_t gmask = group_mask();
  bool done = !live;
  long long res = -1;
#pragma unroll 1
  for (uint32_t i = 0;; ++i) {
#pragma unroll
    for (int j = 0; j < kL; ++j) c[j] = acc[j];
    regs_reduce_lazy(M, c);
    const uint64_t fp = dc_fingerprint(bcast_g0(c[0]), bcast_g0(c[1]), bcast_g0(c[2]), fp_bits);
    uint32_t pos = dc_home(fp, slot_mask);
    bool probing = !done;
#pragma unroll 1
    for (uint32_t probe = 0; probe <= slot_mask && __ballot(probing) != 0; ++probe) {
      const uint32_t j = probing ? ht_j[pos] : kDcEmpty;
      const bool cand = j != kDcEmpty && ht_fp[pos] == fp;  // j < m: a baby step's index
      bool eq = true;
      if (cand) {
        const uint32_t* b = baby + (size_t)j * kW + glane() * kLP;
#pragma unroll
        for (int k = 0; k < kL; ++k) eq &= b[k] == c[k];
      }
      const bool same = cand && (__ballot(cand && !eq) & gmask) == 0;
      if (probing) {
        if (j == kDcEmpty) {
          probing = false;
        } else if (same) {
          // the only baby step equal to c: the probe ends here, in range or not
          const uint64_t t = (uint64_t)i * m + j;
          if (t <= max_count) {
            res = (long long)t;
            done = true;
          }
          probing = false;
        } else {
          pos = (pos + 1) & slot_mask;
        }
      }
    }
    if (i == m || __ballot(!done) == 0) break;
    M.mul(acc, slot);
  }
  if (live && glane() == 0) counts[gid] = res;
}

}  // namespace eg
