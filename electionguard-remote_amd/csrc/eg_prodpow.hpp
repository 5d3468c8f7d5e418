// eg_prodpow.hpp — kernels of the multi-exponentiation out[r] = PROD_i B[r,i]^{e_i} with one
// exponent vector shared by every row (include/eg_hip_prodpow.h; entry points:
// eg_capi_prodpow.inc).  The element layout, the Montgomery multiply and the wave-uniform rule are
// eg_kernels.hpp's: one element per group of kT lanes, tail groups recompute a clamped item, and a
// group that has nothing left to multiply pads with the Montgomery one until its wave is done.
// The exponents are PUBLIC here: digits address memory and decide branches (the branches depend on
// the shared exponents only, so they are the same for every group of a wave).
#pragma once
#include "eg_kernels.hpp"

namespace eg {

// Terms per chunk of the two methods (the results of the chunks are multiplied), and the bucket
// method's segment length for a chunk of m terms: a power of two >= max(16, sqrt(m)), so neither
// the segment pass nor the pass over a bucket's segments chains more than 256 multiplies.
constexpr uint32_t kPpInterTerms = 1u << 12;
constexpr uint32_t kPpBucketTerms = 1u << 16;
__host__ __device__ constexpr uint32_t pp_segment(uint32_t m) {
  uint32_t s = 16;
  while ((uint64_t)s * s < m) s *= 2;
  return s;
}

// out[gid * ostride] = B[r, i] * R mod p for gid = r * m + i: the strided terms of a chunk, dense
// (ostride = 1) or as entry 1 of each term's power table (ostride = 2^w - 1).
template <bool F>
__global__ void __launch_bounds__(kBlock) k_pp_import(const MontConsts* __restrict__ C,
                                                      const uint8_t* __restrict__ be, uint64_t row_stride,
                                                      uint64_t term_stride, uint32_t rows, uint32_t m,
                                                      uint32_t ostride, uint32_t* __restrict__ out) {
  const uint32_t gid = group_id();
  const uint32_t n = rows * m;
  const uint32_t e = gid < n ? gid : n - 1;
  const uint32_t r = e / m, i = e % m;
  uint32_t* slot = group_slot();
  Mont<F> M;
  M.load(C);
  stage_be(slot, be + ((size_t)r * row_stride + (size_t)i * term_stride) * 512);
  wave_sync();
  uint32_t x[kL];
#pragma unroll
  for (int j = 0; j < kL; ++j) x[j] = bits_limb(slot, kLimbBits * (glane() * kL + j));
  wave_sync();
  elem_to_lds(slot, C->r2);
  wave_sync();
  M.mul(x, slot);
  if (gid < n) store_elem(out + (size_t)gid * ostride * kW, x);
}

// ---------------------------------------------------------------------------------
// Interleaved windows: one group per row.  tab holds, per group, m tables of tw = 2^w - 1
// entries b^1..b^tw; entry 1 of the rows' tables is k_pp_import's.  A tail group runs the last
// row's schedule on entry 1 alone and stores nothing, so no group reads what another writes.
// acc[r] = (first ? 1 : acc[r]) * PROD_i b_i^{e_i}.
// ---------------------------------------------------------------------------------
template <bool F>
__global__ void __launch_bounds__(kBlock) k_pp_inter(const MontConsts* __restrict__ C, uint32_t* tab,
                                                     const uint8_t* __restrict__ exps, uint32_t rows, uint32_t m,
                                                     uint32_t w, uint32_t first, uint32_t* acc) {
  const uint32_t gid = group_id();
  const uint32_t row = gid < rows ? gid : rows - 1;
  const uint32_t tw = (1u << w) - 1u;
  uint32_t* slot = group_slot();
  Mont<F> M;
  M.load(C);
  uint32_t x[kL];
  const bool live = gid < rows;
  uint32_t* mine = tab + (size_t)row * m * tw * kW;
#pragma unroll 1
  for (uint32_t i = 0; i < m; ++i) {
    uint32_t* t = mine + (size_t)i * tw * kW;
    load_elem(x, t);
#pragma unroll 1
    for (uint32_t d = 2; d <= tw; ++d) {
      mmul_g(M, x, slot, t);
      if (live) store_elem(t + (size_t)(d - 1) * kW, x);
    }
  }
  load_elem(x, C->one);
  const int rounds = (int)((256u + w - 1u) / w);
#pragma unroll 1
  for (int rd = rounds - 1; rd >= 0; --rd) {
    if (rd != rounds - 1) {
#pragma unroll 1
      for (uint32_t s = 0; s < w; ++s) msqr(M, x, slot);
    }
#pragma unroll 1
    for (uint32_t i = 0; i < m; ++i) {
      // the same digit in every lane of the launch: a scalar branch
      const uint32_t d = __builtin_amdgcn_readfirstlane(be_digit(exps + (size_t)i * 32, 32, rd * (int)w, (int)w));
      if (d) mmul_g(M, x, slot, mine + ((size_t)i * tw + (live ? d - 1 : 0u)) * kW);
    }
  }
  if (!first) mmul_g(M, x, slot, live ? acc + (size_t)row * kW : C->one);
  if (live) store_elem(acc + (size_t)gid * kW, x);
}

// ---------------------------------------------------------------------------------
// Buckets, step 1: digits and a counting sort per window, once for all rows.
//   cnt[w, d]   terms whose w-th c-bit digit is d           (k_pp_hist; zeroed by the caller)
//   start[w, d] exclusive scan of cnt over d                 (k_pp_scan)
//   segoff[w, d] exclusive scan over d of the buckets' segment counts ceil(cnt / S), bucket 0
//               counting none; segoff[w, 2^c] is the window's total (rows of 2^c + 1)
//   perm[w, .]  the term indices ordered by digit            (k_pp_scatter; fill zeroed by the caller)
// The order inside a bucket is whatever the atomics give: the product commutes and is exact.
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_pp_hist(const uint8_t* __restrict__ exps, uint32_t m, uint32_t c,
                                                 uint32_t nwin, uint32_t* __restrict__ cnt) {
  const uint32_t tid = blockIdx.x * 256u + threadIdx.x;
  if (tid >= nwin * m) return;
  const uint32_t w = tid / m, i = tid % m;
  const uint32_t d = be_digit(exps + (size_t)i * 32, 32, (int)(w * c), (int)c);
  atomicAdd(&cnt[((size_t)w << c) + d], 1u);
}

__global__ void __launch_bounds__(256) k_pp_scan(const uint32_t* __restrict__ cnt, uint32_t c, uint32_t seg,
                                                 uint32_t* __restrict__ start, uint32_t* __restrict__ segoff) {
  __shared__ uint32_t s_a[256], s_s[256];
  const uint32_t w = blockIdx.x, t = threadIdx.x;
  const uint32_t B = 1u << c;
  const uint32_t per = (B + 255u) / 256u;
  const uint32_t j0 = t * per, j1 = j0 + per < B ? j0 + per : B;
  const uint32_t* cw = cnt + (size_t)w * B;
  uint32_t a = 0, s = 0;
  for (uint32_t j = j0; j < j1; ++j) {
    a += cw[j];
    s += j ? (cw[j] + seg - 1u) / seg : 0u;
  }
  s_a[t] = a;
  s_s[t] = s;
  __syncthreads();
  if (t == 0) {
    uint32_t ra = 0, rs = 0;
    for (uint32_t k = 0; k < 256u; ++k) {
      const uint32_t va = s_a[k], vs = s_s[k];
      s_a[k] = ra;
      s_s[k] = rs;
      ra += va;
      rs += vs;
    }
    segoff[(size_t)w * (B + 1u) + B] = rs;
  }
  __syncthreads();
  a = s_a[t];
  s = s_s[t];
  for (uint32_t j = j0; j < j1; ++j) {
    start[(size_t)w * B + j] = a;
    segoff[(size_t)w * (B + 1u) + j] = s;
    a += cw[j];
    s += j ? (cw[j] + seg - 1u) / seg : 0u;
  }
}

__global__ void __launch_bounds__(256) k_pp_scatter(const uint8_t* __restrict__ exps, uint32_t m, uint32_t c,
                                                    uint32_t nwin, const uint32_t* __restrict__ start,
                                                    uint32_t* __restrict__ fill, uint32_t* __restrict__ perm) {
  const uint32_t tid = blockIdx.x * 256u + threadIdx.x;
  if (tid >= nwin * m) return;
  const uint32_t w = tid / m, i = tid % m;
  const uint32_t d = be_digit(exps + (size_t)i * 32, 32, (int)(w * c), (int)c);
  const size_t b = ((size_t)w << c) + d;
  const uint32_t pos = start[b] + atomicAdd(&fill[b], 1u);  // < m: start + cnt never passes the window's m
  perm[(size_t)w * m + pos] = i;
}

// ---------------------------------------------------------------------------------
// Buckets, step 2.  k_pp_seg: group (w, slot, r), r fastest, multiplies the members of segment
// `slot` of window w in row r: slot -> (bucket j, segment s of it) by a binary search in segoff,
// members perm[w, start[w, j] + s S + k], k < min(S, cnt - s S), gathered from the imported terms
// E[r, i].  Slots past the window's total are idle.  part[(w * segmax + slot) * rows + r].
// k_pp_bucket: group (w, j, r) multiplies bucket j's segments; an empty bucket (and bucket 0) is
// the Montgomery one.  bk[((w << c) + j) * rows + r].
// Both run each wave to its longest list, padding with the Montgomery one, as k_prod does.
// ---------------------------------------------------------------------------------
template <bool F>
__global__ void __launch_bounds__(kBlock) k_pp_seg(const MontConsts* __restrict__ C, const uint32_t* __restrict__ E,
                                                   const uint32_t* __restrict__ cnt,
                                                   const uint32_t* __restrict__ start,
                                                   const uint32_t* __restrict__ segoff,
                                                   const uint32_t* __restrict__ perm, uint32_t rows, uint32_t m,
                                                   uint32_t c, uint32_t seg, uint32_t segmax, uint32_t nwin,
                                                   uint32_t* __restrict__ part) {
  const uint32_t gid = group_id();
  const uint32_t ngroups = nwin * segmax * rows;
  const uint32_t g = gid < ngroups ? gid : ngroups - 1;
  const uint32_t r = g % rows, t = g / rows;
  const uint32_t slot = t % segmax, w = t / segmax;
  const uint32_t B = 1u << c;
  const uint32_t* so = segoff + (size_t)w * (B + 1u);
  uint32_t len = 0, base = 0;
  if (slot < so[B]) {
    uint32_t lo = 1, hi = B;  // so[lo] <= slot < so[hi]
    while (hi - lo > 1u) {
      const uint32_t mid = (lo + hi) / 2u;
      if (so[mid] <= slot) lo = mid;
      else hi = mid;
    }
    const uint32_t s = slot - so[lo];
    const uint32_t left = cnt[(size_t)w * B + lo] - s * seg;
    len = left < seg ? left : seg;
    base = start[(size_t)w * B + lo] + s * seg;
  }
  const uint32_t* pm = perm + (size_t)w * m + base;
  const uint32_t* Er = E + (size_t)r * m * kW;
  uint32_t* slotp = group_slot();
  Mont<F> M;
  M.load(C);
  uint32_t x[kL];
  load_elem(x, len ? Er + (size_t)pm[0] * kW : C->one);
#pragma unroll 1
  for (uint32_t k = 1; __ballot(k < len) != 0; ++k) {
    const uint32_t* el = k < len ? Er + (size_t)pm[k] * kW : C->one;
    mmul_g(M, x, slotp, el);
  }
  if (gid < ngroups) store_elem(part + (size_t)g * kW, x);
}

template <bool F>
__global__ void __launch_bounds__(kBlock) k_pp_bucket(const MontConsts* __restrict__ C,
                                                      const uint32_t* __restrict__ part,
                                                      const uint32_t* __restrict__ segoff, uint32_t rows, uint32_t c,
                                                      uint32_t segmax, uint32_t nwin, uint32_t* __restrict__ bk) {
  const uint32_t gid = group_id();
  const uint32_t B = 1u << c;
  const uint32_t ngroups = nwin * B * rows;
  const uint32_t g = gid < ngroups ? gid : ngroups - 1;
  const uint32_t r = g % rows, t = g / rows;
  const uint32_t j = t % B, w = t / B;
  const uint32_t* so = segoff + (size_t)w * (B + 1u);
  const uint32_t s0 = so[j];
  const uint32_t ns = j ? so[j + 1] - s0 : 0u;
  const uint32_t* src = part + (((size_t)w * segmax + s0) * rows + r) * kW;
  const size_t step = (size_t)rows * kW;
  uint32_t* slot = group_slot();
  Mont<F> M;
  M.load(C);
  uint32_t x[kL];
  load_elem(x, ns ? src : C->one);
#pragma unroll 1
  for (uint32_t k = 1; __ballot(k < ns) != 0; ++k) {
    const uint32_t* el = k < ns ? src + (size_t)k * step : C->one;
    mmul_g(M, x, slot, el);
  }
  if (gid < ngroups) store_elem(bk + (size_t)g * kW, x);
}

// ---------------------------------------------------------------------------------
// Buckets, step 3: bit products.  Group ((r, w, t), s), s fastest, multiplies members
// k = s ch .. s ch + ch - 1 of the 2^(c-1) buckets j of window w whose bit t is set
// (j = k with a one inserted at bit t); ch divides 2^(c-1), so every group runs ch - 1 multiplies.
// out[((r * nwin + w) * c + t) * nch + s]: with nch == 1 these are Q[r, c w + t] themselves,
// otherwise a k_prod pass over each run of nch finishes them.
// ---------------------------------------------------------------------------------
template <bool F>
__global__ void __launch_bounds__(kBlock) k_pp_bits(const MontConsts* __restrict__ C, const uint32_t* __restrict__ bk,
                                                    uint32_t rows, uint32_t c, uint32_t nwin, uint32_t ch,
                                                    uint32_t nch, uint32_t* __restrict__ out) {
  const uint32_t gid = group_id();
  const uint32_t ngroups = rows * nwin * c * nch;
  const uint32_t g = gid < ngroups ? gid : ngroups - 1;
  const uint32_t s = g % nch, q = g / nch;
  const uint32_t t = q % c, q2 = q / c;
  const uint32_t w = q2 % nwin, r = q2 / nwin;
  const uint32_t low = (1u << t) - 1u;
  uint32_t* slot = group_slot();
  Mont<F> M;
  M.load(C);
  uint32_t x[kL];
  auto member = [&](uint32_t k) -> const uint32_t* {
    const uint32_t j = ((k >> t) << (t + 1u)) | (1u << t) | (k & low);
    return bk + ((((size_t)w << c) + j) * rows + r) * kW;
  };
  const uint32_t k0 = s * ch;
  load_elem(x, member(k0));
#pragma unroll 1
  for (uint32_t k = 1; k < ch; ++k) mmul_g(M, x, slot, member(k0 + k));
  if (gid < ngroups) store_elem(out + (size_t)g * kW, x);
}

// ---------------------------------------------------------------------------------
// Buckets, step 4: acc[r] = (first ? 1 : acc[r]) * PROD_{k<256} Q[r, k]^(2^k), Horner from bit 255:
// 255 squarings and 255 multiplies, one chain per row.  Q rows are qstride >= 256 elements.
// ---------------------------------------------------------------------------------
template <bool F>
__global__ void __launch_bounds__(kBlock) k_pp_horner(const MontConsts* __restrict__ C, const uint32_t* __restrict__ Q,
                                                      uint32_t rows, uint32_t qstride, uint32_t first,
                                                      uint32_t* acc) {
  const uint32_t gid = group_id();
  const uint32_t row = gid < rows ? gid : rows - 1;
  const uint32_t* q = Q + (size_t)row * qstride * kW;
  uint32_t* slot = group_slot();
  Mont<F> M;
  M.load(C);
  uint32_t x[kL];
  load_elem(x, q + (size_t)255 * kW);
#pragma unroll 1
  for (int k = 254; k >= 0; --k) {
    msqr(M, x, slot);
    mmul_g(M, x, slot, q + (size_t)k * kW);
  }
  if (!first) mmul_g(M, x, slot, acc + (size_t)row * kW);
  if (gid < rows) store_elem(acc + (size_t)gid * kW, x);
}

}  // namespace eg
