// eg_codes.hpp — ballot nonces, ballot hashes and confirmation codes (include/eg_hip_codes.h).
//
// Every value is the project's hash_elems over 32-byte "Q" and 512-byte "P" elements,
//   H(e_0 .. e_k) = SHA256("|" + hex(e_0) + "|" + ... + "|") mod q   (32 bytes big-endian),
// written by eg_hash_elems.hpp's HashElems and closed by its single-subtraction mod_q_top (the
// production q).  Q elements enter as the 32 bytes given (not range-checked, not reduced); unlike
// k_hash_check no Q-bar is prefixed.
//
//   N_sel(xi_b, s, t) = H(xi_b, 1, 4 s + t)      t = 0..3: R, u, c_fake, v_fake
//   N_con(xi_b, k)    = H(xi_b, 2, k)
//   h_sel[b,s]        = H(dsel[s], alpha, beta)
//   h_con[b,k]        = H(dcon[k], h_sel[b,off_k] .. h_sel[b,off_k+spc_k-1])
//   B[b]              = H(ballot_id[b], manifest_hash, h_con[b,0] .. h_con[b,nc-1])
//   code[b]           = H(code[b-1], ts[b], B[b])       code[-1] = seed
//
// One thread per hash, 64-bit indices throughout, and no barrier anywhere: a thread past the
// end of the grid simply returns.
#pragma once
#include "eg_hash_elems.hpp"

namespace eg {

// One thread per output scalar: threads [0, nb nsel 4) write sel_nonces (nb, nsel, 4, 32),
// the next nb nc write contest_nonces (nb, nc, 32) -- the encryptor's input layout.
__global__ void __launch_bounds__(256) k_derive_nonces(const uint8_t* __restrict__ q_be,
                                                       const uint8_t* __restrict__ ballot_nonces, uint64_t nb,
                                                       uint32_t nsel, uint32_t nc, uint8_t* __restrict__ sel_nonces,
                                                       uint8_t* __restrict__ contest_nonces, uint32_t hash_minimal) {
  __shared__ uint32_t s_buf[256 * kHashBufStride];
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint64_t per_sel = (uint64_t)nsel * 4, nsn = nb * per_sel;
  if (i >= nsn + nb * nc) return;
  const bool is_sel = i < nsn;
  const uint64_t j = is_sel ? i : i - nsn;
  const uint64_t per = is_sel ? per_sel : (uint64_t)nc;
  const uint64_t b = j / per;
  const uint32_t idx = (uint32_t)(j - b * per);  // 4 s + t, or the contest k
  HashElems H(s_buf, hash_minimal);
  H.q(ballot_nonces + b * 32);
  H.small(is_sel ? 1u : 2u);
  H.small(idx);
  st256((is_sel ? sel_nonces : contest_nonces) + j * 32, H.mod_q_top(ld256(q_be)));
}

// One thread per (ballot, selection): h_sel = H(dsel[s], alpha, beta); cts (n / nsel, nsel, 2, 512).
__global__ void __launch_bounds__(256) k_sel_hash(const uint8_t* __restrict__ q_be, const uint8_t* __restrict__ dsel,
                                                  const uint8_t* __restrict__ cts, uint64_t n, uint32_t nsel,
                                                  uint8_t* __restrict__ out, uint32_t hash_minimal) {
  __shared__ uint32_t s_buf[256 * kHashBufStride];
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  HashElems H(s_buf, hash_minimal);
  H.q(dsel + (i % nsel) * 32);
  H.p(cts + i * 1024);
  H.p(cts + i * 1024 + 512);
  st256(out + i * 32, H.mod_q_top(ld256(q_be)));
}

// A leading 32-byte element of k_seg_hash: item i reads ptr + (i % mod) * 32, so mod = 1 is one
// element shared by every item, mod = the period one per position in the ballot (dcon[k]) and
// mod = the item count one per item (ballot_id[b]).  ptr == nullptr: no such element.
struct SegLead {
  const uint8_t* ptr;
  uint64_t mod;
};

// One thread per item: H(lead0, lead1, run), the run being len consecutive 32-byte hashes.
// Item i = (b, k) with k = i % period: its run starts at hash b * run_stride + first[k] and is
// len[k] long (first == nullptr: starts at b * run_stride, run_len long).  h_con is period nc
// over the selection hashes (run_stride nsel, tables first / spc); B is period 1 over the
// contest hashes (run_stride = run_len = nc).
__global__ void __launch_bounds__(256) k_seg_hash(const uint8_t* __restrict__ q_be, SegLead l0, SegLead l1,
                                                  const uint8_t* __restrict__ hashes,
                                                  const uint32_t* __restrict__ first,
                                                  const uint32_t* __restrict__ len, uint32_t period,
                                                  uint64_t run_stride, uint32_t run_len, uint64_t n,
                                                  uint8_t* __restrict__ out, uint32_t hash_minimal) {
  __shared__ uint32_t s_buf[256 * kHashBufStride];
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint64_t b = i / period;
  const uint32_t k = (uint32_t)(i - b * period);
  const uint64_t start = b * run_stride + (first ? first[k] : 0u);
  const uint32_t m = first ? len[k] : run_len;
  HashElems H(s_buf, hash_minimal);
  if (l0.ptr) H.q(l0.ptr + (i % l0.mod) * 32);
  if (l1.ptr) H.q(l1.ptr + (i % l1.mod) * 32);
  for (uint32_t s = 0; s < m; ++s) H.q(hashes + (start + s) * 32);
  st256(out + i * 32, H.mod_q_top(ld256(q_be)));
}

// One thread per ballot: ok[b] = (codes[b] == H(codes[b-1] or seed, ts[b], B[b])).  The recorded
// code is compared as bytes, so a recorded value >= q never matches.
__global__ void __launch_bounds__(256) k_code_check(const uint8_t* __restrict__ q_be, const uint8_t* __restrict__ seed,
                                                    const uint8_t* __restrict__ ts,
                                                    const uint8_t* __restrict__ ballot_hashes,
                                                    const uint8_t* __restrict__ codes, uint64_t n,
                                                    uint8_t* __restrict__ ok, uint32_t hash_minimal) {
  __shared__ uint32_t s_buf[256 * kHashBufStride];
  const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= n) return;
  HashElems H(s_buf, hash_minimal);
  H.q(b ? codes + (b - 1) * 32 : seed);
  H.q(ts + b * 32);
  H.q(ballot_hashes + b * 32);
  ok[b] = eq256(ld256(codes + b * 32), H.mod_q_top(ld256(q_be))) ? 1 : 0;
}

}  // namespace eg
