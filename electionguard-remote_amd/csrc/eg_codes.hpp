// eg_codes.hpp — ballot nonces, ballot hashes and confirmation codes (include/eg_hip_codes.h).
//
// Every value is the project's hash_elems over 32-byte "Q" and 512-byte "P" elements,
//   H(e_0 .. e_k) = SHA256("|" + hex(e_0) + "|" + ... + "|") mod q   (32 bytes big-endian),
// upper-case hex, fixed width or minimal per the ctx's hash format.  Q elements enter as the 32
// bytes given (not range-checked, not reduced); unlike k_hash_check no Q-bar is prefixed.
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
#include "eg_kernels.hpp"

namespace eg {

// one 64-B block buffer per thread at a 68-B stride, as in k_hash_check: with a 64-B stride
// every lane's byte k sits in the same LDS bank and each buffer access is a 32-way conflict
// (ds_read_b32 / ds_write_b32 bank = word % 32 within a 32-lane half; 17 is odd, so the 32
// lanes' words k land on 32 distinct banks)
constexpr int kCodeBufStride = 17;

// hex of the 32-byte big-endian element whose value is v < 2^32 (the small integers of the
// nonce pre-images): fixed width 56 zeros and v's 8 digits, minimal v's bytes without leading
// zero bytes (0 -> "00")
__device__ __forceinline__ void put_hex_small(Sha256& H, uint32_t v, bool minimal) {
  if (!minimal) {
    for (int i = 0; i < 14; ++i) H.put4(0x30303030u);
    // nibbles most significant first, one per byte, first character in the low byte
    const uint32_t hi = ((v >> 28) & 15u) | (((v >> 24) & 15u) << 8) | (((v >> 20) & 15u) << 16) |
                        (((v >> 16) & 15u) << 24);
    const uint32_t lo = ((v >> 12) & 15u) | (((v >> 8) & 15u) << 8) | (((v >> 4) & 15u) << 16) | ((v & 15u) << 24);
    H.put4(Sha256::hex4(hi));
    H.put4(Sha256::hex4(lo));
    return;
  }
  bool started = false;
  for (int sh = 24; sh >= 0; sh -= 8) {
    const uint32_t byte = (v >> sh) & 0xFFu;
    if (!started && byte == 0 && sh != 0) continue;
    started = true;
    H.put(Sha256::hexc(byte >> 4));
    H.put(Sha256::hexc(byte & 15u));
  }
}

// close the pre-image, reduce the digest mod q (q > 2^255: at most one subtraction)
__device__ __forceinline__ U256 finish_mod_q(Sha256& H, const uint8_t* __restrict__ q_be) {
  uint32_t dig[8];
  H.finish(dig);
  const U256 q = ld256(q_be);
  U256 h;
  for (int k = 0; k < 8; ++k) h.w[k] = dig[7 - k];
  if (!lt256(h, q)) sub256(h, q);
  return h;
}

// One thread per output scalar: threads [0, nb nsel 4) write sel_nonces (nb, nsel, 4, 32),
// the next nb nc write contest_nonces (nb, nc, 32) -- the encryptor's input layout.
__global__ void __launch_bounds__(256) k_derive_nonces(const uint8_t* __restrict__ q_be,
                                                       const uint8_t* __restrict__ ballot_nonces, uint64_t nb,
                                                       uint32_t nsel, uint32_t nc, uint8_t* __restrict__ sel_nonces,
                                                       uint8_t* __restrict__ contest_nonces, uint32_t hash_minimal) {
  __shared__ uint32_t s_buf[256 * kCodeBufStride];
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint64_t per_sel = (uint64_t)nsel * 4, nsn = nb * per_sel;
  if (i >= nsn + nb * nc) return;
  const bool is_sel = i < nsn;
  const uint64_t j = is_sel ? i : i - nsn;
  const uint64_t per = is_sel ? per_sel : (uint64_t)nc;
  const uint64_t b = j / per;
  const uint32_t idx = (uint32_t)(j - b * per);  // 4 s + t, or the contest k
  const bool mn = hash_minimal != 0;
  Sha256 H;
  H.init(s_buf + threadIdx.x * kCodeBufStride);
  H.put('|');
  H.put_hex(ballot_nonces + b * 32, 32, mn);
  H.put('|');
  put_hex_small(H, is_sel ? 1u : 2u, mn);
  H.put('|');
  put_hex_small(H, idx, mn);
  H.put('|');
  st256((is_sel ? sel_nonces : contest_nonces) + j * 32, finish_mod_q(H, q_be));
}

// One thread per (ballot, selection): h_sel = H(dsel[s], alpha, beta); cts (n / nsel, nsel, 2, 512).
__global__ void __launch_bounds__(256) k_sel_hash(const uint8_t* __restrict__ q_be, const uint8_t* __restrict__ dsel,
                                                  const uint8_t* __restrict__ cts, uint64_t n, uint32_t nsel,
                                                  uint8_t* __restrict__ out, uint32_t hash_minimal) {
  __shared__ uint32_t s_buf[256 * kCodeBufStride];
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const bool mn = hash_minimal != 0;
  Sha256 H;
  H.init(s_buf + threadIdx.x * kCodeBufStride);
  H.put('|');
  H.put_hex(dsel + (i % nsel) * 32, 32, mn);
  H.put('|');
  H.put_hex(cts + i * 1024, 512, mn);
  H.put('|');
  H.put_hex(cts + i * 1024 + 512, 512, mn);
  H.put('|');
  st256(out + i * 32, finish_mod_q(H, q_be));
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
  __shared__ uint32_t s_buf[256 * kCodeBufStride];
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const bool mn = hash_minimal != 0;
  const uint64_t b = i / period;
  const uint32_t k = (uint32_t)(i - b * period);
  const uint64_t start = b * run_stride + (first ? first[k] : 0u);
  const uint32_t m = first ? len[k] : run_len;
  Sha256 H;
  H.init(s_buf + threadIdx.x * kCodeBufStride);
  H.put('|');
  if (l0.ptr) {
    H.put_hex(l0.ptr + (i % l0.mod) * 32, 32, mn);
    H.put('|');
  }
  if (l1.ptr) {
    H.put_hex(l1.ptr + (i % l1.mod) * 32, 32, mn);
    H.put('|');
  }
  for (uint32_t s = 0; s < m; ++s) {
    H.put_hex(hashes + (start + s) * 32, 32, mn);
    H.put('|');
  }
  st256(out + i * 32, finish_mod_q(H, q_be));
}

// One thread per ballot: ok[b] = (codes[b] == H(codes[b-1] or seed, ts[b], B[b])).  The recorded
// code is compared as bytes, so a recorded value >= q never matches.
__global__ void __launch_bounds__(256) k_code_check(const uint8_t* __restrict__ q_be, const uint8_t* __restrict__ seed,
                                                    const uint8_t* __restrict__ ts,
                                                    const uint8_t* __restrict__ ballot_hashes,
                                                    const uint8_t* __restrict__ codes, uint64_t n,
                                                    uint8_t* __restrict__ ok, uint32_t hash_minimal) {
  __shared__ uint32_t s_buf[256 * kCodeBufStride];
  const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= n) return;
  const bool mn = hash_minimal != 0;
  Sha256 H;
  H.init(s_buf + threadIdx.x * kCodeBufStride);
  H.put('|');
  H.put_hex(b ? codes + (b - 1) * 32 : seed, 32, mn);
  H.put('|');
  H.put_hex(ts + b * 32, 32, mn);
  H.put('|');
  H.put_hex(ballot_hashes + b * 32, 32, mn);
  H.put('|');
  const U256 h = finish_mod_q(H, q_be);
  const U256 c = ld256(codes + b * 32);
  bool good = true;
  for (int k = 0; k < 8; ++k) good &= (c.w[k] == h.w[k]);
  ok[b] = good ? 1 : 0;
}

}  // namespace eg
