// eg_hash_elems.hpp — the one writer of the project's hash_elems pre-image on the device,
//   H(e_0 .. e_k) = SHA256("|" + hex(e_0) + "|" + ... + "|"),
// over 32-byte "Q" and 512-byte "P" elements: upper-case hex, fixed width or minimal per the
// context's hash format (eg_ctx_set_hash_format).  One thread per hash on eg::Sha256.
//
// A hash kernel declares the block's buffer and then states its pre-image and nothing else:
//   __shared__ uint32_t s_buf[256 * kHashBufStride];
//   HashElems H(s_buf, hash_minimal);
//   H.q(xi); H.small(4); H.small(w);
//   st256(out, H.mod_q_top(ld256(q_be)));
//
// The digest is closed in one of three ways: raw words (digest), or mod q in exactly two forms.
// mod_q_top subtracts q once and is right only for q >= 2^255 (the production q = 2^256 - 189);
// mod_q_any is right for any q > 1 and costs a mulmod256 when one subtraction does not do.  The
// shuffle uses both: its generator seed goes through k_hash_check (top), its leaves, trees and
// challenges through mod_q_any, which is what its small test groups exercise.
#pragma once
#include "eg_sha256.hpp"
#include "eg_u256.hpp"

namespace eg {

// A thread's 64-byte SHA block buffer sits in LDS at a 17-word (68-byte) stride.  With a 64-byte
// stride every lane's byte k would sit in the same LDS bank and each buffer access would be a
// 32-way conflict (ds_read_b32 / ds_write_b32: bank = word % 32 within a 32-lane half); 17 is
// odd, so the 32 lanes' words k land on 32 distinct banks.  The HMAC and stream code
// (eg_hmac.hpp) drives Sha256 directly on the same stride.
constexpr int kHashBufStride = 17;

struct HashElems {
  Sha256 H;
  bool minimal;

  // begin on this thread's slice of the block's buffer (blockDim.x * kHashBufStride words of
  // LDS) in the given format; writes the opening '|'.  Beginning again on the same buffer after
  // a close is fine: a thread owns its slice.
  __device__ __forceinline__ HashElems(uint32_t* block_buf, uint32_t hash_minimal) : minimal(hash_minimal != 0) {
    H.init(block_buf + threadIdx.x * kHashBufStride);
    H.put('|');
  }

  // an element of `bytes` big-endian bytes (32 or 512; 16-byte aligned) and its '|'
  __device__ __forceinline__ void elem(const uint8_t* __restrict__ e, uint32_t bytes) {
    H.put_hex(e, bytes, minimal);
    H.put('|');
  }
  __device__ __forceinline__ void q(const uint8_t* __restrict__ e) { elem(e, 32); }
  __device__ __forceinline__ void p(const uint8_t* __restrict__ e) { elem(e, 512); }

  // the Q element whose value is v < 2^32 (tags, indices, lengths) and its '|': fixed width 56
  // zeros and v's 8 digits, minimal v's bytes without leading zero bytes (0 -> "00")
  __device__ __forceinline__ void small(uint32_t v) {
    if (!minimal) {
      for (int i = 0; i < 14; ++i) H.put4(0x30303030u);
      // nibbles most significant first, one per byte, first character in the low byte
      const uint32_t hi = ((v >> 28) & 15u) | (((v >> 24) & 15u) << 8) | (((v >> 20) & 15u) << 16) |
                          (((v >> 16) & 15u) << 24);
      const uint32_t lo = ((v >> 12) & 15u) | (((v >> 8) & 15u) << 8) | (((v >> 4) & 15u) << 16) | ((v & 15u) << 24);
      H.put4(Sha256::hex4(hi));
      H.put4(Sha256::hex4(lo));
    } else {
      bool started = false;
      for (int sh = 24; sh >= 0; sh -= 8) {
        const uint32_t byte = (v >> sh) & 0xFFu;
        if (!started && byte == 0 && sh != 0) continue;
        started = true;
        H.put(Sha256::hexc(byte >> 4));
        H.put(Sha256::hexc(byte & 15u));
      }
    }
    H.put('|');
  }

  // close: the raw digest words (dig[0] the most significant)
  __device__ __forceinline__ void digest(uint32_t (&dig)[8]) { H.finish(dig); }

  // close mod q, single subtraction.  PRECONDITION q >= 2^255: a digest below 2^256 is then below
  // 2 q.  Never reaches mulmod256.
  __device__ __forceinline__ U256 mod_q_top(const U256& q) {
    U256 h = digest_value();
    if (!lt256(h, q)) sub256(h, q);
    return h;
  }

  // close mod q, any q > 1: the subtraction first, the ladder only for a q far below 2^256
  // (test groups)
  __device__ __forceinline__ U256 mod_q_any(const U256& q) {
    U256 h = digest_value();
    if (!lt256(h, q)) {
      sub256(h, q);
      if (!lt256(h, q)) h = mod256_any(h, q);
    }
    return h;
  }

 private:
  __device__ __forceinline__ U256 digest_value() {
    uint32_t dig[8];
    H.finish(dig);
    U256 h;
#pragma unroll
    for (int k = 0; k < 8; ++k) h.w[k] = dig[7 - k];
    return h;
  }
};

}  // namespace eg
