// eg_hmac.hpp — HMAC-SHA256 on the device SHA-256, and the contest-data kernels
// (include/eg_hip_contestdata.h): a contest's write-ins and overvote status under HashedElGamal.
//
//   r[b,k]  = H(xi_b, 3, k)                                  hash_elems (eg_hash_elems.hpp)
//   kk      = SHA256(c0 || kappa)                            1024 raw bytes; c0 = g^r, kappa = K^r
//   block j = HMAC(kk, 0x01 || "contest" || label || be32(j))    label = ballot_id[b] || be32(k)
//   mk      = HMAC(kk, 0x02 || "contest" || label)
//   c1      = data XOR stream,   c2 = HMAC(mk, c0 || c1)
//
// The HMACs are over raw bytes (the ctx's hex format enters the nonce only).  eg::Sha256 is used
// as it is: raw bytes go in through its put / put4, and a key's ipad and opad blocks are
// compressed once (HmacKey) and every HMAC under that key resumes from the saved states, so a
// stream block costs two compressions instead of four.
//
// As in eg_codes.hpp: one thread per item, 256 threads per block, 64-bit indices, no barrier, the
// block buffer in LDS at kHashBufStride.  A thread owns ONE block buffer, so the stream and
// the MAC are two passes: seal writes c1 and then hashes it back from where it lies (a thread
// reads its own stores), open hashes c1 first and then decrypts it.
#pragma once
#include "eg_hash_elems.hpp"

namespace eg {

constexpr uint32_t kCdMaxBytes = 1024;  // EG_CD_MAX_BYTES

// SHA-256 states after the 64-byte blocks key ^ ipad and key ^ opad
struct HmacKey {
  uint32_t in[8], out[8];
};

// n raw bytes from a 16-byte aligned source, n a multiple of 16
__device__ __forceinline__ void put_raw16(Sha256& H, const uint8_t* __restrict__ p, uint32_t n) {
  const uint4* s = reinterpret_cast<const uint4*>(p);
  for (uint32_t i = 0; i < n / 16; ++i) {
    const uint4 v = s[i];
    H.put4(v.x);
    H.put4(v.y);
    H.put4(v.z);
    H.put4(v.w);
  }
}

// a digest's eight words as the 32 bytes they stand for
__device__ __forceinline__ void put_digest(Sha256& H, const uint32_t (&d)[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) H.put4(__builtin_bswap32(d[i]));
}

__device__ __forceinline__ void sha_resume(Sha256& H, const uint32_t (&st)[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) H.h[i] = st[i];
  H.len = 64;
  H.pend = 0;
}

__device__ __forceinline__ void hmac_pad_state(Sha256& H, const uint32_t (&key)[8], uint32_t pad, uint32_t (&st)[8]) {
  H.init(H.buf);
#pragma unroll
  for (int i = 0; i < 8; ++i) H.put4(__builtin_bswap32(key[i]) ^ pad);
#pragma unroll
  for (int i = 0; i < 8; ++i) H.put4(pad);  // the 16th word compresses
#pragma unroll
  for (int i = 0; i < 8; ++i) st[i] = H.h[i];
}

// the saved states of a 32-byte key given as digest words (zero-padded to the 64-byte block)
__device__ __forceinline__ void hmac_key(Sha256& H, const uint32_t (&key)[8], HmacKey& K) {
  hmac_pad_state(H, key, 0x36363636u, K.in);
  hmac_pad_state(H, key, 0x5c5c5c5cu, K.out);
}

__device__ __forceinline__ void hmac_begin(Sha256& H, const HmacKey& K) { sha_resume(H, K.in); }

__device__ __forceinline__ void hmac_end(Sha256& H, const HmacKey& K, uint32_t (&mac)[8]) {
  uint32_t inner[8];
  H.finish(inner);
  sha_resume(H, K.out);
  put_digest(H, inner);
  H.finish(mac);
}

// domain byte || "contest" || ballot id || be32(k): 44 bytes, word-aligned in the stream
struct CdLabel {
  uint32_t id[8];  // the ballot id's words in memory order
  uint32_t k_be;   // be32(k), first byte low
};
__device__ __forceinline__ void put_cd_prefix(Sha256& H, uint32_t domain, const CdLabel& L) {
  H.put4(domain | ('c' << 8) | ('o' << 16) | ('n' << 24));
  H.put4('t' | ('e' << 8) | ('s' << 16) | ('t' << 24));
#pragma unroll
  for (int i = 0; i < 8; ++i) H.put4(L.id[i]);
  H.put4(L.k_be);
}

// Everything a seal and an open share: the item's label, kk's saved states, and mk's.
struct CdKeys {
  CdLabel L;
  HmacKey kk, mk;
};
__device__ __forceinline__ void cd_keys(Sha256& H, const uint8_t* __restrict__ ballot_ids, uint64_t b, uint32_t k,
                                        const uint8_t* __restrict__ c0, const uint8_t* __restrict__ kappa,
                                        CdKeys& S) {
  const uint32_t* id = reinterpret_cast<const uint32_t*>(ballot_ids + b * 32);
#pragma unroll
  for (int i = 0; i < 8; ++i) S.L.id[i] = id[i];
  S.L.k_be = __builtin_bswap32(k);
  uint32_t d[8];
  H.init(H.buf);
  put_raw16(H, c0, 512);
  put_raw16(H, kappa, 512);
  H.finish(d);
  hmac_key(H, d, S.kk);
  hmac_begin(H, S.kk);
  put_cd_prefix(H, 0x02u, S.L);
  hmac_end(H, S.kk, d);
  hmac_key(H, d, S.mk);
}

// stream block j as digest words: byte t of the block is the (t & 3)-th byte from the top of ks[t >> 2]
__device__ __forceinline__ void cd_stream_block(Sha256& H, const CdKeys& S, uint32_t j, uint32_t (&ks)[8]) {
  hmac_begin(H, S.kk);
  put_cd_prefix(H, 0x01u, S.L);
  H.put4(__builtin_bswap32(j));
  hmac_end(H, S.kk, ks);
}

// dst = (src XOR stream) & mask over nbytes; rows that are whole 4-byte aligned words (the same
// answer for every item of a launch) move a word at a time, others a byte at a time
__device__ __forceinline__ void cd_xor_stream(Sha256& H, const CdKeys& S, const uint8_t* src, uint8_t* dst,
                                              uint32_t nbytes, bool words, uint32_t mask) {
  for (uint32_t j = 0; j * 32 < nbytes; ++j) {
    uint32_t ks[8];
    cd_stream_block(H, S, j, ks);
    const uint32_t off = j * 32, m = nbytes - off < 32u ? nbytes - off : 32u;
    if (words) {
      const uint32_t* s = reinterpret_cast<const uint32_t*>(src + off);
      uint32_t* d = reinterpret_cast<uint32_t*>(dst + off);
      for (uint32_t w = 0; w < m / 4; ++w) d[w] = (s[w] ^ __builtin_bswap32(ks[w])) & mask;
    } else {
      for (uint32_t t = 0; t < m; ++t)
        dst[off + t] = (uint8_t)((src[off + t] ^ (ks[t >> 2] >> (24 - 8 * (t & 3)))) & mask);
    }
  }
}

// HMAC(mk, c0 || c1)
__device__ __forceinline__ void cd_mac(Sha256& H, const CdKeys& S, const uint8_t* __restrict__ c0, const uint8_t* c1,
                                       uint32_t nbytes, bool words, uint32_t (&mac)[8]) {
  hmac_begin(H, S.mk);
  put_raw16(H, c0, 512);
  if (words) {
    const uint32_t* s = reinterpret_cast<const uint32_t*>(c1);
    for (uint32_t w = 0; w < nbytes / 4; ++w) H.put4(s[w]);
  } else {
    for (uint32_t t = 0; t < nbytes; ++t) H.put(c1[t]);
  }
  hmac_end(H, S.mk, mac);
}

__device__ __forceinline__ bool cd_word_rows(const void* a, const void* b, uint32_t nbytes) {
  return ((((uintptr_t)a | (uintptr_t)b) | nbytes) & 3u) == 0;
}

// One thread per (ballot, contest): r[b,k] = H(xi_b, 3, k) -> out (nb, nc, 32).  Tags 1 and 2 are
// k_derive_nonces' selection and contest-proof nonces.
__global__ void __launch_bounds__(256) k_cd_nonces(const uint8_t* __restrict__ q_be,
                                                   const uint8_t* __restrict__ ballot_nonces, uint64_t n, uint32_t nc,
                                                   uint8_t* __restrict__ out, uint32_t hash_minimal) {
  __shared__ uint32_t s_buf[256 * kHashBufStride];
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint64_t b = i / nc;
  HashElems H(s_buf, hash_minimal);
  H.q(ballot_nonces + b * 32);
  H.small(3u);
  H.small((uint32_t)(i - b * nc));
  st256(out + i * 32, H.mod_q_top(ld256(q_be)));
}

// One thread per item: c1 (n, nbytes) = data XOR stream, c2 (n, 32) = HMAC(mk, c0 || c1).
__global__ void __launch_bounds__(256) k_cd_seal(const uint8_t* __restrict__ ballot_ids,
                                                 const uint8_t* __restrict__ c0, const uint8_t* __restrict__ kappa,
                                                 const uint8_t* __restrict__ data, uint64_t n, uint32_t nc,
                                                 uint32_t nbytes, uint8_t* c1, uint8_t* __restrict__ c2) {
  __shared__ uint32_t s_buf[256 * kHashBufStride];
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint64_t b = i / nc;
  const bool words = cd_word_rows(data, c1, nbytes);
  Sha256 H;
  H.init(s_buf + threadIdx.x * kHashBufStride);
  CdKeys S;
  cd_keys(H, ballot_ids, b, (uint32_t)(i - b * nc), c0 + i * 512, kappa + i * 512, S);
  uint8_t* row = c1 + i * nbytes;
  cd_xor_stream(H, S, data + i * nbytes, row, nbytes, words, 0xFFFFFFFFu);
  uint32_t mac[8];
  cd_mac(H, S, c0 + i * 512, row, nbytes, words, mac);
  uint32_t* o = reinterpret_cast<uint32_t*>(c2 + i * 32);
#pragma unroll
  for (int w = 0; w < 8; ++w) o[w] = __builtin_bswap32(mac[w]);
}

// One thread per item: ok = (c2 == HMAC(mk, c0 || c1)), every word compared whatever the others
// gave; data (n, nbytes) = c1 XOR stream under ok's mask, so a failed item's row is zero.
__global__ void __launch_bounds__(256) k_cd_open(const uint8_t* __restrict__ ballot_ids,
                                                 const uint8_t* __restrict__ c0, const uint8_t* __restrict__ kappa,
                                                 const uint8_t* __restrict__ c1, const uint8_t* __restrict__ c2,
                                                 uint64_t n, uint32_t nc, uint32_t nbytes, uint8_t* __restrict__ data,
                                                 uint8_t* __restrict__ ok) {
  __shared__ uint32_t s_buf[256 * kHashBufStride];
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint64_t b = i / nc;
  const bool words = cd_word_rows(data, c1, nbytes);
  Sha256 H;
  H.init(s_buf + threadIdx.x * kHashBufStride);
  CdKeys S;
  cd_keys(H, ballot_ids, b, (uint32_t)(i - b * nc), c0 + i * 512, kappa + i * 512, S);
  uint32_t mac[8];
  cd_mac(H, S, c0 + i * 512, c1 + i * nbytes, nbytes, words, mac);
  const uint32_t* t = reinterpret_cast<const uint32_t*>(c2 + i * 32);
  uint32_t diff = 0;
#pragma unroll
  for (int w = 0; w < 8; ++w) diff |= __builtin_bswap32(mac[w]) ^ t[w];
  const uint32_t good = (uint32_t)(diff == 0);
  cd_xor_stream(H, S, c1 + i * nbytes, data + i * nbytes, nbytes, words, 0u - good);
  ok[i] = (uint8_t)good;
}

}  // namespace eg
