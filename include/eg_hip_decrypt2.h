/* eg_hip_decrypt2.h — threshold decryption with ONE combined Chaum-Pedersen proof per text
 * (ElectionGuard 2.0 style), in libeg_hip.so.  The 1.0 path of eg_hip.h
 * (eg_trustee_decrypt_batch, eg_verify_shares) is untouched.
 *
 * Key ceremony unchanged: guardians j = 1..n_g with x-coordinates x_j, polynomials P_j of degree
 * quorum - 1, public commitments K_{j,m} = g^{a_{j,m}}; K = PROD_j K_{j,0}, s = SUM_j a_{j,0}.
 *
 *   key share          z_i = SUM_j P_j(x_i) mod q (own polynomial included)
 *   share public key   Z_i = g^{z_i} = PROD_j PROD_m K_{j,m}^(x_i^m mod q)
 *   weights            w_i = Lagrange coefficient at 0 of x_i over the available set U, |U| = k >= quorum;
 *                      SUM_{i in U} w_i z_i = s
 *   round 1, guardian i, text t = (A, B):  nonce u;  M_i = A^{z_i}, a_i = g^u, b_i = A^u
 *   combine            M = PROD_{i in U} M_i^{w_i},  a = PROD a_i,  b = PROD b_i
 *   challenge          c = H(Q qbar, Q 0x30, P K, P A, P B, P a, P b, P M)
 *   per guardian       c_i = c * w_i mod q
 *   round 2            v_i = u - c_i * z_i mod q
 *   mediator's check   g^{v_i} Z_i^{c_i} == a_i  and  A^{v_i} M_i^{c_i} == b_i,  with c_i, v_i < q
 *   published          M, (c, v) with v = SUM_{i in U} v_i mod q;  T = B M^-1;  count = dLog_g T
 *   record verifier    a' = g^v K^c, b' = A^v M^c;  ok iff c, v < q and c == H(qbar, 0x30, K, A, B, a', b', M)
 *
 * H is the library's hash_elems: SHA-256 over "|hex|hex|...|" reduced mod q, the hex format the
 * context's (eg_ctx_set_hash_format).  Q elements are 32 bytes, P elements 512; "Q 0x30" is the
 * scalar 0x30, the tag that keeps these challenges apart from the 1.0 share proofs.  A and B are
 * hashed as the bytes given, K as the bytes given, a, b, a', b' and M in canonical form.
 * eg_ctx_set_proof_format does NOT apply: the pre-image order and the minus response above are FIXED.
 *
 * BigInteger semantics: bases are reduced mod p, 0^e = 0 for e > 0, x^0 = 1, outputs are canonical.
 * Exponents of the power kernels (the secret z and the nonce u in commit; c_i, v_i, c, v in check
 * and verify) are used as the 256-bit values given.  The scalars handed to respond (secret, nonces,
 * challenges) are reduced mod q first; the weights of combine and the v_i summed by check likewise.
 * The mediator's check compares the recomputed canonical bytes with the given a_i and b_i bytes,
 * so a given element >= p never matches.
 *
 * Layouts: all arrays are text-major with the guardian inner (big-endian rows):
 *   texts  n x 2 x 512  (A, B)          shares n x k x 512  (M_i)
 *   comm   n x k x 2 x 512  (a_i, b_i)  ci, vi n x k x 32    ok (check) n x k bytes
 *   proofs n x 64  (c, v)               weights k x 32, Z k x 512 (HOST pointers in both variants)
 *
 * commit   is always constant time, like eg_trustee_decrypt_batch, and is that entry's launch: the
 *          pair comb on k_pow<F, true> for A^z and A^u with g^u from g's shared comb table as the
 *          launch's tail; it stops after the export.  Host pointers.
 * respond  v = u - c z mod q by k_response with the minus convention whatever the context's
 *          setting; the secret and the nonces pass through the branch-free mod-q helpers only.  Host
 *          pointers.  The caller must answer each nonce ONCE: two answers with one nonce give away z.
 * combine  M from the chunk body eg_prod_pow_dev runs (rows = texts, strides (k, 1), the k weights
 *          as the shared exponent vector; variable time, the weights are public), a and b from
 *          k_prod, c hashed on the device, c_i by a scalar kernel.
 * check    per (text, guardian) g^{v_i} Z_i^{c_i} (the fixed-base g term fused with a variable base,
 *          or with a cached table of Z_i when the call has at least 8192 texts and at most 8
 *          guardians), A^{v_i}, M_i^{c_i}, one multiply, the export, the compare with the given
 *          bytes and the < q flags into ok; v = SUM_i v_i per text into out_v.
 * verify   K is set under the context lock for the call; g^v K^c from the two radix tables, A^v,
 *          M^c, the device hash with the < q flags.
 *
 * Chunking.  The host variants of combine, check and verify stage through the chunked copy driver
 * with a text as the item; the _dev variants run the same chunks on the caller's device pointers
 * and only enqueue on the context stream.  A chunk holds
 *     max(1, EG_DECRYPT2_CHUNK_JOBS / (4 * k))   texts
 * (k = 1 for commit, respond and verify), 4 k being the mediator's exponentiations per text, so the
 * device memory a call holds does not grow with n.
 *
 * n == 0 returns EG_OK and touches nothing.  EG_ERR_ARG with "decrypt2" in eg_last_error(), before
 * the context is read or anything is allocated: a NULL ctx or required pointer, k == 0 or
 * k > EG_DECRYPT2_MAX_GUARDIANS, n * k > 2^24, a _dev pointer to 512- or 32-byte rows that is not
 * 16-byte aligned.
 */
#ifndef EG_HIP_DECRYPT2_H
#define EG_HIP_DECRYPT2_H

#include "eg_hip.h"

#define EG_DECRYPT2_MAX_GUARDIANS 64
#define EG_DECRYPT2_MAX_ITEMS ((size_t)1 << 24)
#define EG_DECRYPT2_CHUNK_JOBS ((size_t)1 << 16)
#define EG_DECRYPT2_TAG 0x30

#ifdef __cplusplus
extern "C" {
#endif

int eg_decrypt2_commit(eg_ctx* ctx, const uint8_t secret_be[32], const uint8_t* pads, const uint8_t* nonces,
                       size_t n, uint8_t* out_M, uint8_t* out_a, uint8_t* out_b);

int eg_decrypt2_respond(eg_ctx* ctx, const uint8_t secret_be[32], const uint8_t* nonces,
                        const uint8_t* challenges, size_t n, uint8_t* out_v);

int eg_decrypt2_combine(eg_ctx* ctx, const uint8_t K_be[512], const uint8_t qbar_be[32], size_t n, size_t k,
                        const uint8_t* weights, const uint8_t* texts, const uint8_t* shares, const uint8_t* comm,
                        uint8_t* out_M, uint8_t* out_c, uint8_t* out_ci);

int eg_decrypt2_combine_dev(eg_ctx* ctx, const uint8_t K_be[512], const uint8_t qbar_be[32], size_t n, size_t k,
                            const uint8_t* weights, const uint8_t* d_texts, const uint8_t* d_shares,
                            const uint8_t* d_comm, uint8_t* d_out_M, uint8_t* d_out_c, uint8_t* d_out_ci);

int eg_decrypt2_check(eg_ctx* ctx, size_t n, size_t k, const uint8_t* Z, const uint8_t* texts,
                      const uint8_t* shares, const uint8_t* comm, const uint8_t* ci, const uint8_t* vi,
                      uint8_t* ok, uint8_t* out_v);

int eg_decrypt2_check_dev(eg_ctx* ctx, size_t n, size_t k, const uint8_t* Z, const uint8_t* d_texts,
                          const uint8_t* d_shares, const uint8_t* d_comm, const uint8_t* d_ci, const uint8_t* d_vi,
                          uint8_t* d_ok, uint8_t* d_out_v);

int eg_decrypt2_verify(eg_ctx* ctx, const uint8_t K_be[512], const uint8_t qbar_be[32], size_t n,
                       const uint8_t* texts, const uint8_t* M, const uint8_t* proofs, uint8_t* ok);

int eg_decrypt2_verify_dev(eg_ctx* ctx, const uint8_t K_be[512], const uint8_t qbar_be[32], size_t n,
                           const uint8_t* d_texts, const uint8_t* d_M, const uint8_t* d_proofs, uint8_t* d_ok);

#ifdef __cplusplus
}
#endif
#endif /* EG_HIP_DECRYPT2_H */
