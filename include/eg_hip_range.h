/* eg_hip_range.h — disjunctive Chaum-Pedersen proofs that a ciphertext encrypts a value in
 * 0..L, made and checked in batches, in libeg_hip.so.  L = 1 is the selection proof of eg_hip.h
 * byte for byte; larger limits carry cumulative and score voting (ElectionGuard 2.0's option
 * selection limit) and a contest's "at most L" on its aggregate without placeholder selections.
 *
 * An item is a ciphertext (alpha, beta), a limit L with 1 <= L <= EG_RANGE_MAX_LIMIT, the same
 * for every item of a call, and a proof (c_0, v_0, ..., c_L, v_L).  The hash format, the response
 * convention and the pre-image order are the ctx's (eg_ctx_set_hash_format,
 * eg_ctx_set_proof_format), as for the selection proofs.  With e_j = c_j (EG_RESPONSE_MINUS) or
 * -c_j (EG_RESPONSE_PLUS):
 *
 *   verifier   a_j = g^v_j alpha^e_j,  b_j = K^v_j beta^e_j g^(-j e_j),  j = 0..L
 *              c = H(Q-bar; alpha, beta; a_0, b_0, ..., a_L, b_L)  in the ctx's pre-image order
 *              ok = 0 < alpha, beta < p,  alpha^q = beta^q = 1,  every c_j, v_j < q,
 *                   sum_j c_j = c (mod q)
 *   prover     value m <= L, encryption nonce R (alpha = g^R, beta = K^R g^m), nonces
 *              (u, c_0, v_0, ..., c_L, v_L):  a_m = g^u, b_m = K^u;  for j != m the verifier's
 *              values, a_j = g^(v_j + R e_j), b_j = K^(v_j + R e_j) g^((m - j) e_j);
 *              c_m = c - sum_{j != m} c_j,  v_m = u - c_m R (plus: u + c_m R).
 *              The supplied (c_m, v_m) is ignored, so the nonce layout does not depend on m.
 *
 * Layouts, item-major, big-endian:
 *   cts     n * 2 * 512          (alpha, beta)
 *   proofs  n * (L+1) * 2 * 32   (c_0, v_0, ..., c_L, v_L); at L = 1 the rproof layout of eg_hip.h
 *   values  n                    one byte per item
 *   R       n * 32
 *   nonces  n * (2L+3) * 32      u, c_0, v_0, ..., c_L, v_L
 *   ok      n                    flag bytes
 *
 * K is set under the ctx lock for the call (as in eg_encrypt_ballots) and Q-bar goes up per call.
 * The prover is fixed-base only and its job tables do not depend on the values: every branch is
 * computed as a simulated one, the real pair is placed with masks, and with
 * eg_ctx_set_ct_encrypt the fixed-base reads are masked scans (same bytes).  The _dev variants
 * take device pointers (K_be and qbar_be stay host pointers) and are asynchronous on the ctx
 * stream; the host variants stage items in chunks sized in exponentiation jobs, so the memory held
 * does not grow with n and shrinks per item as L grows.  n == 0 returns EG_OK and touches nothing.
 *
 * EG_ERR_ARG with "range" in eg_last_error(), before anything is allocated: a NULL ctx or
 * required pointer, limit == 0 or limit > EG_RANGE_MAX_LIMIT, a _dev pointer to 512-byte or
 * 32-byte rows (cts, proofs, R, nonces) that is not 16-byte aligned, and in eg_range_prove a
 * values[i] > limit (the message names the first such i).  eg_range_prove_dev cannot read the
 * values without a synchronisation: it writes an all-zero proof row for such an item, which
 * eg_range_verify rejects.
 */
#ifndef EG_HIP_RANGE_H
#define EG_HIP_RANGE_H

#include "eg_hip.h"

#define EG_RANGE_MAX_LIMIT 15

#ifdef __cplusplus
extern "C" {
#endif

int eg_range_prove(eg_ctx* ctx, const uint8_t K_be[EG_P_BYTES], const uint8_t qbar_be[EG_Q_BYTES], size_t n,
                   uint32_t limit, const uint8_t* cts, const uint8_t* values, const uint8_t* R,
                   const uint8_t* nonces, uint8_t* proofs);

int eg_range_prove_dev(eg_ctx* ctx, const uint8_t K_be[EG_P_BYTES], const uint8_t qbar_be[EG_Q_BYTES], size_t n,
                       uint32_t limit, const uint8_t* d_cts, const uint8_t* d_values, const uint8_t* d_R,
                       const uint8_t* d_nonces, uint8_t* d_proofs);

int eg_range_verify(eg_ctx* ctx, const uint8_t K_be[EG_P_BYTES], const uint8_t qbar_be[EG_Q_BYTES], size_t n,
                    uint32_t limit, const uint8_t* cts, const uint8_t* proofs, uint8_t* ok);

int eg_range_verify_dev(eg_ctx* ctx, const uint8_t K_be[EG_P_BYTES], const uint8_t qbar_be[EG_Q_BYTES], size_t n,
                        uint32_t limit, const uint8_t* d_cts, const uint8_t* d_proofs, uint8_t* d_ok);

#ifdef __cplusplus
}
#endif
#endif /* EG_HIP_RANGE_H */
