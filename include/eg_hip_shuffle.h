/* eg_hip_shuffle.h — a verifiable re-encryption shuffle of ciphertext rows, in libeg_hip.so
 * (DESIGN.md §19): a mixer permutes and re-encrypts the rows of a ballot table and publishes a proof
 * that anyone can check.  The proof is Terelius-Wikstrom's, in the form of Haenni et al.'s
 * pseudo-code, for rows of width w; the definitions are the library's own.
 *
 * Rows of width w: E is (N, w, 2, 512) holding alpha[i,j], beta[i,j], exactly the cts array of the
 * placeholder-free ballots (eg_hip_ballot2.h); viewed as (N, 2w, 512) it is eg_prod_pow's "terms"
 * layout.  psi is a permutation of 0..N-1 as N uint32, r is (N, w, 32) nonces, K the election key.
 * All indices are 0-based.
 *
 * H is the library's hash_elems: SHA-256 over "|hex|hex|...|" reduced mod q, the hex format the
 * context's (eg_ctx_set_hash_format).  Q elements are 32 bytes, P elements 512; "Q 0x40" is the
 * scalar 0x40.  eg_ctx_set_proof_format does NOT apply: the plus response and the pre-image orders
 * below are FIXED.  Elements given are hashed as the bytes given, elements computed in canonical form.
 *
 *   mix          alpha'[i,j] = alpha[psi(i),j] * g^{r[i,j] mod q}
 *                beta'[i,j]  = beta[psi(i),j]  * K^{r[i,j] mod q}
 *   generators   gen(k) = X_k^cof mod p with cof = (p - 1) / q;  X_k is the 4096-bit big-endian
 *                concatenation D[k,0] || ... || D[k,15];  D[k,t] is the RAW SHA-256 digest (not
 *                reduced mod q) of the pre-image "|hex|hex|hex|hex|" of (Q gseed, Q 0x43, Q k, Q t).
 *                h = gen(0), h_i = gen(i + 1).  G is (N + 2, 512): h, h_0 .. h_{N-1}, then PROD_i h_i.
 *   tagged hashes  leaf(x_0 .. x_{m-1}) = H(Q 0x40, P x_0, ..., P x_{m-1})
 *                T(v_0 .. v_{n-1}) = H(Q 0x41, Q n, Q v_0, ..., Q v_{n-1}) for n <= 256; for larger n, T of
 *                the Ts of consecutive chunks of 256 (the last may be shorter).  T_rows(A) = T of the
 *                leaves of A's rows.
 *   nonces       (4 N + 3 + w, 32) rows in the order rho, rho^, omega^, omega' (N each), omega1, omega2,
 *                omega3, omega4[0..w-1], each reduced mod q on use.  ONE proof per set of nonces.
 *   prover       pc[psi(i)] = g^{rho[psi(i)]} h_i                     (the permutation commitment)
 *                y = H(Q qbar, Q 0x42, Q N, Q w, P K, Q gseed, Q T_rows(E), Q T_rows(E'), Q T_rows(pc))
 *                u_j = H(Q y, Q 0x44, Q j),  u'_i = u_{psi(i)}
 *                R_{-1} = 0, U_{-1} = 1;  R_i = rho^_i + u'_i R_{i-1},  U_i = u'_i U_{i-1}  (mod q)
 *                chain_i = g^{R_i} h^{U_i}  ( = g^{rho^_i} chain_{i-1}^{u'_i} with chain_{-1} = h)
 *                rbar = SUM rho_j, rhat = R_{N-1}, rtilde = SUM rho_j u_j, r*_j = SUM_i r[i,j] u'_i
 *                t1 = g^{omega1}, t2 = g^{omega2}, t3 = g^{omega3} PROD_i h_i^{omega'_i}
 *                t4_j = (g^{-omega4_j} PROD_i alpha'[i,j]^{omega'_i}, K^{-omega4_j} PROD_i beta'[i,j]^{omega'_i})
 *                that_i = g^{omega^_i} chain_{i-1}^{omega'_i}
 *                c = H(Q y, Q 0x45, P t1, P t2, P t3, Q T_rows(t4), Q T_rows(that), Q T_rows(chain))
 *                s1 = omega1 + c rbar, s2 = omega2 + c rhat, s3 = omega3 + c rtilde, s4_j = omega4_j + c r*_j,
 *                s^_i = omega^_i + c rho^_i, s'_i = omega'_i + c u'_i  (mod q);  -e is (q - e) mod q
 *   published    pc (N, 512), chain (N, 512), c (32), s (3 + w, 32), s^ (N, 32), s' (N, 32): no t value
 *   verifier     y, u, U = PROD u_j;  cbar = PROD pc_j (PROD h_i)^-1,  chat = chain_{N-1} h^{-U},
 *                ctilde = PROD pc_j^{u_j},  etilde_j = (PROD_k alpha[k,j]^{u_k}, PROD_k beta[k,j]^{u_k})
 *                t1' = cbar^{-c} g^{s1},  t2' = chat^{-c} g^{s2},  t3' = ctilde^{-c} g^{s3} PROD h_i^{s'_i}
 *                t4'_j = (etilde_j.a^{-c} g^{-s4_j} PROD alpha'[i,j]^{s'_i}, etilde_j.b^{-c} K^{-s4_j} PROD beta'[i,j]^{s'_i})
 *                that'_i = chain_i^{-c} g^{s^_i} chain_{i-1}^{s'_i}
 *                accepts iff (1) RANGE: c and every response are < q; (2) RESIDUE: every element of
 *                E', pc and chain is in (0, p) with x^q = 1, with check_inputs also every element of E
 *                (inverting by q - e is sound only after this test); (3) CHALLENGE: the challenge
 *                hashed from the t' values equals c.  All three tests are always made; ok is 1 iff
 *                none failed, failed_mask names which did (EG_SHUFFLE_FAILED_*).  The recomputation
 *                reduces the responses mod q.
 *
 * BigInteger semantics as everywhere in the library: bases are reduced mod p, outputs are canonical.
 * The mix's nonces are reduced mod q before they are used as exponents.
 *
 * eg_shuffle_generators  cof is an argument (512 big-endian bytes, a HOST pointer in both
 *          variants, like gseed, K and qbar everywhere): it is refused with EG_ERR_ARG unless
 *          cof * q + 1 == p, checked by a host schoolbook multiply.  The power is one k_pow launch over
 *          the N + 1 bases with the shared 512-byte exponent, the path eg_multinv_batch's a^(p-2)
 *          takes; the last row is one product tree.  A generator that is 0 or 1 gives EG_ERR_STATE:
 *          both variants read one flag word back for it (as eg_all_nonzero_dev does), after G is
 *          written.
 * eg_shuffle_mix  g^r and K^r from the two radix tables (K is set under the context lock for the
 *          call), then one gather-multiply out_i = in[psi(i)] * x_i in Montgomery form.
 * eg_shuffle_prove  g^. and K^. from the radix tables; h^{U_i} with h as a shared variable base of
 *          the chain's jobs; the products over N by eg_prod_pow's chunk body; the recurrence by a
 *          levelled scan of affine maps; every hash on the device.
 * eg_shuffle_verify  x^q by k_pow with q as a shared exponent for the residue test, the rest as the
 *          prover's.  ok is one byte, failed_mask one uint32 (device pointers in the _dev variant).
 *
 * Every product of the proof runs over all N rows, so the host variants upload the WHOLE arrays,
 * run the body of the _dev variant and download the outputs: they do not use the chunked
 * staging driver.  The limits below bound the memory a call holds (2 GiB per ciphertext array).
 * The _dev variants only enqueue on the context stream (generators' flag word apart); they read no
 * exponent, permutation or hash on the host.
 *
 * Constant time.  mix and prove read their nonces through the variable-time radix tables and
 * eg_prod_pow's chunk body, as the default encryption does; while eg_ctx_set_ct_pow is on they
 * return EG_ERR_STATE ("variable time") and write nothing.  generators and verify work on public
 * values and run either way.  A constant-time prover is out of scope.  The permutation's memory
 * addresses are NOT hidden either: the gathers read row psi(i) at an address that depends on psi.
 *
 * EG_ERR_ARG with "shuffle" in eg_last_error(), before the context is read or anything is
 * allocated: a NULL ctx or pointer; N == 0 or N > EG_SHUFFLE_MAX_ROWS; w == 0 or
 * N * w > EG_SHUFFLE_MAX_CELLS; a _dev pointer that is not 16-byte aligned; a cof with
 * cof * q + 1 != p (after the context's p and q are read).  The HOST variants of mix and prove also
 * refuse a psi with an entry >= N or a repeated entry.  The _dev variants TRUSTS psi (they cannot
 * look without reading it on the host): an entry >= N is read as N - 1 there, so no address leaves
 * the arrays, and a proof of such a mix does not verify.
 */
#ifndef EG_HIP_SHUFFLE_H
#define EG_HIP_SHUFFLE_H

#include "eg_hip.h"

#define EG_SHUFFLE_MAX_ROWS ((size_t)1 << 20)
#define EG_SHUFFLE_MAX_CELLS ((size_t)1 << 21)
#define EG_SHUFFLE_TAG_LEAF 0x40
#define EG_SHUFFLE_TAG_NODE 0x41
#define EG_SHUFFLE_TAG_SEED 0x42
#define EG_SHUFFLE_TAG_GENERATOR 0x43
#define EG_SHUFFLE_TAG_U 0x44
#define EG_SHUFFLE_TAG_CHALLENGE 0x45
#define EG_SHUFFLE_FAILED_RANGE 1u
#define EG_SHUFFLE_FAILED_RESIDUE 2u
#define EG_SHUFFLE_FAILED_CHALLENGE 4u

#ifdef __cplusplus
extern "C" {
#endif

int eg_shuffle_generators(eg_ctx* ctx, const uint8_t cof_be[512], const uint8_t gseed_be[32], size_t N, uint8_t* G);

int eg_shuffle_generators_dev(eg_ctx* ctx, const uint8_t cof_be[512], const uint8_t gseed_be[32], size_t N,
                              uint8_t* d_G);

int eg_shuffle_mix(eg_ctx* ctx, const uint8_t K_be[512], size_t N, size_t w, const uint8_t* E, const uint32_t* psi,
                   const uint8_t* r, uint8_t* E2);

int eg_shuffle_mix_dev(eg_ctx* ctx, const uint8_t K_be[512], size_t N, size_t w, const uint8_t* d_E,
                       const uint32_t* d_psi, const uint8_t* d_r, uint8_t* d_E2);

int eg_shuffle_prove(eg_ctx* ctx, const uint8_t K_be[512], const uint8_t qbar_be[32], const uint8_t gseed_be[32],
                     size_t N, size_t w, const uint8_t* G, const uint8_t* E, const uint8_t* E2, const uint32_t* psi,
                     const uint8_t* r, const uint8_t* nonces, uint8_t* pc, uint8_t* chain, uint8_t* c, uint8_t* s,
                     uint8_t* s_hat, uint8_t* s_prime);

int eg_shuffle_prove_dev(eg_ctx* ctx, const uint8_t K_be[512], const uint8_t qbar_be[32], const uint8_t gseed_be[32],
                         size_t N, size_t w, const uint8_t* d_G, const uint8_t* d_E, const uint8_t* d_E2,
                         const uint32_t* d_psi, const uint8_t* d_r, const uint8_t* d_nonces, uint8_t* d_pc,
                         uint8_t* d_chain, uint8_t* d_c, uint8_t* d_s, uint8_t* d_s_hat, uint8_t* d_s_prime);

int eg_shuffle_verify(eg_ctx* ctx, const uint8_t K_be[512], const uint8_t qbar_be[32], const uint8_t gseed_be[32],
                      size_t N, size_t w, const uint8_t* G, const uint8_t* E, const uint8_t* E2, const uint8_t* pc,
                      const uint8_t* chain, const uint8_t* c, const uint8_t* s, const uint8_t* s_hat,
                      const uint8_t* s_prime, int check_inputs, uint8_t* ok, uint32_t* failed_mask);

int eg_shuffle_verify_dev(eg_ctx* ctx, const uint8_t K_be[512], const uint8_t qbar_be[32], const uint8_t gseed_be[32],
                          size_t N, size_t w, const uint8_t* d_G, const uint8_t* d_E, const uint8_t* d_E2,
                          const uint8_t* d_pc, const uint8_t* d_chain, const uint8_t* d_c, const uint8_t* d_s,
                          const uint8_t* d_s_hat, const uint8_t* d_s_prime, int check_inputs, uint8_t* d_ok,
                          uint32_t* d_failed_mask);

#ifdef __cplusplus
}
#endif
#endif /* EG_HIP_SHUFFLE_H */
