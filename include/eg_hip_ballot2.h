/* eg_hip_ballot2.h — ballots without placeholder selections (the ElectionGuard 2.0 form),
 * encrypted, verified and tallied in batches, in libeg_hip.so.  Every selection carries a 0..L
 * range proof (eg_hip_range.h) at its contest's option limit, every contest one on its aggregate
 * at the contest limit; there is no padding and no constant proof, so cumulative and score voting,
 * undervotes and empty contests are all plain ballots.
 *
 * A manifest is ncontest triples, one per contest k, in three uint32_t HOST arrays (host pointers
 * in every variant):
 *   nsel[k]    selections; all are real and all enter the tally
 *   olimit[k]  the most one selection may hold   (1 .. EG_RANGE_MAX_LIMIT)
 *   climit[k]  the most the contest may hold     (1 .. EG_RANGE_MAX_LIMIT)
 * NS = sum nsel[k], first[k] = sum_{k' < k} nsel[k'].  Four per-ballot row counts follow:
 *   SP = sum nsel[k] (olimit[k] + 1)      selection proof pairs (c_j, v_j), 64 B each;
 *        selection i of contest k starts at sp_off[k] + i (olimit[k] + 1),
 *        sp_off[k] = sum_{k' < k} nsel[k'] (olimit[k'] + 1)
 *   SN = sum nsel[k] (2 olimit[k] + 4)    selection nonce rows, 32 B each;
 *        selection i of contest k starts at sn_off[k] + i (2 olimit[k] + 4),
 *        sn_off[k] = sum_{k' < k} nsel[k'] (2 olimit[k'] + 4); its rows are R, then the range
 *        prover's u, c_0, v_0, ..., c_L, v_L
 *   CP = sum (climit[k] + 1)              contest proof pairs, 64 B each; contest k starts at
 *        cp_off[k] = sum_{k' < k} (climit[k'] + 1)
 *   CN = sum (2 climit[k] + 3)            contest nonce rows, 32 B each; contest k starts at
 *        cn_off[k] = sum_{k' < k} (2 climit[k'] + 3); its rows are the range prover's
 *
 * Layouts, ballot-major, big-endian:
 *   votes           nb * NS              one byte per selection
 *   sel_nonces      nb * SN * 32
 *   contest_nonces  nb * CN * 32
 *   cts             nb * NS * 2 * 512    (alpha, beta)
 *   sproof          nb * SP * 64
 *   cproof          nb * CP * 64
 *   cast            nb                   flag bytes, may be NULL (every ballot is cast)
 *   ok_sel          nb * NS              flag bytes
 *   ok_contest      nb * ncontest        flag bytes
 *   tally_be        NS * 2 * 512         may be NULL
 *
 * Every row of sel_nonces and contest_nonces is a scalar below q, as the nonces of
 * eg_encrypt_ballots and eg_range_prove are: the calls do not check or reduce them (sum R is a
 * chain of modular additions of reduced operands), and a row of q or more gives unspecified proofs.
 *
 * The hash format, the response sign and the pre-image order are the ctx's, eg_ctx_set_ct_encrypt
 * applies to the encryptor and K is set under the ctx lock for the call, all as in the range
 * (eg_hip_range.h) and manifest (eg_hip_manifest.h) calls.
 *
 * Encryptor.  For selection s of contest k with vote byte m and first nonce row R:
 *   alpha = g^R, beta = K^R g^m, for any byte m;
 *   the selection's proof is exactly eg_range_prove's for ((alpha, beta), m, R, its 2L+3 further
 *   rows) at L = olimit[k];
 *   the contest's proof is eg_range_prove's at L = climit[k] for the aggregate
 *   (A, B) = (prod alpha, prod beta) mod p over the contest's selections, the value M = sum m as
 *   an integer, the nonce sum R mod q and the contest's rows as the nonces.
 *   eg_encrypt_ballots_v2: a vote above olimit[k] or a sum above climit[k] is EG_ERR_ARG before
 *   anything is allocated; the message names the first such ballot and contest, and the selection
 *   when a vote is the cause.  eg_encrypt_ballots_v2_dev cannot read the votes without a
 *   synchronisation: it writes all-zero proof rows for that selection or that contest, as
 *   eg_range_prove_dev does; the ciphertexts are written as defined.
 *
 * Verifier.
 *   ok_sel[b, s]      eg_range_verify's verdict of (cts[b, s], its proof) at olimit[k]
 *   ok_contest[b, k]  eg_range_verify's verdict of the aggregate with the contest's proof at
 *                     climit[k], AND every selection of the contest has 0 < alpha, beta < p and
 *                     alpha^q = beta^q = 1 (eg_hip.h's rule for the contest verdict: the message
 *                     is decided from its selections)
 *   tally_be[s]       the product over the ballots with cast[b] != 0 of cts[b, s], whatever the
 *                     verdicts, combined across chunks; all ones when no ballot is cast.
 *   nballots == 0 touches nothing else.
 *
 * The _dev variants take device pointers for the data (K_be, qbar_be and the three shape arrays
 * stay host pointers) and are asynchronous on the ctx stream.  Ballots run in chunks of
 * max(1, 2^16 / J) ballots, J = sum (2 olimit[k] nsel[k] + 2 climit[k]) being one ballot's
 * verifier jobs; the host variants stage one chunk at a time.
 *
 * EG_ERR_ARG with "ballot2" in eg_last_error(), before anything is allocated or any ballot byte
 * read: a NULL ctx or required pointer, ncontest == 0, nsel[k] == 0, a limit outside
 * 1..EG_RANGE_MAX_LIMIT, NS > 2^20, J > 2^16 (one ballot is then always at most one chunk; as
 * J >= 2 NS this is the bound a wide ballot meets first), a
 * _dev data pointer that is not 16-byte aligned.
 */
#ifndef EG_HIP_BALLOT2_H
#define EG_HIP_BALLOT2_H

#include "eg_hip_range.h"

#ifdef __cplusplus
extern "C" {
#endif

int eg_encrypt_ballots_v2(eg_ctx* ctx, const uint8_t K_be[EG_P_BYTES], const uint8_t qbar_be[EG_Q_BYTES],
                          size_t nballots, size_t ncontest, const uint32_t* nsel, const uint32_t* olimit,
                          const uint32_t* climit, const uint8_t* votes, const uint8_t* sel_nonces,
                          const uint8_t* contest_nonces, uint8_t* cts, uint8_t* sproof, uint8_t* cproof);

int eg_encrypt_ballots_v2_dev(eg_ctx* ctx, const uint8_t K_be[EG_P_BYTES], const uint8_t qbar_be[EG_Q_BYTES],
                              size_t nballots, size_t ncontest, const uint32_t* nsel, const uint32_t* olimit,
                              const uint32_t* climit, const uint8_t* d_votes, const uint8_t* d_sel_nonces,
                              const uint8_t* d_contest_nonces, uint8_t* d_cts, uint8_t* d_sproof, uint8_t* d_cproof);

int eg_verify_ballots_v2(eg_ctx* ctx, const uint8_t K_be[EG_P_BYTES], const uint8_t qbar_be[EG_Q_BYTES],
                         size_t nballots, size_t ncontest, const uint32_t* nsel, const uint32_t* olimit,
                         const uint32_t* climit, const uint8_t* cts, const uint8_t* sproof, const uint8_t* cproof,
                         const uint8_t* cast, uint8_t* ok_sel, uint8_t* ok_contest, uint8_t* tally_be);

int eg_verify_ballots_v2_dev(eg_ctx* ctx, const uint8_t K_be[EG_P_BYTES], const uint8_t qbar_be[EG_Q_BYTES],
                             size_t nballots, size_t ncontest, const uint32_t* nsel, const uint32_t* olimit,
                             const uint32_t* climit, const uint8_t* d_cts, const uint8_t* d_sproof,
                             const uint8_t* d_cproof, const uint8_t* d_cast, uint8_t* d_ok_sel, uint8_t* d_ok_contest,
                             uint8_t* d_tally_be);

#ifdef __cplusplus
}
#endif
#endif /* EG_HIP_BALLOT2_H */
