/* eg_hip_codes2.h — ballot nonces from one per-ballot seed and the opening of challenged ballots
 * for the ballots without placeholder selections of eg_hip_ballot2.h, in libeg_hip.so.
 *
 * H is eg_hip_codes.h's hash_elems (the ctx's hash format, no Q-bar prefix, small integers 32 bytes
 * big-endian); the manifest (nsel, olimit, climit: three uint32_t HOST arrays in every variant) and
 * the row counts NS, SN, CN with sn_off and cn_off are eg_hip_ballot2.h's.  With xi_b a ballot's
 * 32-byte seed (tags 1..4 are eg_hip_codes.h's, eg_hip_contestdata.h's and eg_hip_preencrypt.h's):
 *   sel_nonces[b, r]     = H(Q xi_b, Q 5, Q r)    0 <= r < SN
 *   contest_nonces[b, r] = H(Q xi_b, Q 6, Q r)    0 <= r < CN
 * exactly the inputs of eg_encrypt_ballots_v2: every row is a hash output and so below q.  The R of
 * selection i of contest k is row sn_off[k] + i (2 olimit[k] + 4) of its ballot's sel_nonces.
 *
 * Ballot hashes and the code chain need no entry point of their own: eg_ballot_hashes with
 * spc = nsel hashes a placeholder-free ballot (the proofs do not enter the hashes), and
 * eg_verify_code_chain checks the chain.
 *
 * Opening.  For selection s of contest k of ballot b, R re-derived from xi_b:
 *   ok[b, s]    = (alpha == g^R) and (beta == K^R g^m for one m in 0..olimit[k])
 *   votes[b, s] = that m where ok, else 0
 * An alpha or a beta of 0, of p or more, or matching no m gives ok = 0.  g^R and K^R are the
 * fixed-base batch path's, K set under the ctx lock, and follow eg_ctx_set_ct_pow; the match costs
 * at most olimit[k] <= EG_RANGE_MAX_LIMIT multiplies, no inverse, and nothing is compared on the host.
 *
 * Layouts, ballot-major, big-endian:
 *   ballot_nonces   nb * 32
 *   sel_nonces      nb * SN * 32
 *   contest_nonces  nb * CN * 32
 *   cts             nb * NS * 2 * 512    (alpha, beta)
 *   votes           nb * NS              one byte per selection
 *   ok              nb * NS              flag bytes
 *
 * The _dev variants take device pointers for the data (K_be and the three shape arrays stay host
 * pointers), are asynchronous on the ctx stream and read no ballot byte on the host.
 * eg_derive_ballot_nonces_v2_dev is one launch over the batch and refuses a batch it cannot index
 * (as eg_derive_ballot_nonces_dev does); the host variants stage, and eg_open_ballots_v2_dev runs,
 * in eg_hip_ballot2.h's chunks of max(1, 2^16 / J) ballots.  nballots == 0 returns EG_OK and
 * touches nothing.
 *
 * EG_ERR_ARG with "ballot2" in eg_last_error(), before anything is allocated or any ballot byte
 * read, on eg_hip_ballot2.h's conditions: a NULL ctx or required pointer, ncontest == 0,
 * nsel[k] == 0, a limit outside 1..EG_RANGE_MAX_LIMIT, NS > 2^20, J > 2^16, a _dev data pointer
 * that is not 16-byte aligned (votes and ok, single bytes, are exempt).
 */
#ifndef EG_HIP_CODES2_H
#define EG_HIP_CODES2_H

#include "eg_hip_ballot2.h"

#ifdef __cplusplus
extern "C" {
#endif

int eg_derive_ballot_nonces_v2(eg_ctx* ctx, size_t nballots, size_t ncontest, const uint32_t* nsel,
                               const uint32_t* olimit, const uint32_t* climit, const uint8_t* ballot_nonces,
                               uint8_t* sel_nonces, uint8_t* contest_nonces);

int eg_derive_ballot_nonces_v2_dev(eg_ctx* ctx, size_t nballots, size_t ncontest, const uint32_t* nsel,
                                   const uint32_t* olimit, const uint32_t* climit, const uint8_t* d_ballot_nonces,
                                   uint8_t* d_sel_nonces, uint8_t* d_contest_nonces);

int eg_open_ballots_v2(eg_ctx* ctx, const uint8_t K_be[EG_P_BYTES], size_t nballots, size_t ncontest,
                       const uint32_t* nsel, const uint32_t* olimit, const uint32_t* climit,
                       const uint8_t* ballot_nonces, const uint8_t* cts, uint8_t* votes, uint8_t* ok);

int eg_open_ballots_v2_dev(eg_ctx* ctx, const uint8_t K_be[EG_P_BYTES], size_t nballots, size_t ncontest,
                           const uint32_t* nsel, const uint32_t* olimit, const uint32_t* climit,
                           const uint8_t* d_ballot_nonces, const uint8_t* d_cts, uint8_t* d_votes, uint8_t* d_ok);

#ifdef __cplusplus
}
#endif
#endif /* EG_HIP_CODES2_H */
