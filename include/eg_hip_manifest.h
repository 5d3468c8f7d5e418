/* eg_hip_manifest.h — ballot entry points of libeg_hip.so for manifests whose contests differ in
 * size (a vote-for-1 race among 3, a vote-for-3 board race among 8, a yes/no measure on one
 * ballot).  The entry points of eg_hip.h take one (spc, placeholders, limit) triple for every
 * contest; these take one per contest.
 *
 * Contest k owns spc[k] consecutive selections, placeholders[k] of them last and kept out of the
 * tally, and its constant (selection-limit) proof uses limit[k]:
 *   nsel = sum spc[k],  nreal = sum (spc[k] - placeholders[k]).
 * Layouts are those of the uniform calls, ballot-major, with nsel / ncontest / nreal taken from
 * the arrays:
 *   cts nballots*nsel*2*512, rproof nballots*nsel*4*32, cproof nballots*ncontest*2*32,
 *   ok_sel nballots*nsel, ok_contest nballots*ncontest, tally_be nreal*2*512 (contest-major).
 * Everything else is as in the uniform call of the same name: the key is set under the ctx lock,
 * cast (may be NULL) masks ballots out of the tally, nballots == 0 gives an all-ones tally, a
 * contest is rejected when one of its selections is out of range or a non-residue, the hash and
 * proof format switches and constant-time encryption apply, and ballots run in the same chunks.
 *
 * EG_ERR_ARG with "manifest" in eg_last_error(), before anything is allocated or any ballot byte
 * read: ncontest == 0, a spc[k] == 0, a placeholders[k] >= spc[k], a limit[k] > spc[k], or
 * nsel > 2^20.  The three shape arrays are host pointers in every variant.
 */
#ifndef EG_HIP_MANIFEST_H
#define EG_HIP_MANIFEST_H

#include "eg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int eg_verify_ballots_manifest(eg_ctx* ctx, const uint8_t K_be[EG_P_BYTES], const uint8_t qbar_be[EG_Q_BYTES],
                               size_t nballots, size_t ncontest, const uint32_t* spc, const uint32_t* placeholders,
                               const uint32_t* limit, const uint8_t* cts, const uint8_t* rproof,
                               const uint8_t* cproof, const uint8_t* cast, uint8_t* ok_sel, uint8_t* ok_contest,
                               uint8_t* tally_be);

/* Same, device pointers for the ballot data and the outputs (d_cast and d_tally_be may be NULL),
 * asynchronous on the ctx stream. */
int eg_verify_ballots_manifest_dev(eg_ctx* ctx, const uint8_t K_be[EG_P_BYTES], const uint8_t qbar_be[EG_Q_BYTES],
                                   size_t nballots, size_t ncontest, const uint32_t* spc,
                                   const uint32_t* placeholders, const uint32_t* limit, const uint8_t* d_cts,
                                   const uint8_t* d_rproof, const uint8_t* d_cproof, const uint8_t* d_cast,
                                   uint8_t* d_ok_sel, uint8_t* d_ok_contest, uint8_t* d_tally_be);

/* Encryption with injected nonces: votes nballots*nsel, sel_nonces nballots*nsel*4*32 (R, u, c_fake,
 * v_fake), contest_nonces nballots*ncontest*32; outputs in the verifier's layout. */
int eg_encrypt_ballots_manifest(eg_ctx* ctx, const uint8_t K_be[EG_P_BYTES], const uint8_t qbar_be[EG_Q_BYTES],
                                size_t nballots, size_t ncontest, const uint32_t* spc, const uint8_t* votes,
                                const uint8_t* sel_nonces, const uint8_t* contest_nonces, uint8_t* cts,
                                uint8_t* rproof, uint8_t* cproof);

/* Same, device pointers for the ballot data and the outputs. */
int eg_encrypt_ballots_manifest_dev(eg_ctx* ctx, const uint8_t K_be[EG_P_BYTES], const uint8_t qbar_be[EG_Q_BYTES],
                                    size_t nballots, size_t ncontest, const uint32_t* spc, const uint8_t* d_votes,
                                    const uint8_t* d_sel_nonces, const uint8_t* d_contest_nonces, uint8_t* d_cts,
                                    uint8_t* d_rproof, uint8_t* d_cproof);

#ifdef __cplusplus
}
#endif
#endif /* EG_HIP_MANIFEST_H */
