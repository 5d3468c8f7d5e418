/* eg_hip_codes.h — ballot nonces from one per-ballot seed, ballot hashes and the confirmation
 * (tracking) code chain of libeg_hip.so.
 *
 * H(e_0 .. e_k) is the library's hash_elems: SHA-256 of "|" + hex(e_0) + "|" + ... + "|", hex
 * upper-case and fixed width or minimal per eg_ctx_set_hash_format (read under the ctx lock), the
 * digest read big-endian and reduced mod q, 32 bytes big-endian.  "Q" elements are 32 bytes as
 * given (not range-checked, not reduced), "P" elements 512 bytes as given; no Q-bar is prefixed.
 * The upstream pre-image is unpinned, as for the proofs: these formats are the project's own.
 *
 * With s a selection's position in its ballot (0 .. nsel-1, the layout of eg_hip_manifest.h:
 * contest k owns spc[k] consecutive selections starting at off_k) and small integers 32-byte
 * big-endian:
 *   selection nonce  N_sel(xi_b, s, t) = H(Q xi_b, Q 1, Q 4s+t)    t = 0..3: R, u, c_fake, v_fake
 *   contest nonce    N_con(xi_b, k)    = H(Q xi_b, Q 2, Q k)
 *   selection hash   h_sel[b,s] = H(Q dsel[s], P alpha, P beta)
 *   contest hash     h_con[b,k] = H(Q dcon[k], Q h_sel[b,off_k], .., Q h_sel[b,off_k+spc_k-1])
 *                    (every selection of the contest, placeholders included)
 *   ballot hash      B[b]    = H(Q ballot_id[b], Q manifest_hash, Q h_con[b,0], .., Q h_con[b,nc-1])
 *   code             code[b] = H(Q code[b-1], Q ts[b], Q B[b]),  code[-1] = seed
 * dsel (nsel x 32), dcon (ncontest x 32) and manifest_hash (32) are the manifest's description
 * hashes, supplied by the caller.  Building the chain is sequential (one short hash per ballot)
 * and is the caller's; checking it is parallel and is eg_verify_code_chain.
 *
 * Conventions are those of eg_hip_manifest.h: spc is a host pointer in every variant; the _dev
 * variants take device pointers for everything else and are asynchronous on the ctx stream; the
 * host variants stage ballots in the verifier's chunks.  nballots == 0 returns EG_OK and writes
 * nothing.  EG_ERR_ARG before anything is allocated or read: a NULL required pointer, a _dev data
 * pointer that is not 16-byte aligned (the hex writer loads 16 bytes at a time; ok flags are
 * exempt), or a bad shape -- "manifest" in eg_last_error() for ncontest == 0, a spc[k] == 0 or
 * nsel > 2^20.
 */
#ifndef EG_HIP_CODES_H
#define EG_HIP_CODES_H

#include "eg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ballot_nonces nballots*32 -> sel_nonces nballots*nsel*4*32 and contest_nonces
 * nballots*ncontest*32, exactly the inputs of eg_encrypt_ballots[_manifest]. */
int eg_derive_ballot_nonces(eg_ctx* ctx, size_t nballots, size_t ncontest, const uint32_t* spc,
                            const uint8_t* ballot_nonces, uint8_t* sel_nonces, uint8_t* contest_nonces);

int eg_derive_ballot_nonces_dev(eg_ctx* ctx, size_t nballots, size_t ncontest, const uint32_t* spc,
                                const uint8_t* d_ballot_nonces, uint8_t* d_sel_nonces, uint8_t* d_contest_nonces);

/* cts nballots*nsel*2*512 and ballot_ids nballots*32 -> out_ballot_hash nballots*32, and, where
 * not NULL, out_sel_hash nballots*nsel*32 and out_contest_hash nballots*ncontest*32. */
int eg_ballot_hashes(eg_ctx* ctx, size_t nballots, size_t ncontest, const uint32_t* spc, const uint8_t* dsel,
                     const uint8_t* dcon, const uint8_t manifest_hash[EG_Q_BYTES], const uint8_t* ballot_ids,
                     const uint8_t* cts, uint8_t* out_ballot_hash, uint8_t* out_sel_hash, uint8_t* out_contest_hash);

int eg_ballot_hashes_dev(eg_ctx* ctx, size_t nballots, size_t ncontest, const uint32_t* spc, const uint8_t* d_dsel,
                         const uint8_t* d_dcon, const uint8_t* d_manifest_hash, const uint8_t* d_ballot_ids,
                         const uint8_t* d_cts, uint8_t* d_out_ballot_hash, uint8_t* d_out_sel_hash,
                         uint8_t* d_out_contest_hash);

/* ok[b] = (codes[b] == H(codes[b-1] or seed, timestamps[b], ballot_hashes[b])): seed 32 bytes,
 * the three arrays nballots*32, ok nballots.  A broken link fails the ballot that holds it. */
int eg_verify_code_chain(eg_ctx* ctx, size_t nballots, const uint8_t seed[EG_Q_BYTES], const uint8_t* timestamps,
                         const uint8_t* ballot_hashes, const uint8_t* codes, uint8_t* ok);

int eg_verify_code_chain_dev(eg_ctx* ctx, size_t nballots, const uint8_t* d_seed, const uint8_t* d_timestamps,
                             const uint8_t* d_ballot_hashes, const uint8_t* d_codes, uint8_t* d_ok);

#ifdef __cplusplus
}
#endif
#endif /* EG_HIP_CODES_H */
