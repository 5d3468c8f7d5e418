/* eg_hip_preencrypt.h — pre-encrypted (print-at-home, vote-by-mail) ballots of libeg_hip.so:
 * making them before anyone votes, recording a returned ballot from the marked codes, and the
 * pre-encryption check of a recorded ballot.
 *
 * H, "Q" and "P" elements, the hash format, dcon, manifest_hash, ballot_id and the manifest
 * layout are those of eg_hip_codes.h and eg_hip_manifest.h: contest k owns spc_k = m_k + limit_k
 * consecutive slots from off_k, the real selections first, then limit_k placeholders;
 * nsel = sum spc_k.  Small integers are 32-byte big-endian; xi_b is ballot b's seed (the
 * ballot_nonces of eg_hip_codes.h).  The upstream pre-images are unpinned: these are the
 * project's own.
 *
 * Contest k has spc_k selection vectors of spc_k components.  Vector i < m_k is the choice
 * "selection i", vector i >= m_k the null vector i - m_k (the unused vote that sets placeholder
 * i - m_k); vector i encrypts the unit vector e_i over the contest's slots.  Per ballot there are
 * V = sum spc_k^2 component ciphertexts, voff_k = sum_{k' < k} spc_k'^2:
 *   component index    w(k,i,j) = voff_k + i spc_k + j
 *   component nonce    rho[b,w] = H(Q xi_b, Q 4, Q w)       (tags 1, 2, 3: eg_hip_codes.h, eg_hip_contestdata.h)
 *   component          alpha = g^rho,  beta = K^rho g^[i = j]
 *   component hash     e[b,w] = H(P alpha, P beta)
 *   vector hash        psi[b,k,i] = H(Q dcon[k], Q e[b,w(k,i,0)], .., Q e[b,w(k,i,spc_k-1)])
 *   short code         Omega(psi) = the last code_bytes bytes of psi as an unsigned integer, code_bytes in 1..4
 *   sorted list        the contest's spc_k vector hashes ascending as 256-bit integers, ties to the
 *                      lower i; perm[b, off_k + r] is the vector at rank r
 *   unique             unique[b] = 1 iff no contest of the ballot has two vectors with the same
 *                      short code (the caller re-seeds a ballot with 0)
 *   contest hash       chi[b,k] = H(Q dcon[k], Q sorted[b,off_k], .., Q sorted[b,off_k+spc_k-1])
 *   confirmation hash  C[b] = H(Q ballot_id[b], Q manifest_hash, Q chi[b,0], .., Q chi[b,nc-1]);
 *                      it enters eg_verify_code_chain where the ballot hash B[b] does
 *
 * Recording.  votes (nballots, nsel) is the encryptor's input: slot off_k + i set means "vector i
 * of contest k was chosen", null vectors included, and every contest sums to limit_k.  The
 * recorded ballot's encryption nonce of slot off_k + j is R' = sum_{i chosen} rho[b, w(k,i,j)]
 * mod q; its proof nonces and contest nonce are eg_hip_codes.h's N_sel(xi_b, s, 1..3) and
 * N_con(xi_b, k).  sel_nonces and contest_nonces come out in the encryptor's layout, so
 * eg_encrypt_ballots_manifest[_dev] on the same votes yields the ballot: the slot-wise product of
 * the chosen vectors equals its ciphertexts byte for byte.  Published per contest: the sorted
 * list, the limit_k chosen vectors in ascending rank (index order would tie public ranks to
 * private choices), and each one's rank and short code.  With S = sum limit_k spc_k and
 * T = sum limit_k (soff_k, toff_k the contest's first), chosen vector t of contest k is rows
 * soff_k + t spc_k .. of sel_vecs and entry toff_k + t of sel_rank / sel_codes.
 *
 * Verdict of the pre-encryption check, per (ballot, contest): every element of the chosen vectors
 * is in [1, p); ranks are < spc_k and strictly ascending; the sorted list is strictly ascending;
 * psi recomputed from each chosen vector equals sorted[rank]; each recorded short code equals
 * Omega(psi); for every slot j the products of the chosen vectors' alpha_j and beta_j equal the
 * ballot's (alpha, beta) at off_k + j.  Per ballot: C[b] recomputed from the sorted lists equals
 * the recorded one.  The ballot's own proofs remain eg_verify_ballots_manifest's.
 *
 * Conventions are eg_hip_codes.h's: spc and limits are host pointers in every variant; the _dev
 * variants take device pointers for everything else and are asynchronous on the ctx stream;
 * 512- and 32-byte rows of the _dev variants are 16-byte aligned (u32 rows and flags are exempt);
 * nballots == 0 returns EG_OK and writes nothing.  K is set under the ctx lock for the call.  The
 * exponentiations are the encryptor's fixed-base jobs, so eg_ctx_set_ct_encrypt gives masked scans
 * and the same bytes (rho reveals the vote).  Work is chunked by component ciphertexts:
 * max(1, EG_PRE_CHUNK_CTS / V) ballots per chunk (record and verify: / S), and the host variants
 * stage one chunk at a time.
 *
 * EG_ERR_ARG with "preencrypt" in eg_last_error(), before anything is allocated: a NULL ctx or
 * required pointer, ncontest == 0, a spc[k] == 0 or > EG_PRE_MAX_SPC, a limits[k] == 0 or
 * > spc[k], code_bytes outside 1..4, more than 2^20 slots or 2^22 component ciphertexts per
 * ballot, or a misaligned _dev row pointer.  Votes are data: a contest whose votes do not sum to
 * its limit, hold a value above 1, or whose chosen psi is not in `sorted` gets ok = 0 and
 * unspecified rows; the other contests of the ballot are unaffected.
 */
#ifndef EG_HIP_PREENCRYPT_H
#define EG_HIP_PREENCRYPT_H

#include "eg_hip.h"

#define EG_PRE_MAX_SPC 64
/* component ciphertexts per chunk: one fixed-base launch of 2^18 two-output jobs (the encryptor's
 * per-launch job bound), about 0.6 GB of workspace */
#define EG_PRE_CHUNK_CTS (1u << 18)

#ifdef __cplusplus
extern "C" {
#endif

/* ballot_ids, ballot_nonces nballots*32 -> sorted nballots*nsel*32, perm and codes nballots*nsel
 * u32, unique nballots, conf nballots*32 and, where not NULL, chash nballots*ncontest*32 and
 * vec_cts nballots*V*2*512 (without it the ciphertexts live in workspace only). */
int eg_preencrypt_ballots(eg_ctx* ctx, const uint8_t K_be[EG_P_BYTES], size_t nballots, size_t ncontest,
                          const uint32_t* spc, uint32_t code_bytes, const uint8_t* dcon,
                          const uint8_t manifest_hash[EG_Q_BYTES], const uint8_t* ballot_ids,
                          const uint8_t* ballot_nonces, uint8_t* sorted, uint32_t* perm, uint32_t* codes,
                          uint8_t* unique, uint8_t* conf, uint8_t* chash, uint8_t* vec_cts);

int eg_preencrypt_ballots_dev(eg_ctx* ctx, const uint8_t K_be[EG_P_BYTES], size_t nballots, size_t ncontest,
                              const uint32_t* spc, uint32_t code_bytes, const uint8_t* d_dcon,
                              const uint8_t* d_manifest_hash, const uint8_t* d_ballot_ids,
                              const uint8_t* d_ballot_nonces, uint8_t* d_sorted, uint32_t* d_perm, uint32_t* d_codes,
                              uint8_t* d_unique, uint8_t* d_conf, uint8_t* d_chash, uint8_t* d_vec_cts);

/* votes nballots*nsel and sorted nballots*nsel*32 -> sel_vecs nballots*S*2*512, sel_rank and
 * sel_codes nballots*T u32, sel_nonces nballots*nsel*4*32, contest_nonces nballots*ncontest*32,
 * ok nballots*ncontest.  Only the chosen vectors are encrypted: S ciphertexts, not V. */
int eg_preencrypt_record(eg_ctx* ctx, const uint8_t K_be[EG_P_BYTES], size_t nballots, size_t ncontest,
                         const uint32_t* spc, const uint32_t* limits, uint32_t code_bytes, const uint8_t* dcon,
                         const uint8_t* ballot_nonces, const uint8_t* votes, const uint8_t* sorted, uint8_t* sel_vecs,
                         uint32_t* sel_rank, uint32_t* sel_codes, uint8_t* sel_nonces, uint8_t* contest_nonces,
                         uint8_t* ok);

int eg_preencrypt_record_dev(eg_ctx* ctx, const uint8_t K_be[EG_P_BYTES], size_t nballots, size_t ncontest,
                             const uint32_t* spc, const uint32_t* limits, uint32_t code_bytes, const uint8_t* d_dcon,
                             const uint8_t* d_ballot_nonces, const uint8_t* d_votes, const uint8_t* d_sorted,
                             uint8_t* d_sel_vecs, uint32_t* d_sel_rank, uint32_t* d_sel_codes, uint8_t* d_sel_nonces,
                             uint8_t* d_contest_nonces, uint8_t* d_ok);

/* cts nballots*nsel*2*512 (the recorded ballot's ciphertexts) and conf nballots*32 ->
 * ok_contest nballots*ncontest, ok_conf nballots. */
int eg_preencrypt_verify(eg_ctx* ctx, size_t nballots, size_t ncontest, const uint32_t* spc, const uint32_t* limits,
                         uint32_t code_bytes, const uint8_t* dcon, const uint8_t manifest_hash[EG_Q_BYTES],
                         const uint8_t* ballot_ids, const uint8_t* sel_vecs, const uint32_t* sel_rank,
                         const uint32_t* sel_codes, const uint8_t* sorted, const uint8_t* cts, const uint8_t* conf,
                         uint8_t* ok_contest, uint8_t* ok_conf);

int eg_preencrypt_verify_dev(eg_ctx* ctx, size_t nballots, size_t ncontest, const uint32_t* spc,
                             const uint32_t* limits, uint32_t code_bytes, const uint8_t* d_dcon,
                             const uint8_t* d_manifest_hash, const uint8_t* d_ballot_ids, const uint8_t* d_sel_vecs,
                             const uint32_t* d_sel_rank, const uint32_t* d_sel_codes, const uint8_t* d_sorted,
                             const uint8_t* d_cts, const uint8_t* d_conf, uint8_t* d_ok_contest, uint8_t* d_ok_conf);

#ifdef __cplusplus
}
#endif
#endif /* EG_HIP_PREENCRYPT_H */
