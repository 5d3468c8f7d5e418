/* eg_hip_contestdata.h — a contest's write-in names and overvote / undervote status, encrypted
 * and opened at ballot scale: the HashedElGamalCiphertext (c0, c1, c2, numBytes) of upstream's
 * EncryptedBallot.Contest.contestData, in libeg_hip.so.
 *
 * An item is one (ballot b, contest k) pair, ballot-major: n = nballots * ncontest items.  nbytes
 * is the padded plaintext length, the same for every item of a call, 1 <= nbytes <=
 * EG_CD_MAX_BYTES (a fixed length leaks nothing about the content).  be32(x) is 4 bytes
 * big-endian; P elements are 512 bytes big-endian; HMAC is HMAC-SHA256 over raw bytes with
 * 64-byte blocks (the ctx's hex format enters the nonce only).  The KDF layout is the project's
 * own (the upstream one is unpinned, as for the key ceremony's backups):
 *
 *   nonce       r[b,k] = H(Q xi_b, Q 3, Q k)        hash_elems of eg_hip_codes.h (tags 1 and 2 are
 *                                                   its selection and contest nonces), per
 *                                                   eg_ctx_set_hash_format, mod q
 *   pad         c0 = g^r,  kappa = K^r              (= c0^s for the joint secret s)
 *   label       ballot_id[b] (32 B) || be32(k)      36 bytes
 *   key         kk = SHA256(c0 || kappa)            1024 raw bytes
 *   stream      block j = HMAC(kk, 0x01 || "contest" || label || be32(j)),  j = 0 .. ceil(nbytes/32)-1,
 *               the last block truncated
 *   MAC key     mk = HMAC(kk, 0x02 || "contest" || label)
 *   ciphertext  c1 = data XOR stream (nbytes),  c2 = HMAC(mk, c0 || c1) (32 B)
 *   open        recomputed from (c0, kappa, label): ok = (c2 matches, compared without an early
 *               exit); data = c1 XOR stream where ok, else all zero
 *
 * "contest" keeps these keys apart from the key ceremony's "share" keys.  Contest data does not
 * enter the contest hash, the ballot hash or the codes of eg_hip_codes.h.
 *
 * The two exponentiations of a seal are the fixed-base batch path of eg_fb_pow_batch_dev, on the
 * ctx's g table and K's cached key table (K is set under the ctx lock for the call, as in
 * eg_encrypt_ballots), and therefore follow eg_ctx_set_ct_pow: set it when r must not steer
 * memory addresses.  Opening takes kappa from the caller: the mediator after combining the
 * trustees' shares of (c0, 1), or whoever knows r.
 *
 * Conventions are those of eg_hip_codes.h: the _dev variants take device pointers (K_be stays a
 * host pointer) and are asynchronous on the ctx stream; the host variants stage ballots in the
 * verifier's chunks, so the memory held does not grow with nballots.  nballots == 0 returns EG_OK
 * and writes nothing.  EG_ERR_ARG before anything is allocated or read: a NULL ctx or required
 * pointer, ncontest == 0, nbytes outside [1, EG_CD_MAX_BYTES], or a _dev pointer to 512-byte or
 * 32-byte rows that is not 16-byte aligned.  c1 and data rows are nbytes apart and need no
 * alignment, and neither do the ok flags.
 */
#ifndef EG_HIP_CONTESTDATA_H
#define EG_HIP_CONTESTDATA_H

#include "eg_hip.h"

#define EG_CD_MAX_BYTES 1024

#ifdef __cplusplus
extern "C" {
#endif

/* ballot_nonces nballots*32 -> out_r nballots*ncontest*32. */
int eg_derive_contest_data_nonces(eg_ctx* ctx, size_t nballots, size_t ncontest, const uint8_t* ballot_nonces,
                                  uint8_t* out_r);

int eg_derive_contest_data_nonces_dev(eg_ctx* ctx, size_t nballots, size_t ncontest, const uint8_t* d_ballot_nonces,
                                      uint8_t* d_out_r);

/* ballot_ids nballots*32, nonces_r n*32, data n*nbytes -> out_c0 n*512, out_c1 n*nbytes,
 * out_c2 n*32.  kappa never leaves the device. */
int eg_seal_contest_data(eg_ctx* ctx, const uint8_t K_be[EG_P_BYTES], size_t nballots, size_t ncontest, size_t nbytes,
                         const uint8_t* ballot_ids, const uint8_t* nonces_r, const uint8_t* data, uint8_t* out_c0,
                         uint8_t* out_c1, uint8_t* out_c2);

int eg_seal_contest_data_dev(eg_ctx* ctx, const uint8_t K_be[EG_P_BYTES], size_t nballots, size_t ncontest,
                             size_t nbytes, const uint8_t* d_ballot_ids, const uint8_t* d_nonces_r,
                             const uint8_t* d_data, uint8_t* d_out_c0, uint8_t* d_out_c1, uint8_t* d_out_c2);

/* ballot_ids nballots*32, c0 and kappa n*512, c1 n*nbytes, c2 n*32 -> out_data n*nbytes and
 * out_ok n flag bytes.  A failed MAC clears that item's flag and zeroes its row; the other
 * items are not affected. */
int eg_open_contest_data(eg_ctx* ctx, size_t nballots, size_t ncontest, size_t nbytes, const uint8_t* ballot_ids,
                         const uint8_t* c0, const uint8_t* kappa, const uint8_t* c1, const uint8_t* c2,
                         uint8_t* out_data, uint8_t* out_ok);

int eg_open_contest_data_dev(eg_ctx* ctx, size_t nballots, size_t ncontest, size_t nbytes,
                             const uint8_t* d_ballot_ids, const uint8_t* d_c0, const uint8_t* d_kappa,
                             const uint8_t* d_c1, const uint8_t* d_c2, uint8_t* d_out_data, uint8_t* d_out_ok);

#ifdef __cplusplus
}
#endif
#endif /* EG_HIP_CONTESTDATA_H */
