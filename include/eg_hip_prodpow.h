/* eg_hip_prodpow.h — multi-exponentiation: products of powers over many variable bases with ONE
 * exponent vector shared by every row, in libeg_hip.so.
 *
 *   out[r] = PROD_{i<n} B[r,i]^{e_i} mod p        r = 0..rows-1
 *   B[r,i] = the 512-byte big-endian element at element offset r*row_stride + i*term_stride of bases
 *   e_i    = the 32-byte big-endian row i of exps, used as given (NOT reduced mod q)
 *
 * BigInteger semantics: bases are reduced mod p, x^0 = 1 also for x = 0, 0^e = 0 for e > 0, outputs
 * are canonical.  n == 0 writes ones; rows == 0 returns EG_OK and touches nothing.  The two strides
 * are in ELEMENTS and serve both callers without a transposing copy: a (texts, k, 512) stack of
 * shares is row_stride = k, term_stride = 1; column `col` of an (N, w, 512) array of ciphertext rows
 * is row_stride = 1, term_stride = w.  Rows may overlap: bases are only read.  The bases array must
 * hold (rows-1)*row_stride + (n-1)*term_stride + 1 elements.
 *
 * VARIABLE TIME.  Both methods address memory by exponent digits, so the exponents must be public
 * (Lagrange weights, Fiat-Shamir challenges).  With eg_ctx_set_ct_pow on, every call returns
 * EG_ERR_STATE ("variable time" in eg_last_error()) and writes nothing: the switch's promise is not
 * broken silently.  For secret exponents use eg_powp_batch[_dev] (one constant-time job per term)
 * followed by eg_prod_reduce.
 *
 * Methods (window_bits = 0 lets the plan choose the width):
 *   EG_PRODPOW_INTERLEAVED, window w in 1..5.  One 8-lane group per row: a table b^1..b^(2^w-1) of
 *     each base in workspace, then R = ceil(256/w) digit rounds from the top, w squarings between
 *     rounds and one multiply per term whose digit is non-zero (the digit is the same for every row,
 *     so the branch is wave-uniform).  Terms are taken in chunks of 2^12.  Per row and term chunk of
 *     m terms at most   w*(R-1) + m*(2^w - 2 + R)   Montgomery multiplies.
 *   EG_PRODPOW_BUCKETS, window c in 1..13, W = ceil(256/c).  Per term chunk of m <= 2^16 terms: the
 *     digits are counting-sorted per window once for all rows; bucket products over member segments
 *     of S = max(16, 2^ceil(log2(m)/2)) terms and a second pass over the segments; bit products
 *     Q[c*w + t] = PROD_{j: bit t of j} bucket[w, j]; one Horner pass  PROD_k Q[k]^(2^k)  per row.
 *     Per row and term chunk at most   W*m + W*c*(2^(c-1) - 1) + 511   Montgomery multiplies.
 *   The results of the term chunks are multiplied: one more multiply per further chunk and row.
 *   EG_PRODPOW_AUTO takes the method and width with the smaller bound (buckets from about 150 terms).
 *
 * eg_prod_pow_plan is the function the dispatcher itself calls: it returns the method and width that
 * will run and mont_ops, an UPPER BOUND over all exponent values on the Montgomery multiplies
 * (squarings included) of that schedule for all rows; it is linear in rows.  Not counted: the
 * conversions into and out of Montgomery form (one per term read, one per row written) and the
 * multiplies by the Montgomery one that pad the groups of a wave to its longest segment.  The
 * pointers may be NULL.  It is pure host code: no context, no device.
 *
 * Chunking.  Rows are taken in chunks such that the device memory a call holds beyond its inputs
 * and outputs stays under 2 GiB: the per-row arrays of a chunk (imported terms or power tables,
 * segment and bucket products, bit products) are held to 1.5 GiB, the sort arrays are at most
 * 66 MiB and the product tree's scratch is below 64 MiB.  The host variant stages through the
 * chunked copy driver: per step it uploads the terms of one row chunk and one term chunk, at most
 * max(2^17, the term chunk) elements (64 MiB), so the device memory it holds does not grow with
 * rows*n; few terms make it chunk over rows, many over terms.
 *
 * The _dev variant takes every array as a device pointer, only enqueues on the ctx stream and reads
 * no exponent on the host: digit extraction and sorting are device work.
 *
 * EG_ERR_ARG with "prod_pow" in eg_last_error(), before anything is allocated: a NULL ctx or
 * required pointer (bases and exps may be NULL only when n == 0), n > 2^20, rows > 2^16,
 * rows*n > 2^24, a stride of 0 when its count exceeds 1, a method outside 0..2, a window_bits
 * outside 0..13 (buckets) or 0..5 (interleaved; with EG_PRODPOW_AUTO a forced width must suit
 * at least one method), a _dev pointer that is not 16-byte aligned.
 */
#ifndef EG_HIP_PRODPOW_H
#define EG_HIP_PRODPOW_H

#include "eg_hip.h"

#define EG_PRODPOW_AUTO 0
#define EG_PRODPOW_INTERLEAVED 1
#define EG_PRODPOW_BUCKETS 2

#define EG_PRODPOW_MAX_TERMS ((size_t)1 << 20)
#define EG_PRODPOW_MAX_ROWS ((size_t)1 << 16)
#define EG_PRODPOW_MAX_ITEMS ((size_t)1 << 24)

#ifdef __cplusplus
extern "C" {
#endif

int eg_prod_pow(eg_ctx* ctx, const uint8_t* bases_be, size_t row_stride, size_t term_stride,
                const uint8_t* exps_be, size_t rows, size_t n, int method, int window_bits, uint8_t* out_be);

int eg_prod_pow_dev(eg_ctx* ctx, const uint8_t* d_bases_be, size_t row_stride, size_t term_stride,
                    const uint8_t* d_exps_be, size_t rows, size_t n, int method, int window_bits,
                    uint8_t* d_out_be);

int eg_prod_pow_plan(size_t rows, size_t n, int method, int window_bits, int* method_out, int* window_out,
                     double* mont_ops);

#ifdef __cplusplus
}
#endif
#endif /* EG_HIP_PRODPOW_H */
