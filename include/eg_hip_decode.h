/* eg_hip_decode.h — decoding decrypted texts on the device, in libeg_hip.so: a
 * batch inverse by Montgomery's trick and a baby-step giant-step discrete logarithm to the base g
 * whose table and giant steps live in HBM.
 *
 *   inverse   out[i] = a[i]^-1 mod p, and 0 for a[i] = 0 mod p
 *   decode    counts[i] = the unique t in [0, max_count] with g^t = B[i] * M[i]^-1 mod p, else -1
 *
 * BigInteger semantics as everywhere in the library: inputs are reduced mod p (a value >= p counts as
 * its residue, so p itself counts as 0), outputs are canonical.  n == 0 returns EG_OK and touches
 * nothing.  The _dev variants take every array as a device pointer, only enqueue on the ctx stream
 * and read nothing on the host.  At most EG_DECODE_MAX_TEXTS elements per call; a call holds about
 * 3 KiB of device workspace per element beyond its inputs and outputs.
 *
 * eg_batch_inverse[_dev]   byte for byte what eg_multinv_batch writes, for every input, at about 3
 *          Montgomery multiplies per element instead of 329.  out_be == a_be is allowed.  VARIABLE
 *          TIME and meant for public values (the combined shares M of a decryption): with
 *          eg_ctx_set_ct_pow on, the call returns EG_ERR_STATE ("variable time" in eg_last_error())
 *          and writes nothing; eg_multinv_batch serves secret values.
 *
 *          The segmented trick, on 8-lane groups.  A group walks a segment of S consecutive elements
 *          and writes their prefix products (S - 1 multiplies); the segment totals are inverted by
 *          the same routine, level by level, until at most EG_DECODE_STOP of them remain; those take
 *          a^(p-2) in ONE k_pow launch with the shared 512-byte exponent (eg_shuffle_generators'
 *          path, 5,129 multiplies each); a backward sweep per level turns the inverse of a total
 *          into the inverses of its segment, 2 (S - 1) multiplies.  A zero is replaced by the
 *          Montgomery one on the way in and written as 0 on the way out, so it poisons neither its
 *          segment nor a total.  The plan, from n alone:
 *              S      = min(16, max(4, the least power of two >= ceil(n / 16)))
 *              n_0    = n;  while n_l > EG_DECODE_STOP:  n_(l+1) = ceil(n_l / S), one more level
 *              jobs   = the n_l left (n itself when n <= EG_DECODE_STOP: no level, every element
 *                       takes a^(p-2))
 *              inv_ops = 3 (n - jobs) + 5,129 jobs          (exact: each level costs 3 (n_l - n_(l+1)))
 *          which is below 3 n + 5,129 * 16, so at most 4.26 n from n = 65,536 on.  No thread loops
 *          over n: a group's chain is 3 S multiplies per level.
 *
 * eg_decode_table_create   the baby-step table of g for counts up to max_count <= 2^32, built once
 *          on the device and reused across calls like an eg_fixed_base: with m = floor(sqrt(
 *          max_count)) + 1 it holds the baby steps g^0 .. g^(m-1) and the step g^(-m) (one k_pow launch
 *          on g's radix table), and an open-addressing table of `slots` entries in HBM, slots the
 *          least power of two >= max(16, 2 m) (load factor m / slots <= 1/2), linear probing, filled
 *          on the device by compare-and-swap.  An entry holds j and an fp_bits-bit fingerprint of the
 *          CANONICAL residue of g^j: the low 64 bits of the residue in [0, p) of the element's
 *          Montgomery form, mixed (splitmix64) and cut to the top fp_bits bits; the fingerprint also
 *          fixes the entry's home slot.  fp_bits = 0 means 64; 8..64 are accepted.  The narrow widths
 *          exist ONLY so that tests can force collisions through the comparison path below; they make
 *          no table smaller and every answer stays exact.  The table belongs to its context: destroy
 *          it before the context.  eg_decode_table_destroy(NULL) is EG_OK.
 *
 * eg_decode_counts[_dev]   counts is n little-endian int64.  M_be == NULL decodes y = B[i] itself
 *          (a plain dLog, the reference's dLogG); otherwise y = B[i] * M[i]^-1 through the batch
 *          inverse above, and a row with M[i] = 0 gives y = 0 and -1.  One 8-lane group per text:
 *          for i = 0 .. m the group reduces its working value (< 2p, redundant limbs) to the canonical
 *          residue, takes the fingerprint of THAT, probes, and multiplies by g^(-m).  A HIT COUNTS
 *          ONLY AFTER ALL 144 LIMBS OF THE CANONICAL RESIDUE EQUAL THE STORED BABY STEP'S; a
 *          fingerprint match that fails the comparison continues the probe sequence, and a text
 *          without a verified hit t = i m + j <= max_count continues with the later giant steps.  A
 *          wave leaves the loop when all of its groups are done; the groups that pad the last wave
 *          start as done.  The decode is variable time by nature and its inputs and outputs are
 *          public, so eg_ctx_set_ct_pow does not refuse it.
 *
 * eg_decode_plan   pure host code (no context, no device), the function the dispatcher itself calls.
 *          Every out pointer may be NULL.  seg_len, levels, pow_jobs and inv_ops are the inversion's
 *          (above); m, slots and load the table's; mont_ops = inv_ops + n + n m is an UPPER BOUND on
 *          the Montgomery multiplies of eg_decode_counts with M given: the inversion, one multiply
 *          B * M^-1 and m giant steps per text (a text found early stops early when its whole wave
 *          has).  Not counted: the conversions into and out of Montgomery form (one multiply per
 *          element read, half a multiply per element written), the reductions to canonical form
 *          (no multiply), the table's own m + 1 fixed-base powers, and the multiplies by the
 *          Montgomery one that pad the groups of a wave to its longest segment.
 *
 * EG_ERR_ARG with "decode" in eg_last_error(), before anything is allocated and before the context
 * or the table is read: a NULL ctx, table or required pointer (M_be alone may be NULL), n >
 * EG_DECODE_MAX_TEXTS, max_count > EG_DECODE_MAX_COUNT, fp_bits outside {0, 8..64}, a NULL tab_out, a
 * _dev pointer that is not 16-byte aligned.
 */
#ifndef EG_HIP_DECODE_H
#define EG_HIP_DECODE_H

#include "eg_hip.h"

#define EG_DECODE_MAX_TEXTS ((size_t)1 << 24)
#define EG_DECODE_MAX_COUNT ((uint64_t)1 << 32)
#define EG_DECODE_STOP 16

#ifdef __cplusplus
extern "C" {
#endif

typedef struct eg_decode_table eg_decode_table;

int eg_batch_inverse(eg_ctx* ctx, const uint8_t* a_be, uint8_t* out_be, size_t n);

int eg_batch_inverse_dev(eg_ctx* ctx, const uint8_t* d_a_be, uint8_t* d_out_be, size_t n);

int eg_decode_table_create(eg_ctx* ctx, uint64_t max_count, int fp_bits, eg_decode_table** tab_out);

int eg_decode_table_destroy(eg_decode_table* tab);

int eg_decode_counts(eg_decode_table* tab, const uint8_t* B_be, const uint8_t* M_be, size_t n, int64_t* counts);

int eg_decode_counts_dev(eg_decode_table* tab, const uint8_t* d_B_be, const uint8_t* d_M_be, size_t n,
                         int64_t* d_counts);

int eg_decode_plan(size_t n, uint64_t max_count, uint32_t* seg_len, uint32_t* levels, uint32_t* pow_jobs,
                   uint32_t* m, uint32_t* slots, double* load, double* inv_ops, double* mont_ops);

#ifdef __cplusplus
}
#endif
#endif /* EG_HIP_DECODE_H */
