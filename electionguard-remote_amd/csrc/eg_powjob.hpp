// eg_powjob.hpp — what the host tells k_pow (eg_kernels.hpp): the job record, the launch-uniform
// shape and the shapes that recur.  No HIP in here: tests/cpp/powjob_test.cpp compiles it with a
// plain host compiler, as eg_stage.hpp's test does.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

constexpr uint32_t kNone = 0xFFFFFFFFu;

// One exponentiation job: kJobWords u32 that the device reads by word offset.
//   word  field      meaning
//   0     base       element index of the variable base (kNone = no variable part)
//   1..2  exp[o]     scalar index (32-B BE, or S.exp_bytes) of output o's variable-base exponent;
//                    a gather job (S.gather > 0) keeps its first source job in word 2 (gather_src)
//   3..4  out[o]     output element indices
//   5..8  fb[o][t]   scalar index of fixed-base term t of output o
// A fresh record is all kNone: a field a shape does not use is never read.
constexpr int kJobWords = 9;
constexpr uint32_t kJobBase = 0, kJobExp = 1, kJobGather = 2, kJobOut = 3, kJobFb = 5;

struct PowJob {
  uint32_t base = kNone, exp[2] = {kNone, kNone}, out[2] = {kNone, kNone};
  uint32_t fb[2][2] = {{kNone, kNone}, {kNone, kNone}};
  uint32_t& gather_src() { return exp[1]; }
};
static_assert(sizeof(PowJob) == kJobWords * 4, "k_pow reads a job as kJobWords words");
static_assert(offsetof(PowJob, base) == kJobBase * 4 && offsetof(PowJob, exp) == kJobExp * 4 &&
                  offsetof(PowJob, exp) + 4 == kJobGather * 4 && offsetof(PowJob, out) == kJobOut * 4 &&
                  offsetof(PowJob, fb) == kJobFb * 4,
              "the word offsets are PowJob's fields");

// a host job table of n untouched jobs
inline std::vector<PowJob> new_jobs(size_t n) { return std::vector<PowJob>(n); }

// Launch-uniform shape: nout (0..2), nfb[o] (0..2), tab[o][t] in {0,1} = which FbTab.
// Variable part: fixed 4-bit window, table base^0..base^15 in per-group scratch, or a comb.
struct PowShape {
  uint32_t has_base, nout, nfb[2], tab[2][2];
  uint32_t exp_bytes;  // variable-base exponent length (32, or 512 for inverses)
  uint32_t comb;       // 1: Lim-Lee comb (h = 5) shared by the job's exponents (32-byte only)
  uint32_t gather;     // comb jobs whose base is a PRODUCT of `gather` earlier comb bases (the contest
                       // aggregates A = prod alpha, B = prod beta): y_k = prod of their y_k (ygat,
                       // job gather_src onwards) instead of 208 squarings; 0 = none
  uint32_t resid;      // comb jobs (not gather): also write the residue-test pair of the base B,
                       // z = B^(2^256) (the squaring chain run to the end) and w = B^c, c = 2^256 - q, to
                       // rout[2 gid], rout[2 gid + 1]; B^q == 1 iff z == w and B != 0 (k_resid_check)
  uint32_t shared_comb;  // comb jobs whose 32-entry subset table is PowPart::ctab (one table for every
                         // job, e.g. the trustee's g^u): no per-job precompute
  uint32_t blocks;     // Lim-Lee column blocks v of a plain comb (0/1: one block of cw columns, one
                       // 2^h-entry table; 2 or 3: blocks of ceil(cw / v) columns, tables of
                       // B^(2^(cw r + bw t)), v * 2^h entries).  v > 1 pays when the squaring chain
                       // runs to 2^256 anyway (resid)
  uint32_t rows;       // Lim-Lee rows h of a plain comb (0: kCombH = 5 rows of 52 bits, 32-entry
                       // tables; 4: rows of 64 bits, 16-entry tables -- the constant-time trustee
                       // pair, whose masked scans read every entry of a table, and the EG_SEL_COMB=43
                       // selection jobs, 4 rows x 3 blocks)
  uint32_t fb_small[2][2];  // fixed-base term [o][t] whose scalar is < 2^wbits (the vote m of
                            // beta = K^R g^m): only radix window 0 is applied (host schedule only)
};

// The shapes that recur.  The schedule cache keys on a shape's raw bytes, so every constructor
// starts from PowShape S{} and leaves what it does not use zero.  A one-off shape starts from
// the nearest of these and sets its odd field at the site.  Table 0 is f0 (g's in most
// launches), table 1 is f1 (the key's).
// B^e from the 4-bit window, times nfb0 terms of table 0 (nout = 0: no output, for a shape that
// only wants its table built)
inline PowShape pow_var(uint32_t nout = 1, uint32_t exp_bytes = 32, uint32_t nfb0 = 0) {
  PowShape S{};
  S.has_base = 1; S.nout = nout; S.nfb[0] = nfb0; S.exp_bytes = exp_bytes;
  return S;
}
// g^a from table 0 alone
inline PowShape pow_fb_one() {
  PowShape S{};
  S.nout = 1; S.nfb[0] = 1; S.exp_bytes = 32;
  return S;
}
// g^a ; K^b, or with `third` g^a ; K^b g^c  (an encryption's alpha and beta)
inline PowShape pow_fb_pair(bool third) {
  PowShape S{};
  S.nout = 2; S.nfb[0] = 1; S.nfb[1] = third ? 2u : 1u; S.exp_bytes = 32; S.tab[1][0] = 1;
  return S;
}
// g^v X^c from two tables (a Chaum-Pedersen commitment under a key that has a table)
inline PowShape pow_two_table() {
  PowShape S{};
  S.nout = 1; S.nfb[0] = 2; S.exp_bytes = 32; S.tab[0][1] = 1;
  return S;
}
// The selection verifier's pair on one comb with the residue pair of its base:
// alpha^c0 g^v0 ; alpha^c1 g^v1, or for beta: beta^c0 K^v0 ; beta^c1 K^v1 g^-c1
inline PowShape pow_sel_pair(bool beta, uint32_t rows, uint32_t blocks) {
  PowShape S{};
  S.has_base = 1; S.nout = 2; S.nfb[0] = 1; S.nfb[1] = beta ? 2u : 1u; S.exp_bytes = 32; S.comb = 1; S.resid = 1;
  S.rows = rows; S.blocks = blocks;
  if (beta) S.tab[0][0] = 1, S.tab[1][0] = 1;
  return S;
}
// its follow-up on the product of `gather` of those bases (0: a window job on the product itself):
// A^c g^v, or for beta: B^c K^v g^w
inline PowShape pow_sel_gather(bool beta, uint32_t gather) {
  PowShape S{};
  S.has_base = 1; S.nout = 1; S.nfb[0] = beta ? 2u : 1u; S.exp_bytes = 32; S.comb = gather ? 1u : 0u; S.gather = gather;
  if (beta) S.tab[0][0] = 1;
  return S;
}
// B^e0 ; B^e1 on one comb for secret exponents: ct_rows = 4 scans 16-entry tables, 2 blocks
inline PowShape pow_ct_pair(uint32_t ct_rows) {
  PowShape S{};
  S.has_base = 1; S.nout = 2; S.exp_bytes = 32; S.comb = 1; S.rows = ct_rows; S.blocks = ct_rows == 4 ? 2u : 0u;
  return S;
}
// one power from the launch's shared comb table (PowPart::ctab), no per-job precompute
inline PowShape pow_shared_comb() {
  PowShape S{};
  S.has_base = 1; S.nout = 1; S.exp_bytes = 32; S.comb = 1; S.shared_comb = 1;
  return S;
}
