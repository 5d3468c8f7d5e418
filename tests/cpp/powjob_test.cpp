// Host test of electionguard-remote_amd/csrc/eg_powjob.hpp (tests/test_powjob.py compiles and runs
// it): PowJob's fields sit at the word offsets k_pow reads, an untouched job is nine kNone, and
// every named shape equals, byte for byte, the shape its sites spelled out field by field before
// the constructors existed (the schedule cache keys on those bytes).
#include <cstdio>
#include <cstring>

#include "eg_powjob.hpp"

static int cases = 0, failures = 0;

static void expect(bool ok, const char* what) {
  ++cases;
  if (!ok) {
    ++failures;
    std::fprintf(stderr, "FAIL: %s\n", what);
  }
}

static void same(const PowShape& got, const PowShape& want, const char* what) {
  expect(std::memcmp(&got, &want, sizeof(PowShape)) == 0, what);
}

int main() {
  {  // the layout: values written through the names, read back as words
    PowJob j;
    j.base = 100; j.exp[0] = 101; j.exp[1] = 102; j.out[0] = 103; j.out[1] = 104;
    j.fb[0][0] = 105; j.fb[0][1] = 106; j.fb[1][0] = 107; j.fb[1][1] = 108;
    uint32_t w[kJobWords];
    static_assert(sizeof(w) == sizeof(j), "nine words");
    std::memcpy(w, &j, sizeof(w));
    bool ok = true;
    for (int i = 0; i < kJobWords; ++i) ok = ok && w[i] == 100u + (uint32_t)i;
    expect(ok, "PowJob fields at words 0..8");
    expect(w[kJobBase] == 100 && w[kJobExp] == 101 && w[kJobExp + 1] == 102 && w[kJobOut] == 103 &&
               w[kJobOut + 1] == 104 && w[kJobFb + 2 * 0 + 1] == 106 && w[kJobFb + 2 * 1 + 0] == 107,
           "the word-offset constants name those words");
    j.gather_src() = 7;
    std::memcpy(w, &j, sizeof(w));
    expect(w[kJobGather] == 7 && j.exp[1] == 7 && kJobGather == 2, "gather_src is word 2, the second exponent");
  }
  {  // untouched jobs
    std::vector<PowJob> J = new_jobs(3);
    uint32_t w[3 * kJobWords];
    std::memcpy(w, J.data(), sizeof(w));
    bool ok = J.size() == 3;
    for (uint32_t x : w) ok = ok && x == kNone;
    expect(ok, "an untouched job is nine kNone");
    expect(kNone == 0xFFFFFFFFu && kJobWords == 9, "kNone and kJobWords");
  }
  expect(sizeof(PowShape) == 19 * 4, "PowShape is 19 words");

  // ---- variable base (the share proofs' A^v and M^c, the per-element powP, the inverses) ----
  {
    PowShape S{};
    S.has_base = 1; S.nout = 1; S.exp_bytes = 32;
    same(pow_var(), S, "pow_var()");
  }
  {
    PowShape S{};
    S.has_base = 1; S.nout = 1; S.exp_bytes = 512;
    same(pow_var(1, 512), S, "pow_var(1, 512)");
  }
  {
    PowShape S1{};
    S1.has_base = 1; S1.nout = 1; S1.nfb[0] = 1; S1.exp_bytes = 32;
    same(pow_var(1, 32, 1), S1, "pow_var(1, 32, 1): X^c g^v");
  }
  {  // the shuffle's private sh_shape(base, nfb0, nout) for base = true
    for (uint32_t nfb0 = 0; nfb0 < 2; ++nfb0) {
      PowShape S{};
      S.has_base = 1; S.nout = 1; S.nfb[0] = nfb0; S.exp_bytes = 32;
      same(pow_var(1, 32, nfb0), S, "pow_var against sh_shape(true, nfb0)");
    }
  }
  {  // g's comb table job starts from pow_var(0)
    PowShape S{};
    S.has_base = 1; S.nout = 0; S.exp_bytes = 32; S.comb = 1;
    PowShape T = pow_var(0);
    T.comb = 1;
    same(T, S, "pow_var(0) + comb");
  }
  // ---- fixed-base only ----
  {
    PowShape S{};
    S.nout = 1;
    S.exp_bytes = 32;
    S.has_base = 0;
    S.nfb[0] = 1;
    S.tab[0][0] = 0;
    same(pow_fb_one(), S, "pow_fb_one()");
  }
  {
    PowShape S{};
    S.nout = 2; S.nfb[0] = 1; S.nfb[1] = 1; S.exp_bytes = 32; S.tab[0][0] = 0; S.tab[1][0] = 1;
    same(pow_fb_pair(false), S, "pow_fb_pair(false): g^a ; K^b");
  }
  {
    PowShape S{};
    S.nout = 2; S.nfb[0] = 1; S.nfb[1] = 2; S.exp_bytes = 32; S.tab[1][0] = 1; S.tab[1][1] = 0;
    same(pow_fb_pair(true), S, "pow_fb_pair(true): g^a ; K^b g^c");
  }
  {
    PowShape S1{};
    S1.nout = 1; S1.nfb[0] = 2; S1.exp_bytes = 32; S1.tab[0][0] = 0; S1.tab[0][1] = 1;
    same(pow_two_table(), S1, "pow_two_table(): g^v X^c");
  }
  // the one-off shapes of the encryption launches, as their sites derive them from pow_fb_pair
  {
    PowShape S{};  // g^R ; g^u
    S.nout = 2; S.nfb[0] = 1; S.nfb[1] = 1; S.exp_bytes = 32;
    PowShape T = pow_fb_pair(false);
    T.tab[1][0] = 0;
    same(T, S, "g^R ; g^u from pow_fb_pair(false)");
  }
  {
    PowShape S{};  // K^R g^m ; K^u
    S.nout = 2; S.nfb[0] = 2; S.nfb[1] = 1; S.exp_bytes = 32; S.tab[0][0] = 1; S.tab[0][1] = 0; S.tab[1][0] = 1;
    S.fb_small[0][1] = 1;
    PowShape T = pow_fb_pair(false);
    T.nfb[0] = 2; T.tab[0][0] = 1; T.fb_small[0][1] = 1;
    same(T, S, "K^R g^m ; K^u from pow_fb_pair(false)");
  }
  {
    PowShape S{};  // the pre-encryption component: g^rho ; K^rho g^[i = j]
    S.nout = 2; S.nfb[0] = 1; S.nfb[1] = 2; S.exp_bytes = 32; S.tab[1][0] = 1; S.tab[1][1] = 0;
    S.fb_small[1][1] = 1;
    PowShape T = pow_fb_pair(true);
    T.fb_small[1][1] = 1;
    same(T, S, "g^rho ; K^rho g^d from pow_fb_pair(true)");
  }
  // ---- the selection verifier ----
  for (uint32_t rows : {0u, 4u})
    for (uint32_t blocks : {0u, 2u, 3u}) {
      PowShape SA{};
      SA.has_base = 1; SA.nout = 2; SA.nfb[0] = 1; SA.nfb[1] = 1; SA.exp_bytes = 32; SA.comb = 1; SA.resid = 1;
      SA.rows = rows; SA.blocks = blocks; SA.tab[0][0] = 0; SA.tab[1][0] = 0;
      same(pow_sel_pair(false, rows, blocks), SA, "pow_sel_pair(alpha)");
      PowShape SB{};
      SB.has_base = 1; SB.nout = 2; SB.nfb[0] = 1; SB.nfb[1] = 2; SB.exp_bytes = 32; SB.comb = 1; SB.resid = 1;
      SB.rows = rows; SB.blocks = blocks; SB.tab[0][0] = 1; SB.tab[1][0] = 1; SB.tab[1][1] = 0;
      same(pow_sel_pair(true, rows, blocks), SB, "pow_sel_pair(beta)");
    }
  for (uint32_t gather : {0u, 1u, 3u}) {
    const bool gat = gather != 0;
    PowShape SCA{};
    SCA.has_base = 1; SCA.nout = 1; SCA.nfb[0] = 1; SCA.exp_bytes = 32; SCA.tab[0][0] = 0;
    SCA.comb = gat ? 1u : 0u; SCA.gather = gather;
    same(pow_sel_gather(false, gather), SCA, "pow_sel_gather(a)");
    PowShape SCB{};
    SCB.has_base = 1; SCB.nout = 1; SCB.nfb[0] = 2; SCB.exp_bytes = 32; SCB.tab[0][0] = 1; SCB.tab[0][1] = 0;
    SCB.comb = gat ? 1u : 0u; SCB.gather = gather;
    same(pow_sel_gather(true, gather), SCB, "pow_sel_gather(b)");
  }
  // ---- the constant-time trustee launch ----
  for (uint32_t ct_rows : {0u, 4u, 5u}) {
    PowShape S{};
    S.has_base = 1; S.nout = 2; S.exp_bytes = 32; S.comb = 1; S.rows = ct_rows; S.blocks = ct_rows == 4 ? 2u : 0u;
    same(pow_ct_pair(ct_rows), S, "pow_ct_pair");
  }
  {
    PowShape S{};
    S.has_base = 1; S.nout = 1; S.exp_bytes = 32; S.comb = 1; S.shared_comb = 1;
    same(pow_shared_comb(), S, "pow_shared_comb()");
  }
  std::printf("{\"cases\": %d, \"failures\": %d}\n", cases, failures);
  return failures ? 1 : 0;
}
