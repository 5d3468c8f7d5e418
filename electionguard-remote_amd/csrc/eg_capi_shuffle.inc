// eg_capi_shuffle.inc — the verifiable shuffle: generators, mix, prover and verifier
// (include/eg_hip_shuffle.h; DESIGN.md §19; included by eg_capi.hip after eg_capi_decrypt2.inc: the
// key tables and the job helpers are eg_capi_ballot.inc's).  Kernels: eg_shuffle.hpp, k_pow, k_prod.
// Each entry point and its _dev twin are one body taking `bool host`; the host variants upload the
// whole arrays into the family's own workspace slots (no staging driver: see the header).

static int sh_fail(const std::string& msg) { return fail(EG_ERR_ARG, "shuffle: " + msg); }

static int sh_limits(size_t N, size_t w) {
  if (!N) return sh_fail("no rows (N == 0)");
  if (N > EG_SHUFFLE_MAX_ROWS) return sh_fail("more than 2^20 rows");
  if (!w) return sh_fail("rows of no width (w == 0)");
  if (w > EG_SHUFFLE_MAX_CELLS / N) return sh_fail("N * w exceeds 2^21");
  return EG_OK;
}

// a host call's psi must be a permutation of 0 .. N-1
static int sh_psi_ok(const uint32_t* psi, size_t N) {
  std::vector<uint8_t> seen(N, 0);
  for (size_t i = 0; i < N; ++i) {
    if (psi[i] >= N) return sh_fail("psi has an entry >= N");
    if (seen[psi[i]]++) return sh_fail("psi repeats an entry");
  }
  return EG_OK;
}

// cof * q + 1 == p by a schoolbook multiply on 32-bit words (host)
static bool sh_cofactor_ok(const eg_ctx* c, const uint8_t cof_be[512]) {
  auto word = [](const uint8_t* be, int nbytes, int i) {  // little-endian word i of a big-endian number
    const uint8_t* b = be + nbytes - 4 * (i + 1);
    return (uint32_t)b[0] << 24 | (uint32_t)b[1] << 16 | (uint32_t)b[2] << 8 | (uint32_t)b[3];
  };
  uint32_t pr[137] = {0};
  for (int i = 0; i < 128; ++i) {
    const uint64_t a = word(cof_be, 512, i);
    uint64_t carry = 0;
    for (int j = 0; j < 8; ++j) {
      const uint64_t t = (uint64_t)pr[i + j] + a * word(c->q_be, 32, j) + carry;
      pr[i + j] = (uint32_t)t;
      carry = t >> 32;
    }
    pr[i + 8] = (uint32_t)carry;  // untouched by the rows before
  }
  for (int i = 0; i < 137; ++i)
    if (++pr[i] != 0) break;
  for (int i = 0; i < 128; ++i)
    if (pr[i] != word(c->p_be, 512, i)) return false;
  for (int i = 128; i < 137; ++i)
    if (pr[i]) return false;
  return true;
}

// ---------------------------------------------------------------------------------
// generators
// ---------------------------------------------------------------------------------
static int sh_generators(eg_ctx* c, bool host, const uint8_t* cof_be, const uint8_t* gseed_be, size_t N, uint8_t* G) {
  int rc;
  if (!c || !cof_be || !gseed_be || !G) return sh_fail("null context or pointer");
  if ((rc = sh_limits(N, 1))) return rc;
  if (!host && !aligned16({G})) return sh_fail("device pointer not 16-byte aligned");
  if (!sh_cofactor_ok(c, cof_be)) return sh_fail("cof * q + 1 != p");
  Locked lk(c);
  const size_t n1 = N + 1, E = (size_t)kW * 4;
  // the call's constants: [gseed (32)][cof (512)][flag word, zero (16)]
  std::vector<uint8_t> h(32 + 512 + 16, 0);
  std::memcpy(&h[0], gseed_be, 32);
  std::memcpy(&h[32], cof_be, 512);
  uint8_t *CN = nullptr, *X = nullptr;
  uint32_t *EL = nullptr, *O = nullptr;
  if ((rc = upload(c, W_SH_CONST, h.data(), h.size(), (void**)&CN))) return rc;
  uint32_t* flag = reinterpret_cast<uint32_t*>(CN + 32 + 512);
  if ((rc = ws_get(c, W_SH_X, (N + 2) * 512, (void**)&X))) return rc;
  hipLaunchKernelGGL(k_sh_expand, dim3(cgrid(n1 * 16)), dim3(kBlock), 0, c->stream, CN,
                     (uint32_t)EG_SHUFFLE_TAG_GENERATOR, (uint64_t)(n1 * 16), c->hash_fmt, X);
  HIPCHK(hipGetLastError());
  if ((rc = ws_get(c, W_SH_E, n1 * E, (void**)&EL))) return rc;
  if ((rc = launch_import(c, X, n1, EL, nullptr))) return rc;  // an X_k >= p is reduced
  auto J = new_jobs(n1);
  for (size_t i = 0; i < n1; ++i) {
    PowJob& a = J[i];  // X_i^cof: every job reads the one 512-byte exponent
    a.base = (uint32_t)i; a.exp[0] = 0; a.out[0] = (uint32_t)i;
  }
  if ((rc = ws_get(c, W_SH_O, (N + 2) * E, (void**)&O))) return rc;
  const FbTab Gt = c->gtab->tab();
  if ((rc = launch_pow_jobs(c, W_SH_JOBS, pow_var(1, 512), J, EL, CN + 32, O, Gt, Gt))) return rc;
  if ((rc = run_prod(c, O + kW, GroupMap{1, 1, 0, 0, (uint32_t)N}, 1, N, 1, O + n1 * kW))) return rc;
  uint8_t* GB = host ? X : G;  // the digests are dead after the import
  if ((rc = launch_export(c, O, N + 2, GB))) return rc;
  hipLaunchKernelGGL(k_sh_trivial, dim3(cgrid(n1)), dim3(kBlock), 0, c->stream, GB, (uint64_t)n1, flag);
  HIPCHK(hipGetLastError());
  uint32_t trivial = 0;
  HIPCHK(hipMemcpyAsync(&trivial, flag, 4, hipMemcpyDeviceToHost, c->stream));
  if (host) HIPCHK(hipMemcpyAsync(G, GB, (N + 2) * 512, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (trivial) return fail(EG_ERR_STATE, "shuffle: a generator is 0 or 1 (take another gseed)");
  return EG_OK;
}

extern "C" int eg_shuffle_generators_dev(eg_ctx* c, const uint8_t cof_be[512], const uint8_t gseed_be[32], size_t N,
                                         uint8_t* d_G) {
  return sh_generators(c, false, cof_be, gseed_be, N, d_G);
}

extern "C" int eg_shuffle_generators(eg_ctx* c, const uint8_t cof_be[512], const uint8_t gseed_be[32], size_t N,
                                     uint8_t* G) {
  return sh_generators(c, true, cof_be, gseed_be, N, G);
}

// ---------------------------------------------------------------------------------
// mix
// ---------------------------------------------------------------------------------
static int sh_mix(eg_ctx* c, bool host, const uint8_t* K_be, size_t N, size_t w, const uint8_t* E_be,
                  const uint32_t* psi, const uint8_t* r, uint8_t* E2) {
  int rc;
  if (!c || !K_be || !E_be || !psi || !r || !E2) return sh_fail("null context or pointer");
  if ((rc = sh_limits(N, w))) return rc;
  if (!host && !aligned16({E_be, psi, r, E2})) return sh_fail("device pointer not 16-byte aligned");
  if (host && (rc = sh_psi_ok(psi, N))) return rc;
  Locked lk(c);
  if (c->ct_pow)
    return fail(EG_ERR_STATE, "shuffle: the mix is variable time and eg_ctx_set_ct_pow is on");
  if ((rc = use_key_locked(c, K_be))) return rc;
  const size_t cells = N * w, items = 2 * cells, E = (size_t)kW * 4;
  uint8_t *X = nullptr, *SC = nullptr;
  uint32_t *EL = nullptr, *O = nullptr;
  const uint8_t *d_E = E_be, *d_r = r;
  const uint32_t* d_psi = psi;
  // scalars: [r mod q (cells)], in host mode then the nonces as given
  if ((rc = ws_get(c, W_SH_SC, cells * (host ? 64 : 32), (void**)&SC))) return rc;
  if (host) {
    if ((rc = upload(c, W_SH_X, E_be, items * 512, (void**)&X))) return rc;
    if ((rc = upload(c, W_SH_PSI, psi, N * 4, (void**)&d_psi))) return rc;
    HIPCHK(hipMemcpyAsync(SC + cells * 32, r, cells * 32, hipMemcpyHostToDevice, c->stream));
    d_E = X;
    d_r = SC + cells * 32;
  }
  hipLaunchKernelGGL(k_reduce_q, dim3(cgrid(cells)), dim3(kBlock), 0, c->stream, c->d_q, d_r, (uint64_t)cells, SC);
  HIPCHK(hipGetLastError());
  if ((rc = ws_get(c, W_SH_E, items * E, (void**)&EL))) return rc;
  if ((rc = launch_import(c, d_E, items, EL, nullptr))) return rc;
  auto J = new_jobs(cells);
  for (size_t i = 0; i < cells; ++i) {
    PowJob& a = J[i];  // g^r (out 2 i) and K^r (out 2 i + 1)
    a.out[0] = (uint32_t)(2 * i); a.out[1] = (uint32_t)(2 * i + 1); a.fb[0][0] = (uint32_t)i; a.fb[1][0] = (uint32_t)i;
  }
  if ((rc = ws_get(c, W_SH_O, items * E, (void**)&O))) return rc;
  if ((rc = launch_pow_jobs(c, W_SH_JOBS, pow_fb_pair(false), J, nullptr, SC, O, c->gtab->tab(), c->Ktab->tab())))
    return rc;
  // row i of the output takes row psi(i) of the input: in place over the powers
  LAUNCH_F(c, k_sh_gather_mul, dim3(grid_for(items)), c->d, EL, d_psi, (uint32_t)N, (uint32_t)(2 * w), O,
           (uint64_t)items, O);
  HIPCHK(hipGetLastError());
  if ((rc = launch_export(c, O, items, host ? X : E2))) return rc;
  if (host) {
    HIPCHK(hipMemcpyAsync(E2, X, items * 512, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  return EG_OK;
}

extern "C" int eg_shuffle_mix_dev(eg_ctx* c, const uint8_t K_be[512], size_t N, size_t w, const uint8_t* d_E,
                                  const uint32_t* d_psi, const uint8_t* d_r, uint8_t* d_E2) {
  return sh_mix(c, false, K_be, N, w, d_E, d_psi, d_r, d_E2);
}

extern "C" int eg_shuffle_mix(eg_ctx* c, const uint8_t K_be[512], size_t N, size_t w, const uint8_t* E,
                              const uint32_t* psi, const uint8_t* r, uint8_t* E2) {
  return sh_mix(c, true, K_be, N, w, E, psi, r, E2);
}

// ---------------------------------------------------------------------------------
// the proof: shared pieces (the caller holds the lock; device pointers; ctx stream)
// ---------------------------------------------------------------------------------
// the call's constants in W_SH_CONST, 32-byte rows: gseed, the tags 0x42 and 0x45, N, w, q - 1, q,
// the flag word (zero), then K (16 rows)
enum { kShGseed = 0, kShTagSeed = 1, kShN = 2, kShW = 3, kShTagC = 4, kShQm1 = 5, kShQ = 6, kShFlag = 7, kShK = 8 };
static int sh_consts(eg_ctx* c, const uint8_t* K_be, const uint8_t* gseed_be, size_t N, size_t w, uint8_t** out) {
  std::vector<uint8_t> h((kShK + 16) * 32, 0);
  auto put = [&](int row, uint64_t v) {
    for (int i = 0; i < 8; ++i) h[row * 32 + 31 - i] = (uint8_t)(v >> (8 * i));
  };
  std::memcpy(&h[kShGseed * 32], gseed_be, 32);
  put(kShTagSeed, EG_SHUFFLE_TAG_SEED);
  put(kShTagC, EG_SHUFFLE_TAG_CHALLENGE);
  put(kShN, N);
  put(kShW, w);
  std::memcpy(&h[kShQ * 32], c->q_be, 32);
  std::memcpy(&h[kShQm1 * 32], c->q_be, 32);
  for (int i = 31, borrow = 1; borrow && i >= 0; --i) {  // q - 1
    borrow = h[kShQm1 * 32 + i] == 0;
    h[kShQm1 * 32 + i] = (uint8_t)(h[kShQm1 * 32 + i] - 1);
  }
  std::memcpy(&h[kShK * 32], K_be, 512);
  return upload(c, W_SH_CONST, h.data(), h.size(), (void**)out);
}

// host variants: every array goes up whole, the body runs on the copies, the outputs come back
struct ShIO {
  eg_ctx* c;
  bool host;
  struct Item {
    void** dev;
    const void* src;
    void* dst;
    size_t bytes, off;
  };
  std::vector<Item> items;
  template <class T>
  void in(const T*& p, size_t bytes) { items.push_back(Item{(void**)&p, p, nullptr, bytes, 0}); }
  template <class T>
  void out(T*& p, size_t bytes) { items.push_back(Item{(void**)&p, nullptr, p, bytes, 0}); }
  int begin() {
    if (!host) return EG_OK;
    size_t total = 0;
    for (Item& it : items) it.off = total, total += (it.bytes + 255) / 256 * 256;
    uint8_t* base = nullptr;
    int rc = ws_get(c, W_SH_IO, total, (void**)&base);
    if (rc) return rc;
    for (Item& it : items) {
      *it.dev = base + it.off;
      if (it.src) HIPCHK(hipMemcpyAsync(base + it.off, it.src, it.bytes, hipMemcpyHostToDevice, c->stream));
    }
    return EG_OK;
  }
  int end() {
    if (!host) return EG_OK;
    for (Item& it : items)
      if (it.dst) HIPCHK(hipMemcpyAsync(it.dst, *it.dev, it.bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return EG_OK;
  }
};

// out = T_rows: the leaves of n rows of m elements, then the levels of T
static int sh_tree_rows(eg_ctx* c, const uint8_t* rows, size_t n, size_t m, uint8_t* out) {
  int rc;
  uint8_t* H = nullptr;
  const size_t l1 = (n + 255) / 256 + 1;
  if ((rc = ws_get(c, W_SH_H, (n + 2 * l1) * 32, (void**)&H))) return rc;
  hipLaunchKernelGGL(k_sh_leaf, dim3(cgrid(n)), dim3(kBlock), 0, c->stream, c->d_q, rows, (uint64_t)m, (uint64_t)n,
                     c->hash_fmt, H);
  HIPCHK(hipGetLastError());
  uint8_t* ping[2] = {H + n * 32, H + (n + l1) * 32};
  const uint8_t* cur = H;
  size_t len = n;
  for (int pi = 0; len > 256; pi ^= 1) {  // one launch per level the tree has above the last
    const size_t nl = (len + 255) / 256;
    hipLaunchKernelGGL(k_sh_tree, dim3(cgrid(nl)), dim3(kBlock), 0, c->stream, c->d_q, cur, (uint64_t)len, c->hash_fmt,
                       ping[pi]);
    HIPCHK(hipGetLastError());
    cur = ping[pi];
    len = nl;
  }
  hipLaunchKernelGGL(k_sh_tree, dim3(1), dim3(kBlock), 0, c->stream, c->d_q, cur, (uint64_t)len, c->hash_fmt, out);
  HIPCHK(hipGetLastError());
  return EG_OK;
}

// out[row] (Montgomery) = PROD_i B[row, i]^{e_i} over all n terms: eg_prod_pow_dev's loop over
// pp_chunk_locked, rows in groups within its limits of 2^16 rows and 2^24 items and its row budget
static int sh_pp(eg_ctx* c, const uint8_t* bases, size_t rs, size_t ts, const uint8_t* exps, size_t rows, size_t n,
                 uint32_t* out) {
  int rc, mt = 0, w = 0;
  const size_t E = (size_t)kW * 4;
  const size_t rmax = std::min<size_t>(std::min<size_t>(rows, EG_PRODPOW_MAX_ROWS), EG_PRODPOW_MAX_ITEMS / n);
  if ((rc = eg_prod_pow_plan(rmax, n, EG_PRODPOW_AUTO, 0, &mt, &w, nullptr))) return rc;
  const size_t tc = std::min(n, pp_term_chunk(mt));
  const size_t rcn = std::max<size_t>(1, std::min(rmax, kPpRowBudget / pp_shape(mt, w, tc).per_row(tc)));
  for (size_t r0 = 0; r0 < rows; r0 += rcn) {
    const size_t rr = std::min(rcn, rows - r0);
    for (size_t t0 = 0; t0 < n; t0 += tc) {
      const size_t m = std::min(tc, n - t0);
      if ((rc = pp_chunk_locked(c, pp_shape(mt, w, m), bases + (r0 * rs + t0 * ts) * 512, rs, ts, exps + t0 * 32, rr,
                                m, t0 == 0)))
        return rc;
    }
    uint32_t* acc = nullptr;
    if ((rc = ws_get(c, W_PP_ACC, rr * E, (void**)&acc))) return rc;
    HIPCHK(hipMemcpyAsync(out + r0 * kW, acc, rr * E, hipMemcpyDeviceToDevice, c->stream));
  }
  return EG_OK;
}

// out[col] = SUM_i a[col cs + i is] b[i] mod q (b optional), or the product of the a's: levels of 256
static int sh_dot(eg_ctx* c, bool prod, const uint8_t* a, size_t cs, size_t is, const uint8_t* b, size_t n, size_t cols,
                  uint8_t* out) {
  int rc;
  const size_t nb0 = (n + 255) / 256, nb1 = (nb0 + 255) / 256;
  uint8_t* D = nullptr;
  if ((rc = ws_get(c, W_SH_D, cols * (nb0 + nb1) * 32, (void**)&D))) return rc;
  uint8_t* ping[2] = {D, D + cols * nb0 * 32};
  for (int pi = 0;; pi ^= 1) {
    const size_t nb = (n + 255) / 256;
    uint8_t* dst = nb == 1 ? out : ping[pi];
    if (prod)
      hipLaunchKernelGGL(k_sh_dot<true>, dim3((unsigned)cols, (unsigned)nb), dim3(kBlock), 0, c->stream, c->d_q, a,
                         (uint64_t)cs, (uint64_t)is, b, (uint64_t)n, dst);
    else
      hipLaunchKernelGGL(k_sh_dot<false>, dim3((unsigned)cols, (unsigned)nb), dim3(kBlock), 0, c->stream, c->d_q, a,
                         (uint64_t)cs, (uint64_t)is, b, (uint64_t)n, dst);
    HIPCHK(hipGetLastError());
    if (nb == 1) return EG_OK;
    a = dst, cs = nb, is = 1, b = nullptr, n = nb;
  }
}

// the inclusive scan of the maps (A[i], B[i]) in place: a level per factor of 256, then the way down
static int sh_scan(eg_ctx* c, uint8_t* A, uint8_t* B, size_t n, uint8_t* T) {
  const size_t nb = (n + 255) / 256;
  uint8_t *totA = T, *totB = T + nb * 32;
  hipLaunchKernelGGL(k_sh_scan, dim3((unsigned)nb), dim3(kBlock), 0, c->stream, c->d_q, A, B, (uint64_t)n, totA, totB);
  HIPCHK(hipGetLastError());
  if (nb == 1) return EG_OK;
  int rc = sh_scan(c, totA, totB, nb, T + 2 * nb * 32);
  if (rc) return rc;
  hipLaunchKernelGGL(k_sh_scan_apply, dim3((unsigned)nb), dim3(kBlock), 0, c->stream, c->d_q, A, B, (uint64_t)n, totA,
                     totB);
  HIPCHK(hipGetLastError());
  return EG_OK;
}

static int sh_reduce(eg_ctx* c, const uint8_t* in, size_t n, uint8_t* out) {
  hipLaunchKernelGGL(k_reduce_q, dim3(cgrid(n)), dim3(kBlock), 0, c->stream, c->d_q, in, (uint64_t)n, out);
  HIPCHK(hipGetLastError());
  return EG_OK;
}
static int sh_neg(eg_ctx* c, const uint8_t* in, size_t n, uint8_t* out) {
  hipLaunchKernelGGL(k_sh_neg, dim3(cgrid(n)), dim3(kBlock), 0, c->stream, c->d_q, in, (uint64_t)n, out);
  HIPCHK(hipGetLastError());
  return EG_OK;
}
static int sh_mul(eg_ctx* c, const uint32_t* a, uint32_t sa, const uint32_t* b, uint32_t sb, size_t n, uint32_t* out) {
  LAUNCH_F(c, k_mul, dim3(grid_for(n)), c->d, a, sa, b, sb, (uint32_t)n, out, 1u);
  HIPCHK(hipGetLastError());
  return EG_OK;
}

// c = H(Q y, Q 0x45, P t1, P t2, P t3, Q T4, Q That, Q Tchain): t123 three rows of 512 bytes
static int sh_challenge_hash(eg_ctx* c, const uint8_t* CN, const uint8_t* y, const uint8_t* t123, const uint8_t* T3,
                             uint8_t* out) {
  const HashSrc no{nullptr, 0, 0};
  hipLaunchKernelGGL(k_hash_check, dim3(1), dim3(256), 0, c->stream, c->d_q, y, 1u, 7u,
                     HashSrc{CN + kShTagC * 32, 32, 0}, HashSrc{t123, 512, 0}, HashSrc{t123 + 512, 512, 0},
                     HashSrc{t123 + 1024, 512, 0}, HashSrc{T3, 32, 0}, HashSrc{T3 + 32, 32, 0},
                     HashSrc{T3 + 64, 32, 0}, no, nullptr, 0u, 0u, kNone, nullptr, nullptr, 0u, nullptr, out,
                     c->hash_fmt);
  HIPCHK(hipGetLastError());
  return EG_OK;
}

// y = H(Q qbar, Q 0x42, Q N, Q w, P K, Q gseed, Q T_rows(E), Q T_rows(E'), Q T_rows(pc)) into y; T3: 3 rows of work
static int sh_seed(eg_ctx* c, const uint8_t* CN, size_t N, size_t w, const uint8_t* E_be, const uint8_t* E2,
                   const uint8_t* pc, uint8_t* T3, uint8_t* y) {
  int rc;
  if ((rc = sh_tree_rows(c, E_be, N, 2 * w, T3)) || (rc = sh_tree_rows(c, E2, N, 2 * w, T3 + 32)) ||
      (rc = sh_tree_rows(c, pc, N, 1, T3 + 64)))
    return rc;
  return launch_hash(c, 1,
                     {HashSrc{CN + kShTagSeed * 32, 32, 0}, HashSrc{CN + kShN * 32, 32, 0}, HashSrc{CN + kShW * 32, 32, 0},
                      HashSrc{CN + kShK * 32, 512, 0}, HashSrc{CN + kShGseed * 32, 32, 0}, HashSrc{T3, 32, 0},
                      HashSrc{T3 + 32, 32, 0}, HashSrc{T3 + 64, 32, 0}},
                     nullptr, 0, 0, kNone, nullptr, nullptr, 0, nullptr, y);
}

// ---------------------------------------------------------------------------------
// prove
// ---------------------------------------------------------------------------------
static int sh_prove_locked(eg_ctx* c, const uint8_t* CN, size_t N, size_t w, const uint8_t* G, const uint8_t* E_be,
                           const uint8_t* E2, const uint32_t* psi, const uint8_t* r, const uint8_t* nonces, uint8_t* o_pc,
                           uint8_t* o_chain, uint8_t* o_c, uint8_t* o_s, uint8_t* o_shat, uint8_t* o_sp) {
  int rc;
  const size_t E = (size_t)kW * 4, cells = N * w, NN = 4 * N + 3 + w;
  // scalars (32-byte rows): the nonces mod q in the ABI's order, then u, u', R, U, -omega4, the
  // witnesses (rbar, rhat, rtilde, r*), y, c, six tree roots
  const size_t iRho = 0, iRhoH = N, iOmH = 2 * N, iOmP = 3 * N, iOm = 4 * N, iOm4 = 4 * N + 3;
  const size_t iU = NN, iUP = iU + N, iR = iUP + N, iUU = iR + N, iNW4 = iUU + N, iWit = iNW4 + w, iY = iWit + 3 + w,
               iC = iY + 1, iT = iC + 1, nSC = iT + 6;
  uint8_t *SC = nullptr, *RR = nullptr, *T = nullptr, *BE1 = nullptr, *BE2 = nullptr;
  uint32_t *EG = nullptr, *O1 = nullptr, *O2 = nullptr, *O3 = nullptr, *TX = nullptr, *INV = nullptr;
  auto sc = [&](size_t i) { return SC + i * 32; };
  const FbTab Gt = c->gtab->tab(), Kt = c->Ktab->tab();
  if ((rc = ws_get(c, W_SH_SC, nSC * 32, (void**)&SC)) || (rc = ws_get(c, W_SH_R, cells * 32, (void**)&RR))) return rc;
  if ((rc = sh_reduce(c, nonces, NN, SC)) || (rc = sh_reduce(c, r, cells, RR))) return rc;
  if ((rc = ws_get(c, W_SH_E, (N + 2) * E, (void**)&EG))) return rc;
  if ((rc = launch_import(c, G, N + 2, EG, nullptr))) return rc;
  // the permutation commitment pc[j] = g^{rho_j} h_{psi^-1(j)}
  if ((rc = ws_get(c, W_SH_O, N * E, (void**)&O1)) || (rc = ws_get(c, W_SH_PSI2, N * 4, (void**)&INV))) return rc;
  {
    auto J = new_jobs(N);
    for (size_t j = 0; j < N; ++j) J[j].out[0] = (uint32_t)j, J[j].fb[0][0] = (uint32_t)(iRho + j);
    if ((rc = launch_pow_jobs(c, W_SH_JOBS, pow_fb_one(), J, nullptr, SC, O1, Gt, Gt))) return rc;
  }
  HIPCHK(hipMemsetAsync(INV, 0, N * 4, c->stream));
  hipLaunchKernelGGL(k_sh_invert, dim3(cgrid(N)), dim3(kBlock), 0, c->stream, psi, (uint64_t)N, INV);
  HIPCHK(hipGetLastError());
  LAUNCH_F(c, k_sh_gather_mul, dim3(grid_for(N)), c->d, EG + kW, INV, (uint32_t)N, 1u, O1, (uint64_t)N, O1);
  HIPCHK(hipGetLastError());
  if ((rc = launch_export(c, O1, N, o_pc))) return rc;
  // y, u, u' and the chain's exponents
  if ((rc = sh_seed(c, CN, N, w, E_be, E2, o_pc, sc(iT), sc(iY)))) return rc;
  hipLaunchKernelGGL(k_sh_challenges, dim3(cgrid(N)), dim3(kBlock), 0, c->stream, c->d_q, sc(iY), psi, (uint64_t)N,
                     c->hash_fmt, sc(iU), sc(iUP));
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(sc(iUU), sc(iUP), N * 32, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(sc(iR), sc(iRhoH), N * 32, hipMemcpyDeviceToDevice, c->stream));
  const size_t nb = (N + 255) / 256;
  if ((rc = ws_get(c, W_SH_T, (2 * nb + 64) * 2 * 32, (void**)&T))) return rc;
  if ((rc = sh_scan(c, sc(iUU), sc(iR), N, T))) return rc;
  // chain_i = g^{R_i} h^{U_i}: h a shared variable base; O2 = [h, chain_0 .. chain_{N-1}]
  if ((rc = ws_get(c, W_SH_O2, (N + 1) * E, (void**)&O2))) return rc;
  HIPCHK(hipMemcpyAsync(O2, EG, E, hipMemcpyDeviceToDevice, c->stream));
  {
    auto J = new_jobs(N);
    for (size_t i = 0; i < N; ++i) {
      PowJob& a = J[i];
      a.base = 0; a.exp[0] = (uint32_t)(iUU + i); a.out[0] = (uint32_t)(1 + i); a.fb[0][0] = (uint32_t)(iR + i);
    }
    if ((rc = launch_pow_jobs(c, W_SH_JOBS, pow_var(1, 32, 1), J, EG, SC, O2, Gt, Gt))) return rc;
  }
  if ((rc = launch_export(c, O2 + kW, N, o_chain))) return rc;
  // witnesses
  if ((rc = sh_dot(c, false, sc(iRho), 0, 1, nullptr, N, 1, sc(iWit)))) return rc;
  HIPCHK(hipMemcpyAsync(sc(iWit + 1), sc(iR + N - 1), 32, hipMemcpyDeviceToDevice, c->stream));
  if ((rc = sh_dot(c, false, sc(iRho), 0, 1, sc(iU), N, 1, sc(iWit + 2)))) return rc;
  if ((rc = sh_dot(c, false, RR, 1, w, sc(iUP), N, w, sc(iWit + 3)))) return rc;
  // commitments: TX = [t1, t2, t3, t4 (2 w)] [g^om3, g^-om4_j, K^-om4_j] [the products over N]
  const size_t nT = 3 + 2 * w, oF = nT, oP = nT + 1 + 2 * w;
  if ((rc = sh_neg(c, sc(iOm4), w, sc(iNW4)))) return rc;
  if ((rc = ws_get(c, W_SH_TX, (oP + 1 + 2 * w) * E, (void**)&TX))) return rc;
  {
    auto J = new_jobs(3);
    const uint32_t outs[3] = {0, 1, (uint32_t)oF};
    for (int k = 0; k < 3; ++k) J[k].out[0] = outs[k], J[k].fb[0][0] = (uint32_t)(iOm + k);
    if ((rc = launch_pow_jobs(c, W_SH_JOBS, pow_fb_one(), J, nullptr, SC, TX, Gt, Gt))) return rc;
    auto J4 = new_jobs(w);
    for (size_t j = 0; j < w; ++j) {
      PowJob& a = J4[j];
      a.out[0] = (uint32_t)(oF + 1 + 2 * j); a.out[1] = a.out[0] + 1; a.fb[0][0] = (uint32_t)(iNW4 + j); a.fb[1][0] = a.fb[0][0];
    }
    if ((rc = launch_pow_jobs(c, W_SH_JOBS, pow_fb_pair(false), J4, nullptr, SC, TX, Gt, Kt))) return rc;
  }
  if ((rc = sh_pp(c, G + 512, N, 1, sc(iOmP), 1, N, TX + oP * kW))) return rc;
  if ((rc = sh_pp(c, E2, 1, 2 * w, sc(iOmP), 2 * w, N, TX + (oP + 1) * kW))) return rc;
  if ((rc = sh_mul(c, TX + oF * kW, 1, TX + oP * kW, 1, 1 + 2 * w, TX + 2 * kW))) return rc;
  if ((rc = ws_get(c, W_SH_BE, nT * 512, (void**)&BE1))) return rc;
  if ((rc = launch_export(c, TX, nT, BE1))) return rc;
  // that_i = g^{omhat_i} chain_{i-1}^{om'_i}
  if ((rc = ws_get(c, W_SH_O3, N * E, (void**)&O3))) return rc;
  {
    auto J = new_jobs(N);
    for (size_t i = 0; i < N; ++i) {
      PowJob& a = J[i];
      a.base = (uint32_t)i; a.exp[0] = (uint32_t)(iOmP + i); a.out[0] = (uint32_t)i; a.fb[0][0] = (uint32_t)(iOmH + i);
    }
    if ((rc = launch_pow_jobs(c, W_SH_JOBS, pow_var(1, 32, 1), J, O2, SC, O3, Gt, Gt))) return rc;
  }
  if ((rc = ws_get(c, W_SH_BE2, N * 512, (void**)&BE2))) return rc;
  if ((rc = launch_export(c, O3, N, BE2))) return rc;
  // the challenge and the responses
  if ((rc = sh_tree_rows(c, BE1 + 3 * 512, w, 2, sc(iT + 3))) || (rc = sh_tree_rows(c, BE2, N, 1, sc(iT + 4))) ||
      (rc = sh_tree_rows(c, o_chain, N, 1, sc(iT + 5))))
    return rc;
  if ((rc = sh_challenge_hash(c, CN, sc(iY), BE1, sc(iT + 3), sc(iC)))) return rc;
  HIPCHK(hipMemcpyAsync(o_c, sc(iC), 32, hipMemcpyDeviceToDevice, c->stream));
  auto respond = [&](size_t om, size_t x, size_t n, uint8_t* out) {
    hipLaunchKernelGGL(k_sh_respond, dim3(cgrid(n)), dim3(kBlock), 0, c->stream, c->d_q, sc(iC), sc(om), sc(x),
                       (uint64_t)n, out);
  };
  respond(iOm, iWit, 3 + w, o_s);
  respond(iOmH, iRhoH, N, o_shat);
  respond(iOmP, iUP, N, o_sp);
  HIPCHK(hipGetLastError());
  return EG_OK;
}

static int sh_prove(eg_ctx* c, bool host, const uint8_t* K_be, const uint8_t* qbar_be, const uint8_t* gseed_be, size_t N,
                    size_t w, const uint8_t* G, const uint8_t* E_be, const uint8_t* E2, const uint32_t* psi,
                    const uint8_t* r, const uint8_t* nonces, uint8_t* o_pc, uint8_t* o_chain, uint8_t* o_c, uint8_t* o_s,
                    uint8_t* o_shat, uint8_t* o_sp) {
  int rc;
  if (!c || !K_be || !qbar_be || !gseed_be || !G || !E_be || !E2 || !psi || !r || !nonces || !o_pc || !o_chain ||
      !o_c || !o_s || !o_shat || !o_sp)
    return sh_fail("null context or pointer");
  if ((rc = sh_limits(N, w))) return rc;
  if (!host && !aligned16({G, E_be, E2, psi, r, nonces, o_pc, o_chain, o_c, o_s, o_shat, o_sp}))
    return sh_fail("device pointer not 16-byte aligned");
  if (host && (rc = sh_psi_ok(psi, N))) return rc;
  Locked lk(c);
  if (c->ct_pow)
    return fail(EG_ERR_STATE, "shuffle: the prover is variable time and eg_ctx_set_ct_pow is on");
  if ((rc = use_key_locked(c, K_be))) return rc;
  HIPCHK(hipMemcpyAsync(c->d_qbar, qbar_be, 32, hipMemcpyHostToDevice, c->stream));
  uint8_t* CN = nullptr;
  if ((rc = sh_consts(c, K_be, gseed_be, N, w, &CN))) return rc;
  ShIO io{c, host, {}};
  io.in(G, (N + 2) * 512);
  io.in(E_be, N * w * 1024);
  io.in(E2, N * w * 1024);
  io.in(psi, N * 4);
  io.in(r, N * w * 32);
  io.in(nonces, (4 * N + 3 + w) * 32);
  io.out(o_pc, N * 512);
  io.out(o_chain, N * 512);
  io.out(o_c, 32);
  io.out(o_s, (3 + w) * 32);
  io.out(o_shat, N * 32);
  io.out(o_sp, N * 32);
  if ((rc = io.begin())) return rc;
  if ((rc = sh_prove_locked(c, CN, N, w, G, E_be, E2, psi, r, nonces, o_pc, o_chain, o_c, o_s, o_shat, o_sp))) return rc;
  return io.end();
}

extern "C" int eg_shuffle_prove_dev(eg_ctx* c, const uint8_t K_be[512], const uint8_t qbar_be[32],
                                    const uint8_t gseed_be[32], size_t N, size_t w, const uint8_t* d_G,
                                    const uint8_t* d_E, const uint8_t* d_E2, const uint32_t* d_psi, const uint8_t* d_r,
                                    const uint8_t* d_nonces, uint8_t* d_pc, uint8_t* d_chain, uint8_t* d_c, uint8_t* d_s,
                                    uint8_t* d_s_hat, uint8_t* d_s_prime) {
  return sh_prove(c, false, K_be, qbar_be, gseed_be, N, w, d_G, d_E, d_E2, d_psi, d_r, d_nonces, d_pc, d_chain, d_c,
                  d_s, d_s_hat, d_s_prime);
}

extern "C" int eg_shuffle_prove(eg_ctx* c, const uint8_t K_be[512], const uint8_t qbar_be[32],
                                const uint8_t gseed_be[32], size_t N, size_t w, const uint8_t* G, const uint8_t* E,
                                const uint8_t* E2, const uint32_t* psi, const uint8_t* r, const uint8_t* nonces,
                                uint8_t* pc, uint8_t* chain, uint8_t* c_out, uint8_t* s, uint8_t* s_hat,
                                uint8_t* s_prime) {
  return sh_prove(c, true, K_be, qbar_be, gseed_be, N, w, G, E, E2, psi, r, nonces, pc, chain, c_out, s, s_hat, s_prime);
}

// ---------------------------------------------------------------------------------
// verify
// ---------------------------------------------------------------------------------
constexpr size_t kShResidChunk = (size_t)1 << 18;  // elements per residue launch (bounds its workspace)

// flag |= 2 unless every one of n elements is in (0, p) with x^q = 1: x^q by k_pow with q as the
// shared exponent, the export, a compare with 1 (an x of 0 gives 0)
static int sh_residues(eg_ctx* c, const uint8_t* CN, const uint8_t* els, size_t n, uint32_t* flag) {
  int rc;
  const size_t E = (size_t)kW * 4, ch = std::min(n, kShResidChunk);
  uint32_t *RE = nullptr, *RO = nullptr;
  uint8_t *LT = nullptr, *RB = nullptr;
  if ((rc = ws_get(c, W_SH_E, ch * E, (void**)&RE)) || (rc = ws_get(c, W_SH_O, ch * E, (void**)&RO)) ||
      (rc = ws_get(c, W_SH_LT, ch, (void**)&LT)) || (rc = ws_get(c, W_SH_X, ch * 512, (void**)&RB)))
    return rc;
  auto J = new_jobs(ch);
  for (size_t i = 0; i < ch; ++i) {
    PowJob& a = J[i];
    a.base = (uint32_t)i; a.exp[0] = 0; a.out[0] = (uint32_t)i;
  }
  const uint32_t* dj = nullptr;
  if ((rc = upload_jobs(c, W_SH_JOBS, J, &dj))) return rc;
  const FbTab Gt = c->gtab->tab();
  for (size_t i0 = 0; i0 < n; i0 += ch) {
    const size_t m = std::min(ch, n - i0);
    if ((rc = launch_import(c, els + i0 * 512, m, RE, LT))) return rc;
    if ((rc = launch_pow(c, {pow_var(), dj, m}, RE, CN + kShQ * 32, RO, Gt, Gt))) return rc;
    if ((rc = launch_export(c, RO, m, RB))) return rc;
    hipLaunchKernelGGL(k_sh_resid, dim3(cgrid(m)), dim3(kBlock), 0, c->stream, RB, LT, (uint64_t)m, flag);
    HIPCHK(hipGetLastError());
  }
  return EG_OK;
}

static int sh_verify_locked(eg_ctx* c, const uint8_t* CN, size_t N, size_t w, const uint8_t* G, const uint8_t* E_be,
                            const uint8_t* E2, const uint8_t* pc, const uint8_t* chain, const uint8_t* cc,
                            const uint8_t* s, const uint8_t* shat, const uint8_t* sp, int check_inputs, uint8_t* ok,
                            uint32_t* mask) {
  int rc;
  const size_t E = (size_t)kW * 4;
  uint32_t* flag = reinterpret_cast<uint32_t*>(const_cast<uint8_t*>(CN) + kShFlag * 32);
  // scalars: c, -c, U, -U, q - 1, y, c', six tree roots, pad; then s, -s4, s^, s', u (all mod q)
  const size_t iC = 0, iNC = 1, iUt = 2, iNU = 3, iQm1 = 4, iY = 5, iC2 = 6, iT = 7, iS = 16, iNS4 = iS + 3 + w,
               iSH = iNS4 + w, iSP = iSH + N, iU = iSP + N, nSC = iU + N;
  uint8_t *SC = nullptr, *BE1 = nullptr, *BE2 = nullptr;
  auto sc = [&](size_t i) { return SC + i * 32; };
  if ((rc = ws_get(c, W_SH_SC, nSC * 32, (void**)&SC))) return rc;
  // 1. range
  const std::pair<const uint8_t*, size_t> scal[4] = {{cc, 1}, {s, 3 + w}, {shat, N}, {sp, N}};
  const size_t red[4] = {iC, iS, iSH, iSP};
  for (int k = 0; k < 4; ++k) {
    hipLaunchKernelGGL(k_sh_range, dim3(cgrid(scal[k].second)), dim3(kBlock), 0, c->stream, c->d_q, scal[k].first,
                       (uint64_t)scal[k].second, flag);
    HIPCHK(hipGetLastError());
    if ((rc = sh_reduce(c, scal[k].first, scal[k].second, sc(red[k])))) return rc;
  }
  if ((rc = sh_neg(c, sc(iC), 1, sc(iNC))) || (rc = sh_neg(c, sc(iS + 3), w, sc(iNS4)))) return rc;
  HIPCHK(hipMemcpyAsync(sc(iQm1), CN + kShQm1 * 32, 32, hipMemcpyDeviceToDevice, c->stream));
  // 2. residues
  if ((rc = sh_residues(c, CN, E2, 2 * N * w, flag)) || (rc = sh_residues(c, CN, pc, N, flag)) ||
      (rc = sh_residues(c, CN, chain, N, flag)))
    return rc;
  if (check_inputs && (rc = sh_residues(c, CN, E_be, 2 * N * w, flag))) return rc;
  // 3. y, u, U
  if ((rc = sh_seed(c, CN, N, w, E_be, E2, pc, sc(iT), sc(iY)))) return rc;
  hipLaunchKernelGGL(k_sh_challenges, dim3(cgrid(N)), dim3(kBlock), 0, c->stream, c->d_q, sc(iY),
                     (const uint32_t*)nullptr, (uint64_t)N, c->hash_fmt, sc(iU), (uint8_t*)nullptr);
  HIPCHK(hipGetLastError());
  if ((rc = sh_dot(c, true, sc(iU), 0, 1, nullptr, N, 1, sc(iUt))) || (rc = sh_neg(c, sc(iUt), 1, sc(iNU)))) return rc;
  // elements V = [G (N + 2)] [pc (N)] [h, chain (N + 1)]; derived W = [cbar, chat, ctilde, etilde (2 w)]
  // [PROD pc, (PROD h)^-1, h^-U]; outputs X = [t1' .. (3 + 2 w)] [products (1 + 2 w)] [t3', t4' (1 + 2 w)]
  // [that' halves (2 N)]
  const size_t vP = N + 2, vC = 2 * N + 2, nT = 3 + 2 * w, wT = nT, xP = nT, xM = xP + 1 + 2 * w, xH = xM + 1 + 2 * w;
  uint32_t *V = nullptr, *W = nullptr, *X = nullptr, *Y = nullptr;
  if ((rc = ws_get(c, W_SH_V, (3 * N + 3) * E, (void**)&V)) || (rc = ws_get(c, W_SH_W, (nT + 3) * E, (void**)&W)) ||
      (rc = ws_get(c, W_SH_TX, (xH + 2 * N) * E, (void**)&X)) || (rc = ws_get(c, W_SH_O3, N * E, (void**)&Y)))
    return rc;
  if ((rc = launch_import(c, G, N + 2, V, nullptr)) || (rc = launch_import(c, pc, N, V + vP * kW, nullptr)) ||
      (rc = launch_import(c, chain, N, V + (vC + 1) * kW, nullptr)))
    return rc;
  HIPCHK(hipMemcpyAsync(V + vC * kW, V, E, hipMemcpyDeviceToDevice, c->stream));
  const FbTab Gt = c->gtab->tab(), Kt = c->Ktab->tab();
  if ((rc = run_prod(c, V + vP * kW, GroupMap{1, 1, 0, 0, (uint32_t)N}, 1, N, 1, W + wT * kW))) return rc;
  {
    auto J = new_jobs(2);
    J[0].base = (uint32_t)(N + 1); J[0].exp[0] = (uint32_t)iQm1; J[0].out[0] = (uint32_t)(wT + 1);
    J[1].base = 0; J[1].exp[0] = (uint32_t)iNU; J[1].out[0] = (uint32_t)(wT + 2);
    if ((rc = launch_pow_jobs(c, W_SH_JOBS, pow_var(), J, V, SC, W, Gt, Gt))) return rc;
  }
  if ((rc = sh_mul(c, W + wT * kW, 1, W + (wT + 1) * kW, 1, 1, W))) return rc;                 // cbar
  if ((rc = sh_mul(c, V + (vC + N) * kW, 1, W + (wT + 2) * kW, 1, 1, W + kW))) return rc;      // chat
  if ((rc = sh_pp(c, pc, N, 1, sc(iU), 1, N, W + 2 * kW))) return rc;                          // ctilde
  if ((rc = sh_pp(c, E_be, 1, 2 * w, sc(iU), 2 * w, N, W + 3 * kW))) return rc;                // etilde
  // 4. t1', t2', t3', t4': D^{-c} times a fixed-base term (g's table, K's for the betas) ...
  {
    auto JA = new_jobs(3 + w), JB = new_jobs(w);
    for (size_t k = 0; k < 3 + w; ++k) {
      PowJob& a = JA[k];
      const size_t e = k < 3 ? k : 3 + 2 * (k - 3);
      a.base = (uint32_t)e; a.exp[0] = (uint32_t)iNC; a.out[0] = (uint32_t)e; a.fb[0][0] = (uint32_t)(k < 3 ? iS + k : iNS4 + (k - 3));
    }
    for (size_t j = 0; j < w; ++j) {
      PowJob& b = JB[j];
      b.base = (uint32_t)(4 + 2 * j); b.exp[0] = (uint32_t)iNC; b.out[0] = b.base; b.fb[0][0] = (uint32_t)(iNS4 + j);
    }
    if ((rc = launch_pow_jobs(c, W_SH_JOBS, pow_var(1, 32, 1), JA, W, SC, X, Gt, Gt))) return rc;
    if ((rc = launch_pow_jobs(c, W_SH_JOBS, pow_var(1, 32, 1), JB, W, SC, X, Kt, Kt))) return rc;
  }
  // ... and for t3' and t4' times the products over N with the exponents s'
  if ((rc = sh_pp(c, G + 512, N, 1, sc(iSP), 1, N, X + xP * kW))) return rc;
  if ((rc = sh_pp(c, E2, 1, 2 * w, sc(iSP), 2 * w, N, X + (xP + 1) * kW))) return rc;
  if ((rc = sh_mul(c, X + 2 * kW, 1, X + xP * kW, 1, 1 + 2 * w, X + xM * kW))) return rc;
  if ((rc = ws_get(c, W_SH_BE, nT * 512, (void**)&BE1))) return rc;
  if ((rc = launch_export(c, X, 2, BE1)) || (rc = launch_export(c, X + xM * kW, 1 + 2 * w, BE1 + 1024))) return rc;
  // 5. that'_i = chain_i^{-c} g^{s^_i} * chain_{i-1}^{s'_i}
  {
    auto JA = new_jobs(N), JB = new_jobs(N);
    for (size_t i = 0; i < N; ++i) {
      PowJob& a = JA[i];
      a.base = (uint32_t)(vC + 1 + i); a.exp[0] = (uint32_t)iNC; a.out[0] = (uint32_t)(xH + 2 * i); a.fb[0][0] = (uint32_t)(iSH + i);
      PowJob& b = JB[i];
      b.base = (uint32_t)(vC + i); b.exp[0] = (uint32_t)(iSP + i); b.out[0] = (uint32_t)(xH + 2 * i + 1);
    }
    if ((rc = launch_pow_jobs(c, W_SH_JOBS, pow_var(1, 32, 1), JA, V, SC, X, Gt, Gt))) return rc;
    if ((rc = launch_pow_jobs(c, W_SH_JOBS, pow_var(), JB, V, SC, X, Gt, Gt))) return rc;
  }
  LAUNCH_F(c, k_mul, dim3(grid_for(N)), c->d, X + xH * kW, 2u, X + (xH + 1) * kW, 2u, (uint32_t)N, Y, 1u);
  HIPCHK(hipGetLastError());
  if ((rc = ws_get(c, W_SH_BE2, N * 512, (void**)&BE2))) return rc;
  if ((rc = launch_export(c, Y, N, BE2))) return rc;
  // 6. the challenge again, and the verdict
  if ((rc = sh_tree_rows(c, BE1 + 3 * 512, w, 2, sc(iT + 3))) || (rc = sh_tree_rows(c, BE2, N, 1, sc(iT + 4))) ||
      (rc = sh_tree_rows(c, chain, N, 1, sc(iT + 5))))
    return rc;
  if ((rc = sh_challenge_hash(c, CN, sc(iY), BE1, sc(iT + 3), sc(iC2)))) return rc;
  hipLaunchKernelGGL(k_sh_verdict, dim3(1), dim3(64), 0, c->stream, cc, sc(iC2), flag, ok, mask);
  HIPCHK(hipGetLastError());
  return EG_OK;
}

static int sh_verify(eg_ctx* c, bool host, const uint8_t* K_be, const uint8_t* qbar_be, const uint8_t* gseed_be,
                     size_t N, size_t w, const uint8_t* G, const uint8_t* E_be, const uint8_t* E2, const uint8_t* pc,
                     const uint8_t* chain, const uint8_t* cc, const uint8_t* s, const uint8_t* shat, const uint8_t* sp,
                     int check_inputs, uint8_t* ok, uint32_t* mask) {
  int rc;
  if (!c || !K_be || !qbar_be || !gseed_be || !G || !E_be || !E2 || !pc || !chain || !cc || !s || !shat || !sp || !ok ||
      !mask)
    return sh_fail("null context or pointer");
  if ((rc = sh_limits(N, w))) return rc;
  if (!host && !aligned16({G, E_be, E2, pc, chain, cc, s, shat, sp, ok, mask}))
    return sh_fail("device pointer not 16-byte aligned");
  Locked lk(c);
  if ((rc = use_key_locked(c, K_be))) return rc;
  HIPCHK(hipMemcpyAsync(c->d_qbar, qbar_be, 32, hipMemcpyHostToDevice, c->stream));
  uint8_t* CN = nullptr;
  if ((rc = sh_consts(c, K_be, gseed_be, N, w, &CN))) return rc;
  ShIO io{c, host, {}};
  io.in(G, (N + 2) * 512);
  io.in(E_be, N * w * 1024);
  io.in(E2, N * w * 1024);
  io.in(pc, N * 512);
  io.in(chain, N * 512);
  io.in(cc, 32);
  io.in(s, (3 + w) * 32);
  io.in(shat, N * 32);
  io.in(sp, N * 32);
  io.out(ok, 1);
  io.out(mask, 4);
  if ((rc = io.begin())) return rc;
  if ((rc = sh_verify_locked(c, CN, N, w, G, E_be, E2, pc, chain, cc, s, shat, sp, check_inputs, ok, mask))) return rc;
  return io.end();
}

extern "C" int eg_shuffle_verify_dev(eg_ctx* c, const uint8_t K_be[512], const uint8_t qbar_be[32],
                                     const uint8_t gseed_be[32], size_t N, size_t w, const uint8_t* d_G,
                                     const uint8_t* d_E, const uint8_t* d_E2, const uint8_t* d_pc,
                                     const uint8_t* d_chain, const uint8_t* d_c, const uint8_t* d_s,
                                     const uint8_t* d_s_hat, const uint8_t* d_s_prime, int check_inputs, uint8_t* d_ok,
                                     uint32_t* d_failed_mask) {
  return sh_verify(c, false, K_be, qbar_be, gseed_be, N, w, d_G, d_E, d_E2, d_pc, d_chain, d_c, d_s, d_s_hat, d_s_prime,
                   check_inputs, d_ok, d_failed_mask);
}

extern "C" int eg_shuffle_verify(eg_ctx* c, const uint8_t K_be[512], const uint8_t qbar_be[32],
                                 const uint8_t gseed_be[32], size_t N, size_t w, const uint8_t* G, const uint8_t* E,
                                 const uint8_t* E2, const uint8_t* pc, const uint8_t* chain, const uint8_t* c_in,
                                 const uint8_t* s, const uint8_t* s_hat, const uint8_t* s_prime, int check_inputs,
                                 uint8_t* ok, uint32_t* failed_mask) {
  return sh_verify(c, true, K_be, qbar_be, gseed_be, N, w, G, E, E2, pc, chain, c_in, s, s_hat, s_prime, check_inputs,
                   ok, failed_mask);
}
