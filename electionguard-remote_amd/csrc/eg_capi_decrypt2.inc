// eg_capi_decrypt2.inc — threshold decryption with one combined proof per text
// (include/eg_hip_decrypt2.h; DESIGN.md §18; included by eg_capi.hip after eg_capi_prodpow.inc:
// the trustee launch, the share-key tables and the hash helpers are eg_capi_ballot.inc's, the
// combine's chunk body eg_capi_prodpow.inc's).  Kernels: eg_decrypt2.hpp, k_pow, k_prod, k_mul,
// k_response, k_hash_check.  combine, check and verify and their _dev twins are one body each
// taking `bool host`, around one staged run (eg_stage.hpp) with a text as the item.

static_assert(EG_DECRYPT2_MAX_ITEMS == EG_PRODPOW_MAX_ITEMS, "the combine runs eg_prod_pow's chunk body");

static int d2_fail(const std::string& msg) { return fail(EG_ERR_ARG, "decrypt2: " + msg); }

// texts per chunk: 4 k exponentiations per text in the mediator (the formula of the header)
static size_t d2_chunk(size_t k) { return std::max<size_t>(1, EG_DECRYPT2_CHUNK_JOBS / (4 * k)); }

static int d2_limits(size_t n, size_t k) {
  if (!k) return d2_fail("no guardian (k == 0)");
  if (k > EG_DECRYPT2_MAX_GUARDIANS) return d2_fail("more than 64 guardians");
  if (n > EG_DECRYPT2_MAX_ITEMS / k) return d2_fail("n * k exceeds 2^24");
  return EG_OK;
}

// the call's constants in W_D2_CONST (the caller holds the lock): [tag 0x30 (32)][K (512)][rows]
constexpr size_t kD2Rows = 32 + 512;
static int d2_consts(eg_ctx* c, const uint8_t* K_be, const uint8_t* rows, size_t bytes, uint8_t** out) {
  int rc;
  std::vector<uint8_t> h(kD2Rows + bytes, 0);
  h[31] = EG_DECRYPT2_TAG;
  if (K_be) std::memcpy(&h[32], K_be, 512);
  if (bytes) std::memcpy(&h[kD2Rows], rows, bytes);
  if ((rc = ws_get(c, W_D2_CONST, h.size(), (void**)out))) return rc;
  HIPCHK(hipMemcpyAsync(*out, h.data(), h.size(), hipMemcpyHostToDevice, c->stream));
  return EG_OK;
}

// ---------------------------------------------------------------------------------
// round 1 and round 2 (the trustee; host pointers)
// ---------------------------------------------------------------------------------
extern "C" int eg_decrypt2_commit(eg_ctx* c, const uint8_t secret_be[32], const uint8_t* pads, const uint8_t* nonces,
                                  size_t n, uint8_t* out_M, uint8_t* out_a, uint8_t* out_b) {
  int rc;
  if (!c || !secret_be) return d2_fail("null context or secret");
  if ((rc = d2_limits(n, 1))) return rc;
  if (!n) return EG_OK;
  if (!pads || !nonces || !out_M || !out_a || !out_b) return d2_fail("null array");
  Locked L(c);
  // g's shared comb table first: building it runs its own job through W_JOBS / W_SCR
  const uint32_t* gc = nullptr;
  if ((rc = g_comb_table(c, &gc))) return rc;
  const size_t ch = d2_chunk(1);
  for (size_t i0 = 0; i0 < n; i0 += ch) {
    const size_t m = std::min(ch, n - i0);
    uint8_t *d_t = nullptr, *SC = nullptr, *OBE = nullptr;
    uint32_t *E = nullptr, *O = nullptr;
    if ((rc = upload(c, W_H0, pads + i0 * 512, m * 512, (void**)&d_t))) return rc;
    if ((rc = ws_get(c, W_SCAL, (m + 1) * 32, (void**)&SC))) return rc;
    HIPCHK(hipMemcpyAsync(SC, secret_be, 32, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(SC + 32, nonces + i0 * 32, m * 32, hipMemcpyHostToDevice, c->stream));
    if ((rc = ws_get(c, W_E0, m * kW * 4, (void**)&E))) return rc;
    if ((rc = launch_import(c, d_t, m, E, nullptr))) return rc;
    if ((rc = ws_get(c, W_E1, m * 3 * kW * 4, (void**)&O))) return rc;
    // M = A^z (out 3 i), a = g^u (out 3 i + 1), b = A^u (out 3 i + 2): z and u only ever drive the
    // constant-time comb
    if ((rc = trustee_pair_launch(c, gc, E, 1, SC, m, O))) return rc;
    if ((rc = ws_get(c, W_BE0, m * 3 * 512, (void**)&OBE))) return rc;
    if ((rc = launch_export(c, O, m * 3, OBE))) return rc;
    HIPCHK(hipMemcpy2DAsync(out_M + i0 * 512, 512, OBE, 1536, 512, m, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpy2DAsync(out_a + i0 * 512, 512, OBE + 512, 1536, 512, m, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpy2DAsync(out_b + i0 * 512, 512, OBE + 1024, 1536, 512, m, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  return EG_OK;
}

extern "C" int eg_decrypt2_respond(eg_ctx* c, const uint8_t secret_be[32], const uint8_t* nonces,
                                   const uint8_t* challenges, size_t n, uint8_t* out_v) {
  int rc;
  if (!c || !secret_be) return d2_fail("null context or secret");
  if ((rc = d2_limits(n, 1))) return rc;
  if (!n) return EG_OK;
  if (!nonces || !challenges || !out_v) return d2_fail("null array");
  Locked L(c);
  const size_t ch = d2_chunk(1);
  for (size_t i0 = 0; i0 < n; i0 += ch) {
    const size_t m = std::min(ch, n - i0);
    // scalars: [z][u x m][c x m], reduced mod q in place by the branch-free ladder
    uint8_t *SC = nullptr, *PR = nullptr;
    if ((rc = ws_get(c, W_SCAL, (2 * m + 1) * 32, (void**)&SC))) return rc;
    HIPCHK(hipMemcpyAsync(SC, secret_be, 32, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(SC + 32, nonces + i0 * 32, m * 32, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(SC + (1 + m) * 32, challenges + i0 * 32, m * 32, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_reduce_q, dim3(cgrid(2 * m + 1)), dim3(kBlock), 0, c->stream, c->d_q, SC, (uint64_t)(2 * m + 1), SC);
    HIPCHK(hipGetLastError());
    if ((rc = ws_get(c, W_OK1, m * 64, (void**)&PR))) return rc;
    hipLaunchKernelGGL(k_response, dim3(cgrid(m)), dim3(256), 0, c->stream, c->d_q, SC + 32, SC + (1 + m) * 32, SC, 0u,
                       (uint32_t)m, PR, 0u);  // the minus convention, whatever the ctx's
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy2DAsync(out_v + i0 * 32, 32, PR + 32, 64, 32, m, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  return EG_OK;
}

// ---------------------------------------------------------------------------------
// combine (the mediator between the rounds)
// ---------------------------------------------------------------------------------
// One chunk of m <= d2_chunk(k) texts on device pointers (the caller holds the lock; d_qbar is set;
// CN: the call's constants with the k weights as its rows).
static int d2_combine_chunk_locked(eg_ctx* c, const PpShape& S, size_t m, size_t k, const uint8_t* CN,
                                   const uint8_t* texts, const uint8_t* shares, const uint8_t* comm, uint8_t* out_M,
                                   uint8_t* out_c, uint8_t* out_ci) {
  int rc;
  const size_t E = (size_t)kW * 4;
  // M = PROD_i M_i^{w_i}: eg_prod_pow_dev's chunk body, rows within its per-row budget
  const size_t rcn = std::max<size_t>(1, std::min(m, kPpRowBudget / S.per_row(k)));
  for (size_t r0 = 0; r0 < m; r0 += rcn) {
    const size_t rr = std::min(rcn, m - r0);
    uint32_t* acc = nullptr;
    if ((rc = pp_chunk_locked(c, S, shares + r0 * k * 512, k, 1, CN + kD2Rows, rr, k, true))) return rc;
    if ((rc = ws_get(c, W_PP_ACC, rr * E, (void**)&acc))) return rc;
    if ((rc = launch_export(c, acc, rr, out_M + r0 * 512))) return rc;
  }
  // a = PROD a_i, b = PROD b_i: groups (text, which) of k elements, 2 apart
  uint32_t *CE = nullptr, *AB = nullptr;
  uint8_t* ABBE = nullptr;
  if ((rc = ws_get(c, W_E0, m * k * 2 * E, (void**)&CE))) return rc;
  if ((rc = launch_import(c, comm, m * k * 2, CE, nullptr))) return rc;
  if ((rc = ws_get(c, W_E1, m * 2 * E, (void**)&AB))) return rc;
  if ((rc = run_prod(c, CE, GroupMap{2, 1, 1, 0, (uint32_t)(2 * k)}, m * 2, k, 2, AB))) return rc;
  if ((rc = ws_get(c, W_BE0, m * 2 * 512, (void**)&ABBE))) return rc;
  if ((rc = launch_export(c, AB, m * 2, ABBE))) return rc;
  // c = H(qbar, 0x30, K, A, B, a, b, M) on the device, then c_i = c w_i
  if ((rc = launch_hash(c, (uint32_t)m,
                        {HashSrc{CN, 32, 0}, HashSrc{CN + 32, 512, 0}, HashSrc{texts, 512, 1024},
                         HashSrc{texts + 512, 512, 1024}, HashSrc{ABBE, 512, 1024}, HashSrc{ABBE + 512, 512, 1024},
                         HashSrc{out_M, 512, 512}},
                        nullptr, 0, 0, kNone, nullptr, nullptr, 0, nullptr, out_c)))
    return rc;
  hipLaunchKernelGGL(k_d2_ci, dim3(cgrid(m * k)), dim3(kBlock), 0, c->stream, c->d_q, out_c, CN + kD2Rows,
                     (uint64_t)(m * k), (uint32_t)k, out_ci);
  HIPCHK(hipGetLastError());
  return EG_OK;
}

static int d2_combine(eg_ctx* c, bool host, const uint8_t* K_be, const uint8_t* qbar_be, size_t n, size_t k,
                      const uint8_t* weights, const uint8_t* texts, const uint8_t* shares, const uint8_t* comm,
                      uint8_t* out_M, uint8_t* out_c, uint8_t* out_ci) {
  int rc;
  if (!c || !K_be || !qbar_be || !weights) return d2_fail("null context, key, qbar or weights");
  if ((rc = d2_limits(n, k))) return rc;
  if (!n) return EG_OK;
  if (!texts || !shares || !comm || !out_M || !out_c || !out_ci) return d2_fail("null array");
  if (!host && !aligned16({texts, shares, comm, out_M, out_c, out_ci}))
    return d2_fail("device pointer not 16-byte aligned");
  const size_t ch = d2_chunk(k);
  int mt = 0, w = 0;
  if ((rc = eg_prod_pow_plan(std::min(n, ch), k, EG_PRODPOW_AUTO, 0, &mt, &w, nullptr))) return rc;
  const PpShape S = pp_shape(mt, w, k);
  Locked lk(c);
  HIPCHK(hipMemcpyAsync(c->d_qbar, qbar_be, 32, hipMemcpyHostToDevice, c->stream));
  uint8_t* CN = nullptr;
  if ((rc = d2_consts(c, K_be, weights, k * 32, &CN))) return rc;
  Stage st(c, host, n, ch);
  st.in(texts, 1024);
  st.in(shares, k * 512);
  st.in(comm, k * 1024);
  st.out(out_M, 512);
  st.out(out_c, 32);
  st.out(out_ci, k * 32);
  return st.run([&](size_t m) {
    return d2_combine_chunk_locked(c, S, m, k, CN, texts, shares, comm, out_M, out_c, out_ci);
  });
}

extern "C" int eg_decrypt2_combine_dev(eg_ctx* c, const uint8_t K_be[512], const uint8_t qbar_be[32], size_t n,
                                       size_t k, const uint8_t* weights, const uint8_t* d_texts,
                                       const uint8_t* d_shares, const uint8_t* d_comm, uint8_t* d_out_M,
                                       uint8_t* d_out_c, uint8_t* d_out_ci) {
  return d2_combine(c, false, K_be, qbar_be, n, k, weights, d_texts, d_shares, d_comm, d_out_M, d_out_c, d_out_ci);
}

extern "C" int eg_decrypt2_combine(eg_ctx* c, const uint8_t K_be[512], const uint8_t qbar_be[32], size_t n, size_t k,
                                   const uint8_t* weights, const uint8_t* texts, const uint8_t* shares,
                                   const uint8_t* comm, uint8_t* out_M, uint8_t* out_c, uint8_t* out_ci) {
  return d2_combine(c, true, K_be, qbar_be, n, k, weights, texts, shares, comm, out_M, out_c, out_ci);
}

// ---------------------------------------------------------------------------------
// check (the mediator after round 2)
// ---------------------------------------------------------------------------------
// One chunk of m texts, N = m k items j = t k + i.  Elements [Z (k)][A, B (2 m)][M_i (N)], scalars
// [c_i (N)][v_i (N)], outputs [a, b (2 N)][A^v, M_i^c (2 N)].  kt: the guardians' cached tables, or
// empty for variable bases Z_i (d_Z: their bytes).
static int d2_check_chunk_locked(eg_ctx* c, size_t m, size_t k, const uint8_t* d_Z,
                                 const std::vector<eg_fixed_base*>& kt, const uint8_t* texts, const uint8_t* shares,
                                 const uint8_t* comm, const uint8_t* ci, const uint8_t* vi, uint8_t* ok,
                                 uint8_t* out_v) {
  int rc;
  const size_t N = m * k, oT = k, oS = k + 2 * m;
  const bool tabs = !kt.empty();
  uint32_t *E = nullptr, *O = nullptr;
  uint8_t *SC = nullptr, *OKR = nullptr, *OBE = nullptr;
  if ((rc = ws_get(c, W_E0, (oS + N) * kW * 4, (void**)&E))) return rc;
  if (!tabs && (rc = launch_import(c, d_Z, k, E, nullptr))) return rc;
  if ((rc = launch_import(c, texts, 2 * m, E + oT * kW, nullptr))) return rc;
  if ((rc = launch_import(c, shares, N, E + oS * kW, nullptr))) return rc;
  if ((rc = ws_get(c, W_SCAL, N * 64, (void**)&SC))) return rc;
  HIPCHK(hipMemcpyAsync(SC, ci, N * 32, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(SC + N * 32, vi, N * 32, hipMemcpyDeviceToDevice, c->stream));
  if ((rc = ws_get(c, W_OK0, N, (void**)&OKR))) return rc;
  hipLaunchKernelGGL(k_d2_range, dim3(cgrid(N)), dim3(kBlock), 0, c->stream, c->d_q, ci, vi, 32u, (uint64_t)N, OKR);
  HIPCHK(hipGetLastError());
  if ((rc = ws_get(c, W_E1, 4 * N * kW * 4, (void**)&O))) return rc;
  if ((rc = ws_get(c, W_BE0, 2 * N * 512, (void**)&OBE))) return rc;
  // elements [Z (k)][A, B (2 m)][M_i (N)], scalars [c_i (N)][v_i (N)]; Z_i a variable base
  // (item j's is element j % k) unless the guardians' tables are given; outputs: pairs
  // a = Z_i^{c_i} g^{v_i}, b = A^{v_i} M_i^{c_i}, the factors of b behind them
  CpLayout CP{};
  CP.n = N; CP.k = k;
  CP.eX = 0; CP.nX = (uint32_t)k; CP.eA = (uint32_t)oT; CP.eM = (uint32_t)oS;
  CP.sC = 0; CP.sV = (uint32_t)N; CP.ds = 1; CP.sNeg = kNone;
  CP.so = 2; CP.oT = (uint32_t)(2 * N); CP.dT = 2;
  for (eg_fixed_base* t : kt) CP.tabs.push_back(t->tab());
  if ((rc = cp_recompute(c, CP, E, SC, O, OBE))) return rc;
  hipLaunchKernelGGL(k_d2_match, dim3(cgrid(N)), dim3(kBlock), 0, c->stream, OBE, comm, OKR, (uint64_t)N, ok);
  hipLaunchKernelGGL(k_d2_vsum, dim3(cgrid(m)), dim3(kBlock), 0, c->stream, c->d_q, vi, (uint64_t)m, (uint32_t)k, out_v);
  HIPCHK(hipGetLastError());
  return EG_OK;
}

static int d2_check(eg_ctx* c, bool host, size_t n, size_t k, const uint8_t* Z, const uint8_t* texts,
                    const uint8_t* shares, const uint8_t* comm, const uint8_t* ci, const uint8_t* vi, uint8_t* ok,
                    uint8_t* out_v) {
  int rc;
  if (!c || !Z) return d2_fail("null context or share keys");
  if ((rc = d2_limits(n, k))) return rc;
  if (!n) return EG_OK;
  if (!texts || !shares || !comm || !ci || !vi || !ok || !out_v) return d2_fail("null array");
  if (!host && !aligned16({texts, shares, comm, ci, vi, out_v})) return d2_fail("device pointer not 16-byte aligned");
  Locked lk(c);
  // a call of many texts and few guardians reads Z_i^c from the guardians' cached radix tables, as
  // eg_verify_shares does for one key; k <= the cache's size, so none of them is dropped meanwhile
  std::vector<eg_fixed_base*> kt;
  if (n >= kShareTableMin && k <= kShareTableCache) {
    kt.resize(k);
    for (size_t i = 0; i < k; ++i)
      if ((rc = share_key_table(c, Z + i * 512, &kt[i]))) return rc;
  }
  uint8_t* CN = nullptr;
  if ((rc = d2_consts(c, nullptr, Z, k * 512, &CN))) return rc;
  Stage st(c, host, n, d2_chunk(k));
  st.in(texts, 1024);
  st.in(shares, k * 512);
  st.in(comm, k * 1024);
  st.in(ci, k * 32);
  st.in(vi, k * 32);
  st.out(ok, k);
  st.out(out_v, 32);
  return st.run([&](size_t m) {
    return d2_check_chunk_locked(c, m, k, CN + kD2Rows, kt, texts, shares, comm, ci, vi, ok, out_v);
  });
}

extern "C" int eg_decrypt2_check_dev(eg_ctx* c, size_t n, size_t k, const uint8_t* Z, const uint8_t* d_texts,
                                     const uint8_t* d_shares, const uint8_t* d_comm, const uint8_t* d_ci,
                                     const uint8_t* d_vi, uint8_t* d_ok, uint8_t* d_out_v) {
  return d2_check(c, false, n, k, Z, d_texts, d_shares, d_comm, d_ci, d_vi, d_ok, d_out_v);
}

extern "C" int eg_decrypt2_check(eg_ctx* c, size_t n, size_t k, const uint8_t* Z, const uint8_t* texts,
                                 const uint8_t* shares, const uint8_t* comm, const uint8_t* ci, const uint8_t* vi,
                                 uint8_t* ok, uint8_t* out_v) {
  return d2_check(c, true, n, k, Z, texts, shares, comm, ci, vi, ok, out_v);
}

// ---------------------------------------------------------------------------------
// verify (anyone, from the record)
// ---------------------------------------------------------------------------------
// One chunk of m texts: eg_verify_shares' structure with K's table for the key term and the
// tagged pre-image.  Elements [A, B (2 m)][M (m)], scalars the proof rows (c, v), outputs
// [a', b' (2 m)][A^v, M^c (2 m)].
static int d2_verify_chunk_locked(eg_ctx* c, size_t m, const uint8_t* CN, const uint8_t* texts, const uint8_t* M,
                                  const uint8_t* proofs, uint8_t* ok) {
  int rc;
  uint32_t *E = nullptr, *O = nullptr;
  uint8_t *SC = nullptr, *OKR = nullptr, *OBE = nullptr;
  if ((rc = ws_get(c, W_E0, 3 * m * kW * 4, (void**)&E))) return rc;
  if ((rc = launch_import(c, texts, 2 * m, E, nullptr))) return rc;
  if ((rc = launch_import(c, M, m, E + 2 * m * kW, nullptr))) return rc;
  if ((rc = ws_get(c, W_SCAL, m * 64, (void**)&SC))) return rc;
  HIPCHK(hipMemcpyAsync(SC, proofs, m * 64, hipMemcpyDeviceToDevice, c->stream));
  if ((rc = ws_get(c, W_OK0, m, (void**)&OKR))) return rc;
  hipLaunchKernelGGL(k_d2_range, dim3(cgrid(m)), dim3(kBlock), 0, c->stream, c->d_q, proofs, proofs + 32, 64u,
                     (uint64_t)m, OKR);
  HIPCHK(hipGetLastError());
  if ((rc = ws_get(c, W_E1, 4 * m * kW * 4, (void**)&O))) return rc;
  if ((rc = ws_get(c, W_BE0, 2 * m * 512, (void**)&OBE))) return rc;
  // elements [A, B (2 m)][M (m)], scalars the proof rows (c, v); the key is K's table, so no
  // X elements (eX, nX unused); outputs: pairs a' = g^v K^c, b' = A^v M^c, b's factors behind them
  CpLayout CP{};
  CP.n = m; CP.k = 1;
  CP.eA = 0; CP.eM = (uint32_t)(2 * m);
  CP.sC = 0; CP.sV = 1; CP.ds = 2; CP.sNeg = kNone;
  CP.so = 2; CP.oT = (uint32_t)(2 * m); CP.dT = 2;
  CP.tabs = {c->Ktab->tab()};
  if ((rc = cp_recompute(c, CP, E, SC, O, OBE))) return rc;
  return launch_hash(c, (uint32_t)m,
                     {HashSrc{CN, 32, 0}, key_src(c), HashSrc{texts, 512, 1024}, HashSrc{texts + 512, 512, 1024},
                      HashSrc{OBE, 512, 1024}, HashSrc{OBE + 512, 512, 1024}, HashSrc{M, 512, 512}},
                     proofs, 2, 0, kNone, OKR, nullptr, 0, ok, nullptr);
}

static int d2_verify(eg_ctx* c, bool host, const uint8_t* K_be, const uint8_t* qbar_be, size_t n, const uint8_t* texts,
                     const uint8_t* M, const uint8_t* proofs, uint8_t* ok) {
  int rc;
  if (!c || !K_be || !qbar_be) return d2_fail("null context, key or qbar");
  if ((rc = d2_limits(n, 1))) return rc;
  if (!n) return EG_OK;
  if (!texts || !M || !proofs || !ok) return d2_fail("null array");
  if (!host && !aligned16({texts, M, proofs})) return d2_fail("device pointer not 16-byte aligned");
  Locked lk(c);
  if ((rc = use_key_locked(c, K_be))) return rc;
  HIPCHK(hipMemcpyAsync(c->d_qbar, qbar_be, 32, hipMemcpyHostToDevice, c->stream));
  uint8_t* CN = nullptr;
  if ((rc = d2_consts(c, K_be, nullptr, 0, &CN))) return rc;
  Stage st(c, host, n, d2_chunk(1));
  st.in(texts, 1024);
  st.in(M, 512);
  st.in(proofs, 64);
  st.out(ok, 1);
  return st.run([&](size_t m) { return d2_verify_chunk_locked(c, m, CN, texts, M, proofs, ok); });
}

extern "C" int eg_decrypt2_verify_dev(eg_ctx* c, const uint8_t K_be[512], const uint8_t qbar_be[32], size_t n,
                                      const uint8_t* d_texts, const uint8_t* d_M, const uint8_t* d_proofs,
                                      uint8_t* d_ok) {
  return d2_verify(c, false, K_be, qbar_be, n, d_texts, d_M, d_proofs, d_ok);
}

extern "C" int eg_decrypt2_verify(eg_ctx* c, const uint8_t K_be[512], const uint8_t qbar_be[32], size_t n,
                                  const uint8_t* texts, const uint8_t* M, const uint8_t* proofs, uint8_t* ok) {
  return d2_verify(c, true, K_be, qbar_be, n, texts, M, proofs, ok);
}
