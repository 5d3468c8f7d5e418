// eg_capi_range.inc — 0..L range proofs of ciphertexts (include/eg_hip_range.h; included by
// eg_capi.hip after eg_capi_contestdata.inc: the key, table, job-cache and launch helpers are
// eg_capi_ballot.inc's).  Kernels: eg_range.hpp and k_pow.  eg_range_verify / eg_range_prove and
// their _dev twins are one body each taking `bool host`, around one staged run (eg_stage.hpp) of
// the chunk function.
//
// Verifier jobs per item (B = L + 1 branches).  Branches 0 and 1 are the selection verifier's
// pair jobs, one per base: the alpha job is its SA shape (a_0, a_1; comb shared by e_0, e_1), the
// beta job its SB shape (b_0, b_1 with the g term -e_1), both with the residue pair (resid = 1)
// and both keeping their comb powers y_k = base^(2^(52 k)) (yout).  Every further branch j >= 2 is
// one single-output comb job per base that takes those powers back (gather = 1: four loads instead
// of 208 squarings) and builds only its 32-entry subset table.  A gather job's record holds the
// source job in J[2], where a pair job holds its second exponent, so gather jobs carry one
// exponent each; DESIGN.md §13 has the multiply counts of this choice against rebuilt pairs.

static_assert(EG_RANGE_MAX_LIMIT == 15, "eg_hip_range.h and the chunk sizing disagree");

// Items per chunk: a chunk holds at most kRangeChunkJobs verifier jobs (2 L per item), so the
// k_pow scratch and the commitment space shrink per item as L grows (32,768 items at L = 1, 2,184
// at L = 15).  The prover (L + 2 jobs per item) uses the same item count.
static constexpr size_t kRangeChunkJobs = (size_t)1 << 16;
static size_t range_chunk(uint32_t L) { return std::max<size_t>(1, kRangeChunkJobs / (2 * (size_t)L)); }

static int range_args(eg_ctx* c, const uint8_t* K_be, const uint8_t* qbar_be, size_t n, uint32_t L, bool data_ok) {
  if (!c || !K_be || !qbar_be || (n && !data_ok)) return fail(EG_ERR_ARG, "range: null argument");
  if (L < 1 || L > EG_RANGE_MAX_LIMIT) return fail(EG_ERR_ARG, "range: limit outside [1, 15]");
  return EG_OK;
}

// ---------------------------------------------------------------------------------
// verify
// ---------------------------------------------------------------------------------
// One chunk of n <= range_chunk(L) items, device pointers, enqueued on the ctx stream (d_qbar and
// the key are set by the caller, who holds the lock).
static int range_verify_chunk_locked(eg_ctx* c, size_t n, uint32_t L, const uint8_t* d_cts, const uint8_t* d_proofs,
                                     uint8_t* d_ok) {
  const FbTab G = c->gtab->tab(), K = c->Ktab->tab();
  const size_t B = (size_t)L + 1, nx = n * (B - 2);  // nx: jobs of the branches past the first pair, per base
  int rc;
  uint32_t *E = nullptr, *COMM = nullptr, *YA = nullptr, *YB = nullptr, *RZ = nullptr;
  uint8_t *LTP = nullptr, *SC = nullptr, *OKS = nullptr, *COMM_BE = nullptr;
  // scalars: [proof rows n*2B (c_j, v_j)][g terms n*B (-j e_j)]
  const size_t off_g = n * 2 * B;
  if ((rc = ws_get(c, W_E0, n * 2 * kW * 4, (void**)&E))) return rc;
  if ((rc = ws_get(c, W_E1, n * 2 * B * kW * 4, (void**)&COMM))) return rc;
  if ((rc = ws_get(c, W_FLAGS, n * 2, (void**)&LTP))) return rc;
  if ((rc = ws_get(c, W_SCAL, (off_g + n * B) * 32, (void**)&SC))) return rc;
  if ((rc = ws_get(c, W_OK0, n, (void**)&OKS))) return rc;
  if ((rc = ws_get(c, W_BE0, n * 2 * B * 512, (void**)&COMM_BE))) return rc;
  if ((rc = ws_get(c, W_YA, n * (kCombH - 1) * kW * 4, (void**)&YA))) return rc;
  if ((rc = ws_get(c, W_YB, n * (kCombH - 1) * kW * 4, (void**)&YB))) return rc;
  if ((rc = ws_get(c, W_RZ, n * 4 * kW * 4, (void**)&RZ))) return rc;
  // 1. import the ciphertexts (range flags alpha, beta < p)
  if ((rc = launch_import(c, d_cts, n * 2, E, LTP))) return rc;
  // 2. scalars: a working copy of the proofs (negated in place under EG_RESPONSE_PLUS), the g terms
  HIPCHK(hipMemcpyAsync(SC, d_proofs, n * B * 64, hipMemcpyDeviceToDevice, c->stream));
  hipLaunchKernelGGL(k_range_scalars, dim3(cgrid(n)), dim3(kBlock), 0, c->stream, c->d_q, SC, (uint64_t)n, L,
                     SC + off_g * 32, OKS, c->resp_plus);
  HIPCHK(hipGetLastError());
  // 3. commitments
  const std::string key = "rv/" + std::to_string(n) + "/" + std::to_string(L);
  std::vector<const uint32_t*> jv;
  rc = cached_job_set(c, key, {"A", "B", "XA", "XB"}, [&]() {
    auto A = new_jobs(n), Bj = new_jobs(n), XA = new_jobs(nx), XB = new_jobs(nx);
    for (size_t i = 0; i < n; ++i) {
      const uint32_t s0 = (uint32_t)(i * 2 * B), o0 = (uint32_t)(i * 2 * B);  // scalar / commitment row of item i
      PowJob& a = A[i];
      PowJob& b = Bj[i];
      a.base = (uint32_t)(i * 2); a.exp[0] = s0; a.exp[1] = s0 + 2; a.out[0] = o0; a.out[1] = o0 + 2;
      a.fb[0][0] = s0 + 1; a.fb[1][0] = s0 + 3;
      b.base = (uint32_t)(i * 2 + 1); b.exp[0] = s0; b.exp[1] = s0 + 2; b.out[0] = o0 + 1; b.out[1] = o0 + 3;
      b.fb[0][0] = s0 + 1; b.fb[1][0] = s0 + 3; b.fb[1][1] = (uint32_t)(off_g + i * B + 1);
      for (size_t j = 2; j < B; ++j) {
        PowJob& xa = XA[i * (B - 2) + (j - 2)];
        PowJob& xb = XB[i * (B - 2) + (j - 2)];
        const uint32_t cj = s0 + (uint32_t)(2 * j), vj = cj + 1;
        xa.base = (uint32_t)(i * 2); xa.exp[0] = cj; xa.gather_src() = (uint32_t)i;
        xa.out[0] = o0 + (uint32_t)(2 * j); xa.fb[0][0] = vj;
        xb.base = (uint32_t)(i * 2 + 1); xb.exp[0] = cj; xb.gather_src() = (uint32_t)i;
        xb.out[0] = o0 + (uint32_t)(2 * j + 1); xb.fb[0][0] = vj; xb.fb[0][1] = (uint32_t)(off_g + i * B + j);
      }
    }
    return JobSet{std::move(A), std::move(Bj), std::move(XA), std::move(XB)};
  }, jv);
  if (rc) return rc;
  const bool gat = c->use_comb != 0;
  // the selection verifier's shapes: a_0 = alpha^e0 g^v0, a_1 = alpha^e1 g^v1 and
  // b_0 = beta^e0 K^v0, b_1 = beta^e1 K^v1 g^-e1; the beta pair jobs ride in the alpha launch's
  // last sub-launch
  const PowPop PA{pow_sel_pair(false, c->sel_rows, c->sel_blocks), jv[0], n, gat ? YA : nullptr, nullptr, RZ};
  const PowPop PB{pow_sel_pair(true, c->sel_rows, c->sel_blocks), jv[1], n, gat ? YB : nullptr, nullptr,
                  RZ + n * 2 * kW};
  if ((rc = launch_pow(c, PA, E, SC, COMM, G, K, {PB}))) return rc;
  if (nx) {
    // a_j = alpha^ej g^vj and b_j = beta^ej K^vj g^(-j ej) on the pair job's comb powers
    const PowPop XA{pow_sel_gather(false, gat ? 1u : 0u), jv[2], nx, nullptr, YA};
    const PowPop XB{pow_sel_gather(true, gat ? 1u : 0u), jv[3], nx, nullptr, YB};
    if ((rc = launch_pow(c, XA, E, SC, COMM, G, K, {XB}))) return rc;
  }
  // alpha^q == 1 and beta^q == 1 fold into the range flags.  From here on LTP (W_FLAGS) holds, for
  // item i of this call, its alpha's flag at [2 i] and its beta's at [2 i + 1]: range (k_import)
  // AND residue.  b2_verify_chunk_locked (eg_capi_ballot2.inc) reads them there after this
  // function returns and before its next call, for the contests' verdicts: keep the slot and layout.
  LAUNCH_F(c, k_resid_check, dim3(grid_for(n)), c->d, RZ, (uint32_t)n, LTP, 2u);
  LAUNCH_F(c, k_resid_check, dim3(grid_for(n)), c->d, RZ + n * 2 * kW, (uint32_t)n, LTP + 1, 2u);
  HIPCHK(hipGetLastError());
  // 4. canonical bytes of the commitments, 5. the Fiat-Shamir check on the caller's proof rows
  if ((rc = launch_export(c, COMM, n * 2 * B, COMM_BE))) return rc;
  hipLaunchKernelGGL(k_range_hash, dim3(cgrid(n)), dim3(kBlock), 0, c->stream, c->d_q, c->d_qbar, (uint64_t)n, L, d_cts,
                     COMM_BE, c->keys.front().d_K, c->pre_order, d_proofs, OKS, LTP, d_ok, (uint8_t*)nullptr,
                     c->hash_fmt);
  HIPCHK(hipGetLastError());
  return EG_OK;
}

// the key, qbar, then the items in chunks: in host mode the device holds one chunk however many come in
static int range_verify(eg_ctx* c, bool host, const uint8_t* K_be, const uint8_t* qbar_be, size_t n, uint32_t L,
                        const uint8_t* cts, const uint8_t* proofs, uint8_t* ok) {
  int rc;
  if ((rc = range_args(c, K_be, qbar_be, n, L, cts && proofs && ok))) return rc;
  if (!host && !aligned16({cts, proofs})) return fail(EG_ERR_ARG, "range: device pointer not 16-byte aligned");
  if (!n) return EG_OK;
  Locked lk(c);
  if ((rc = use_key_locked(c, K_be))) return rc;
  HIPCHK(hipMemcpyAsync(c->d_qbar, qbar_be, 32, hipMemcpyHostToDevice, c->stream));
  Stage st(c, host, n, range_chunk(L));
  st.in(cts, 1024);
  st.in(proofs, ((size_t)L + 1) * 64);
  st.out(ok, 1);
  return st.run([&](size_t m) { return range_verify_chunk_locked(c, m, L, cts, proofs, ok); });
}

extern "C" int eg_range_verify_dev(eg_ctx* c, const uint8_t K_be[512], const uint8_t qbar_be[32], size_t n, uint32_t L,
                                   const uint8_t* d_cts, const uint8_t* d_proofs, uint8_t* d_ok) {
  return range_verify(c, false, K_be, qbar_be, n, L, d_cts, d_proofs, d_ok);
}

extern "C" int eg_range_verify(eg_ctx* c, const uint8_t K_be[512], const uint8_t qbar_be[32], size_t n, uint32_t L,
                               const uint8_t* cts, const uint8_t* proofs, uint8_t* ok) {
  return range_verify(c, true, K_be, qbar_be, n, L, cts, proofs, ok);
}

// ---------------------------------------------------------------------------------
// prove
// ---------------------------------------------------------------------------------
// One chunk of n <= range_chunk(L) items, device pointers.  Fixed-base only, like
// encrypt_chunk_locked: per item B simulated pairs (a_j, b_j) = (g^s_j, K^s_j g^t_j) into the
// item's commitment row and the real pair (g^u, K^u) apart, whatever the value; k_range_order
// then puts the real pair at branch m with masks.  The job tables do not depend on the values.
static int range_prove_chunk_locked(eg_ctx* c, size_t n, uint32_t L, const uint8_t* d_cts, const uint8_t* d_values,
                                    const uint8_t* d_R, const uint8_t* d_nonces, uint8_t* d_proofs) {
  int rc;
  FbTab G{}, K{};
  if ((rc = enc_tables_locked(c, &G, &K))) return rc;
  const bool ct = c->ct_encrypt != 0;
  const size_t B = (size_t)L + 1, nw = 2 * B + 1;
  // scalars: [nonces n*nw (u, c_0, v_0, ...)][s n*B][t n*B]
  const size_t off_s = n * nw, off_t = off_s + n * B;
  // elements: [commitments n*2B][real pairs n*2]
  const size_t oRE = n * 2 * B, nU = oRE + n * 2;
  uint8_t *SC = nullptr, *CH = nullptr, *COMM_BE = nullptr;
  uint32_t* U = nullptr;
  if ((rc = ws_get(c, W_SCAL, (off_t + n * B) * 32, (void**)&SC))) return rc;
  if ((rc = ws_get(c, W_E0, nU * kW * 4, (void**)&U))) return rc;
  if ((rc = ws_get(c, W_BE0, oRE * 512, (void**)&COMM_BE))) return rc;
  if ((rc = ws_get(c, W_OK0, n * 32, (void**)&CH))) return rc;
  HIPCHK(hipMemcpyAsync(SC, d_nonces, n * nw * 32, hipMemcpyDeviceToDevice, c->stream));
  hipLaunchKernelGGL(k_range_prep, dim3(cgrid(n)), dim3(kBlock), 0, c->stream, c->d_q, d_values, SC, d_R, (uint64_t)n,
                     L, SC + off_s * 32, SC + off_t * 32, c->resp_plus);
  HIPCHK(hipGetLastError());
  const std::string key = "rp/" + std::to_string(n) + "/" + std::to_string(L);
  std::vector<const uint32_t*> jv;
  rc = cached_job_set(c, key, {"S", "R"}, [&]() {
    auto S = new_jobs(n * B), Rj = new_jobs(n);
    for (size_t i = 0; i < n; ++i) {
      for (size_t j = 0; j < B; ++j) {
        PowJob& s = S[i * B + j];  // a_j = g^s_j ; b_j = K^s_j g^t_j
        const uint32_t sj = (uint32_t)(off_s + i * B + j);
        s.out[0] = (uint32_t)(i * 2 * B + 2 * j); s.out[1] = s.out[0] + 1; s.fb[0][0] = sj; s.fb[1][0] = sj;
        s.fb[1][1] = (uint32_t)(off_t + i * B + j);
      }
      PowJob& r = Rj[i];  // g^u ; K^u
      r.out[0] = (uint32_t)(oRE + i * 2); r.out[1] = r.out[0] + 1; r.fb[0][0] = (uint32_t)(i * nw); r.fb[1][0] = r.fb[0][0];
    }
    return JobSet{std::move(S), std::move(Rj)};
  }, jv);
  if (rc) return rc;
  // the real pairs fill the simulated pairs' last round
  if ((rc = launch_pow(c, {pow_fb_pair(true), jv[0], n * B}, U, SC, U, G, K, {{pow_fb_pair(false), jv[1], n}, {}, ct})))
    return rc;
  constexpr size_t kQuads = 2 * kW / 4;
  hipLaunchKernelGGL(k_range_order, dim3(cgrid(n * kQuads)), dim3(kBlock), 0, c->stream, U, U + oRE * kW, d_values,
                     (uint64_t)n, L);
  HIPCHK(hipGetLastError());
  if ((rc = launch_export(c, U, oRE, COMM_BE))) return rc;
  hipLaunchKernelGGL(k_range_hash, dim3(cgrid(n)), dim3(kBlock), 0, c->stream, c->d_q, c->d_qbar, (uint64_t)n, L, d_cts,
                     COMM_BE, c->keys.front().d_K, c->pre_order, (const uint8_t*)nullptr, (const uint8_t*)nullptr,
                     (const uint8_t*)nullptr, (uint8_t*)nullptr, CH, c->hash_fmt);
  hipLaunchKernelGGL(k_range_finish, dim3(cgrid(n)), dim3(kBlock), 0, c->stream, c->d_q, d_values, SC, d_R, CH,
                     (uint64_t)n, L, d_proofs, c->resp_plus);
  HIPCHK(hipGetLastError());
  return EG_OK;
}

// host values are checked here and name the item; device values past L give an all-zero proof
static int range_prove(eg_ctx* c, bool host, const uint8_t* K_be, const uint8_t* qbar_be, size_t n, uint32_t L,
                       const uint8_t* cts, const uint8_t* values, const uint8_t* R, const uint8_t* nonces,
                       uint8_t* proofs) {
  int rc;
  if ((rc = range_args(c, K_be, qbar_be, n, L, cts && values && R && nonces && proofs))) return rc;
  if (!host && !aligned16({cts, R, nonces, proofs}))
    return fail(EG_ERR_ARG, "range: device pointer not 16-byte aligned");
  for (size_t i = 0; host && i < n; ++i)
    if (values[i] > L)
      return fail(EG_ERR_ARG, "range: values[" + std::to_string(i) + "] = " + std::to_string((unsigned)values[i]) +
                                  " exceeds the limit " + std::to_string(L));
  if (!n) return EG_OK;
  Locked lk(c);
  if ((rc = use_key_locked(c, K_be))) return rc;
  HIPCHK(hipMemcpyAsync(c->d_qbar, qbar_be, 32, hipMemcpyHostToDevice, c->stream));
  const size_t B = (size_t)L + 1;
  Stage st(c, host, n, range_chunk(L));
  st.in(cts, 1024);
  st.in(values, 1);
  st.in(R, 32);
  st.in(nonces, (2 * B + 1) * 32);
  st.out(proofs, B * 64);
  return st.run([&](size_t m) { return range_prove_chunk_locked(c, m, L, cts, values, R, nonces, proofs); });
}

extern "C" int eg_range_prove_dev(eg_ctx* c, const uint8_t K_be[512], const uint8_t qbar_be[32], size_t n, uint32_t L,
                                  const uint8_t* d_cts, const uint8_t* d_values, const uint8_t* d_R,
                                  const uint8_t* d_nonces, uint8_t* d_proofs) {
  return range_prove(c, false, K_be, qbar_be, n, L, d_cts, d_values, d_R, d_nonces, d_proofs);
}

extern "C" int eg_range_prove(eg_ctx* c, const uint8_t K_be[512], const uint8_t qbar_be[32], size_t n, uint32_t L,
                              const uint8_t* cts, const uint8_t* values, const uint8_t* R, const uint8_t* nonces,
                              uint8_t* proofs) {
  return range_prove(c, true, K_be, qbar_be, n, L, cts, values, R, nonces, proofs);
}
