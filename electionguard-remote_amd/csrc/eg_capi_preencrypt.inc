// eg_capi_preencrypt.inc — pre-encrypted ballots (include/eg_hip_preencrypt.h; included by
// eg_capi.hip after eg_capi_range.inc: the shape checks, table cache, key and launch helpers are
// eg_capi_ballot.inc's and eg_capi_manifest.inc's, derive_locked eg_capi_codes.inc's).  Kernels:
// eg_preencrypt.hpp, k_seg_hash and k_derive_nonces of eg_codes.hpp, and for every group operation
// the existing k_pow / k_prod_tab / import / export.  Each of the three entry points and its _dev
// twin are one body taking `bool host`, around one staged run (eg_stage.hpp) of the chunk function.
//
// A component is one fixed-base job of the encryptor's kind, (alpha, beta) = (g^rho, K^rho g^d)
// with d = [i = j] a one-window term (PowShape.fb_small, as the vote m of beta = K^R g^m), on the
// tables of enc_tables_locked: with eg_ctx_set_ct_encrypt the reads are masked scans.

static_assert(EG_PRE_CHUNK_CTS <= kPowMaxJobs, "a chunk of components is one k_pow sub-launch");

static constexpr size_t kPreMaxCts = (size_t)1 << 22;  // component ciphertexts per ballot

// The validated shape of one call: the manifest's and the per-ballot tables of the kernels.
struct PreShape {
  ManShape M;
  size_t V = 0, S = 0, T = 0;
  std::vector<uint32_t> voff, soff, toff;      // per contest
  std::vector<uint32_t> kof;                   // per slot (= per vector): its contest
  std::vector<uint32_t> diag, vfirst, vlen;    // per component: [i = j]; per vector: first component, spc
  std::vector<uint32_t> uk, ul;                // per chosen component: contest, t spc_k + j
  std::vector<uint32_t> tfirst, tlen, tk;      // per chosen vector: first chosen component, spc, contest
  std::string key;
};

static int pre_fail(const std::string& msg) { return fail(EG_ERR_ARG, "preencrypt: " + msg); }

static int pre_check(eg_ctx* c, size_t nc, const uint32_t* spc, const uint32_t* limits, bool want_limits,
                     uint32_t code_bytes, bool ptrs_ok) {
  if (!c || !spc || (want_limits && !limits) || !ptrs_ok) return pre_fail("null argument");
  if (!nc) return pre_fail("no contests");
  if (code_bytes < 1 || code_bytes > 4) return pre_fail("code_bytes outside 1..4");
  size_t nsel = 0, V = 0;
  for (size_t k = 0; k < nc; ++k) {
    const std::string ck = "contest " + std::to_string(k);
    if (!spc[k]) return pre_fail(ck + " has no selections");
    if (spc[k] > EG_PRE_MAX_SPC) return pre_fail(ck + " has more than 64 selections");
    if (want_limits && (!limits[k] || limits[k] > spc[k])) return pre_fail(ck + " has a limit outside 1..spc");
    nsel += spc[k];
    V += (size_t)spc[k] * spc[k];
    if (nsel > kMaxSelections) return pre_fail("more than 2^20 selections per ballot");
    if (V > kPreMaxCts) return pre_fail("more than 2^22 component ciphertexts per ballot");
  }
  return EG_OK;
}

static PreShape pre_shape(size_t nc, const uint32_t* spc, const uint32_t* limits) {
  PreShape P;
  P.M = man_shape(nc, spc, nullptr, limits);
  P.key = P.M.key;
  for (size_t k = 0; k < nc; ++k) {
    const uint32_t m = spc[k], L = limits ? limits[k] : 0u;
    P.voff.push_back((uint32_t)P.V);
    P.soff.push_back((uint32_t)P.S);
    P.toff.push_back((uint32_t)P.T);
    for (uint32_t i = 0; i < m; ++i) {
      P.kof.push_back((uint32_t)k);
      P.vfirst.push_back((uint32_t)P.V + i * m);
      P.vlen.push_back(m);
      for (uint32_t j = 0; j < m; ++j) P.diag.push_back(i == j ? 1u : 0u);
    }
    for (uint32_t t = 0; t < L; ++t) {
      P.tfirst.push_back((uint32_t)P.S + t * m);
      P.tlen.push_back(m);
      P.tk.push_back((uint32_t)k);
      for (uint32_t j = 0; j < m; ++j) {
        P.uk.push_back((uint32_t)k);
        P.ul.push_back(t * m + j);
      }
    }
    P.V += (size_t)m * m;
    P.S += (size_t)L * m;
    P.T += L;
  }
  return P;
}

static size_t pre_chunk(size_t per_ballot) { return std::max<size_t>(1, EG_PRE_CHUNK_CTS / per_ballot); }

// n component jobs: (alpha, beta) -> elements 2i, 2i + 1; rho is scalar i, [i = j] scalar n + i
static std::vector<PowJob> pre_jobs(size_t n) {
  auto J = new_jobs(n);
  for (size_t i = 0; i < n; ++i) {
    PowJob& j = J[i];
    j.out[0] = (uint32_t)(2 * i); j.out[1] = j.out[0] + 1;
    j.fb[0][0] = (uint32_t)i; j.fb[1][0] = (uint32_t)i; j.fb[1][1] = (uint32_t)(n + i);
  }
  return J;
}

// the n components whose scalars lie in SC ([rho n][unit n]) -> Montgomery elements U (n * 2)
static int pre_pow_locked(eg_ctx* c, const uint32_t* jobs, size_t n, const uint8_t* SC, uint32_t* U) {
  int rc;
  FbTab G{}, K{};
  if ((rc = enc_tables_locked(c, &G, &K))) return rc;
  PowShape S = pow_fb_pair(true);
  S.fb_small[1][1] = 1;  // [i = j] is 0 or 1: one window of g's table
  return launch_pow(c, {S, jobs, n}, U, SC, U, G, K, pow_ct(c->ct_encrypt != 0));
}

// psi of vectors whose components are consecutive ciphertexts: cts (nbc * per * 1024 B) ->
// comp hashes E -> psi (nbc * nvec * 32), vector v of a ballot being first[v] .. + len[v] with
// contest vk[v]
static int pre_vector_hashes(eg_ctx* c, size_t nbc, size_t per, size_t nvec, const uint8_t* d_cts,
                             const uint8_t* d_dcon, const uint32_t* first, const uint32_t* len, const uint32_t* vk,
                             uint8_t* psi) {
  int rc;
  uint8_t *E = nullptr, *DX = nullptr;
  const size_t n = nbc * per;
  if ((rc = ws_get(c, W_OK0, n * 32, (void**)&E))) return rc;
  if ((rc = ws_get(c, W_H7, nvec * 32, (void**)&DX))) return rc;
  hipLaunchKernelGGL(k_pre_comp_hash, dim3(cgrid(n)), dim3(256), 0, c->stream, c->d_q, d_cts, (uint64_t)n, E,
                     c->hash_fmt);
  hipLaunchKernelGGL(k_pre_expand, dim3(cgrid(nvec)), dim3(256), 0, c->stream, d_dcon, vk, (uint64_t)nvec, DX);
  hipLaunchKernelGGL(k_seg_hash, dim3(cgrid(nbc * nvec)), dim3(256), 0, c->stream, c->d_q,
                     SegLead{DX, (uint64_t)nvec}, SegLead{nullptr, 1}, E, first, len, (uint32_t)nvec, (uint64_t)per, 0u,
                     (uint64_t)(nbc * nvec), psi, c->hash_fmt);
  HIPCHK(hipGetLastError());
  return EG_OK;
}

// chi from the sorted lists and C from chi: chash (nbc * nc * 32), conf (nbc * 32)
static int pre_conf_hashes(eg_ctx* c, const PreShape& P, size_t nbc, const uint8_t* d_dcon, const uint8_t* d_mh,
                           const uint8_t* d_ids, const uint8_t* d_sorted, const uint32_t* off, const uint32_t* spc,
                           uint8_t* chash, uint8_t* conf) {
  const size_t nc = P.M.nc, ncn = nbc * nc;
  hipLaunchKernelGGL(k_seg_hash, dim3(cgrid(ncn)), dim3(256), 0, c->stream, c->d_q, SegLead{d_dcon, (uint64_t)nc},
                     SegLead{nullptr, 1}, d_sorted, off, spc, (uint32_t)nc, (uint64_t)P.M.nsel, 0u, (uint64_t)ncn,
                     chash, c->hash_fmt);
  hipLaunchKernelGGL(k_seg_hash, dim3(cgrid(nbc)), dim3(256), 0, c->stream, c->d_q, SegLead{d_ids, (uint64_t)nbc},
                     SegLead{d_mh, 1}, chash, nullptr, nullptr, 1u, (uint64_t)nc, (uint32_t)nc, (uint64_t)nbc, conf,
                     c->hash_fmt);
  HIPCHK(hipGetLastError());
  return EG_OK;
}

// ---------------------------------------------------------------------------------
// pre-encryption
// ---------------------------------------------------------------------------------
// One chunk of <= pre_chunk(V) ballots, device pointers (the key is set by the caller, who holds
// the lock).  d_chash / d_vec may be null: workspace then.
static int pre_chunk_locked(eg_ctx* c, const PreShape& P, size_t nbc, uint32_t cb, const uint8_t* d_dcon,
                            const uint8_t* d_mh, const uint8_t* d_ids, const uint8_t* d_bn, uint8_t* d_sorted,
                            uint32_t* d_perm, uint32_t* d_codes, uint8_t* d_unique, uint8_t* d_conf, uint8_t* d_chash,
                            uint8_t* d_vec) {
  int rc;
  const size_t nc = P.M.nc, nsel = P.M.nsel, V = P.V, n = nbc * V;
  std::vector<const uint32_t*> tv;
  rc = cached_job_set(c, "pe/" + std::to_string(nbc) + "/" + P.key, {"diag", "vfirst", "vlen", "kof", "off", "spc", "jobs"},
                      [&]() {
                        return JobSet{P.diag, P.vfirst, P.vlen, P.kof, P.M.first, P.M.spc,
                                                                  pre_jobs(n)};
                      }, tv);
  if (rc) return rc;
  uint8_t *SC = nullptr, *PSI = nullptr;
  uint32_t* U = nullptr;
  if ((rc = ws_get(c, W_SCAL, n * 2 * 32, (void**)&SC))) return rc;
  if ((rc = ws_get(c, W_E0, n * 2 * kW * 4, (void**)&U))) return rc;
  if (!d_vec && (rc = ws_get(c, W_BE0, n * 1024, (void**)&d_vec))) return rc;
  if (!d_chash && (rc = ws_get(c, W_H8, nbc * nc * 32, (void**)&d_chash))) return rc;
  if ((rc = ws_get(c, W_OK1, nbc * nsel * 32, (void**)&PSI))) return rc;
  hipLaunchKernelGGL(k_pre_nonces, dim3(cgrid(n)), dim3(256), 0, c->stream, c->d_q, d_bn, (uint64_t)nbc, (uint32_t)V,
                     tv[0], SC, SC + n * 32, c->hash_fmt);
  HIPCHK(hipGetLastError());
  if ((rc = pre_pow_locked(c, tv[6], n, SC, U))) return rc;
  if ((rc = launch_export(c, U, n * 2, d_vec))) return rc;
  if ((rc = pre_vector_hashes(c, nbc, V, nsel, d_vec, d_dcon, tv[1], tv[2], tv[3], PSI))) return rc;
  HIPCHK(hipMemsetAsync(d_unique, 1, nbc, c->stream));
  hipLaunchKernelGGL(k_pre_sort, dim3(cgrid(nbc * nc)), dim3(256), 0, c->stream, PSI, (uint64_t)nbc, (uint32_t)nc,
                     (uint32_t)nsel, tv[4], tv[5], cb, d_sorted, d_perm, d_codes, d_unique);
  HIPCHK(hipGetLastError());
  return pre_conf_hashes(c, P, nbc, d_dcon, d_mh, d_ids, d_sorted, tv[4], tv[5], d_chash, d_conf);
}

// in host mode the device holds one chunk however many ballots come in
static int preencrypt_ballots(eg_ctx* c, bool host, const uint8_t* K_be, size_t nb, size_t nc, const uint32_t* spc,
                              uint32_t cb, const uint8_t* dcon, const uint8_t* mh, const uint8_t* ids,
                              const uint8_t* bn, uint8_t* sorted, uint32_t* perm, uint32_t* codes, uint8_t* unique,
                              uint8_t* conf, uint8_t* chash, uint8_t* vec) {
  int rc;
  if ((rc = pre_check(c, nc, spc, nullptr, false, cb,
                      K_be && (!nb || (dcon && mh && ids && bn && sorted && perm && codes && unique && conf)))))
    return rc;
  if (!host && !aligned16({dcon, mh, ids, bn, sorted, conf, chash, vec}))
    return pre_fail("device pointer not 16-byte aligned");
  if (!nb) return EG_OK;
  const PreShape P = pre_shape(nc, spc, nullptr);
  const size_t nsel = P.M.nsel;
  Locked L(c);
  if ((rc = use_key_locked(c, K_be))) return rc;
  Stage st(c, host, nb, pre_chunk(P.V));
  st.once(dcon, nc * 32);
  st.once(mh, 32);
  st.in(ids, 32);
  st.in(bn, 32);
  st.out(sorted, nsel * 32);
  st.out(perm, nsel * 4);
  st.out(codes, nsel * 4);
  st.out(unique, 1);
  st.out(conf, 32);
  st.out(chash, nc * 32);
  st.out(vec, P.V * 1024);
  return st.run([&](size_t n) {
    return pre_chunk_locked(c, P, n, cb, dcon, mh, ids, bn, sorted, perm, codes, unique, conf, chash, vec);
  });
}

extern "C" int eg_preencrypt_ballots_dev(eg_ctx* c, const uint8_t K_be[512], size_t nb, size_t nc, const uint32_t* spc,
                                         uint32_t cb, const uint8_t* d_dcon, const uint8_t* d_mh, const uint8_t* d_ids,
                                         const uint8_t* d_bn, uint8_t* d_sorted, uint32_t* d_perm, uint32_t* d_codes,
                                         uint8_t* d_unique, uint8_t* d_conf, uint8_t* d_chash, uint8_t* d_vec) {
  return preencrypt_ballots(c, false, K_be, nb, nc, spc, cb, d_dcon, d_mh, d_ids, d_bn, d_sorted, d_perm, d_codes,
                            d_unique, d_conf, d_chash, d_vec);
}

extern "C" int eg_preencrypt_ballots(eg_ctx* c, const uint8_t K_be[512], size_t nb, size_t nc, const uint32_t* spc,
                                     uint32_t cb, const uint8_t* dcon, const uint8_t manifest_hash[32],
                                     const uint8_t* ids, const uint8_t* bn, uint8_t* sorted, uint32_t* perm,
                                     uint32_t* codes, uint8_t* unique, uint8_t* conf, uint8_t* chash, uint8_t* vec) {
  return preencrypt_ballots(c, true, K_be, nb, nc, spc, cb, dcon, manifest_hash, ids, bn, sorted, perm, codes, unique,
                            conf, chash, vec);
}

// ---------------------------------------------------------------------------------
// recording
// ---------------------------------------------------------------------------------
// One chunk of <= pre_chunk(S) ballots, device pointers.  Only the chosen vectors are encrypted.
static int record_chunk_locked(eg_ctx* c, const PreShape& P, size_t nbc, uint32_t cb, const uint8_t* d_dcon,
                               const uint8_t* d_bn, const uint8_t* d_votes, const uint8_t* d_sorted, uint8_t* d_sv,
                               uint32_t* d_rank, uint32_t* d_codes, uint8_t* d_sn, uint8_t* d_cn, uint8_t* d_ok) {
  int rc;
  const size_t nc = P.M.nc, nsel = P.M.nsel, S = P.S, T = P.T, n = nbc * S;
  std::vector<const uint32_t*> tv;
  rc = cached_job_set(c, "pr/" + std::to_string(nbc) + "/" + P.key,
                      {"uk", "ul", "off", "spc", "voff", "soff", "toff", "limit", "tfirst", "tlen", "tk", "kof", "jobs"},
                      [&]() {
                        return JobSet{P.uk, P.ul, P.M.first, P.M.spc, P.voff, P.soff,
                                                                  P.toff, P.M.limit, P.tfirst, P.tlen, P.tk, P.kof,
                                                                  pre_jobs(n)};
                      }, tv);
  if (rc) return rc;
  const uint32_t *uk = tv[0], *ul = tv[1], *off = tv[2], *spc = tv[3], *voff = tv[4], *soff = tv[5], *toff = tv[6],
                 *limit = tv[7];
  uint8_t *SC = nullptr, *NAT = nullptr, *PSIC = nullptr;
  uint32_t *U = nullptr, *RK = nullptr, *PL = nullptr;
  if ((rc = ws_get(c, W_SCAL, n * 2 * 32, (void**)&SC))) return rc;
  if ((rc = ws_get(c, W_E0, n * 2 * kW * 4, (void**)&U))) return rc;
  if ((rc = ws_get(c, W_BE0, n * 1024, (void**)&NAT))) return rc;  // the chosen vectors in vote order
  if ((rc = ws_get(c, W_OK1, nbc * T * 32, (void**)&PSIC))) return rc;
  if ((rc = ws_get(c, W_H8, nbc * T * 4, (void**)&RK))) return rc;
  if ((rc = ws_get(c, W_OFF, nbc * T * 4, (void**)&PL))) return rc;
  hipLaunchKernelGGL(k_pre_rec_nonces, dim3(cgrid(n)), dim3(256), 0, c->stream, c->d_q, d_bn, d_votes, (uint64_t)nbc,
                     (uint32_t)S, (uint32_t)nsel, uk, ul, off, spc, voff, SC, SC + n * 32, c->hash_fmt);
  HIPCHK(hipGetLastError());
  if ((rc = pre_pow_locked(c, tv[12], n, SC, U))) return rc;
  if ((rc = launch_export(c, U, n * 2, NAT))) return rc;
  if ((rc = pre_vector_hashes(c, nbc, S, T, NAT, d_dcon, tv[8], tv[9], tv[10], PSIC))) return rc;
  hipLaunchKernelGGL(k_pre_place, dim3(cgrid(nbc * nc)), dim3(256), 0, c->stream, d_votes, PSIC, d_sorted,
                     (uint64_t)nbc, (uint32_t)nc, (uint32_t)nsel, (uint32_t)T, off, spc, toff, limit, cb, RK, d_rank,
                     d_codes, PL, d_ok);
  hipLaunchKernelGGL(k_pre_copy_rows, dim3(cgrid(n * 64)), dim3(256), 0, c->stream, NAT, PL, (uint64_t)nbc,
                     (uint32_t)S, (uint32_t)T, uk, ul, spc, soff, toff, d_sv);
  HIPCHK(hipGetLastError());
  // the proof and contest nonces are eg_derive_ballot_nonces'; R is replaced by the chosen vectors' sum
  if ((rc = derive_locked(c, nbc, nsel, nc, d_bn, d_sn, d_cn))) return rc;
  hipLaunchKernelGGL(k_pre_rec_sums, dim3(cgrid(nbc * nsel)), dim3(256), 0, c->stream, c->d_q, SC, (uint64_t)nbc,
                     (uint32_t)nsel, (uint32_t)S, tv[11], off, spc, soff, limit, d_sn);
  HIPCHK(hipGetLastError());
  return EG_OK;
}

static int preencrypt_record(eg_ctx* c, bool host, const uint8_t* K_be, size_t nb, size_t nc, const uint32_t* spc,
                             const uint32_t* limits, uint32_t cb, const uint8_t* dcon, const uint8_t* bn,
                             const uint8_t* votes, const uint8_t* sorted, uint8_t* sv, uint32_t* rank, uint32_t* codes,
                             uint8_t* sn, uint8_t* cn, uint8_t* ok) {
  int rc;
  if ((rc = pre_check(c, nc, spc, limits, true, cb,
                      K_be && (!nb || (dcon && bn && votes && sorted && sv && rank && codes && sn && cn && ok)))))
    return rc;
  if (!host && !aligned16({dcon, bn, sorted, sv, sn, cn})) return pre_fail("device pointer not 16-byte aligned");
  if (!nb) return EG_OK;
  const PreShape P = pre_shape(nc, spc, limits);
  const size_t nsel = P.M.nsel;
  Locked L(c);
  if ((rc = use_key_locked(c, K_be))) return rc;
  Stage st(c, host, nb, pre_chunk(P.S));
  st.once(dcon, nc * 32);
  st.in(bn, 32);
  st.in(votes, nsel);
  st.in(sorted, nsel * 32);
  st.out(sv, P.S * 1024);
  st.out(rank, P.T * 4);
  st.out(codes, P.T * 4);
  st.out(sn, nsel * 128);
  st.out(cn, nc * 32);
  st.out(ok, nc);
  return st.run([&](size_t n) {
    return record_chunk_locked(c, P, n, cb, dcon, bn, votes, sorted, sv, rank, codes, sn, cn, ok);
  });
}

extern "C" int eg_preencrypt_record_dev(eg_ctx* c, const uint8_t K_be[512], size_t nb, size_t nc, const uint32_t* spc,
                                        const uint32_t* limits, uint32_t cb, const uint8_t* d_dcon,
                                        const uint8_t* d_bn, const uint8_t* d_votes, const uint8_t* d_sorted,
                                        uint8_t* d_sv, uint32_t* d_rank, uint32_t* d_codes, uint8_t* d_sn,
                                        uint8_t* d_cn, uint8_t* d_ok) {
  return preencrypt_record(c, false, K_be, nb, nc, spc, limits, cb, d_dcon, d_bn, d_votes, d_sorted, d_sv, d_rank,
                           d_codes, d_sn, d_cn, d_ok);
}

extern "C" int eg_preencrypt_record(eg_ctx* c, const uint8_t K_be[512], size_t nb, size_t nc, const uint32_t* spc,
                                    const uint32_t* limits, uint32_t cb, const uint8_t* dcon, const uint8_t* bn,
                                    const uint8_t* votes, const uint8_t* sorted, uint8_t* sv, uint32_t* rank,
                                    uint32_t* codes, uint8_t* sn, uint8_t* cn, uint8_t* ok) {
  return preencrypt_record(c, true, K_be, nb, nc, spc, limits, cb, dcon, bn, votes, sorted, sv, rank, codes, sn, cn,
                           ok);
}

// ---------------------------------------------------------------------------------
// the pre-encryption check
// ---------------------------------------------------------------------------------
// classes of contests with equal (spc, limit): one k_prod_tab population each (its group length
// and element stride are launch-wide)
static std::vector<std::vector<uint32_t>> pre_classes(const PreShape& P) {
  std::map<std::pair<uint32_t, uint32_t>, std::vector<uint32_t>> by;
  for (size_t k = 0; k < P.M.nc; ++k) by[{P.M.spc[k], P.M.limit[k]}].push_back((uint32_t)k);
  std::vector<std::vector<uint32_t>> out;
  for (auto& kv : by) out.push_back(std::move(kv.second));
  return out;
}

// One chunk of <= pre_chunk(S) ballots, device pointers.
static int preverify_chunk_locked(eg_ctx* c, const PreShape& P, size_t nbc, uint32_t cb, const uint8_t* d_dcon,
                                  const uint8_t* d_mh, const uint8_t* d_ids, const uint8_t* d_sv,
                                  const uint32_t* d_rank, const uint32_t* d_codes, const uint8_t* d_sorted,
                                  const uint8_t* d_cts, const uint8_t* d_conf, uint8_t* d_okc, uint8_t* d_okb) {
  int rc;
  const size_t nc = P.M.nc, nsel = P.M.nsel, S = P.S, T = P.T, n = nbc * S;
  const auto cls = pre_classes(P);
  std::vector<std::string> names{"off", "spc", "soff", "toff", "limit", "tfirst", "tlen", "tk"};
  for (size_t ci = 0; ci < cls.size(); ++ci)
    for (const char* nm : {"in", "out"}) names.push_back(nm + std::to_string(ci));
  std::vector<const uint32_t*> tv;
  rc = cached_job_set(c, "pv/" + P.key, names, [&]() {
    JobSet out{P.M.first, P.M.spc, P.soff, P.toff, P.M.limit, P.tfirst, P.tlen, P.tk};
    for (const auto& members : cls) {  // group (k, j, comp): chosen rows soff_k + j (+ t spc_k) -> slot off_k + j
      std::vector<uint32_t> in, ot;
      for (uint32_t k : members)
        for (uint32_t j = 0; j < P.M.spc[k]; ++j)
          for (uint32_t comp = 0; comp < 2; ++comp) {
            in.push_back((P.soff[k] + j) * 2 + comp);
            ot.push_back((P.M.first[k] + j) * 2 + comp);
          }
      out.push_back(std::move(in));
      out.push_back(std::move(ot));
    }
    return out;
  }, tv);
  if (rc) return rc;
  const uint32_t *off = tv[0], *spc = tv[1], *soff = tv[2], *toff = tv[3], *limit = tv[4];
  uint32_t *E = nullptr, *PR = nullptr;
  uint8_t *FL = nullptr, *PR_BE = nullptr, *PSIC = nullptr, *CH = nullptr, *CF = nullptr;
  if ((rc = ws_get(c, W_E0, n * 2 * kW * 4, (void**)&E))) return rc;
  if ((rc = ws_get(c, W_E1, nbc * nsel * 2 * kW * 4, (void**)&PR))) return rc;
  if ((rc = ws_get(c, W_FLAGS, n * 2, (void**)&FL))) return rc;
  if ((rc = ws_get(c, W_BE0, nbc * nsel * 1024, (void**)&PR_BE))) return rc;
  if ((rc = ws_get(c, W_OK1, nbc * T * 32, (void**)&PSIC))) return rc;
  if ((rc = ws_get(c, W_H8, nbc * nc * 32, (void**)&CH))) return rc;
  if ((rc = ws_get(c, W_OFF, nbc * 32, (void**)&CF))) return rc;
  // 1. the chosen vectors' elements: range flags, Montgomery form, slot-wise products
  if ((rc = launch_import(c, d_sv, n * 2, E, FL))) return rc;
  hipLaunchKernelGGL(k_pre_nonzero, dim3(cgrid(n * 2)), dim3(256), 0, c->stream, d_sv, (uint64_t)(n * 2), FL);
  HIPCHK(hipGetLastError());
  for (size_t ci = 0; ci < cls.size(); ++ci) {
    const uint32_t k0 = cls[ci].front(), m = P.M.spc[k0], L = P.M.limit[k0];
    const size_t period = cls[ci].size() * m * 2;
    if ((rc = run_prod_tab(c, E, tv[8 + ci * 2], period, 2 * S, nbc * period, L, 2 * m, PR, tv[9 + ci * 2], 2 * nsel)))
      return rc;
  }
  if ((rc = launch_export(c, PR, nbc * nsel * 2, PR_BE))) return rc;
  // 2. psi of the chosen vectors, chi and C from the sorted lists
  if ((rc = pre_vector_hashes(c, nbc, S, T, d_sv, d_dcon, tv[5], tv[6], tv[7], PSIC))) return rc;
  if ((rc = pre_conf_hashes(c, P, nbc, d_dcon, d_mh, d_ids, d_sorted, off, spc, CH, CF))) return rc;
  // 3. the verdicts
  hipLaunchKernelGGL(k_pre_verify, dim3(cgrid(nbc * nc)), dim3(256), 0, c->stream, FL, d_rank, d_codes, PSIC, d_sorted,
                     PR_BE, d_cts, (uint64_t)nbc, (uint32_t)nc, (uint32_t)nsel, (uint32_t)S, (uint32_t)T, off, spc, soff,
                     toff, limit, cb, d_okc);
  hipLaunchKernelGGL(k_pre_conf_check, dim3(cgrid(nbc)), dim3(256), 0, c->stream, CF, d_conf, (uint64_t)nbc, d_okb);
  HIPCHK(hipGetLastError());
  return EG_OK;
}

static int preencrypt_verify(eg_ctx* c, bool host, size_t nb, size_t nc, const uint32_t* spc, const uint32_t* limits,
                             uint32_t cb, const uint8_t* dcon, const uint8_t* mh, const uint8_t* ids,
                             const uint8_t* sv, const uint32_t* rank, const uint32_t* codes, const uint8_t* sorted,
                             const uint8_t* cts, const uint8_t* conf, uint8_t* okc, uint8_t* okb) {
  int rc;
  if ((rc = pre_check(c, nc, spc, limits, true, cb,
                      !nb || (dcon && mh && ids && sv && rank && codes && sorted && cts && conf && okc && okb))))
    return rc;
  if (!host && !aligned16({dcon, mh, ids, sv, sorted, cts, conf}))
    return pre_fail("device pointer not 16-byte aligned");
  if (!nb) return EG_OK;
  const PreShape P = pre_shape(nc, spc, limits);
  const size_t nsel = P.M.nsel;
  Locked L(c);
  Stage st(c, host, nb, pre_chunk(P.S));
  st.once(dcon, nc * 32);
  st.once(mh, 32);
  st.in(ids, 32);
  st.in(sv, P.S * 1024);
  st.in(rank, P.T * 4);
  st.in(codes, P.T * 4);
  st.in(sorted, nsel * 32);
  st.in(cts, nsel * 1024);
  st.in(conf, 32);
  st.out(okc, nc);
  st.out(okb, 1);
  return st.run([&](size_t n) {
    return preverify_chunk_locked(c, P, n, cb, dcon, mh, ids, sv, rank, codes, sorted, cts, conf, okc, okb);
  });
}

extern "C" int eg_preencrypt_verify_dev(eg_ctx* c, size_t nb, size_t nc, const uint32_t* spc, const uint32_t* limits,
                                        uint32_t cb, const uint8_t* d_dcon, const uint8_t* d_mh, const uint8_t* d_ids,
                                        const uint8_t* d_sv, const uint32_t* d_rank, const uint32_t* d_codes,
                                        const uint8_t* d_sorted, const uint8_t* d_cts, const uint8_t* d_conf,
                                        uint8_t* d_okc, uint8_t* d_okb) {
  return preencrypt_verify(c, false, nb, nc, spc, limits, cb, d_dcon, d_mh, d_ids, d_sv, d_rank, d_codes, d_sorted,
                           d_cts, d_conf, d_okc, d_okb);
}

extern "C" int eg_preencrypt_verify(eg_ctx* c, size_t nb, size_t nc, const uint32_t* spc, const uint32_t* limits,
                                    uint32_t cb, const uint8_t* dcon, const uint8_t manifest_hash[32],
                                    const uint8_t* ids, const uint8_t* sv, const uint32_t* rank, const uint32_t* codes,
                                    const uint8_t* sorted, const uint8_t* cts, const uint8_t* conf, uint8_t* okc,
                                    uint8_t* okb) {
  return preencrypt_verify(c, true, nb, nc, spc, limits, cb, dcon, manifest_hash, ids, sv, rank, codes, sorted, cts,
                           conf, okc, okb);
}
