// eg_capi_codes2.inc — ballot nonces from a per-ballot seed and the opening of challenged ballots
// for the placeholder-free ballot (include/eg_hip_codes2.h; DESIGN.md §16; included by eg_capi.hip
// after eg_capi_ballot2.inc, whose shape checks (b2_check), shape (B2Shape) and chunk size these
// share; pow_dev and cd_tables_locked are eg_capi_contestdata.inc's).  Kernels: eg_codes2.hpp.  Each entry point and its _dev twin are one body taking
// `bool host` around one staged run (eg_stage.hpp) of its chunk function; an item is a ballot.

static int c2_args(eg_ctx* c, size_t nb, size_t nc, const uint32_t* nsel, const uint32_t* olimit,
                   const uint32_t* climit, bool head_ok, bool data_ok, B2Shape& M) {
  if (!c || !head_ok || !nsel || !olimit || !climit || (nb && !data_ok)) return b2_fail("null argument");
  return b2_check(nc, nsel, olimit, climit, M);
}

// ---------------------------------------------------------------------------------
// nonces
// ---------------------------------------------------------------------------------
static int c2_derive_locked(eg_ctx* c, const B2Shape& M, size_t nb, const uint8_t* d_bn, uint8_t* d_sn,
                            uint8_t* d_cn) {
  const size_t n = nb * (M.SN + M.CN);
  hipLaunchKernelGGL(k_b2_derive_nonces, dim3(cgrid(n)), dim3(256), 0, c->stream, c->d_q, d_bn, (uint64_t)nb,
                     (uint32_t)M.SN, (uint32_t)M.CN, d_sn, d_cn, c->hash_fmt);
  HIPCHK(hipGetLastError());
  return EG_OK;
}

// host: staged in the ballot2 verifier's chunks; device: the whole batch is one launch
static int c2_derive(eg_ctx* c, bool host, size_t nb, size_t nc, const uint32_t* nsel, const uint32_t* olimit,
                     const uint32_t* climit, const uint8_t* bn, uint8_t* sn, uint8_t* cn) {
  int rc;
  B2Shape M;
  if ((rc = c2_args(c, nb, nc, nsel, olimit, climit, true, bn && sn && cn, M))) return rc;
  if (!host && !aligned16({bn, sn, cn})) return b2_fail("device pointer not 16-byte aligned");
  if (!nb) return EG_OK;
  b2_build(nc, nsel, olimit, climit, M);
  if (!host && nb > kMaxCodeItems / (M.SN + M.CN)) return b2_fail("batch too large");
  Locked lk(c);
  Stage st(c, host, nb, host ? M.chunk() : nb);
  st.in(bn, 32);
  st.out(sn, M.SN * 32);
  st.out(cn, M.CN * 32);
  return st.run([&](size_t m) { return c2_derive_locked(c, M, m, bn, sn, cn); });
}

extern "C" int eg_derive_ballot_nonces_v2_dev(eg_ctx* c, size_t nb, size_t nc, const uint32_t* nsel,
                                              const uint32_t* olimit, const uint32_t* climit, const uint8_t* d_bn,
                                              uint8_t* d_sn, uint8_t* d_cn) {
  return c2_derive(c, false, nb, nc, nsel, olimit, climit, d_bn, d_sn, d_cn);
}

extern "C" int eg_derive_ballot_nonces_v2(eg_ctx* c, size_t nb, size_t nc, const uint32_t* nsel,
                                          const uint32_t* olimit, const uint32_t* climit, const uint8_t* bn,
                                          uint8_t* sn, uint8_t* cn) {
  return c2_derive(c, true, nb, nc, nsel, olimit, climit, bn, sn, cn);
}

// ---------------------------------------------------------------------------------
// open
// ---------------------------------------------------------------------------------
// The opening's per-selection table, cached under its own key (the ballot2 table "b2/" + key keeps
// its bytes): NS rows of R in the ballot's selection nonces, then NS option limits.
static int c2_table(eg_ctx* c, const B2Shape& M, const uint32_t** T) {
  const std::string key = "b2o/" + M.key;
  auto it = c->cache.find(key);
  if (it != c->cache.end()) {
    *T = (const uint32_t*)it->second.ptr;
    return EG_OK;
  }
  std::vector<uint32_t> row, lim;
  for (size_t k = 0; k < M.nc; ++k)
    for (uint32_t i = 0; i < M.nsel[k]; ++i) {
      row.push_back(M.sn_off[k] + i * (2 * M.olimit[k] + 4));
      lim.push_back(M.olimit[k]);
    }
  row.insert(row.end(), lim.begin(), lim.end());
  return cached_jobs(c, key, row, T);
}

// One chunk of nbc <= M.chunk() ballots, device pointers (the key is set by the caller, who holds
// the lock): R per selection, g^R and K^R through the fixed-base batch path, then the match.
static int c2_open_chunk_locked(eg_ctx* c, const B2Shape& M, size_t nbc, const uint8_t* d_bn, const uint8_t* d_cts,
                                uint8_t* d_votes, uint8_t* d_ok) {
  int rc;
  const size_t n = nbc * M.NS;
  uint8_t *R = nullptr, *GR = nullptr, *KR = nullptr;
  if ((rc = ws_get(c, W_C2_R, n * 32, (void**)&R))) return rc;
  if ((rc = ws_get(c, W_C2_GR, n * 512, (void**)&GR))) return rc;
  if ((rc = ws_get(c, W_C2_KR, n * 512, (void**)&KR))) return rc;
  const uint32_t* T = nullptr;
  if ((rc = c2_table(c, M, &T))) return rc;
  hipLaunchKernelGGL(k_b2_derive_r, dim3(cgrid(n)), dim3(256), 0, c->stream, c->d_q, d_bn, T, (uint32_t)M.NS,
                     (uint64_t)n, R, c->hash_fmt);
  HIPCHK(hipGetLastError());
  FbTab gt, kt;
  if ((rc = cd_tables_locked(c, &gt, &kt))) return rc;
  if ((rc = pow_dev(c, nullptr, R, GR, n, &gt))) return rc;
  if ((rc = pow_dev(c, nullptr, R, KR, n, &kt))) return rc;
  // the batch path may have rebuilt the job cache: the table is fetched again
  if ((rc = c2_table(c, M, &T))) return rc;
  // g in Montgomery form is entry (0, 1) of g's radix table
  LAUNCH_F(c, k_b2_match, dim3(grid_for(n)), c->d, c->gtab->d_tab + kW, GR, KR, d_cts, T + M.NS, (uint32_t)M.NS,
           (uint32_t)n, d_votes, d_ok);
  HIPCHK(hipGetLastError());
  return EG_OK;
}

static int c2_open(eg_ctx* c, bool host, const uint8_t* K_be, size_t nb, size_t nc, const uint32_t* nsel,
                   const uint32_t* olimit, const uint32_t* climit, const uint8_t* bn, const uint8_t* cts,
                   uint8_t* votes, uint8_t* ok) {
  int rc;
  B2Shape M;
  if ((rc = c2_args(c, nb, nc, nsel, olimit, climit, K_be != nullptr, bn && cts && votes && ok, M))) return rc;
  if (!host && !aligned16({bn, cts})) return b2_fail("device pointer not 16-byte aligned");
  if (!nb) return EG_OK;
  b2_build(nc, nsel, olimit, climit, M);
  Locked lk(c);
  if ((rc = use_key_locked(c, K_be))) return rc;
  Stage st(c, host, nb, M.chunk());
  st.in(bn, 32);
  st.in(cts, M.NS * 1024);
  st.out(votes, M.NS);
  st.out(ok, M.NS);
  return st.run([&](size_t m) { return c2_open_chunk_locked(c, M, m, bn, cts, votes, ok); });
}

extern "C" int eg_open_ballots_v2_dev(eg_ctx* c, const uint8_t K_be[512], size_t nb, size_t nc, const uint32_t* nsel,
                                      const uint32_t* olimit, const uint32_t* climit, const uint8_t* d_bn,
                                      const uint8_t* d_cts, uint8_t* d_votes, uint8_t* d_ok) {
  return c2_open(c, false, K_be, nb, nc, nsel, olimit, climit, d_bn, d_cts, d_votes, d_ok);
}

extern "C" int eg_open_ballots_v2(eg_ctx* c, const uint8_t K_be[512], size_t nb, size_t nc, const uint32_t* nsel,
                                  const uint32_t* olimit, const uint32_t* climit, const uint8_t* bn,
                                  const uint8_t* cts, uint8_t* votes, uint8_t* ok) {
  return c2_open(c, true, K_be, nb, nc, nsel, olimit, climit, bn, cts, votes, ok);
}
