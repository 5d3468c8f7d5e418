// eg_capi_contestdata.inc — contest data (write-ins, overvote status) under HashedElGamal
// (include/eg_hip_contestdata.h; included by eg_capi.hip after eg_capi_codes.inc, whose item cap
// these share).  The kernels are eg_hmac.hpp's, one thread per item; the two
// exponentiations c0 = g^r and kappa = K^r are the fixed-base batch path (pow_dev), on the ctx's g
// table and K's cached key table, so they follow eg_ctx_set_ct_pow like eg_fb_pow_batch_dev.
// Each entry point and its _dev twin are one body taking `bool host` around one staged run
// (eg_stage.hpp) of its chunk function; an item of the run is a ballot.

static int pow_dev(eg_ctx* c, const uint8_t* d_base_be, const uint8_t* d_exp_be, uint8_t* d_out_be, size_t n,
                   const FbTab* fbonly);  // eg_capi.hip, below the includes

static_assert(kCdMaxBytes == EG_CD_MAX_BYTES, "eg_hmac.hpp and eg_hip_contestdata.h disagree");

static int cd_shape_args(eg_ctx* c, size_t nb, size_t nc, size_t nbytes, bool has_nbytes, bool data_ok) {
  if (!c || !data_ok) return fail(EG_ERR_ARG, "null argument");
  if (!nc) return fail(EG_ERR_ARG, "ncontest == 0");
  if (has_nbytes && (nbytes < 1 || nbytes > kCdMaxBytes)) return fail(EG_ERR_ARG, "nbytes outside [1, 1024]");
  if (nc > kMaxSelections || (nb && nb > kMaxCodeItems / nc)) return fail(EG_ERR_ARG, "batch too large");
  return EG_OK;
}

// ---------------------------------------------------------------------------------
// nonces
// ---------------------------------------------------------------------------------
static int cd_nonces_locked(eg_ctx* c, size_t nb, size_t nc, const uint8_t* d_bn, uint8_t* d_r) {
  const size_t n = nb * nc;
  hipLaunchKernelGGL(k_cd_nonces, dim3(cgrid(n)), dim3(256), 0, c->stream, c->d_q, d_bn, (uint64_t)n, (uint32_t)nc,
                     d_r, c->hash_fmt);
  HIPCHK(hipGetLastError());
  return EG_OK;
}

// host: staged in the verifier's chunks; device: the whole batch is one launch
static int cd_nonces(eg_ctx* c, bool host, size_t nb, size_t nc, const uint8_t* bn, uint8_t* r) {
  int rc;
  if ((rc = cd_shape_args(c, nb, nc, 0, false, !nb || (bn && r)))) return rc;
  if (!host && !aligned16({bn, r})) return fail(EG_ERR_ARG, "device pointer not 16-byte aligned");
  if (!nb) return EG_OK;
  Locked L(c);
  Stage st(c, host, nb, host ? ballot_chunk(nc) : nb);
  st.in(bn, 32);
  st.out(r, nc * 32);
  return st.run([&](size_t n) { return cd_nonces_locked(c, n, nc, bn, r); });
}

extern "C" int eg_derive_contest_data_nonces_dev(eg_ctx* c, size_t nb, size_t nc, const uint8_t* d_bn, uint8_t* d_r) {
  return cd_nonces(c, false, nb, nc, d_bn, d_r);
}

extern "C" int eg_derive_contest_data_nonces(eg_ctx* c, size_t nb, size_t nc, const uint8_t* bn, uint8_t* out_r) {
  return cd_nonces(c, true, nb, nc, bn, out_r);
}

// ---------------------------------------------------------------------------------
// seal
// ---------------------------------------------------------------------------------
// g's and the current key's tables as the fixed-base batch path reads them
static int cd_tables_locked(eg_ctx* c, FbTab* g, FbTab* k) {
  *g = c->gtab->tab();
  *k = c->Ktab->tab();
  if (!c->ct_pow) return EG_OK;
  int rc;
  if ((rc = ct_table_locked(c, c->gtab, g))) return rc;
  return ct_table_locked(c, c->Ktab, k);
}

// One chunk of <= ballot_chunk(nc) ballots, device pointers; kappa lives in workspace only.
static int seal_chunk_locked(eg_ctx* c, size_t nbc, size_t nc, size_t nbytes, const uint8_t* d_ids,
                             const uint8_t* d_r, const uint8_t* d_data, uint8_t* d_c0, uint8_t* d_c1, uint8_t* d_c2) {
  int rc;
  const size_t n = nbc * nc;
  FbTab gt, kt;
  uint8_t* d_kappa = nullptr;
  if ((rc = cd_tables_locked(c, &gt, &kt))) return rc;
  if ((rc = ws_get(c, W_H5, n * 512, (void**)&d_kappa))) return rc;
  if ((rc = pow_dev(c, nullptr, d_r, d_c0, n, &gt))) return rc;
  if ((rc = pow_dev(c, nullptr, d_r, d_kappa, n, &kt))) return rc;
  hipLaunchKernelGGL(k_cd_seal, dim3(cgrid(n)), dim3(256), 0, c->stream, d_ids, d_c0, d_kappa, d_data, (uint64_t)n,
                     (uint32_t)nc, (uint32_t)nbytes, d_c1, d_c2);
  HIPCHK(hipGetLastError());
  return EG_OK;
}

// staged in the verifier's chunks: in host mode the device holds one chunk however many ballots come in
static int cd_seal(eg_ctx* c, bool host, const uint8_t* K_be, size_t nb, size_t nc, size_t nbytes, const uint8_t* ids,
                   const uint8_t* r, const uint8_t* data, uint8_t* c0, uint8_t* c1, uint8_t* c2) {
  int rc;
  if ((rc = cd_shape_args(c, nb, nc, nbytes, true, K_be && (!nb || (ids && r && data && c0 && c1 && c2))))) return rc;
  if (!host && !aligned16({ids, r, c0, c2})) return fail(EG_ERR_ARG, "device pointer not 16-byte aligned");
  if (!nb) return EG_OK;
  Locked L(c);
  if ((rc = use_key_locked(c, K_be))) return rc;
  Stage st(c, host, nb, ballot_chunk(nc));
  st.in(ids, 32);
  st.in(r, nc * 32);
  st.in(data, nc * nbytes);
  st.out(c0, nc * 512);
  st.out(c1, nc * nbytes);
  st.out(c2, nc * 32);
  return st.run([&](size_t n) { return seal_chunk_locked(c, n, nc, nbytes, ids, r, data, c0, c1, c2); });
}

extern "C" int eg_seal_contest_data_dev(eg_ctx* c, const uint8_t K_be[512], size_t nb, size_t nc, size_t nbytes,
                                        const uint8_t* d_ids, const uint8_t* d_r, const uint8_t* d_data,
                                        uint8_t* d_c0, uint8_t* d_c1, uint8_t* d_c2) {
  return cd_seal(c, false, K_be, nb, nc, nbytes, d_ids, d_r, d_data, d_c0, d_c1, d_c2);
}

extern "C" int eg_seal_contest_data(eg_ctx* c, const uint8_t K_be[512], size_t nb, size_t nc, size_t nbytes,
                                    const uint8_t* ids, const uint8_t* r, const uint8_t* data, uint8_t* out_c0,
                                    uint8_t* out_c1, uint8_t* out_c2) {
  return cd_seal(c, true, K_be, nb, nc, nbytes, ids, r, data, out_c0, out_c1, out_c2);
}

// ---------------------------------------------------------------------------------
// open
// ---------------------------------------------------------------------------------
static int open_locked(eg_ctx* c, size_t n, size_t nc, size_t nbytes, const uint8_t* d_ids, const uint8_t* d_c0,
                       const uint8_t* d_kappa, const uint8_t* d_c1, const uint8_t* d_c2, uint8_t* d_data,
                       uint8_t* d_ok) {
  hipLaunchKernelGGL(k_cd_open, dim3(cgrid(n)), dim3(256), 0, c->stream, d_ids, d_c0, d_kappa, d_c1, d_c2,
                     (uint64_t)n, (uint32_t)nc, (uint32_t)nbytes, d_data, d_ok);
  HIPCHK(hipGetLastError());
  return EG_OK;
}

// host: staged in the verifier's chunks; device: every item's ballot is i / ncontest, so one launch
// covers the batch
static int cd_open(eg_ctx* c, bool host, size_t nb, size_t nc, size_t nbytes, const uint8_t* ids, const uint8_t* c0,
                   const uint8_t* kappa, const uint8_t* c1, const uint8_t* c2, uint8_t* data, uint8_t* ok) {
  int rc;
  if ((rc = cd_shape_args(c, nb, nc, nbytes, true, !nb || (ids && c0 && kappa && c1 && c2 && data && ok)))) return rc;
  if (!host && !aligned16({ids, c0, kappa, c2})) return fail(EG_ERR_ARG, "device pointer not 16-byte aligned");
  if (!nb) return EG_OK;
  Locked L(c);
  Stage st(c, host, nb, host ? ballot_chunk(nc) : nb);
  st.in(ids, 32);
  st.in(c0, nc * 512);
  st.in(kappa, nc * 512);
  st.in(c1, nc * nbytes);
  st.in(c2, nc * 32);
  st.out(data, nc * nbytes);
  st.out(ok, nc);
  return st.run([&](size_t n) { return open_locked(c, n * nc, nc, nbytes, ids, c0, kappa, c1, c2, data, ok); });
}

extern "C" int eg_open_contest_data_dev(eg_ctx* c, size_t nb, size_t nc, size_t nbytes, const uint8_t* d_ids,
                                        const uint8_t* d_c0, const uint8_t* d_kappa, const uint8_t* d_c1,
                                        const uint8_t* d_c2, uint8_t* d_data, uint8_t* d_ok) {
  return cd_open(c, false, nb, nc, nbytes, d_ids, d_c0, d_kappa, d_c1, d_c2, d_data, d_ok);
}

extern "C" int eg_open_contest_data(eg_ctx* c, size_t nb, size_t nc, size_t nbytes, const uint8_t* ids,
                                    const uint8_t* c0, const uint8_t* kappa, const uint8_t* c1, const uint8_t* c2,
                                    uint8_t* out_data, uint8_t* out_ok) {
  return cd_open(c, true, nb, nc, nbytes, ids, c0, kappa, c1, c2, out_data, out_ok);
}
