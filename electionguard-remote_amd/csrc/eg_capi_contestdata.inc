// eg_capi_contestdata.inc — contest data (write-ins, overvote status) under HashedElGamal
// (include/eg_hip_contestdata.h; included by eg_capi.hip after eg_capi_codes.inc, whose grid and
// alignment helpers these share).  The kernels are eg_hmac.hpp's, one thread per item; the two
// exponentiations c0 = g^r and kappa = K^r are the fixed-base batch path (pow_dev), on the ctx's g
// table and K's cached key table, so they follow eg_ctx_set_ct_pow like eg_fb_pow_batch_dev.

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

extern "C" int eg_derive_contest_data_nonces_dev(eg_ctx* c, size_t nb, size_t nc, const uint8_t* d_bn, uint8_t* d_r) {
  int rc;
  if ((rc = cd_shape_args(c, nb, nc, 0, false, !nb || (d_bn && d_r)))) return rc;
  if (!aligned16({d_bn, d_r})) return fail(EG_ERR_ARG, "device pointer not 16-byte aligned");
  if (!nb) return EG_OK;
  Locked L(c);
  return cd_nonces_locked(c, nb, nc, d_bn, d_r);
}

extern "C" int eg_derive_contest_data_nonces(eg_ctx* c, size_t nb, size_t nc, const uint8_t* bn, uint8_t* out_r) {
  int rc;
  if ((rc = cd_shape_args(c, nb, nc, 0, false, !nb || (bn && out_r)))) return rc;
  if (!nb) return EG_OK;
  const size_t chunk = ballot_chunk(nc), first = std::min(chunk, nb);
  Locked L(c);
  uint8_t *d_bn = nullptr, *d_r = nullptr;
  if ((rc = ws_get(c, W_H0, first * 32, (void**)&d_bn))) return rc;
  if ((rc = ws_get(c, W_H1, first * nc * 32, (void**)&d_r))) return rc;
  for (size_t b0 = 0; b0 < nb; b0 += chunk) {
    const size_t n = std::min(chunk, nb - b0);
    HIPCHK(hipMemcpyAsync(d_bn, bn + b0 * 32, n * 32, hipMemcpyHostToDevice, c->stream));
    if ((rc = cd_nonces_locked(c, n, nc, d_bn, d_r))) return rc;
    HIPCHK(hipMemcpyAsync(out_r + b0 * nc * 32, d_r, n * nc * 32, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  return EG_OK;
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

extern "C" int eg_seal_contest_data_dev(eg_ctx* c, const uint8_t K_be[512], size_t nb, size_t nc, size_t nbytes,
                                        const uint8_t* d_ids, const uint8_t* d_r, const uint8_t* d_data,
                                        uint8_t* d_c0, uint8_t* d_c1, uint8_t* d_c2) {
  int rc;
  if ((rc = cd_shape_args(c, nb, nc, nbytes, true, K_be && (!nb || (d_ids && d_r && d_data && d_c0 && d_c1 && d_c2)))))
    return rc;
  if (!aligned16({d_ids, d_r, d_c0, d_c2})) return fail(EG_ERR_ARG, "device pointer not 16-byte aligned");
  if (!nb) return EG_OK;
  const size_t chunk = ballot_chunk(nc);
  Locked L(c);
  if ((rc = use_key_locked(c, K_be))) return rc;
  for (size_t b0 = 0; b0 < nb; b0 += chunk) {
    const size_t n = std::min(chunk, nb - b0), i0 = b0 * nc;
    if ((rc = seal_chunk_locked(c, n, nc, nbytes, d_ids + b0 * 32, d_r + i0 * 32, d_data + i0 * nbytes,
                                d_c0 + i0 * 512, d_c1 + i0 * nbytes, d_c2 + i0 * 32)))
      return rc;
  }
  return EG_OK;
}

extern "C" int eg_seal_contest_data(eg_ctx* c, const uint8_t K_be[512], size_t nb, size_t nc, size_t nbytes,
                                    const uint8_t* ids, const uint8_t* r, const uint8_t* data, uint8_t* out_c0,
                                    uint8_t* out_c1, uint8_t* out_c2) {
  int rc;
  if ((rc = cd_shape_args(c, nb, nc, nbytes, true, K_be && (!nb || (ids && r && data && out_c0 && out_c1 && out_c2)))))
    return rc;
  if (!nb) return EG_OK;
  const size_t chunk = ballot_chunk(nc), first = std::min(chunk, nb) * nc;
  Locked L(c);
  if ((rc = use_key_locked(c, K_be))) return rc;
  uint8_t *d_ids = nullptr, *d_r = nullptr, *d_data = nullptr, *d_c0 = nullptr, *d_c1 = nullptr, *d_c2 = nullptr;
  if ((rc = ws_get(c, W_H0, first / nc * 32, (void**)&d_ids))) return rc;
  if ((rc = ws_get(c, W_H1, first * 32, (void**)&d_r))) return rc;
  if ((rc = ws_get(c, W_H2, first * nbytes, (void**)&d_data))) return rc;
  if ((rc = ws_get(c, W_H3, first * 512, (void**)&d_c0))) return rc;
  if ((rc = ws_get(c, W_H4, first * nbytes, (void**)&d_c1))) return rc;
  if ((rc = ws_get(c, W_H6, first * 32, (void**)&d_c2))) return rc;
  // staged in the verifier's chunks: the device holds one chunk however many ballots come in
  for (size_t b0 = 0; b0 < nb; b0 += chunk) {
    const size_t nbc = std::min(chunk, nb - b0), n = nbc * nc, i0 = b0 * nc;
    HIPCHK(hipMemcpyAsync(d_ids, ids + b0 * 32, nbc * 32, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_r, r + i0 * 32, n * 32, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_data, data + i0 * nbytes, n * nbytes, hipMemcpyHostToDevice, c->stream));
    if ((rc = seal_chunk_locked(c, nbc, nc, nbytes, d_ids, d_r, d_data, d_c0, d_c1, d_c2))) return rc;
    HIPCHK(hipMemcpyAsync(out_c0 + i0 * 512, d_c0, n * 512, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(out_c1 + i0 * nbytes, d_c1, n * nbytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(out_c2 + i0 * 32, d_c2, n * 32, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  return EG_OK;
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

extern "C" int eg_open_contest_data_dev(eg_ctx* c, size_t nb, size_t nc, size_t nbytes, const uint8_t* d_ids,
                                        const uint8_t* d_c0, const uint8_t* d_kappa, const uint8_t* d_c1,
                                        const uint8_t* d_c2, uint8_t* d_data, uint8_t* d_ok) {
  int rc;
  if ((rc = cd_shape_args(c, nb, nc, nbytes, true,
                          !nb || (d_ids && d_c0 && d_kappa && d_c1 && d_c2 && d_data && d_ok))))
    return rc;
  if (!aligned16({d_ids, d_c0, d_kappa, d_c2})) return fail(EG_ERR_ARG, "device pointer not 16-byte aligned");
  if (!nb) return EG_OK;
  Locked L(c);
  // every item's ballot is i / ncontest, so one launch covers the batch (nothing is staged)
  return open_locked(c, nb * nc, nc, nbytes, d_ids, d_c0, d_kappa, d_c1, d_c2, d_data, d_ok);
}

extern "C" int eg_open_contest_data(eg_ctx* c, size_t nb, size_t nc, size_t nbytes, const uint8_t* ids,
                                    const uint8_t* c0, const uint8_t* kappa, const uint8_t* c1, const uint8_t* c2,
                                    uint8_t* out_data, uint8_t* out_ok) {
  int rc;
  if ((rc = cd_shape_args(c, nb, nc, nbytes, true, !nb || (ids && c0 && kappa && c1 && c2 && out_data && out_ok))))
    return rc;
  if (!nb) return EG_OK;
  const size_t chunk = ballot_chunk(nc), first = std::min(chunk, nb) * nc;
  Locked L(c);
  uint8_t *d_ids = nullptr, *d_c0 = nullptr, *d_kappa = nullptr, *d_c1 = nullptr, *d_c2 = nullptr, *d_data = nullptr,
          *d_ok = nullptr;
  if ((rc = ws_get(c, W_H0, first / nc * 32, (void**)&d_ids))) return rc;
  if ((rc = ws_get(c, W_H3, first * 512, (void**)&d_c0))) return rc;
  if ((rc = ws_get(c, W_H5, first * 512, (void**)&d_kappa))) return rc;
  if ((rc = ws_get(c, W_H4, first * nbytes, (void**)&d_c1))) return rc;
  if ((rc = ws_get(c, W_H6, first * 32, (void**)&d_c2))) return rc;
  if ((rc = ws_get(c, W_H2, first * nbytes, (void**)&d_data))) return rc;
  if ((rc = ws_get(c, W_H1, first, (void**)&d_ok))) return rc;
  for (size_t b0 = 0; b0 < nb; b0 += chunk) {
    const size_t nbc = std::min(chunk, nb - b0), n = nbc * nc, i0 = b0 * nc;
    HIPCHK(hipMemcpyAsync(d_ids, ids + b0 * 32, nbc * 32, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_c0, c0 + i0 * 512, n * 512, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_kappa, kappa + i0 * 512, n * 512, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_c1, c1 + i0 * nbytes, n * nbytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_c2, c2 + i0 * 32, n * 32, hipMemcpyHostToDevice, c->stream));
    if ((rc = open_locked(c, n, nc, nbytes, d_ids, d_c0, d_kappa, d_c1, d_c2, d_data, d_ok))) return rc;
    HIPCHK(hipMemcpyAsync(out_data + i0 * nbytes, d_data, n * nbytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(out_ok + i0, d_ok, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  return EG_OK;
}
