// eg_capi_codes.inc — ballot nonces, ballot hashes and the confirmation-code chain
// (include/eg_hip_codes.h; included by eg_capi.hip after eg_capi_manifest.inc, whose shape
// checks and table cache these share).  The kernels are eg_codes.hpp's, one thread per hash.

// grid of a one-thread-per-item launch; an item count past 2^31 blocks is refused by the callers
static constexpr size_t kMaxCodeItems = ((size_t)1 << 31) * 256 - 256;
static inline unsigned cgrid(size_t n) { return (unsigned)((n + 255) / 256); }

static bool aligned16(std::initializer_list<const void*> ps) {
  for (const void* p : ps)
    if ((uintptr_t)p & 15) return false;
  return true;
}

static int codes_shape_args(eg_ctx* c, size_t nc, const uint32_t* spc, bool data_ok) {
  if (!c || !spc || !data_ok) return fail(EG_ERR_ARG, "null argument");
  return man_check(nc, spc, nullptr, nullptr);
}

// ---------------------------------------------------------------------------------
// nonces
// ---------------------------------------------------------------------------------
static int derive_locked(eg_ctx* c, size_t nb, size_t nsel, size_t nc, const uint8_t* d_bn, uint8_t* d_sn,
                         uint8_t* d_cn) {
  const size_t n = nb * (nsel * 4 + nc);
  hipLaunchKernelGGL(k_derive_nonces, dim3(cgrid(n)), dim3(256), 0, c->stream, c->d_q, d_bn, (uint64_t)nb,
                     (uint32_t)nsel, (uint32_t)nc, d_sn, d_cn, c->hash_fmt);
  HIPCHK(hipGetLastError());
  return EG_OK;
}

extern "C" int eg_derive_ballot_nonces_dev(eg_ctx* c, size_t nb, size_t nc, const uint32_t* spc,
                                           const uint8_t* d_bn, uint8_t* d_sn, uint8_t* d_cn) {
  int rc;
  if ((rc = codes_shape_args(c, nc, spc, !nb || (d_bn && d_sn && d_cn)))) return rc;
  if (!aligned16({d_bn, d_sn, d_cn})) return fail(EG_ERR_ARG, "device pointer not 16-byte aligned");
  if (!nb) return EG_OK;
  const ManShape M = man_shape(nc, spc, nullptr, nullptr);
  if (nb > kMaxCodeItems / (M.nsel * 4 + nc)) return fail(EG_ERR_ARG, "batch too large");
  Locked L(c);
  return derive_locked(c, nb, M.nsel, nc, d_bn, d_sn, d_cn);
}

extern "C" int eg_derive_ballot_nonces(eg_ctx* c, size_t nb, size_t nc, const uint32_t* spc, const uint8_t* bn,
                                       uint8_t* sn, uint8_t* cn) {
  int rc;
  if ((rc = codes_shape_args(c, nc, spc, !nb || (bn && sn && cn)))) return rc;
  if (!nb) return EG_OK;
  const ManShape M = man_shape(nc, spc, nullptr, nullptr);
  const size_t nsel = M.nsel, chunk = ballot_chunk(nsel);
  Locked L(c);
  uint8_t *d_bn = nullptr, *d_sn = nullptr, *d_cn = nullptr;
  const size_t first = std::min(chunk, nb);
  if ((rc = ws_get(c, W_H0, first * 32, (void**)&d_bn))) return rc;
  if ((rc = ws_get(c, W_H1, first * nsel * 128, (void**)&d_sn))) return rc;
  if ((rc = ws_get(c, W_H2, first * nc * 32, (void**)&d_cn))) return rc;
  for (size_t b0 = 0; b0 < nb; b0 += chunk) {
    const size_t n = std::min(chunk, nb - b0);
    HIPCHK(hipMemcpyAsync(d_bn, bn + b0 * 32, n * 32, hipMemcpyHostToDevice, c->stream));
    if ((rc = derive_locked(c, n, nsel, nc, d_bn, d_sn, d_cn))) return rc;
    HIPCHK(hipMemcpyAsync(sn + b0 * nsel * 128, d_sn, n * nsel * 128, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(cn + b0 * nc * 32, d_cn, n * nc * 32, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  return EG_OK;
}

// ---------------------------------------------------------------------------------
// ballot hashes
// ---------------------------------------------------------------------------------
// One chunk of <= ballot_chunk(nsel) ballots, device pointers.  hs / hc: where the chunk's
// selection and contest hashes go (the caller's buffers, or workspace when it wants neither).
static int hash_chunk_locked(eg_ctx* c, const ManShape& M, size_t nbc, const uint8_t* d_dsel, const uint8_t* d_dcon,
                             const uint8_t* d_mh, const uint8_t* d_ids, const uint8_t* d_cts, uint8_t* d_B,
                             uint8_t* hs, uint8_t* hc) {
  int rc;
  const size_t nc = M.nc, nsel = M.nsel, ns = nbc * nsel, ncn = nbc * nc;
  if (!hs && (rc = ws_get(c, W_OK0, ns * 32, (void**)&hs))) return rc;
  if (!hc && (rc = ws_get(c, W_OK1, ncn * 32, (void**)&hc))) return rc;
  std::vector<const uint32_t*> jv;
  if ((rc = cached_job_set(c, "ch/" + M.key, {"first", "spc"},
                           [&]() { return std::vector<std::vector<uint32_t>>{M.first, M.spc}; }, jv)))
    return rc;
  hipLaunchKernelGGL(k_sel_hash, dim3(cgrid(ns)), dim3(256), 0, c->stream, c->d_q, d_dsel, d_cts, (uint64_t)ns,
                     (uint32_t)nsel, hs, c->hash_fmt);
  hipLaunchKernelGGL(k_seg_hash, dim3(cgrid(ncn)), dim3(256), 0, c->stream, c->d_q, SegLead{d_dcon, (uint64_t)nc},
                     SegLead{nullptr, 1}, hs, jv[0], jv[1], (uint32_t)nc, (uint64_t)nsel, 0u, (uint64_t)ncn, hc,
                     c->hash_fmt);
  hipLaunchKernelGGL(k_seg_hash, dim3(cgrid(nbc)), dim3(256), 0, c->stream, c->d_q, SegLead{d_ids, (uint64_t)nbc},
                     SegLead{d_mh, 1}, hc, nullptr, nullptr, 1u, (uint64_t)nc, (uint32_t)nc, (uint64_t)nbc, d_B,
                     c->hash_fmt);
  HIPCHK(hipGetLastError());
  return EG_OK;
}

extern "C" int eg_ballot_hashes_dev(eg_ctx* c, size_t nb, size_t nc, const uint32_t* spc, const uint8_t* d_dsel,
                                    const uint8_t* d_dcon, const uint8_t* d_mh, const uint8_t* d_ids,
                                    const uint8_t* d_cts, uint8_t* d_B, uint8_t* d_hs, uint8_t* d_hc) {
  int rc;
  if ((rc = codes_shape_args(c, nc, spc, !nb || (d_dsel && d_dcon && d_mh && d_ids && d_cts && d_B)))) return rc;
  if (!aligned16({d_dsel, d_dcon, d_mh, d_ids, d_cts, d_B, d_hs, d_hc}))
    return fail(EG_ERR_ARG, "device pointer not 16-byte aligned");
  if (!nb) return EG_OK;
  const ManShape M = man_shape(nc, spc, nullptr, nullptr);
  const size_t nsel = M.nsel, chunk = ballot_chunk(nsel);
  Locked L(c);
  for (size_t b0 = 0; b0 < nb; b0 += chunk) {
    const size_t n = std::min(chunk, nb - b0);
    if ((rc = hash_chunk_locked(c, M, n, d_dsel, d_dcon, d_mh, d_ids + b0 * 32, d_cts + b0 * nsel * 1024,
                                d_B + b0 * 32, d_hs ? d_hs + b0 * nsel * 32 : nullptr,
                                d_hc ? d_hc + b0 * nc * 32 : nullptr)))
      return rc;
  }
  return EG_OK;
}

extern "C" int eg_ballot_hashes(eg_ctx* c, size_t nb, size_t nc, const uint32_t* spc, const uint8_t* dsel,
                                const uint8_t* dcon, const uint8_t manifest_hash[32], const uint8_t* ids,
                                const uint8_t* cts, uint8_t* out_B, uint8_t* out_hs, uint8_t* out_hc) {
  int rc;
  if ((rc = codes_shape_args(c, nc, spc, !nb || (dsel && dcon && manifest_hash && ids && cts && out_B)))) return rc;
  if (!nb) return EG_OK;
  const ManShape M = man_shape(nc, spc, nullptr, nullptr);
  const size_t nsel = M.nsel, chunk = ballot_chunk(nsel), first = std::min(chunk, nb);
  Locked L(c);
  // the manifest's description hashes in one buffer: [dsel nsel][dcon nc][manifest_hash]
  uint8_t *d_desc = nullptr, *d_ids = nullptr, *d_cts = nullptr, *d_B = nullptr, *d_hs = nullptr, *d_hc = nullptr;
  if ((rc = ws_get(c, W_H1, (nsel + nc + 1) * 32, (void**)&d_desc))) return rc;
  if ((rc = ws_get(c, W_H0, first * nsel * 1024, (void**)&d_cts))) return rc;
  if ((rc = ws_get(c, W_H2, first * 32, (void**)&d_ids))) return rc;
  if ((rc = ws_get(c, W_H3, first * 32, (void**)&d_B))) return rc;
  if ((rc = ws_get(c, W_OK0, first * nsel * 32, (void**)&d_hs))) return rc;
  if ((rc = ws_get(c, W_OK1, first * nc * 32, (void**)&d_hc))) return rc;
  HIPCHK(hipMemcpyAsync(d_desc, dsel, nsel * 32, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(d_desc + nsel * 32, dcon, nc * 32, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(d_desc + (nsel + nc) * 32, manifest_hash, 32, hipMemcpyHostToDevice, c->stream));
  // staged in the verifier's chunks, so the device holds one chunk of ciphertexts however many
  // ballots the caller passes
  for (size_t b0 = 0; b0 < nb; b0 += chunk) {
    const size_t n = std::min(chunk, nb - b0);
    HIPCHK(hipMemcpyAsync(d_cts, cts + b0 * nsel * 1024, n * nsel * 1024, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_ids, ids + b0 * 32, n * 32, hipMemcpyHostToDevice, c->stream));
    if ((rc = hash_chunk_locked(c, M, n, d_desc, d_desc + nsel * 32, d_desc + (nsel + nc) * 32, d_ids, d_cts, d_B,
                                d_hs, d_hc)))
      return rc;
    HIPCHK(hipMemcpyAsync(out_B + b0 * 32, d_B, n * 32, hipMemcpyDeviceToHost, c->stream));
    if (out_hs) HIPCHK(hipMemcpyAsync(out_hs + b0 * nsel * 32, d_hs, n * nsel * 32, hipMemcpyDeviceToHost, c->stream));
    if (out_hc) HIPCHK(hipMemcpyAsync(out_hc + b0 * nc * 32, d_hc, n * nc * 32, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  return EG_OK;
}

// ---------------------------------------------------------------------------------
// the code chain
// ---------------------------------------------------------------------------------
static int chain_args(eg_ctx* c, size_t nb, const void* seed, const void* ts, const void* B, const void* codes,
                      const void* ok) {
  if (!c || (nb && (!seed || !ts || !B || !codes || !ok))) return fail(EG_ERR_ARG, "null argument");
  if (nb > kMaxCodeItems) return fail(EG_ERR_ARG, "batch too large");
  return EG_OK;
}

extern "C" int eg_verify_code_chain_dev(eg_ctx* c, size_t nb, const uint8_t* d_seed, const uint8_t* d_ts,
                                        const uint8_t* d_B, const uint8_t* d_codes, uint8_t* d_ok) {
  int rc;
  if ((rc = chain_args(c, nb, d_seed, d_ts, d_B, d_codes, d_ok))) return rc;
  if (!aligned16({d_seed, d_ts, d_B, d_codes})) return fail(EG_ERR_ARG, "device pointer not 16-byte aligned");
  if (!nb) return EG_OK;
  Locked L(c);
  hipLaunchKernelGGL(k_code_check, dim3(cgrid(nb)), dim3(256), 0, c->stream, c->d_q, d_seed, d_ts, d_B, d_codes,
                     (uint64_t)nb, d_ok, c->hash_fmt);
  HIPCHK(hipGetLastError());
  return EG_OK;
}

extern "C" int eg_verify_code_chain(eg_ctx* c, size_t nb, const uint8_t seed[32], const uint8_t* ts, const uint8_t* B,
                                    const uint8_t* codes, uint8_t* ok) {
  int rc;
  if ((rc = chain_args(c, nb, seed, ts, B, codes, ok))) return rc;
  if (!nb) return EG_OK;
  Locked L(c);
  // one upload: [seed][ts nb][B nb][codes nb]
  uint8_t *d_in = nullptr, *d_ok = nullptr;
  if ((rc = ws_get(c, W_H0, (1 + 3 * nb) * 32, (void**)&d_in))) return rc;
  if ((rc = ws_get(c, W_H3, nb, (void**)&d_ok))) return rc;
  uint8_t *d_ts = d_in + 32, *d_B = d_ts + nb * 32, *d_codes = d_B + nb * 32;
  HIPCHK(hipMemcpyAsync(d_in, seed, 32, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(d_ts, ts, nb * 32, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(d_B, B, nb * 32, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(d_codes, codes, nb * 32, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_code_check, dim3(cgrid(nb)), dim3(256), 0, c->stream, c->d_q, d_in, d_ts, d_B, d_codes,
                     (uint64_t)nb, d_ok, c->hash_fmt);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(ok, d_ok, nb, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return EG_OK;
}
