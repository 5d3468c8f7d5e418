// eg_capi_codes.inc — ballot nonces, ballot hashes and the confirmation-code chain
// (include/eg_hip_codes.h; included by eg_capi.hip after eg_capi_manifest.inc, whose shape
// checks and table cache these share).  The kernels are eg_codes.hpp's, one thread per hash.
// Each entry point and its _dev twin are one body taking `bool host`: the checks, then one staged
// run of its chunk function (eg_stage.hpp), which copies the columns in host mode and only
// advances the caller's pointers in device mode.

// an item count past 2^31 blocks of a one-thread-per-item launch is refused by the callers
static constexpr size_t kMaxCodeItems = ((size_t)1 << 31) * 256 - 256;

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

// host: staged in the verifier's chunks; device: the whole batch is one launch
static int derive_ballot_nonces(eg_ctx* c, bool host, size_t nb, size_t nc, const uint32_t* spc, const uint8_t* bn,
                                uint8_t* sn, uint8_t* cn) {
  int rc;
  if ((rc = codes_shape_args(c, nc, spc, !nb || (bn && sn && cn)))) return rc;
  if (!host && !aligned16({bn, sn, cn})) return fail(EG_ERR_ARG, "device pointer not 16-byte aligned");
  if (!nb) return EG_OK;
  const ManShape M = man_shape(nc, spc, nullptr, nullptr);
  const size_t nsel = M.nsel;
  if (!host && nb > kMaxCodeItems / (nsel * 4 + nc)) return fail(EG_ERR_ARG, "batch too large");
  Locked L(c);
  Stage st(c, host, nb, host ? ballot_chunk(nsel) : nb);
  st.in(bn, 32);
  st.out(sn, nsel * 128);
  st.out(cn, nc * 32);
  return st.run([&](size_t n) { return derive_locked(c, n, nsel, nc, bn, sn, cn); });
}

extern "C" int eg_derive_ballot_nonces_dev(eg_ctx* c, size_t nb, size_t nc, const uint32_t* spc,
                                           const uint8_t* d_bn, uint8_t* d_sn, uint8_t* d_cn) {
  return derive_ballot_nonces(c, false, nb, nc, spc, d_bn, d_sn, d_cn);
}

extern "C" int eg_derive_ballot_nonces(eg_ctx* c, size_t nb, size_t nc, const uint32_t* spc, const uint8_t* bn,
                                       uint8_t* sn, uint8_t* cn) {
  return derive_ballot_nonces(c, true, nb, nc, spc, bn, sn, cn);
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
                           [&]() { return JobSet{M.first, M.spc}; }, jv)))
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

// staged in the verifier's chunks, so in host mode the device holds one chunk of ciphertexts
// however many ballots the caller passes
static int ballot_hashes(eg_ctx* c, bool host, size_t nb, size_t nc, const uint32_t* spc, const uint8_t* dsel,
                         const uint8_t* dcon, const uint8_t* mh, const uint8_t* ids, const uint8_t* cts, uint8_t* B,
                         uint8_t* hs, uint8_t* hc) {
  int rc;
  if ((rc = codes_shape_args(c, nc, spc, !nb || (dsel && dcon && mh && ids && cts && B)))) return rc;
  if (!host && !aligned16({dsel, dcon, mh, ids, cts, B, hs, hc}))
    return fail(EG_ERR_ARG, "device pointer not 16-byte aligned");
  if (!nb) return EG_OK;
  const ManShape M = man_shape(nc, spc, nullptr, nullptr);
  const size_t nsel = M.nsel;
  Locked L(c);
  Stage st(c, host, nb, ballot_chunk(nsel));
  st.once(dsel, nsel * 32);
  st.once(dcon, nc * 32);
  st.once(mh, 32);
  st.in(ids, 32);
  st.in(cts, nsel * 1024);
  st.out(B, 32);
  st.out(hs, nsel * 32);
  st.out(hc, nc * 32);
  return st.run([&](size_t n) { return hash_chunk_locked(c, M, n, dsel, dcon, mh, ids, cts, B, hs, hc); });
}

extern "C" int eg_ballot_hashes_dev(eg_ctx* c, size_t nb, size_t nc, const uint32_t* spc, const uint8_t* d_dsel,
                                    const uint8_t* d_dcon, const uint8_t* d_mh, const uint8_t* d_ids,
                                    const uint8_t* d_cts, uint8_t* d_B, uint8_t* d_hs, uint8_t* d_hc) {
  return ballot_hashes(c, false, nb, nc, spc, d_dsel, d_dcon, d_mh, d_ids, d_cts, d_B, d_hs, d_hc);
}

extern "C" int eg_ballot_hashes(eg_ctx* c, size_t nb, size_t nc, const uint32_t* spc, const uint8_t* dsel,
                                const uint8_t* dcon, const uint8_t manifest_hash[32], const uint8_t* ids,
                                const uint8_t* cts, uint8_t* out_B, uint8_t* out_hs, uint8_t* out_hc) {
  return ballot_hashes(c, true, nb, nc, spc, dsel, dcon, manifest_hash, ids, cts, out_B, out_hs, out_hc);
}

// ---------------------------------------------------------------------------------
// the code chain
// ---------------------------------------------------------------------------------
static int chain_locked(eg_ctx* c, size_t nb, const uint8_t* d_seed, const uint8_t* d_ts, const uint8_t* d_B,
                        const uint8_t* d_codes, uint8_t* d_ok) {
  hipLaunchKernelGGL(k_code_check, dim3(cgrid(nb)), dim3(256), 0, c->stream, c->d_q, d_seed, d_ts, d_B, d_codes,
                     (uint64_t)nb, d_ok, c->hash_fmt);
  HIPCHK(hipGetLastError());
  return EG_OK;
}

// one launch in both modes: a link reads the recorded code before it
static int verify_code_chain(eg_ctx* c, bool host, size_t nb, const uint8_t* seed, const uint8_t* ts, const uint8_t* B,
                             const uint8_t* codes, uint8_t* ok) {
  if (!c || (nb && (!seed || !ts || !B || !codes || !ok))) return fail(EG_ERR_ARG, "null argument");
  if (nb > kMaxCodeItems) return fail(EG_ERR_ARG, "batch too large");
  if (!host && !aligned16({seed, ts, B, codes})) return fail(EG_ERR_ARG, "device pointer not 16-byte aligned");
  if (!nb) return EG_OK;
  Locked L(c);
  Stage st(c, host, nb, nb);
  st.once(seed, 32);
  st.in(ts, 32);
  st.in(B, 32);
  st.in(codes, 32);
  st.out(ok, 1);
  return st.run([&](size_t n) { return chain_locked(c, n, seed, ts, B, codes, ok); });
}

extern "C" int eg_verify_code_chain_dev(eg_ctx* c, size_t nb, const uint8_t* d_seed, const uint8_t* d_ts,
                                        const uint8_t* d_B, const uint8_t* d_codes, uint8_t* d_ok) {
  return verify_code_chain(c, false, nb, d_seed, d_ts, d_B, d_codes, d_ok);
}

extern "C" int eg_verify_code_chain(eg_ctx* c, size_t nb, const uint8_t seed[32], const uint8_t* ts, const uint8_t* B,
                                    const uint8_t* codes, uint8_t* ok) {
  return verify_code_chain(c, true, nb, seed, ts, B, codes, ok);
}
