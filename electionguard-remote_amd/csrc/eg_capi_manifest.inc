// eg_capi_manifest.inc — the ballot entry points for manifests of unequal contests
// (include/eg_hip_manifest.h; included by eg_capi.hip after eg_capi_ballot.inc).  Contest k of a
// ballot owns spc[k] consecutive selections, placeholders[k] of them last, and its constant
// proof uses limit[k].
//
// This file checks the lists and builds the table-addressed ManShape from them; the chunk
// routines, the contest layer and the four drivers are eg_capi_ballot.inc's.  These entries
// always build the table-addressed shape, also when every contest is alike, so the same ballots
// can be run through both arms of the contest layer.

// The argument checks of eg_hip_manifest.h, before anything is allocated or any ballot byte is
// read: the scan stops at the first contest that takes nsel past kMaxSelections, so a huge
// ncontest costs at most kMaxSelections + 1 steps.  ph / limit may be null (the encryptor).
static int man_check(size_t nc, const uint32_t* spc, const uint32_t* ph, const uint32_t* limit) {
  if (!nc) return fail(EG_ERR_ARG, "bad manifest: no contests");
  size_t nsel = 0;
  for (size_t k = 0; k < nc; ++k) {
    if (!spc[k]) return fail(EG_ERR_ARG, "bad manifest: contest " + std::to_string(k) + " has no selections");
    if (ph && ph[k] >= spc[k])
      return fail(EG_ERR_ARG, "bad manifest: contest " + std::to_string(k) + " has no real selection");
    // a limit above the contest's size has no honest proof, and k_scalar_prep's L * c folds
    // q out of the product L times
    if (limit && limit[k] > spc[k])
      return fail(EG_ERR_ARG, "bad manifest: contest " + std::to_string(k) + " has a limit above its selections");
    nsel += spc[k];
    if (nsel > kMaxSelections) return fail(EG_ERR_ARG, "bad manifest: more than 2^20 selections per ballot");
  }
  return EG_OK;
}

static ManShape man_shape(size_t nc, const uint32_t* spc, const uint32_t* ph, const uint32_t* limit) {
  ManShape M;
  M.nc = nc;
  M.fam = "m";
  M.spc.assign(spc, spc + nc);
  M.first.resize(nc);
  if (limit) M.limit.assign(limit, limit + nc);
  std::map<uint32_t, std::vector<uint32_t>> by;
  for (size_t k = 0; k < nc; ++k) {
    M.first[k] = (uint32_t)M.nsel;
    const uint32_t nr = spc[k] - (ph ? ph[k] : 0u);
    for (uint32_t s = 0; s < nr; ++s) M.real.push_back((uint32_t)M.nsel + s);
    M.nsel += spc[k];
    by[spc[k]].push_back((uint32_t)k);
  }
  M.nreal = M.real.size();
  for (auto& kv : by) {
    const size_t n = kv.second.size();
    M.cls.push_back(ManShape::Class{kv.first, n, std::move(kv.second), std::to_string(M.cls.size())});
  }
  auto list = [&](const uint32_t* v) {
    std::string s;
    for (size_t k = 0; k < nc; ++k) s += std::to_string(v[k]) + ",";
    return s;
  };
  M.key = list(spc);
  if (ph) M.key += "/" + list(ph);
  if (limit) M.key += "/" + list(limit);
  return M;
}

static int man_verify_args(eg_ctx* c, const uint8_t* K_be, const uint8_t* qbar_be, size_t nb, size_t nc,
                           const uint32_t* spc, const uint32_t* ph, const uint32_t* limit, const void* cts,
                           const void* rproof, const void* cproof, const void* ok_sel, const void* ok_con) {
  if (!c || !K_be || !qbar_be || !spc || !ph || !limit || (nb && (!cts || !rproof || !cproof || !ok_sel || !ok_con)))
    return fail(EG_ERR_ARG, "null argument");
  return man_check(nc, spc, ph, limit);
}

extern "C" int eg_verify_ballots_manifest_dev(eg_ctx* c, const uint8_t K_be[512], const uint8_t qbar_be[32], size_t nb,
                                              size_t nc, const uint32_t* spc, const uint32_t* ph,
                                              const uint32_t* limit, const uint8_t* d_cts, const uint8_t* d_rproof,
                                              const uint8_t* d_cproof, const uint8_t* d_cast, uint8_t* d_ok_sel,
                                              uint8_t* d_ok_con, uint8_t* d_tally_be) {
  int rc;
  if ((rc = man_verify_args(c, K_be, qbar_be, nb, nc, spc, ph, limit, d_cts, d_rproof, d_cproof, d_ok_sel, d_ok_con)))
    return rc;
  const ManShape M = man_shape(nc, spc, ph, limit);
  Locked L(c);
  if ((rc = use_key_locked(c, K_be))) return rc;
  return verify_dev_locked(c, M, qbar_be, nb, d_cts, d_rproof, d_cproof, d_cast, d_ok_sel, d_ok_con, d_tally_be);
}

extern "C" int eg_verify_ballots_manifest(eg_ctx* c, const uint8_t K_be[512], const uint8_t qbar_be[32], size_t nb,
                                          size_t nc, const uint32_t* spc, const uint32_t* ph, const uint32_t* limit,
                                          const uint8_t* cts, const uint8_t* rproof, const uint8_t* cproof,
                                          const uint8_t* cast, uint8_t* ok_sel, uint8_t* ok_con, uint8_t* tally_be) {
  int rc;
  if ((rc = man_verify_args(c, K_be, qbar_be, nb, nc, spc, ph, limit, cts, rproof, cproof, ok_sel, ok_con))) return rc;
  const ManShape M = man_shape(nc, spc, ph, limit);
  Locked L(c);
  if ((rc = use_key_locked(c, K_be))) return rc;
  return verify_host_locked(c, M, qbar_be, nb, cts, rproof, cproof, cast, ok_sel, ok_con, tally_be);
}

static int man_encrypt_args(eg_ctx* c, const uint8_t* K_be, const uint8_t* qbar_be, size_t nb, size_t nc,
                            const uint32_t* spc, const void* votes, const void* sn, const void* cn, const void* cts,
                            const void* rproof, const void* cproof) {
  if (!c || !K_be || !qbar_be || !spc || (nb && (!votes || !sn || !cn || !cts || !rproof || !cproof)))
    return fail(EG_ERR_ARG, "null argument");
  return man_check(nc, spc, nullptr, nullptr);
}

extern "C" int eg_encrypt_ballots_manifest(eg_ctx* c, const uint8_t K_be[512], const uint8_t qbar_be[32], size_t nb,
                                           size_t nc, const uint32_t* spc, const uint8_t* votes,
                                           const uint8_t* sel_nonces, const uint8_t* contest_nonces, uint8_t* cts,
                                           uint8_t* rproof, uint8_t* cproof) {
  int rc;
  if ((rc = man_encrypt_args(c, K_be, qbar_be, nb, nc, spc, votes, sel_nonces, contest_nonces, cts, rproof, cproof)))
    return rc;
  if (!nb) return EG_OK;
  const ManShape M = man_shape(nc, spc, nullptr, nullptr);
  Locked L(c);
  if ((rc = use_key_locked(c, K_be))) return rc;
  return encrypt_host_locked(c, M, qbar_be, nb, votes, sel_nonces, contest_nonces, cts, rproof, cproof);
}

extern "C" int eg_encrypt_ballots_manifest_dev(eg_ctx* c, const uint8_t K_be[512], const uint8_t qbar_be[32],
                                               size_t nb, size_t nc, const uint32_t* spc, const uint8_t* d_votes,
                                               const uint8_t* d_sel_nonces, const uint8_t* d_contest_nonces,
                                               uint8_t* d_cts, uint8_t* d_rproof, uint8_t* d_cproof) {
  int rc;
  if ((rc = man_encrypt_args(c, K_be, qbar_be, nb, nc, spc, d_votes, d_sel_nonces, d_contest_nonces, d_cts, d_rproof,
                             d_cproof)))
    return rc;
  if (!nb) return EG_OK;
  const ManShape M = man_shape(nc, spc, nullptr, nullptr);
  Locked L(c);
  if ((rc = use_key_locked(c, K_be))) return rc;
  return encrypt_dev_locked(c, M, qbar_be, nb, d_votes, d_sel_nonces, d_contest_nonces, d_cts, d_rproof, d_cproof);
}
