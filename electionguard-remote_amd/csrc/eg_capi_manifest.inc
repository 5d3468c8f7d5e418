// eg_capi_manifest.inc — the ballot entry points for manifests of unequal contests
// (include/eg_hip_manifest.h; included by eg_capi.hip after eg_capi_ballot.inc, whose helpers
// these share).  Contest k of a ballot owns spc[k] consecutive selections, placeholders[k] of
// them last, and its constant proof uses limit[k].
//
// The selection part of a chunk is verify_chunk_locked's / encrypt_chunk_locked's on
// ns = nbc * nsel jobs: a selection job does not know its contest.  The contest layer differs:
//   * contests are grouped into CLASSES of equal spc (PowShape.gather is part of k_pow's op
//     program, so one contest population per class);
//   * a class's aggregates A = prod alpha, B = prod beta come from k_prod_tab, addressed
//     through a device table of the class's first selections and scattered into ballot-major
//     contest order (where export and hash read them, exactly as in the uniform path);
//   * the contest flags, the -L c scalar and the nonce sums read per-contest tables;
//   * the tally is one k_prod_tab over the table of real selections.

// The validated shape of one call (host side).
struct ManShape {
  size_t nc = 0, nsel = 0, nreal = 0;
  std::vector<uint32_t> spc, first, limit, real;  // per contest; real: the real selections' indices
  struct Class {
    uint32_t spc;
    std::vector<uint32_t> members;  // contest indices, ascending
  };
  std::vector<Class> cls;  // ascending spc
  std::string key;         // the spc list (verify: and the placeholders and limits), for the table cache
};

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
  for (auto& kv : by) M.cls.push_back(ManShape::Class{kv.first, std::move(kv.second)});
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

// run_prod with table-addressed groups (k_prod_tab): group g starts at element
// tab[g % period] + (g / period) * period_stride and its product goes to element
// otab[g % period] + (g / period) * ostride of d_out (otab == nullptr: element g).
static int run_prod_tab(eg_ctx* c, const uint32_t* d_in, const uint32_t* tab, size_t period, size_t period_stride,
                        size_t groups, size_t len, size_t stride, uint32_t* d_out, const uint32_t* otab,
                        size_t ostride, const uint8_t* mask = nullptr) {
  if (!groups) return EG_OK;
  if (len == 0) return fail(EG_ERR_ARG, "empty product");
  const uint32_t chunk = len > 32 ? 8u : 32u;  // as run_prod
  const size_t maxpart = groups * ((len + chunk - 1) / chunk);
  uint32_t* tmp = nullptr;
  int rc = ws_get(c, W_TMP, std::max<size_t>(1, maxpart) * kW * 4 * 2, (void**)&tmp);
  if (rc) return rc;
  uint32_t* ping[2] = {tmp, tmp + maxpart * kW};
  size_t cur_len = len, cur_stride = stride, cur_pstride = period_stride;
  const uint32_t* src = d_in;
  int pi = 0;
  while (true) {
    const uint32_t nchunk = (uint32_t)((cur_len + chunk - 1) / chunk);
    const uint32_t ch = nchunk == 1 ? (uint32_t)cur_len : chunk;
    const bool last = nchunk == 1;
    LAUNCH_F(c, k_prod_tab, dim3(grid_for(groups * nchunk)), c->d, src, tab, (uint32_t)period, (uint32_t)cur_pstride,
             (uint32_t)groups, (uint32_t)cur_len, (uint32_t)cur_stride, ch, nchunk, last ? d_out : ping[pi],
             last ? otab : nullptr, (uint32_t)ostride, mask);
    HIPCHK(hipGetLastError());
    if (last) break;
    mask = nullptr;  // later passes multiply partial products: group g's are contiguous at g * nchunk
    tab = nullptr;
    src = ping[pi];
    cur_pstride = nchunk;
    cur_len = nchunk;
    cur_stride = 1;
    pi ^= 1;
  }
  return EG_OK;
}

// the in / out tables of class ci's aggregate product: entry mi * 2 + comp of member contest k
static std::vector<uint32_t> class_in_table(const ManShape& M, size_t ci) {
  std::vector<uint32_t> t;
  for (uint32_t k : M.cls[ci].members)
    for (uint32_t comp = 0; comp < 2; ++comp) t.push_back(M.first[k] * 2 + comp);
  return t;
}
static std::vector<uint32_t> class_out_table(const ManShape& M, size_t ci) {
  std::vector<uint32_t> t;
  for (uint32_t k : M.cls[ci].members)
    for (uint32_t comp = 0; comp < 2; ++comp) t.push_back(k * 2 + comp);
  return t;
}

// every class's aggregates of nbc ballots: elems (ballot-major ciphertext pairs) -> agg[(b nc + k) 2 + comp]
static int man_aggregates(eg_ctx* c, const ManShape& M, size_t nbc, const uint32_t* elems,
                          const std::vector<const uint32_t*>& tin, const std::vector<const uint32_t*>& tout,
                          uint32_t* agg) {
  for (size_t ci = 0; ci < M.cls.size(); ++ci) {
    const size_t period = M.cls[ci].members.size() * 2;
    const int rc = run_prod_tab(c, elems, tin[ci], period, 2 * M.nsel, nbc * period, M.cls[ci].spc, 2, agg, tout[ci],
                                2 * M.nc);
    if (rc) return rc;
  }
  return EG_OK;
}

// One chunk of <= ballot_chunk(nsel) ballots; arguments as verify_chunk_locked.
static int verify_chunk_manifest_locked(eg_ctx* c, const ManShape& M, size_t nbc, const uint8_t* cts,
                                        const uint8_t* d_rproof, const uint8_t* d_cproof, const uint8_t* d_cast,
                                        uint8_t* d_ok_sel, uint8_t* d_ok_con, uint32_t* tally, bool first) {
  const FbTab G = c->gtab->tab(), K = c->Ktab->tab();
  const size_t nc = M.nc, nsel = M.nsel, nreal = M.nreal, ncls = M.cls.size();
  const size_t ns = nbc * nsel, ncn = nbc * nc;
  int rc;
  uint32_t *E = nullptr, *COMM = nullptr;
  uint8_t *LTP = nullptr, *SC = nullptr, *OKR = nullptr, *OKC = nullptr, *COMM_BE = nullptr, *CP_BE = nullptr;
  if ((rc = ws_get(c, W_E0, (ns * 2 + ncn * 2) * kW * 4, (void**)&E))) return rc;
  if ((rc = ws_get(c, W_E1, (ns * 4 + ncn * 2) * kW * 4, (void**)&COMM))) return rc;
  if ((rc = ws_get(c, W_FLAGS, ns * 2, (void**)&LTP))) return rc;
  const size_t off_c = ns * 4, off_neg = off_c + ncn * 2, off_negL = off_neg + ns;
  if ((rc = ws_get(c, W_SCAL, (off_negL + ncn) * 32, (void**)&SC))) return rc;
  if ((rc = ws_get(c, W_OK0, ns, (void**)&OKR))) return rc;
  if ((rc = ws_get(c, W_OK1, ncn, (void**)&OKC))) return rc;
  if ((rc = ws_get(c, W_BE0, (ns * 4 + ncn * 2) * 512, (void**)&COMM_BE))) return rc;
  if ((rc = ws_get(c, W_BE1, ncn * 2 * 512, (void**)&CP_BE))) return rc;
  // The chunk's tables, one cached set (a second set could be freed by the first's cache_bound):
  // the per-contest tables, the tally's table of real selections, the selection jobs, and per
  // class the aggregate product's in / out tables and the contest jobs.
  std::vector<std::string> names{"first", "spc", "limit", "tally", "A", "B"};
  for (size_t ci = 0; ci < ncls; ++ci)
    for (const char* n : {"in", "out", "CA", "CB"}) names.push_back(n + std::to_string(ci));
  std::vector<const uint32_t*> jv;
  rc = cached_job_set(c, "mv/" + std::to_string(nbc) + "/" + M.key, names, [&]() {
    std::vector<std::vector<uint32_t>> out{M.first, M.spc, M.limit};
    std::vector<uint32_t> tt;
    for (uint32_t r : M.real)
      for (uint32_t comp = 0; comp < 2; ++comp) tt.push_back(r * 2 + comp);
    out.push_back(std::move(tt));
    auto A = new_jobs(ns), B = new_jobs(ns);
    for (size_t i = 0; i < ns; ++i) {  // as verify_chunk_locked
      uint32_t* a = &A[i * kJobWords];
      uint32_t* b = &B[i * kJobWords];
      const uint32_t c0 = (uint32_t)(i * 4), v0 = c0 + 1, c1 = c0 + 2, v1 = c0 + 3;
      a[0] = (uint32_t)(i * 2); a[1] = c0; a[2] = c1; a[3] = (uint32_t)(i * 4 + 0); a[4] = (uint32_t)(i * 4 + 2);
      a[5] = v0; a[7] = v1;
      b[0] = (uint32_t)(i * 2 + 1); b[1] = c0; b[2] = c1; b[3] = (uint32_t)(i * 4 + 1); b[4] = (uint32_t)(i * 4 + 3);
      b[5] = v0; b[7] = v1; b[8] = (uint32_t)(off_neg + i);
    }
    out.push_back(std::move(A));
    out.push_back(std::move(B));
    for (size_t ci = 0; ci < ncls; ++ci) {
      const auto& mem = M.cls[ci].members;
      const size_t m = mem.size();
      auto CA = new_jobs(nbc * m), CB = new_jobs(nbc * m);
      for (size_t bi = 0; bi < nbc; ++bi)
        for (size_t mi = 0; mi < m; ++mi) {
          const size_t j = bi * nc + mem[mi];  // the contest's place in every ballot-major array
          uint32_t* a = &CA[(bi * m + mi) * kJobWords];
          uint32_t* b = &CB[(bi * m + mi) * kJobWords];
          const uint32_t cc = (uint32_t)(off_c + j * 2), vv = cc + 1;
          a[0] = (uint32_t)(ns * 2 + j * 2); a[1] = cc; a[3] = (uint32_t)(ns * 4 + j * 2); a[5] = vv;
          b[0] = (uint32_t)(ns * 2 + j * 2 + 1); b[1] = cc; b[3] = (uint32_t)(ns * 4 + j * 2 + 1); b[5] = vv;
          b[6] = (uint32_t)(off_negL + j);
          a[2] = b[2] = (uint32_t)(bi * nsel + M.first[mem[mi]]);  // gather: the contest's first selection job
        }
      out.push_back(class_in_table(M, ci));
      out.push_back(class_out_table(M, ci));
      out.push_back(std::move(CA));
      out.push_back(std::move(CB));
    }
    return out;
  }, jv);
  if (rc) return rc;
  const uint32_t *tFirst = jv[0], *tSpc = jv[1], *tLimit = jv[2], *tTally = jv[3], *jA = jv[4], *jB = jv[5];
  std::vector<const uint32_t*> tin(ncls), tout(ncls), jCA(ncls), jCB(ncls);
  for (size_t ci = 0; ci < ncls; ++ci) {
    tin[ci] = jv[6 + ci * 4]; tout[ci] = jv[7 + ci * 4]; jCA[ci] = jv[8 + ci * 4]; jCB[ci] = jv[9 + ci * 4];
  }
  // 1. import ciphertexts (range flags alpha, beta < p)
  if ((rc = launch_import(c, cts, ns * 2, E, LTP))) return rc;
  // 2. scalars: proofs + derived exponents (-c1, -L_k c) + range flags
  HIPCHK(hipMemcpyAsync(SC, d_rproof, ns * 128, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(SC + off_c * 32, d_cproof, ncn * 64, hipMemcpyDeviceToDevice, c->stream));
  hipLaunchKernelGGL(k_scalar_prep, dim3(tgrid(ns)), dim3(256), 0, c->stream, c->d_q, SC, (uint32_t)ns, 4u, 2u, 1u,
                     SC + off_neg * 32, OKR, c->resp_plus, 0x5u);
  hipLaunchKernelGGL(k_scalar_prep_tab, dim3(tgrid(ncn)), dim3(256), 0, c->stream, c->d_q, SC + off_c * 32,
                     (uint32_t)ncn, 2u, 0u, tLimit, (uint32_t)nc, SC + off_negL * 32, OKC, c->resp_plus, 0x1u);
  HIPCHK(hipGetLastError());
  // 3. contest aggregates -> E[ns*2 + j*2 + {0,1}], class by class
  uint32_t* CP = E + ns * 2 * kW;
  if ((rc = man_aggregates(c, M, nbc, E, tin, tout, CP))) return rc;
  // 4. commitments: the selection launches of verify_chunk_locked (alpha + a beta head that
  // fills launch 1's last round; the other betas), then the contest populations of every class
  const bool gat = c->use_comb != 0;
  uint32_t *YA = nullptr, *YB = nullptr, *RZ = nullptr;
  if (gat) {
    if ((rc = ws_get(c, W_YA, ns * (kCombH - 1) * kW * 4, (void**)&YA))) return rc;
    if ((rc = ws_get(c, W_YB, ns * (kCombH - 1) * kW * 4, (void**)&YB))) return rc;
  }
  if ((rc = ws_get(c, W_RZ, ns * 4 * kW * 4, (void**)&RZ))) return rc;
  const uint32_t srows = c->sel_rows, sblocks = c->sel_blocks;
  PowShape SA{};  // alpha: a0 = alpha^c0 g^v0, a1 = alpha^c1 g^v1
  SA.has_base = 1; SA.nout = 2; SA.nfb[0] = 1; SA.nfb[1] = 1; SA.exp_bytes = 32; SA.comb = 1; SA.resid = 1;
  SA.rows = srows; SA.blocks = sblocks; SA.tab[0][0] = 0; SA.tab[1][0] = 0;
  PowShape SB{};  // beta: b0 = beta^c0 K^v0, b1 = beta^c1 K^v1 g^-c1
  SB.has_base = 1; SB.nout = 2; SB.nfb[0] = 1; SB.nfb[1] = 2; SB.exp_bytes = 32; SB.comb = 1; SB.resid = 1;
  SB.rows = srows; SB.blocks = sblocks; SB.tab[0][0] = 1; SB.tab[1][0] = 1; SB.tab[1][1] = 0;
  // the contest populations: contest a = A^c g^v (needs the alpha y_k: any launch after 1) and
  // contest b = B^c K^v g^-Lc (needs the beta y_k: any launch after 2) of each class
  struct Pop { PowShape S; const uint32_t* jobs; size_t n; const uint32_t* ygat; };
  std::vector<Pop> pa, pb;
  for (size_t ci = 0; ci < ncls; ++ci) {
    const uint32_t gather = gat ? M.cls[ci].spc : 0u;
    const size_t n = nbc * M.cls[ci].members.size();
    PowShape SCA{};
    SCA.has_base = 1; SCA.nout = 1; SCA.nfb[0] = 1; SCA.exp_bytes = 32; SCA.tab[0][0] = 0;
    SCA.comb = gat ? 1u : 0u; SCA.gather = gather;
    PowShape SCB{};
    SCB.has_base = 1; SCB.nout = 1; SCB.nfb[0] = 2; SCB.exp_bytes = 32; SCB.tab[0][0] = 1; SCB.tab[0][1] = 0;
    SCB.comb = gat ? 1u : 0u; SCB.gather = gather;
    pa.push_back(Pop{SCA, jCA[ci], n, YA});
    pb.push_back(Pop{SCB, jCB[ci], n, YB});
  }
  size_t xb = 0;
  size_t slots = c->pow_slots;
  if (const char* ov = getenv("EG_POW_SLOTS")) slots = (size_t)strtoull(ov, nullptr, 10);  // test override
  if (slots) {  // the beta head, as verify_chunk_locked without EG_CB_EARLY
    auto last_blocks = [](size_t n) { return n ? (size_t)grid_for(n - (n - 1) / kPowMaxJobs * kPowMaxJobs) : 0; };
    const size_t fill1 = (slots - last_blocks(ns) % slots) % slots;
    xb = std::min(ns, fill1 * kGroupsPerBlock);
  }
  auto tail_of = [](const Pop& p) {
    PowTail T{};
    T.S = p.S; T.jobs = p.jobs; T.njobs = p.n; T.ygat = p.ygat;
    return T;
  };
  {
    PowTail T{};
    T.S = SB; T.jobs = jB; T.njobs = xb; T.yout = YB; T.rout = RZ + ns * 2 * kW;
    if ((rc = launch_pow(c, SA, jA, ns, E, SC, COMM, G, K, YA, nullptr, &T, RZ))) return rc;
  }
  // Launch 2 takes up to two contest-a populations as its tails; what is left of contest a and
  // every contest-b population follow three to a launch (a main part and two tails).  A tail is
  // never split into sub-launches, so only populations of at most kPowMaxJobs jobs ride as one.
  // At most 2 + (C - 2) + C <= 2 + 2 C launch_pow calls for C classes; one class gives the
  // uniform path's three.
  std::vector<Pop> rest;
  {
    std::vector<PowTail> tl;
    for (const Pop& p : pa) {
      if (tl.size() < 2 && p.n <= kPowMaxJobs) tl.push_back(tail_of(p));
      else rest.push_back(p);
    }
    if (const char* dbg = getenv("EG_DEBUG_SCHED"); dbg && dbg[0] == '1')
      fprintf(stderr, "eg verify schedule (manifest): ns %zu ncn %zu classes %zu slots %zu: beta head %zu, "
                      "contest a in launch 2: %zu\n", ns, ncn, ncls, slots, xb, tl.size());
    if ((rc = launch_pow(c, SB, jB + xb * kJobWords, ns - xb, E, SC, COMM, G, K,
                         gat ? YB + xb * (kCombH - 1) * kW : nullptr, nullptr, tl.size() > 0 ? &tl[0] : nullptr,
                         RZ + (ns + xb) * 2 * kW, false, nullptr, nullptr, tl.size() > 1 ? &tl[1] : nullptr)))
      return rc;
  }
  rest.insert(rest.end(), pb.begin(), pb.end());
  // alpha^q == 1 and beta^q == 1 (valid residues) fold into the range flags the hash check reads
  LAUNCH_F(c, k_resid_check, dim3(grid_for(ns)), c->d, RZ, (uint32_t)ns, LTP, 2u);
  LAUNCH_F(c, k_resid_check, dim3(grid_for(ns)), c->d, RZ + ns * 2 * kW, (uint32_t)ns, LTP + 1, 2u);
  HIPCHK(hipGetLastError());
  uint8_t* CRF = nullptr;  // (A, B) flags per contest: the AND of its selections' flags
  if ((rc = ws_get(c, W_CRF, ncn * 2, (void**)&CRF))) return rc;
  hipLaunchKernelGGL(k_contest_flags_seg, dim3(tgrid(ncn * 2)), dim3(256), 0, c->stream, LTP, (uint32_t)ncn,
                     (uint32_t)nc, (uint32_t)nsel, tFirst, tSpc, CRF);
  HIPCHK(hipGetLastError());
  for (size_t i = 0; i < rest.size();) {
    const Pop& main = rest[i++];
    PowTail T[2];
    size_t nt = 0;
    while (nt < 2 && i < rest.size() && rest[i].n <= kPowMaxJobs) T[nt++] = tail_of(rest[i++]);
    if ((rc = launch_pow(c, main.S, main.jobs, main.n, E, SC, COMM, G, K, nullptr, main.ygat, nt > 0 ? &T[0] : nullptr,
                         nullptr, false, nullptr, nullptr, nt > 1 ? &T[1] : nullptr)))
      return rc;
  }
  // 5. canonical bytes of commitments and contest aggregates
  if ((rc = launch_export(c, COMM, ns * 4 + ncn * 2, COMM_BE))) return rc;
  if ((rc = launch_export(c, CP, ncn * 2, CP_BE))) return rc;
  // 6. Fiat-Shamir checks
  if ((rc = launch_hash(c, (uint32_t)ns,
                        preimage(c, {HashSrc{cts, 512, 1024}, HashSrc{cts + 512, 512, 1024}},
                                 {HashSrc{COMM_BE, 512, 2048}, HashSrc{COMM_BE + 512, 512, 2048},
                                  HashSrc{COMM_BE + 1024, 512, 2048}, HashSrc{COMM_BE + 1536, 512, 2048}},
                                 key_src(c)),
                        d_rproof, 4, 0, 2, OKR, LTP, 2, d_ok_sel, nullptr)))
    return rc;
  const uint8_t* CC_BE = COMM_BE + ns * 4 * 512;
  if ((rc = launch_hash(c, (uint32_t)ncn,
                        preimage(c, {HashSrc{CP_BE, 512, 1024}, HashSrc{CP_BE + 512, 512, 1024}},
                                 {HashSrc{CC_BE, 512, 1024}, HashSrc{CC_BE + 512, 512, 1024}}, key_src(c)),
                        d_cproof, 2, 0, kNone, OKC, CRF, 2, d_ok_con, nullptr)))
    return rc;
  // 7. tally over this chunk's cast ballots: one group per (real selection, component)
  if (tally) {
    uint32_t* T = first ? tally : tally + nreal * 2 * kW;
    if ((rc = run_prod_tab(c, E, tTally, nreal * 2, 0, nreal * 2, nbc, nsel * 2, T, nullptr, 0, d_cast))) return rc;
    if (!first) {
      LAUNCH_F(c, k_mul, dim3(grid_for(nreal * 2)), c->d, tally, 1u, T, 1u, (uint32_t)(nreal * 2), tally, 1u);
      HIPCHK(hipGetLastError());
    }
  }
  return EG_OK;
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
  const size_t nsel = M.nsel, nreal = M.nreal;
  if (!nb) {
    if (d_tally_be) {
      std::vector<uint8_t> one(nreal * 2 * 512);
      ones_be(one.data(), nreal * 2);
      HIPCHK(hipMemcpyAsync(d_tally_be, one.data(), one.size(), hipMemcpyHostToDevice, c->stream));
      HIPCHK(hipStreamSynchronize(c->stream));
    }
    return EG_OK;
  }
  if (!c->Ktab) return fail(EG_ERR_STATE, "election key not set (eg_set_election_key)");
  HIPCHK(hipMemcpyAsync(c->d_qbar, qbar_be, 32, hipMemcpyHostToDevice, c->stream));
  uint32_t* tally = nullptr;  // running tally (Montgomery) + one chunk's product, nreal*2 elements each
  if (d_tally_be && (rc = ws_get(c, W_E2, nreal * 2 * 2 * kW * 4, (void**)&tally))) return rc;
  const size_t chunk = ballot_chunk(nsel);
  for (size_t b0 = 0; b0 < nb; b0 += chunk) {
    const size_t nbc = std::min(chunk, nb - b0);
    if ((rc = verify_chunk_manifest_locked(c, M, nbc, d_cts + b0 * nsel * 1024, d_rproof + b0 * nsel * 128,
                                           d_cproof + b0 * nc * 64, d_cast ? d_cast + b0 : nullptr,
                                           d_ok_sel + b0 * nsel, d_ok_con + b0 * nc, tally, b0 == 0)))
      return rc;
  }
  return d_tally_be ? launch_export(c, tally, nreal * 2, d_tally_be) : EG_OK;
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
  const size_t nsel = M.nsel, nreal = M.nreal;
  if (!nb) {
    if (tally_be) ones_be(tally_be, nreal * 2);
    return EG_OK;
  }
  // streamed through two upload buffers exactly as eg_verify_ballots
  if (!c->Ktab) return fail(EG_ERR_STATE, "election key not set (eg_set_election_key)");
  HIPCHK(hipMemcpyAsync(c->d_qbar, qbar_be, 32, hipMemcpyHostToDevice, c->stream));
  if ((rc = ensure_copy_stream(c))) return rc;
  const size_t chunk = ballot_chunk(nsel);
  uint32_t* tally = nullptr;
  uint8_t *d_oks = nullptr, *d_okc = nullptr, *d_cast = nullptr;
  if (tally_be && (rc = ws_get(c, W_E2, nreal * 2 * 2 * kW * 4, (void**)&tally))) return rc;
  if ((rc = ws_get(c, W_H3, nb * nsel, (void**)&d_oks))) return rc;
  if ((rc = ws_get(c, W_H4, nb * nc, (void**)&d_okc))) return rc;
  if (cast && tally_be && (rc = upload(c, W_CAST, cast, nb, (void**)&d_cast))) return rc;
  static constexpr Slot kUp[2][3] = {{W_H0, W_H1, W_H2}, {W_H6, W_H7, W_H8}};
  const size_t first = std::min(chunk, nb);
  uint8_t* up[2][3] = {};
  for (int k = 0; k < (nb > chunk ? 2 : 1); ++k) {  // sized once, before any copy is queued
    if ((rc = ws_get(c, kUp[k][0], first * nsel * 1024, (void**)&up[k][0])) ||
        (rc = ws_get(c, kUp[k][1], first * nsel * 128, (void**)&up[k][1])) ||
        (rc = ws_get(c, kUp[k][2], first * nc * 64, (void**)&up[k][2])))
      return rc;
  }
  size_t k = 0;
  for (size_t b0 = 0; b0 < nb; b0 += chunk, ++k) {
    const size_t nbc = std::min(chunk, nb - b0);
    const int u = (int)(k & 1);
    if (k >= 2) HIPCHK(hipStreamWaitEvent(c->copy, c->done_ev[u], 0));  // chunk k-2 no longer reads set u
    HIPCHK(hipMemcpyAsync(up[u][0], cts + b0 * nsel * 1024, nbc * nsel * 1024, hipMemcpyHostToDevice, c->copy));
    HIPCHK(hipMemcpyAsync(up[u][1], rproof + b0 * nsel * 128, nbc * nsel * 128, hipMemcpyHostToDevice, c->copy));
    HIPCHK(hipMemcpyAsync(up[u][2], cproof + b0 * nc * 64, nbc * nc * 64, hipMemcpyHostToDevice, c->copy));
    HIPCHK(hipEventRecord(c->up_ev[u], c->copy));
    HIPCHK(hipStreamWaitEvent(c->stream, c->up_ev[u], 0));
    if ((rc = verify_chunk_manifest_locked(c, M, nbc, up[u][0], up[u][1], up[u][2], d_cast ? d_cast + b0 : nullptr,
                                           d_oks + b0 * nsel, d_okc + b0 * nc, tally, b0 == 0)))
      return rc;
    HIPCHK(hipEventRecord(c->done_ev[u], c->stream));
  }
  HIPCHK(hipMemcpyAsync(ok_sel, d_oks, nb * nsel, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(ok_con, d_okc, nb * nc, hipMemcpyDeviceToHost, c->stream));
  if (tally_be) {
    uint8_t* d_t = nullptr;
    if ((rc = ws_get(c, W_H5, nreal * 2 * 512, (void**)&d_t))) return rc;
    if ((rc = launch_export(c, tally, nreal * 2, d_t))) return rc;
    HIPCHK(hipMemcpyAsync(tally_be, d_t, nreal * 2 * 512, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  return EG_OK;
}

// ---------------------------------------------------------------------------------
// encryption
// ---------------------------------------------------------------------------------
// One chunk; arguments, output sets and the vote-independent job tables as encrypt_chunk_locked
// (the selection and contest-commitment jobs do not depend on the contests' sizes: only the
// nonce sums and the aggregates do).
static int encrypt_chunk_manifest_locked(eg_ctx* c, const ManShape& M, size_t nb, const uint8_t* d_votes,
                                         const uint8_t* sel_nonces, const uint8_t* contest_nonces, bool dev_nonces,
                                         int set, const uint8_t** d_cts, const uint8_t** d_rproof,
                                         const uint8_t** d_cproof) {
  int rc;
  FbTab G{}, K{};
  if ((rc = enc_tables_locked(c, &G, &K))) return rc;
  const bool ct = c->ct_encrypt != 0;
  const size_t nc = M.nc, nsel = M.nsel, ns = nb * nsel, ncn = nb * nc, ncls = M.cls.size();
  // scalars: [sel nonces ns*4 (R,u,cf,vf)][contest nonces ncn][derived ns*3 (m,sf,sg)][rsum ncn]
  const size_t off_cn = ns * 4, off_der = off_cn + ncn, off_rs = off_der + ns * 3, nscal = off_rs + ncn;
  uint8_t *SC = nullptr, *CH = nullptr, *CHC = nullptr, *d_rp = nullptr, *d_cp = nullptr;
  uint8_t* UBE = nullptr;
  uint32_t* U = nullptr;
  if ((rc = ws_get(c, W_SCAL, nscal * 32, (void**)&SC))) return rc;
  // unified element space: [ciphertexts ns*2][selection commitments ns*4][A,B ncn*2][contest a,b ncn*2]
  const size_t oCT = 0, oCM = ns * 2, oCP = oCM + ns * 4, oCC = oCP + ncn * 2, nU = oCC + ncn * 2;
  if ((rc = ws_get(c, W_E0, nU * kW * 4, (void**)&U))) return rc;
  std::vector<std::string> names{"first", "spc", "1", "2", "3", "4"};
  for (size_t ci = 0; ci < ncls; ++ci)
    for (const char* n : {"in", "out"}) names.push_back(n + std::to_string(ci));
  std::vector<const uint32_t*> jv;
  rc = cached_job_set(c, "me/" + std::to_string(nb) + "/" + M.key, names, [&]() {
    std::vector<std::vector<uint32_t>> out{M.first, M.spc};
    auto J1 = new_jobs(ns), J2 = new_jobs(ns), J3 = new_jobs(ns), J4 = new_jobs(ncn);
    for (size_t i = 0; i < ns; ++i) {  // as encrypt_chunk_locked
      const uint32_t R = (uint32_t)(i * 4), u = R + 1;
      const uint32_t dm = (uint32_t)(off_der + i * 3), sf = dm + 1, sg = dm + 2;
      const uint32_t cm = (uint32_t)(oCM + i * 4);
      uint32_t* a = &J1[i * kJobWords];  // alpha = g^R ; a_real = g^u                -> slot 0
      a[3] = (uint32_t)(oCT + i * 2); a[4] = cm; a[5] = R; a[7] = u;
      uint32_t* b = &J2[i * kJobWords];  // beta = K^R g^m ; b_real = K^u             -> slot 1
      b[3] = (uint32_t)(oCT + i * 2 + 1); b[4] = cm + 1; b[5] = R; b[6] = dm; b[7] = u;
      uint32_t* d = &J3[i * kJobWords];  // a_fake = g^sf ; b_fake = K^sf g^sg       -> slots 2, 3
      d[3] = cm + 2; d[4] = cm + 3; d[5] = sf; d[7] = sf; d[8] = sg;
    }
    for (size_t j = 0; j < ncn; ++j) {
      uint32_t* a = &J4[j * kJobWords];  // a = g^u_c ; b = K^u_c
      a[3] = (uint32_t)(oCC + j * 2); a[4] = (uint32_t)(oCC + j * 2 + 1);
      a[5] = (uint32_t)(off_cn + j); a[7] = (uint32_t)(off_cn + j);
    }
    for (auto* J : {&J1, &J2, &J3, &J4}) out.push_back(std::move(*J));
    for (size_t ci = 0; ci < ncls; ++ci) {
      out.push_back(class_in_table(M, ci));
      out.push_back(class_out_table(M, ci));
    }
    return out;
  }, jv);
  if (rc) return rc;
  const uint32_t *tFirst = jv[0], *tSpc = jv[1], *j1 = jv[2], *j2 = jv[3], *j3 = jv[4], *j4 = jv[5];
  std::vector<const uint32_t*> tin(ncls), tout(ncls);
  for (size_t ci = 0; ci < ncls; ++ci) {
    tin[ci] = jv[6 + ci * 2]; tout[ci] = jv[7 + ci * 2];
  }
  const hipMemcpyKind nk = dev_nonces ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  HIPCHK(hipMemcpyAsync(SC, sel_nonces, ns * 128, nk, c->stream));
  HIPCHK(hipMemcpyAsync(SC + off_cn * 32, contest_nonces, ncn * 32, nk, c->stream));
  hipLaunchKernelGGL(k_enc_prep, dim3(tgrid(ns)), dim3(256), 0, c->stream, c->d_q, d_votes, SC, (uint32_t)ns,
                     SC + off_der * 32, c->resp_plus);
  hipLaunchKernelGGL(k_enc_rsum_seg, dim3(tgrid(ncn)), dim3(256), 0, c->stream, c->d_q, SC, (uint32_t)ncn,
                     (uint32_t)nc, (uint32_t)nsel, tFirst, tSpc, SC + off_rs * 32);
  HIPCHK(hipGetLastError());
  {
    PowShape S{};
    S.nout = 2; S.nfb[0] = 1; S.nfb[1] = 1; S.exp_bytes = 32;
    PowTail T{};
    T.S.nout = 2; T.S.nfb[0] = 1; T.S.nfb[1] = 1; T.S.exp_bytes = 32; T.S.tab[1][0] = 1;
    T.jobs = j4; T.njobs = ncn;
    if ((rc = launch_pow(c, S, j1, ns, U, SC, U, G, K, nullptr, nullptr, &T, nullptr, ct))) return rc;
  }
  {
    PowShape S{};
    S.nout = 2; S.nfb[0] = 2; S.nfb[1] = 1; S.exp_bytes = 32; S.tab[0][0] = 1; S.tab[0][1] = 0; S.tab[1][0] = 1;
    S.fb_small[0][1] = 1;
    PowTail T{};
    T.S.nout = 2; T.S.nfb[0] = 1; T.S.nfb[1] = 2; T.S.exp_bytes = 32; T.S.tab[1][0] = 1; T.S.tab[1][1] = 0;
    T.jobs = j3; T.njobs = ns;
    if ((rc = launch_pow(c, S, j2, ns, U, SC, U, G, K, nullptr, nullptr, &T, nullptr, ct))) return rc;
  }
  hipLaunchKernelGGL(k_enc_order, dim3(tgrid(ns * (2 * kW / 4))), dim3(256), 0, c->stream, U + oCM * kW, d_votes,
                     (uint32_t)ns);
  HIPCHK(hipGetLastError());
  if ((rc = man_aggregates(c, M, nb, U + oCT * kW, tin, tout, U + oCP * kW))) return rc;
  uint8_t* const want_cts = const_cast<uint8_t*>(*d_cts);
  uint8_t* const want_rp = const_cast<uint8_t*>(*d_rproof);
  uint8_t* const want_cp = const_cast<uint8_t*>(*d_cproof);
  if ((rc = ws_get(c, set ? W_EB0 : W_BE0, nU * 512, (void**)&UBE))) return rc;
  if (want_cts) {  // the ciphertexts (elements [oCT, oCM)) straight into the caller's buffer
    if ((rc = launch_export(c, U, oCM, want_cts))) return rc;
    if ((rc = launch_export(c, U + oCM * kW, nU - oCM, UBE + oCM * 512))) return rc;
  } else {
    if ((rc = launch_export(c, U, nU, UBE))) return rc;
  }
  if ((rc = ws_get(c, W_OK0, ns * 32, (void**)&CH))) return rc;
  if ((rc = ws_get(c, W_OK1, ncn * 32, (void**)&CHC))) return rc;
  const uint8_t* CT_BE = want_cts ? want_cts : UBE + oCT * 512;
  const uint8_t* CM_BE = UBE + oCM * 512;
  const uint8_t* CP_BE = UBE + oCP * 512;
  const uint8_t* CC_BE = UBE + oCC * 512;
  if ((rc = launch_hash(c, (uint32_t)ns,
                        preimage(c, {HashSrc{CT_BE, 512, 1024}, HashSrc{CT_BE + 512, 512, 1024}},
                                 {HashSrc{CM_BE, 512, 2048}, HashSrc{CM_BE + 512, 512, 2048},
                                  HashSrc{CM_BE + 1024, 512, 2048}, HashSrc{CM_BE + 1536, 512, 2048}},
                                 key_src(c)),
                        nullptr, 0, 0, kNone, nullptr, nullptr, 0, nullptr, CH)))
    return rc;
  if ((rc = launch_hash(c, (uint32_t)ncn,
                        preimage(c, {HashSrc{CP_BE, 512, 1024}, HashSrc{CP_BE + 512, 512, 1024}},
                                 {HashSrc{CC_BE, 512, 1024}, HashSrc{CC_BE + 512, 512, 1024}}, key_src(c)),
                        nullptr, 0, 0, kNone, nullptr, nullptr, 0, nullptr, CHC)))
    return rc;
  if (want_rp) d_rp = want_rp;
  else if ((rc = ws_get(c, set ? W_EB1 : W_FLAGS, ns * 128, (void**)&d_rp))) return rc;
  if (want_cp) d_cp = want_cp;
  else if ((rc = ws_get(c, set ? W_EB2 : W_EA2, ncn * 64 + 64, (void**)&d_cp))) return rc;
  hipLaunchKernelGGL(k_enc_finish, dim3(tgrid(ns)), dim3(256), 0, c->stream, c->d_q, d_votes, SC, CH, (uint32_t)ns,
                     d_rp, c->resp_plus);
  hipLaunchKernelGGL(k_response, dim3(tgrid(ncn)), dim3(256), 0, c->stream, c->d_q, SC + off_cn * 32, CHC,
                     SC + off_rs * 32, 32u, (uint32_t)ncn, d_cp, c->resp_plus);
  HIPCHK(hipGetLastError());
  *d_cts = CT_BE;
  *d_rproof = d_rp;
  *d_cproof = d_cp;
  return EG_OK;
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
  HIPCHK(hipMemcpyAsync(c->d_qbar, qbar_be, 32, hipMemcpyHostToDevice, c->stream));
  if ((rc = ensure_copy_stream(c))) return rc;
  // the software pipeline of eg_encrypt_ballots: chunk k computes while chunk k-1's outputs go back
  const size_t nsel = M.nsel, chunk = host_chunk(nb, nsel);
  uint8_t* d_votes = nullptr;
  if ((rc = upload(c, W_H0, votes, nb * nsel, (void**)&d_votes))) return rc;
  struct Out { size_t b0, n; const uint8_t *cts, *rp, *cp; } prev{};
  auto copy_back = [&](const Out& o, int set) -> int {
    HIPCHK(hipStreamWaitEvent(c->copy, c->done_ev[set], 0));
    HIPCHK(hipMemcpyAsync(cts + o.b0 * nsel * 1024, o.cts, o.n * nsel * 1024, hipMemcpyDeviceToHost, c->copy));
    HIPCHK(hipMemcpyAsync(rproof + o.b0 * nsel * 128, o.rp, o.n * nsel * 128, hipMemcpyDeviceToHost, c->copy));
    HIPCHK(hipMemcpyAsync(cproof + o.b0 * nc * 64, o.cp, o.n * nc * 64, hipMemcpyDeviceToHost, c->copy));
    HIPCHK(hipEventRecord(c->up_ev[set], c->copy));
    return EG_OK;
  };
  size_t k = 0;
  for (size_t b0 = 0; b0 < nb; b0 += chunk, ++k) {
    const size_t n = std::min(chunk, nb - b0);
    const int set = (int)(k & 1);
    if (k >= 2) HIPCHK(hipStreamWaitEvent(c->stream, c->up_ev[set], 0));  // chunk k-2's outputs are home
    Out cur{b0, n, nullptr, nullptr, nullptr};
    if ((rc = encrypt_chunk_manifest_locked(c, M, n, d_votes + b0 * nsel, sel_nonces + b0 * nsel * 128,
                                            contest_nonces + b0 * nc * 32, false, set, &cur.cts, &cur.rp, &cur.cp)))
      break;
    HIPCHK(hipEventRecord(c->done_ev[set], c->stream));
    if (k >= 1 && (rc = copy_back(prev, 1 - set))) break;
    prev = cur;
  }
  if (!rc) rc = copy_back(prev, (int)((k - 1) & 1));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipStreamSynchronize(c->copy));
  return rc;
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
  const size_t nsel = M.nsel, chunk = ballot_chunk(nsel);
  HIPCHK(hipMemcpyAsync(c->d_qbar, qbar_be, 32, hipMemcpyHostToDevice, c->stream));
  size_t k = 0;
  for (size_t b0 = 0; b0 < nb; b0 += chunk, ++k) {
    const size_t n = std::min(chunk, nb - b0);
    // the kernels write the caller's device buffers directly
    const uint8_t *o_cts = d_cts + b0 * nsel * 1024, *o_rp = d_rproof + b0 * nsel * 128,
                  *o_cp = d_cproof + b0 * nc * 64;
    if ((rc = encrypt_chunk_manifest_locked(c, M, n, d_votes + b0 * nsel, d_sel_nonces + b0 * nsel * 128,
                                            d_contest_nonces + b0 * nc * 32, true, (int)(k & 1), &o_cts, &o_rp,
                                            &o_cp)))
      return rc;
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  return EG_OK;
}
