// eg_capi_ballot2.inc — ballots without placeholder selections (include/eg_hip_ballot2.h;
// DESIGN.md §15; included by eg_capi.hip after eg_capi_range.inc, whose chunk functions it calls).
// Kernels: eg_ballot2.hpp.  eg_encrypt_ballots_v2 / eg_verify_ballots_v2 and their _dev twins are
// one body each taking `bool host`, around one staged run (eg_stage.hpp) of the chunk function.
//
// A ballot's proofs are range proofs of mixed limits in ragged rows; range_prove_chunk_locked and
// range_verify_chunk_locked take ONE limit and contiguous items.  A chunk therefore runs LIMIT
// CLASS by limit class: class L holds every selection of a contest with olimit == L and every
// contest with climit == L.  Its items are gathered into contiguous arrays (selections first,
// ballot-major, then contests), one unchanged range chunk call proves or verifies them, and the
// proofs or verdicts are scattered back.  The contest items' ciphertexts are the aggregates
// (k_prod_tab, one launch per class of equal nsel, on the chunk's imported ciphertexts), their
// nonce the contest's sum of R and their value the sum of votes (k_b2_sums).  No step reads a
// ballot byte on the host, so the _dev variants only enqueue once a shape's tables are up (first-use
// uploads and a job-cache rebuild synchronise, as everywhere).

static constexpr size_t kB2MaxSelections = (size_t)1 << 20;

// The validated shape of one call and the device table built from it: every per-manifest index
// array packed into ONE cached table (the job cache drops all its tables once it holds 64, so a
// manifest of fifteen limit classes must not own dozens of them), addressed through offsets.
struct B2Shape {
  size_t nc = 0, NS = 0, SP = 0, SN = 0, CP = 0, CN = 0, J = 0;
  std::vector<uint32_t> nsel, olimit, climit, first, sp_off, sn_off, cp_off, cn_off;
  struct Limit {  // one limit class
    uint32_t L;
    std::vector<uint32_t> sel, con;              // its selections s and contests k, ascending
    size_t t_sel, t_sp, t_sn, t_con, t_cp, t_cn;  // table offsets: s, proof row, nonce row; k, proof row, nonce row
    size_t per() const { return sel.size() + con.size(); }
  };
  std::vector<Limit> lim;  // ascending L
  struct Size {            // the contests of one selection count (one aggregate launch)
    uint32_t nsel;
    std::vector<uint32_t> con;
    size_t t_in, t_out;
  };
  std::vector<Size> size;
  size_t t_first = 0, t_nsel = 0, t_snoff = 0, t_olimit = 0, t_climit = 0, t_snrow = 0;
  std::vector<uint32_t> table;
  std::string key;
  size_t chunk() const { return std::max<size_t>(1, kRangeChunkJobs / J); }
};

static int b2_fail(const std::string& msg) { return fail(EG_ERR_ARG, "ballot2: " + msg); }

// The argument checks of eg_hip_ballot2.h on the three host arrays; fills the sums and offsets.
// The scan stops at the first contest past a bound, so a huge ncontest costs a bounded walk.
static int b2_check(size_t nc, const uint32_t* nsel, const uint32_t* olimit, const uint32_t* climit, B2Shape& M) {
  if (!nc) return b2_fail("no contests");
  for (size_t k = 0; k < nc; ++k) {
    const std::string who = "contest " + std::to_string(k);
    if (!nsel[k]) return b2_fail(who + " has no selections");
    if (olimit[k] < 1 || olimit[k] > EG_RANGE_MAX_LIMIT) return b2_fail(who + ": option limit outside [1, 15]");
    if (climit[k] < 1 || climit[k] > EG_RANGE_MAX_LIMIT) return b2_fail(who + ": contest limit outside [1, 15]");
    M.NS += nsel[k];
    // the header's bound; J >= 2 NS below meets its own bound first, so this one states a limit of
    // the 32-bit tables and cannot be the refusal a caller sees
    if (M.NS > kB2MaxSelections) return b2_fail("more than 2^20 selections per ballot");
    M.J += 2 * (size_t)olimit[k] * nsel[k] + 2 * (size_t)climit[k];
    if (M.J > kRangeChunkJobs) return b2_fail("one ballot holds more than 2^16 verifier jobs");
  }
  M.nc = nc;
  return EG_OK;
}

static void b2_build(size_t nc, const uint32_t* nsel, const uint32_t* olimit, const uint32_t* climit, B2Shape& M) {
  M.nsel.assign(nsel, nsel + nc);
  M.olimit.assign(olimit, olimit + nc);
  M.climit.assign(climit, climit + nc);
  std::map<uint32_t, B2Shape::Limit> lim;
  std::map<uint32_t, B2Shape::Size> size;
  std::vector<uint32_t> sp_row, sn_row;  // per selection
  uint32_t ns = 0;
  for (size_t k = 0; k < nc; ++k) {
    M.first.push_back(ns);
    M.sp_off.push_back((uint32_t)M.SP);
    M.sn_off.push_back((uint32_t)M.SN);
    M.cp_off.push_back((uint32_t)M.CP);
    M.cn_off.push_back((uint32_t)M.CN);
    for (uint32_t i = 0; i < nsel[k]; ++i) {
      lim[olimit[k]].sel.push_back(ns + i);
      sp_row.push_back((uint32_t)M.SP + i * (olimit[k] + 1));
      sn_row.push_back((uint32_t)M.SN + i * (2 * olimit[k] + 4));
    }
    lim[climit[k]].con.push_back((uint32_t)k);
    size[nsel[k]].con.push_back((uint32_t)k);
    ns += nsel[k];
    M.SP += (size_t)nsel[k] * (olimit[k] + 1);
    M.SN += (size_t)nsel[k] * (2 * olimit[k] + 4);
    M.CP += climit[k] + 1;
    M.CN += 2 * climit[k] + 3;
    M.key += std::to_string(nsel[k]) + "." + std::to_string(olimit[k]) + "." + std::to_string(climit[k]) + ",";
  }
  std::vector<uint32_t>& T = M.table;
  auto put = [&T](const std::vector<uint32_t>& v) {
    const size_t at = T.size();
    T.insert(T.end(), v.begin(), v.end());
    return at;
  };
  M.t_first = put(M.first);
  M.t_nsel = put(M.nsel);
  M.t_snoff = put(M.sn_off);
  M.t_olimit = put(M.olimit);
  M.t_climit = put(M.climit);
  M.t_snrow = put(sn_row);
  for (auto& kv : lim) {
    B2Shape::Limit& C = kv.second;
    C.L = kv.first;
    std::vector<uint32_t> sp, sn, cp, cn;
    for (uint32_t s : C.sel) { sp.push_back(sp_row[s]); sn.push_back(sn_row[s]); }
    for (uint32_t k : C.con) { cp.push_back(M.cp_off[k]); cn.push_back(M.cn_off[k]); }
    C.t_sel = put(C.sel); C.t_sp = put(sp); C.t_sn = put(sn);
    C.t_con = put(C.con); C.t_cp = put(cp); C.t_cn = put(cn);
    M.lim.push_back(std::move(C));
  }
  for (auto& kv : size) {
    B2Shape::Size& Z = kv.second;
    Z.nsel = kv.first;
    std::vector<uint32_t> in, out;  // entry mi * 2 + comp of member contest k (add_class_tables' layout)
    for (uint32_t k : Z.con)
      for (uint32_t comp = 0; comp < 2; ++comp) {
        in.push_back(M.first[k] * 2 + comp);
        out.push_back(k * 2 + comp);
      }
    Z.t_in = put(in);
    Z.t_out = put(out);
    M.size.push_back(std::move(Z));
  }
}

// The chunk's packed class arrays: class ci's items start at item base[ci] (x 1024 B of
// ciphertexts, x 1 B of values / verdicts, x 32 B of R), its proof rows at pbase[ci] pairs of 64 B
// and its nonce rows at nbase[ci] rows of 32 B.
struct B2Layout {
  std::vector<size_t> base, pbase, nbase;
  size_t items = 0, pairs = 0, rows = 0;
  B2Layout(const B2Shape& M, size_t nbc) {
    for (const auto& C : M.lim) {
      base.push_back(items); pbase.push_back(pairs); nbase.push_back(rows);
      const size_t n = nbc * C.per();
      items += n; pairs += n * (C.L + 1); rows += n * (2 * (size_t)C.L + 3);
    }
  }
};

static void b2_rows(eg_ctx* c, const void* ragged, void* packed, const uint32_t* tab, size_t per, size_t quads,
                    size_t nitems, size_t ballot_quads, uint32_t mul, uint32_t shift, bool scatter) {
  if (!nitems) return;
  hipLaunchKernelGGL(k_b2_rows, dim3(cgrid(nitems * quads)), dim3(kBlock), 0, c->stream, (uint4*)ragged, (uint4*)packed,
                     tab, (uint32_t)per, (uint32_t)quads, (uint64_t)nitems, (uint64_t)ballot_quads, mul, shift,
                     scatter ? 1u : 0u);
}
static void b2_bytes(eg_ctx* c, const void* ragged, void* packed, const uint32_t* tab, size_t per, size_t nitems,
                     size_t ballot_bytes, bool scatter) {
  if (!nitems) return;
  hipLaunchKernelGGL(k_b2_bytes, dim3(cgrid(nitems)), dim3(kBlock), 0, c->stream, (uint8_t*)ragged, (uint8_t*)packed, tab,
                     (uint32_t)per, (uint64_t)nitems, (uint64_t)ballot_bytes, scatter ? 1u : 0u);
}

// aggregates (A, B) = (prod alpha, prod beta) of nbc ballots' contests from the imported
// ciphertexts E into agg[(b nc + k) 2 + comp], one k_prod_tab launch per selection count, then
// their canonical bytes (the contest items' ciphertexts)
static int b2_aggregates(eg_ctx* c, const B2Shape& M, const uint32_t* T, size_t nbc, const uint32_t* E, uint32_t* agg,
                         uint8_t* agg_be) {
  int rc;
  for (const auto& Z : M.size) {
    const size_t period = Z.con.size() * 2;
    if ((rc = run_prod_tab(c, E, T + Z.t_in, period, 2 * M.NS, nbc * period, Z.nsel, 2, agg, T + Z.t_out, 2 * M.nc)))
      return rc;
  }
  return launch_export(c, agg, nbc * M.nc * 2, agg_be);
}

// ---------------------------------------------------------------------------------
// verify + tally
// ---------------------------------------------------------------------------------
// One chunk of nbc <= M.chunk() ballots, device pointers, enqueued on the ctx stream (d_qbar and
// the key are set by the caller, who holds the lock).  tally (optional): the running tally and
// one chunk's product, NS * 2 elements each.
static int b2_verify_chunk_locked(eg_ctx* c, const B2Shape& M, size_t nbc, const uint8_t* cts, const uint8_t* sproof,
                                  const uint8_t* cproof, const uint8_t* cast, uint8_t* ok_sel, uint8_t* ok_con,
                                  uint32_t* tally, bool first) {
  int rc;
  const size_t ns = nbc * M.NS, ncn = nbc * M.nc;
  const B2Layout V(M, nbc);
  uint32_t *E = nullptr, *AGG = nullptr;
  uint8_t *LT = nullptr, *AGG_BE = nullptr, *CTS = nullptr, *PRF = nullptr, *OK = nullptr, *FL = nullptr, *OKC = nullptr;
  if ((rc = ws_get(c, W_B2_E, ns * 2 * kW * 4, (void**)&E))) return rc;
  if ((rc = ws_get(c, W_B2_LT, ns * 2, (void**)&LT))) return rc;
  if ((rc = ws_get(c, W_B2_AGG, ncn * 2 * kW * 4, (void**)&AGG))) return rc;
  if ((rc = ws_get(c, W_B2_AGGBE, ncn * 1024, (void**)&AGG_BE))) return rc;
  if ((rc = ws_get(c, W_B2_CTS, V.items * 1024, (void**)&CTS))) return rc;
  if ((rc = ws_get(c, W_B2_PRF, V.pairs * 64, (void**)&PRF))) return rc;
  if ((rc = ws_get(c, W_B2_OK, V.items, (void**)&OK))) return rc;
  if ((rc = ws_get(c, W_B2_FL, ns, (void**)&FL))) return rc;
  if ((rc = ws_get(c, W_B2_OKC, ncn, (void**)&OKC))) return rc;
  const uint32_t* T = nullptr;
  if ((rc = cached_jobs(c, "b2/" + M.key, M.table, &T))) return rc;
  // 1. the chunk's ciphertexts, imported once for the aggregates and the tally
  if ((rc = launch_import(c, cts, ns * 2, E, LT))) return rc;
  if ((rc = b2_aggregates(c, M, T, nbc, E, AGG, AGG_BE))) return rc;
  // 2. every class's items, gathered
  for (size_t ci = 0; ci < M.lim.size(); ++ci) {
    const auto& C = M.lim[ci];
    const size_t nS = nbc * C.sel.size(), nC = nbc * C.con.size(), pq = ((size_t)C.L + 1) * 4;
    uint8_t* cc = CTS + V.base[ci] * 1024;
    uint8_t* pp = PRF + V.pbase[ci] * 64;
    b2_rows(c, cts, cc, T + C.t_sel, C.sel.size(), 64, nS, M.NS * 64, 64, 0, false);
    b2_rows(c, AGG_BE, cc + nS * 1024, T + C.t_con, C.con.size(), 64, nC, M.nc * 64, 64, 0, false);
    b2_rows(c, sproof, pp, T + C.t_sp, C.sel.size(), pq, nS, M.SP * 4, 4, 0, false);
    b2_rows(c, cproof, pp + nS * pq * 16, T + C.t_cp, C.con.size(), pq, nC, M.CP * 4, 4, 0, false);
  }
  HIPCHK(hipGetLastError());
  // 3. one range chunk call per class.  It may rebuild the job cache, so T is fetched again
  // before its next use; it leaves its items' range + residue flags in W_FLAGS, which the
  // selections' part is read from before the next call overwrites them.
  for (size_t ci = 0; ci < M.lim.size(); ++ci) {
    const auto& C = M.lim[ci];
    const size_t n = nbc * C.per(), nS = nbc * C.sel.size();
    if ((rc = range_verify_chunk_locked(c, n, C.L, CTS + V.base[ci] * 1024, PRF + V.pbase[ci] * 64, OK + V.base[ci])))
      return rc;
    if (!nS) continue;
    if ((rc = cached_jobs(c, "b2/" + M.key, M.table, &T))) return rc;
    hipLaunchKernelGGL(k_b2_flags, dim3(cgrid(nS)), dim3(kBlock), 0, c->stream, (const uint8_t*)c->ws[W_FLAGS].ptr,
                       T + C.t_sel, (uint32_t)C.sel.size(), (uint64_t)nS, (uint32_t)M.NS, FL);
    HIPCHK(hipGetLastError());
  }
  // 4. verdicts back to ballot order; the contests' fold with their selections' flags
  if ((rc = cached_jobs(c, "b2/" + M.key, M.table, &T))) return rc;
  for (size_t ci = 0; ci < M.lim.size(); ++ci) {
    const auto& C = M.lim[ci];
    const size_t nS = nbc * C.sel.size(), nC = nbc * C.con.size();
    b2_bytes(c, ok_sel, OK + V.base[ci], T + C.t_sel, C.sel.size(), nS, M.NS, true);
    b2_bytes(c, OKC, OK + V.base[ci] + nS, T + C.t_con, C.con.size(), nC, M.nc, true);
  }
  hipLaunchKernelGGL(k_b2_verdict, dim3(cgrid(ncn)), dim3(kBlock), 0, c->stream, OKC, FL, T + M.t_first, T + M.t_nsel,
                     (uint32_t)M.nc, (uint32_t)M.NS, (uint64_t)ncn, ok_con);
  HIPCHK(hipGetLastError());
  // 5. the tally over this chunk's cast ballots, every selection
  if (tally) {
    const size_t nt = M.NS * 2;
    uint32_t* TP = first ? tally : tally + nt * kW;
    if ((rc = run_prod(c, E, GroupMap{(uint32_t)nt, 1, 1, 0, 0}, nt, nbc, nt, TP, cast))) return rc;
    if (!first) {
      LAUNCH_F(c, k_mul, dim3(grid_for(nt)), c->d, tally, 1u, TP, 1u, (uint32_t)nt, tally, 1u);
      HIPCHK(hipGetLastError());
    }
  }
  return EG_OK;
}

static int b2_args(eg_ctx* c, const uint8_t* K_be, const uint8_t* qbar_be, size_t nb, size_t nc, const uint32_t* nsel,
                   const uint32_t* olimit, const uint32_t* climit, bool data_ok, B2Shape& M) {
  if (!c || !K_be || !qbar_be || !nsel || !olimit || !climit || (nb && !data_ok)) return b2_fail("null argument");
  return b2_check(nc, nsel, olimit, climit, M);
}

static int b2_verify(eg_ctx* c, bool host, const uint8_t* K_be, const uint8_t* qbar_be, size_t nb, size_t nc,
                     const uint32_t* nsel, const uint32_t* olimit, const uint32_t* climit, const uint8_t* cts,
                     const uint8_t* sproof, const uint8_t* cproof, const uint8_t* cast, uint8_t* ok_sel,
                     uint8_t* ok_con, uint8_t* tally_be) {
  int rc;
  B2Shape M;
  if ((rc = b2_args(c, K_be, qbar_be, nb, nc, nsel, olimit, climit, cts && sproof && cproof && ok_sel && ok_con, M)))
    return rc;
  if (!host && !aligned16({cts, sproof, cproof, tally_be})) return b2_fail("device pointer not 16-byte aligned");
  const size_t nt = M.NS * 2;
  Locked lk(c);
  if (!nb) {
    if (!tally_be) return EG_OK;
    std::vector<uint8_t> one(nt * 512);
    ones_be(one.data(), nt);
    if (host) {
      std::memcpy(tally_be, one.data(), one.size());
      return EG_OK;
    }
    HIPCHK(hipMemcpyAsync(tally_be, one.data(), one.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));  // `one` leaves with this frame
    return EG_OK;
  }
  b2_build(nc, nsel, olimit, climit, M);
  if ((rc = use_key_locked(c, K_be))) return rc;
  HIPCHK(hipMemcpyAsync(c->d_qbar, qbar_be, 32, hipMemcpyHostToDevice, c->stream));
  uint32_t* tally = nullptr;
  if (tally_be && (rc = ws_get(c, W_B2_TALLY, nt * 2 * kW * 4, (void**)&tally))) return rc;
  Stage st(c, host, nb, M.chunk());
  st.in(cts, M.NS * 1024);
  st.in(sproof, M.SP * 64);
  st.in(cproof, M.CP * 64);
  if (cast) st.in(cast, 1);
  st.out(ok_sel, M.NS);
  st.out(ok_con, M.nc);
  bool first = true;
  rc = st.run([&](size_t m) {
    const int r = b2_verify_chunk_locked(c, M, m, cts, sproof, cproof, cast, ok_sel, ok_con, tally, first);
    first = false;
    return r;
  });
  if (rc || !tally_be) return rc;
  if (!host) return launch_export(c, tally, nt, tally_be);
  uint8_t* d_t = nullptr;
  if ((rc = ws_get(c, W_B2_TBE, nt * 512, (void**)&d_t))) return rc;
  if ((rc = launch_export(c, tally, nt, d_t))) return rc;
  HIPCHK(hipMemcpyAsync(tally_be, d_t, nt * 512, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return EG_OK;
}

extern "C" int eg_verify_ballots_v2_dev(eg_ctx* c, const uint8_t K_be[512], const uint8_t qbar_be[32], size_t nb,
                                        size_t nc, const uint32_t* nsel, const uint32_t* olimit, const uint32_t* climit,
                                        const uint8_t* d_cts, const uint8_t* d_sproof, const uint8_t* d_cproof,
                                        const uint8_t* d_cast, uint8_t* d_ok_sel, uint8_t* d_ok_con, uint8_t* d_tally_be) {
  return b2_verify(c, false, K_be, qbar_be, nb, nc, nsel, olimit, climit, d_cts, d_sproof, d_cproof, d_cast, d_ok_sel,
                   d_ok_con, d_tally_be);
}

extern "C" int eg_verify_ballots_v2(eg_ctx* c, const uint8_t K_be[512], const uint8_t qbar_be[32], size_t nb, size_t nc,
                                    const uint32_t* nsel, const uint32_t* olimit, const uint32_t* climit,
                                    const uint8_t* cts, const uint8_t* sproof, const uint8_t* cproof, const uint8_t* cast,
                                    uint8_t* ok_sel, uint8_t* ok_con, uint8_t* tally_be) {
  return b2_verify(c, true, K_be, qbar_be, nb, nc, nsel, olimit, climit, cts, sproof, cproof, cast, ok_sel, ok_con,
                   tally_be);
}

// ---------------------------------------------------------------------------------
// encrypt
// ---------------------------------------------------------------------------------
// One chunk of nbc <= M.chunk() ballots, device pointers.  Fixed-base only: the ciphertext jobs
// (alpha, beta) = (g^R, K^R g^m), one per selection and of the range prover's simulated-pair shape,
// then per class one unchanged range prover call.  No job table depends on a vote.
static int b2_encrypt_chunk_locked(eg_ctx* c, const B2Shape& M, size_t nbc, const uint8_t* votes, const uint8_t* sn,
                                   const uint8_t* cn, uint8_t* cts, uint8_t* sproof, uint8_t* cproof) {
  int rc;
  FbTab G{}, K{};
  if ((rc = enc_tables_locked(c, &G, &K))) return rc;
  const size_t ns = nbc * M.NS, ncn = nbc * M.nc;
  const B2Layout V(M, nbc);
  uint32_t *E = nullptr, *AGG = nullptr;
  uint8_t *SC = nullptr, *AGG_BE = nullptr, *CTS = nullptr, *PRF = nullptr, *VAL = nullptr, *RS = nullptr, *NON = nullptr,
          *RSUM = nullptr, *SUMV = nullptr;
  if ((rc = ws_get(c, W_B2_E, ns * 2 * kW * 4, (void**)&E))) return rc;
  if ((rc = ws_get(c, W_B2_SC, ns * 64, (void**)&SC))) return rc;
  if ((rc = ws_get(c, W_B2_AGG, ncn * 2 * kW * 4, (void**)&AGG))) return rc;
  if ((rc = ws_get(c, W_B2_AGGBE, ncn * 1024, (void**)&AGG_BE))) return rc;
  if ((rc = ws_get(c, W_B2_CTS, V.items * 1024, (void**)&CTS))) return rc;
  if ((rc = ws_get(c, W_B2_PRF, V.pairs * 64, (void**)&PRF))) return rc;
  if ((rc = ws_get(c, W_B2_OK, V.items, (void**)&VAL))) return rc;
  if ((rc = ws_get(c, W_B2_R, V.items * 32, (void**)&RS))) return rc;
  if ((rc = ws_get(c, W_B2_NON, V.rows * 32, (void**)&NON))) return rc;
  if ((rc = ws_get(c, W_B2_RSUM, ncn * 32, (void**)&RSUM))) return rc;
  if ((rc = ws_get(c, W_B2_OKC, ncn, (void**)&SUMV))) return rc;
  // the manifest's table and the ciphertext jobs, one cached set (a second set's cache_bound
  // could free the first)
  const std::string key = "b2e/" + std::to_string(nbc) + "/" + M.key;
  std::vector<const uint32_t*> tv;
  auto tables = [&]() {
    return cached_job_set(c, key, {"T", "CT"}, [&]() {
      auto J = new_jobs(ns);
      for (size_t i = 0; i < ns; ++i) {  // alpha = g^R ; beta = K^R g^m
        PowJob& x = J[i];
        x.out[0] = (uint32_t)(i * 2); x.out[1] = x.out[0] + 1;
        x.fb[0][0] = x.out[0]; x.fb[1][0] = x.out[0]; x.fb[1][1] = x.out[0] + 1;
      }
      return JobSet{M.table, std::move(J)};
    }, tv);
  };
  if ((rc = tables())) return rc;
  const uint32_t* T = tv[0];
  // 1. scalars: the ciphertext jobs' (R, m); per contest sum R, sum m and the over-limit mask
  hipLaunchKernelGGL(k_b2_ctscal, dim3(cgrid(ns)), dim3(kBlock), 0, c->stream, votes, sn, T + M.t_snrow, (uint32_t)M.NS,
                     (uint64_t)M.SN, (uint64_t)ns, SC);
  hipLaunchKernelGGL(k_b2_sums, dim3(cgrid(ncn)), dim3(kBlock), 0, c->stream, c->d_q, votes, sn, T + M.t_first,
                     T + M.t_nsel, T + M.t_snoff, T + M.t_olimit, T + M.t_climit, (uint32_t)M.nc, (uint32_t)M.NS,
                     (uint64_t)M.SN, (uint64_t)ncn, RSUM, SUMV);
  HIPCHK(hipGetLastError());
  // 2. ciphertexts, their bytes straight into the caller's rows, and the aggregates
  if ((rc = launch_pow(c, {pow_fb_pair(true), tv[1], ns}, E, SC, E, G, K, pow_ct(c->ct_encrypt != 0)))) return rc;
  if ((rc = launch_export(c, E, ns * 2, cts))) return rc;
  if ((rc = b2_aggregates(c, M, T, nbc, E, AGG, AGG_BE))) return rc;
  // 3. every class's items, gathered
  for (size_t ci = 0; ci < M.lim.size(); ++ci) {
    const auto& C = M.lim[ci];
    const size_t nS = nbc * C.sel.size(), nC = nbc * C.con.size(), nq = (2 * (size_t)C.L + 3) * 2;
    const size_t pS = C.sel.size(), pC = C.con.size();
    uint8_t* cc = CTS + V.base[ci] * 1024;
    uint8_t* vv = VAL + V.base[ci];
    uint8_t* rr = RS + V.base[ci] * 32;
    uint8_t* nn = NON + V.nbase[ci] * 32;
    b2_rows(c, cts, cc, T + C.t_sel, pS, 64, nS, M.NS * 64, 64, 0, false);
    b2_rows(c, AGG_BE, cc + nS * 1024, T + C.t_con, pC, 64, nC, M.nc * 64, 64, 0, false);
    b2_bytes(c, votes, vv, T + C.t_sel, pS, nS, M.NS, false);
    b2_bytes(c, SUMV, vv + nS, T + C.t_con, pC, nC, M.nc, false);
    b2_rows(c, sn, rr, T + C.t_sn, pS, 2, nS, M.SN * 2, 2, 0, false);
    b2_rows(c, RSUM, rr + nS * 32, T + C.t_con, pC, 2, nC, M.nc * 2, 2, 0, false);
    b2_rows(c, sn, nn, T + C.t_sn, pS, nq, nS, M.SN * 2, 2, 2, false);  // past the selection's R row
    b2_rows(c, cn, nn + nS * nq * 16, T + C.t_cn, pC, nq, nC, M.CN * 2, 2, 0, false);
  }
  HIPCHK(hipGetLastError());
  // 4. one range prover call per class (it may rebuild the job cache: the table is fetched again)
  for (size_t ci = 0; ci < M.lim.size(); ++ci) {
    const auto& C = M.lim[ci];
    if ((rc = range_prove_chunk_locked(c, nbc * C.per(), C.L, CTS + V.base[ci] * 1024, VAL + V.base[ci],
                                       RS + V.base[ci] * 32, NON + V.nbase[ci] * 32, PRF + V.pbase[ci] * 64)))
      return rc;
  }
  if ((rc = tables())) return rc;
  T = tv[0];
  // 5. proofs back to the ballots' rows
  for (size_t ci = 0; ci < M.lim.size(); ++ci) {
    const auto& C = M.lim[ci];
    const size_t nS = nbc * C.sel.size(), nC = nbc * C.con.size(), pq = ((size_t)C.L + 1) * 4;
    uint8_t* pp = PRF + V.pbase[ci] * 64;
    b2_rows(c, sproof, pp, T + C.t_sp, C.sel.size(), pq, nS, M.SP * 4, 4, 0, true);
    b2_rows(c, cproof, pp + nS * pq * 16, T + C.t_cp, C.con.size(), pq, nC, M.CP * 4, 4, 0, true);
  }
  HIPCHK(hipGetLastError());
  return EG_OK;
}

// host votes are checked here and name the ballot and contest; device votes past a limit give
// all-zero proof rows
static int b2_check_votes(const B2Shape& M, const uint32_t* nsel, const uint32_t* olimit, const uint32_t* climit,
                          size_t nb, const uint8_t* votes) {
  for (size_t b = 0; b < nb; ++b) {
    const uint8_t* v = votes + b * M.NS;
    for (size_t k = 0; k < M.nc; v += nsel[k], ++k) {
      const std::string who = "ballot " + std::to_string(b) + " contest " + std::to_string(k);
      size_t sum = 0;
      for (uint32_t i = 0; i < nsel[k]; ++i) {
        if (v[i] > olimit[k])
          return b2_fail(who + " selection " + std::to_string(i) + " holds " + std::to_string((unsigned)v[i]) +
                         ", above its option limit " + std::to_string(olimit[k]));
        sum += v[i];
      }
      if (sum > climit[k])
        return b2_fail(who + " holds " + std::to_string(sum) + ", above its contest limit " +
                       std::to_string(climit[k]));
    }
  }
  return EG_OK;
}

static int b2_encrypt(eg_ctx* c, bool host, const uint8_t* K_be, const uint8_t* qbar_be, size_t nb, size_t nc,
                      const uint32_t* nsel, const uint32_t* olimit, const uint32_t* climit, const uint8_t* votes,
                      const uint8_t* sn, const uint8_t* cn, uint8_t* cts, uint8_t* sproof, uint8_t* cproof) {
  int rc;
  B2Shape M;
  if ((rc = b2_args(c, K_be, qbar_be, nb, nc, nsel, olimit, climit, votes && sn && cn && cts && sproof && cproof, M)))
    return rc;
  if (!host && !aligned16({sn, cn, cts, sproof, cproof})) return b2_fail("device pointer not 16-byte aligned");
  if (host && (rc = b2_check_votes(M, nsel, olimit, climit, nb, votes))) return rc;
  if (!nb) return EG_OK;
  b2_build(nc, nsel, olimit, climit, M);
  Locked lk(c);
  if ((rc = use_key_locked(c, K_be))) return rc;
  HIPCHK(hipMemcpyAsync(c->d_qbar, qbar_be, 32, hipMemcpyHostToDevice, c->stream));
  Stage st(c, host, nb, M.chunk());
  st.in(votes, M.NS);
  st.in(sn, M.SN * 32);
  st.in(cn, M.CN * 32);
  st.out(cts, M.NS * 1024);
  st.out(sproof, M.SP * 64);
  st.out(cproof, M.CP * 64);
  return st.run([&](size_t m) { return b2_encrypt_chunk_locked(c, M, m, votes, sn, cn, cts, sproof, cproof); });
}

extern "C" int eg_encrypt_ballots_v2_dev(eg_ctx* c, const uint8_t K_be[512], const uint8_t qbar_be[32], size_t nb,
                                         size_t nc, const uint32_t* nsel, const uint32_t* olimit, const uint32_t* climit,
                                         const uint8_t* d_votes, const uint8_t* d_sel_nonces,
                                         const uint8_t* d_contest_nonces, uint8_t* d_cts, uint8_t* d_sproof,
                                         uint8_t* d_cproof) {
  return b2_encrypt(c, false, K_be, qbar_be, nb, nc, nsel, olimit, climit, d_votes, d_sel_nonces, d_contest_nonces, d_cts,
                    d_sproof, d_cproof);
}

extern "C" int eg_encrypt_ballots_v2(eg_ctx* c, const uint8_t K_be[512], const uint8_t qbar_be[32], size_t nb, size_t nc,
                                     const uint32_t* nsel, const uint32_t* olimit, const uint32_t* climit,
                                     const uint8_t* votes, const uint8_t* sel_nonces, const uint8_t* contest_nonces,
                                     uint8_t* cts, uint8_t* sproof, uint8_t* cproof) {
  return b2_encrypt(c, true, K_be, qbar_be, nb, nc, nsel, olimit, climit, votes, sel_nonces, contest_nonces, cts, sproof,
                    cproof);
}
