// eg_capi_ballot.inc — ballot-level entry points of libeg_hip.so (included by
// eg_capi.hip): verification + tally, encryption, trustee decryption shares.
//
//   eg_verify_ballots[_dev]  Verifier(record, 11).verify() + runAccumulateBallots
//                            (RunRemoteWorkflowTest.java:151,179-182)
//   eg_encrypt_ballots       batchEncryption(..., CheckType.None) (RunRemoteWorkflowTest.java:140-141)
//   eg_trustee_decrypt_batch DecryptingTrustee.directDecrypt / compensatedDecrypt
//                            (RunRemoteDecryptingTrustee.java:189-193, 227-232)
//   eg_verify_shares         share-proof check inside Decryption.decrypt (RunRemoteDecryptor.java:261-262)
//
// Verification and encryption have one chunk path for every ballot shape: verify_chunk_locked,
// encrypt_chunk_locked and the four drivers around them (host / device pointers) take a ManShape.
// The selection part of a chunk works on ns = nbc * nsel jobs and does not know the contests.
// The contest layer (aggregates, contest scalars, contest flags, nonce sums, tally) and the
// k_pow launch plan are the only places that tell a uniform shape (the entry points here:
// arithmetic addressing, the benchmark's kernels and plan) from a table-addressed one (the
// entry points of eg_capi_manifest.inc: per-contest device tables).

// The words of one cached host table: job records, or the u32 index tables that ride in the same
// cached sets (built on a cache miss only).
struct JobTable {
  std::vector<uint32_t> w;
  JobTable(std::vector<uint32_t> v) : w(std::move(v)) {}
  JobTable(const std::vector<PowJob>& j) : w(j.size() * kJobWords) {
    if (!w.empty()) std::memcpy(w.data(), j.data(), w.size() * 4);  // an empty table has no storage to copy
  }
};
using JobSet = std::vector<JobTable>;

// One device copy of a host job table (freed again when the upload fails).  EG_TEST_FAIL_JOBS=k
// (read at context creation, tests only) makes the k-th upload of the context fail as an
// out-of-memory hipMalloc would.
static int upload_job_table(eg_ctx* c, const std::vector<uint32_t>& host, DevBuf* out) {
  DevBuf b;
  b.bytes = std::max<size_t>(4, host.size() * 4);
  if (c->test_fail_jobs > 0 && --c->test_fail_jobs == 0)
    return fail(EG_ERR_NOMEM, "hipMalloc job table failed (EG_TEST_FAIL_JOBS)");
  if (hipMalloc(&b.ptr, b.bytes) != hipSuccess)
    return fail(EG_ERR_NOMEM, "hipMalloc job table " + std::to_string(b.bytes) + " B failed");
  const hipError_t e = hipMemcpy(b.ptr, host.data(), host.size() * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    hipFree(b.ptr);
    return fail(EG_ERR_HIP, std::string("hipMemcpy job table: ") + hipGetErrorString(e));
  }
  *out = b;
  return EG_OK;
}

// drop the whole shape cache once it holds 64 tables (a long-running caller fed many batch sizes),
// after every launch that may still read one of them
static int cache_bound(eg_ctx* c) {
  if (c->cache.size() < 64) return EG_OK;
  HIPCHK(hipStreamSynchronize(c->stream));
  for (auto& kv : c->cache) HIPCHK(hipFree(kv.second.ptr));
  c->cache.clear();
  return EG_OK;
}

static int cached_jobs(eg_ctx* c, const std::string& key, const std::vector<uint32_t>& host, const uint32_t** out) {
  auto it = c->cache.find(key);
  if (it == c->cache.end()) {
    DevBuf b;
    const int rc = upload_job_table(c, host, &b);
    if (rc) return rc;
    it = c->cache.emplace(key, b).first;
  }
  *out = (const uint32_t*)it->second.ptr;
  return EG_OK;
}
// copies the table to words BEFORE the lookup: for callers that have already missed (identity_pow_jobs)
static int cached_jobs(eg_ctx* c, const std::string& key, const std::vector<PowJob>& host, const uint32_t** out) {
  return cached_jobs(c, key, JobTable(host).w, out);
}

// The job tables of one launch shape, cached as a set under key + "/" + name: a hit needs EVERY
// name present, and a miss builds the host tables (make) and uploads all of them before any is
// inserted, so an upload that fails (out of memory) leaves no partial set behind that a later
// call could take for a hit and hand a null table to k_pow (ADVICE r03).
static int cached_job_set(eg_ctx* c, const std::string& key, const std::vector<std::string>& names,
                          const std::function<JobSet()>& make,
                          std::vector<const uint32_t*>& out) {
  out.assign(names.size(), nullptr);
  bool hit = true;
  for (size_t i = 0; i < names.size() && hit; ++i) {
    auto it = c->cache.find(key + "/" + names[i]);
    hit = it != c->cache.end() && it->second.ptr;
    if (hit) out[i] = (const uint32_t*)it->second.ptr;
  }
  if (hit) return EG_OK;
  for (const auto& n : names) {  // a stale partial set (cannot arise any more; kept defensive)
    auto it = c->cache.find(key + "/" + n);
    if (it != c->cache.end()) {
      HIPCHK(hipStreamSynchronize(c->stream));
      if (it->second.ptr) hipFree(it->second.ptr);
      c->cache.erase(it);
    }
  }
  int rc = cache_bound(c);
  if (rc) return rc;
  const JobSet host = make();
  std::vector<DevBuf> bufs;
  for (const auto& h : host) {
    DevBuf b;
    if ((rc = upload_job_table(c, h.w, &b))) {
      for (auto& x : bufs) hipFree(x.ptr);
      return rc;
    }
    bufs.push_back(b);
  }
  for (size_t i = 0; i < names.size(); ++i) {
    c->cache.emplace(key + "/" + names[i], bufs[i]);
    out[i] = (const uint32_t*)bufs[i].ptr;
  }
  return EG_OK;
}

static int upload_jobs(eg_ctx* c, Slot s, const std::vector<PowJob>& host, const uint32_t** out) {
  void* d = nullptr;
  const size_t bytes = host.size() * sizeof(PowJob);
  int rc = ws_get(c, s, std::max<size_t>(4, bytes), &d);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(d, host.data(), bytes, hipMemcpyHostToDevice, c->stream));
  *out = (const uint32_t*)d;
  return EG_OK;
}

// a host job table, uploaded into workspace slot s and run as one population of shape S
static int launch_pow_jobs(eg_ctx* c, Slot s, const PowShape& S, const std::vector<PowJob>& J, const uint32_t* elems,
                           const uint8_t* scal, uint32_t* out, FbTab f0, FbTab f1, const PowOpts& o = {}) {
  const uint32_t* dj = nullptr;
  const int rc = upload_jobs(c, s, J, &dj);
  return rc ? rc : launch_pow(c, {S, dj, J.size()}, elems, scal, out, f0, f1, o);
}

static int launch_hash(eg_ctx* c, uint32_t n, std::vector<HashSrc> src, const uint8_t* proofs, uint32_t pw,
                       uint32_t ci0, uint32_t ci1, const uint8_t* pre_ok, const uint8_t* pre_ok2, uint32_t pre2_div,
                       uint8_t* ok, uint8_t* out_h) {
  if (!n) return EG_OK;
  if (src.size() > 8) return fail(EG_ERR_ARG, "more than 8 hash elements");
  while (src.size() < 8) src.push_back(HashSrc{nullptr, 0, 0});
  hipLaunchKernelGGL(k_hash_check, dim3(cgrid(n)), dim3(256), 0, c->stream, c->d_q, c->d_qbar, n,
                     (uint32_t)(std::count_if(src.begin(), src.end(), [](const HashSrc& h) { return h.ptr != nullptr; })),
                     src[0], src[1], src[2], src[3], src[4], src[5], src[6], src[7], proofs, pw, ci0, ci1, pre_ok,
                     pre_ok2, pre2_div, ok, out_h, c->hash_fmt);
  HIPCHK(hipGetLastError());
  return EG_OK;
}

// The Fiat-Shamir pre-image after Q-bar in the ctx's order (eg_ctx_set_proof_format): the proof's
// message elements (alpha, beta / A, B / pad, data), its commitments, then its extra elements (the
// share M), with the public key (K, or the guardian's K_i) first for EG_PREIMAGE_WITH_KEY.
static std::vector<HashSrc> preimage(const eg_ctx* c, const std::vector<HashSrc>& msg,
                                     const std::vector<HashSrc>& comm, const HashSrc& key,
                                     const std::vector<HashSrc>& extra = {}) {
  std::vector<HashSrc> v;
  if (c->pre_order == EG_PREIMAGE_WITH_KEY) v.push_back(key);
  const bool cf = c->pre_order == EG_PREIMAGE_COMMITMENTS_FIRST;
  v.insert(v.end(), (cf ? comm : msg).begin(), (cf ? comm : msg).end());
  v.insert(v.end(), (cf ? msg : comm).begin(), (cf ? msg : comm).end());
  v.insert(v.end(), extra.begin(), extra.end());
  return v;
}

// the current election key's bytes in HBM (a stride-0 hash element shared by every proof)
static HashSrc key_src(const eg_ctx* c) { return HashSrc{c->keys.front().d_K, 512, 0}; }

// Key tables kept per ctx: at most kKeyTabsMax keys, and older ones are dropped once the tables
// pass kKeyTabsBytes (one 22-bit table is 32 GB); the current key is never dropped.
static constexpr size_t kKeyTabsMax = 4;
static constexpr size_t kKeyTabsBytes = (size_t)72 << 30;
static size_t fb_bytes(const eg_fixed_base* fb) { return fb ? ((size_t)fb->nwin << fb->wbits) * kW * 4 : 0; }

// make keys[i] the current key (front of the MRU list)
static void key_front(eg_ctx* c, size_t i) {
  std::rotate(c->keys.begin(), c->keys.begin() + i, c->keys.begin() + i + 1);
  c->Ktab = c->keys.front().fb;
  std::memcpy(c->K_be, c->keys.front().K.data(), 512);
}

// K's radix table at wbits becomes the current key table (built unless cached); set_g: g's table
// follows the width (eg_set_election_key)
static int set_key_locked(eg_ctx* c, const uint8_t K_be[512], int wbits, bool set_g = true) {
  size_t hit = c->keys.size();
  for (size_t i = 0; i < c->keys.size() && hit == c->keys.size(); ++i)
    if (c->keys[i].fb->wbits == wbits && std::memcmp(c->keys[i].K.data(), K_be, 512) == 0) hit = i;
  if (hit < c->keys.size()) {
    key_front(c, hit);
  } else {
    eg_fixed_base* kt = nullptr;
    int rc = fb_create_locked(c, K_be, wbits, &kt);
    if (rc) return rc;
    eg_ctx::KeyTabs e;
    std::memcpy(e.K.data(), K_be, 512);
    e.fb = kt;
    if (hipMalloc(&e.d_K, 512) != hipSuccess) {
      eg_fixed_base_destroy(kt);
      return fail(EG_ERR_NOMEM, "hipMalloc key bytes failed");
    }
    HIPCHK(hipMemcpy(e.d_K, K_be, 512, hipMemcpyHostToDevice));
    c->keys.insert(c->keys.begin(), e);
    key_front(c, 0);
    size_t bytes = 0;
    for (const auto& k : c->keys) bytes += fb_bytes(k.fb) + fb_bytes(k.ct);
    while (c->keys.size() > 1 && (c->keys.size() > kKeyTabsMax || bytes > kKeyTabsBytes)) {
      HIPCHK(hipStreamSynchronize(c->stream));  // no queued launch still reads the dropped table
      bytes -= fb_bytes(c->keys.back().fb) + fb_bytes(c->keys.back().ct);
      eg_fixed_base_destroy(c->keys.back().fb);
      eg_fixed_base_destroy(c->keys.back().ct);
      if (c->keys.back().d_K) hipFree(c->keys.back().d_K);
      c->keys.pop_back();
    }
  }
  if (set_g && c->gtab->wbits != wbits) {
    eg_fixed_base* gt = nullptr;
    int rc = fb_create_locked(c, c->g_be, wbits, &gt);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    // the handle stays (eg_ctx_g_table and queued per-element jobs hold it): the new table moves
    // into it and the old one leaves with gt (g's constant-time companion is width-independent)
    std::swap(c->gtab->d_tab, gt->d_tab);
    std::swap(c->gtab->wbits, gt->wbits);
    std::swap(c->gtab->nwin, gt->nwin);
    eg_fixed_base_destroy(gt);
  }
  return EG_OK;
}

extern "C" int eg_set_election_key(eg_ctx* c, const uint8_t K_be[512], int wbits) {
  if (!c || !K_be) return fail(EG_ERR_ARG, "null argument");
  Locked L(c);
  return set_key_locked(c, K_be, wbits);
}

// ---------------------------------------------------------------------------------
// the ballot shape and the contest layer
// ---------------------------------------------------------------------------------
static constexpr size_t kVerifyChunk = 16384;
// Very wide manifests get fewer ballots per chunk, so one chunk never holds more than
// kChunkSelections selection jobs (~14 KB of device working set each, plus the k_pow
// scratch) and the 32-bit job and element indices stay far from overflow.  The configs'
// manifests (24 and 120 selections) keep the full 16,384-ballot chunks.
static constexpr size_t kChunkSelections = (size_t)1 << 21;
static constexpr size_t kMaxSelections = (size_t)1 << 20;  // selections per ballot
static size_t ballot_chunk(size_t nsel) {
  return std::max<size_t>(1, std::min(kVerifyChunk, kChunkSelections / std::max<size_t>(nsel, 1)));
}
// Host-pointer encryption overlaps chunk k's output copy (27 KB per 4x(5+1) ballot, as long
// as the kernels) with chunk k+1's kernels, which needs at least two chunks: a batch that fits
// one chunk is cut into up to four (of >= 2,048 ballots), so only the last quarter's copy is
// exposed (10k ballots: 115-134k -> 182k ballots/s, profiles/r02_ab_subchunk_*.log).  The
// verifier keeps whole chunks: its input copy is ~4% of its kernel time, and quarter-size
// launches cost it 11% in k_pow efficiency.
static size_t host_chunk(size_t nb, size_t nsel) {
  const size_t c = ballot_chunk(nsel);
  if (nb > c) return c;
  return std::min(c, std::max<size_t>(2048, (nb + 3) / 4));
}
static bool manifest_ok(size_t nc, size_t spc) {
  return nc && spc && nc <= kMaxSelections && spc <= kMaxSelections && nc * spc <= kMaxSelections;
}

// The validated shape of one call (host side).  Contest k of a ballot owns spc[k] consecutive
// selections from first[k], the placeholders last, and its constant proof uses limit[k].  The
// contests are grouped into CLASSES of equal spc: PowShape.gather is part of k_pow's op
// program, so a chunk has one contest job population per class.
//   * table-addressed (man_shape, eg_capi_manifest.inc): the per-contest vectors are filled and
//     go to the device as tables;
//   * uniform (uniform_shape): nc contests of uspc selections, uph placeholders and limit ulimit,
//     one class holding every contest.  No per-contest vector is filled (a 2^20-contest ballot
//     must not build megabyte tables or a megabyte key per call); the contest layer below
//     addresses such a shape by arithmetic.
struct ManShape {
  size_t nc = 0, nsel = 0, nreal = 0;
  bool uniform = false;
  uint32_t uspc = 0, uph = 0, ulimit = 0;         // the uniform shape's contest
  std::vector<uint32_t> spc, first, limit, real;  // per contest; real: the real selections' indices
  struct Class {
    uint32_t spc;
    size_t n;                       // contests in the class
    std::vector<uint32_t> members;  // their indices, ascending (uniform: contest mi, not listed)
    std::string tag;                // suffix of the class's table names in the cache
  };
  std::vector<Class> cls;  // ascending spc
  std::string fam;         // prefix of the cache keys ("m": table-addressed)
  std::string key;         // the spc list (verify: and the placeholders and limits), for the table cache
  uint32_t member(const Class& C, size_t mi) const { return uniform ? (uint32_t)mi : C.members[mi]; }
  uint32_t first_of(uint32_t k) const { return uniform ? k * uspc : first[k]; }
};

static ManShape uniform_shape(size_t nc, size_t spc, size_t ph, uint32_t limit) {
  ManShape M;
  M.uniform = true;
  M.nc = nc;
  M.nsel = nc * spc;
  M.nreal = nc * (spc - ph);
  M.uspc = (uint32_t)spc; M.uph = (uint32_t)ph; M.ulimit = limit;
  M.cls.push_back(ManShape::Class{(uint32_t)spc, nc, {}, ""});
  M.key = std::to_string(nc) + "/" + std::to_string(spc);
  return M;
}

// The host tables of one cached set (cached_job_set) in upload order, each with the place its
// device copy's address goes to.
struct TableList {
  std::vector<std::string> names;
  std::vector<std::function<JobTable()>> make;
  std::vector<const uint32_t**> dst;
  void add(const std::string& name, const uint32_t** d, std::function<JobTable()> f) {
    names.push_back(name); dst.push_back(d); make.push_back(std::move(f));
  }
};
static int fetch_tables(eg_ctx* c, const std::string& key, const TableList& L) {
  std::vector<const uint32_t*> dev;
  const int rc = cached_job_set(c, key, L.names, [&]() {
    JobSet host;
    for (const auto& f : L.make) host.push_back(f());
    return host;
  }, dev);
  for (size_t i = 0; !rc && i < dev.size(); ++i) *L.dst[i] = dev[i];
  return rc;
}

// The device tables the contest layer reads; a uniform shape has none (all stay null).
struct ContestTabs {
  const uint32_t *first = nullptr, *spc = nullptr, *limit = nullptr, *tally = nullptr;
  std::vector<const uint32_t*> in, out;  // per class: the aggregate product's in / out tables
  explicit ContestTabs(const ManShape& M) : in(M.cls.size(), nullptr), out(M.cls.size(), nullptr) {}
};
// Whether a set holds per-contest tables is decided here: the tables that lead a table-addressed
// shape's set (verify: with the limits and the tally's table of real selections), and below
// class ci's aggregate product tables (entry mi * 2 + comp of member contest k).
static void add_contest_tables(TableList& L, const ManShape& M, ContestTabs& T, bool verify) {
  if (M.uniform) return;
  L.add("first", &T.first, [&M]() { return M.first; });
  L.add("spc", &T.spc, [&M]() { return M.spc; });
  if (!verify) return;
  L.add("limit", &T.limit, [&M]() { return M.limit; });
  L.add("tally", &T.tally, [&M]() {
    std::vector<uint32_t> t;
    for (uint32_t r : M.real)
      for (uint32_t comp = 0; comp < 2; ++comp) t.push_back(r * 2 + comp);
    return t;
  });
}
static void add_class_tables(TableList& L, const ManShape& M, ContestTabs& T, size_t ci) {
  if (M.uniform) return;
  const ManShape::Class& C = M.cls[ci];
  L.add("in" + C.tag, &T.in[ci], [&M, &C]() {
    std::vector<uint32_t> t;
    for (uint32_t k : C.members)
      for (uint32_t comp = 0; comp < 2; ++comp) t.push_back(M.first[k] * 2 + comp);
    return t;
  });
  L.add("out" + C.tag, &T.out[ci], [&C]() {
    std::vector<uint32_t> t;
    for (uint32_t k : C.members)
      for (uint32_t comp = 0; comp < 2; ++comp) t.push_back(k * 2 + comp);
    return t;
  });
}

// The five steps that know the contests' sizes, each with an arithmetic arm (uniform shapes:
// the kernels and arguments the uniform entry points have always used) and a table arm.
// Aggregates A = prod alpha, B = prod beta of nbc ballots' contests: elems (ballot-major
// ciphertext pairs) -> agg[(b nc + k) 2 + comp].  The table arm runs class by class, addressed
// through the class's first selections and scattered into ballot-major contest order.
static int contest_aggregates(eg_ctx* c, const ManShape& M, const ContestTabs& T, size_t nbc, const uint32_t* elems,
                              uint32_t* agg) {
  if (M.uniform)
    return run_prod(c, elems, GroupMap{2, (uint32_t)M.nc, 1, 2 * M.uspc, (uint32_t)(2 * M.nsel)}, nbc * M.nc * 2,
                    M.uspc, 2, agg);
  for (size_t ci = 0; ci < M.cls.size(); ++ci) {
    const size_t period = M.cls[ci].n * 2;
    const int rc = run_prod_tab(c, elems, T.in[ci], period, 2 * M.nsel, nbc * period, M.cls[ci].spc, 2, agg,
                                T.out[ci], 2 * M.nc);
    if (rc) return rc;
  }
  return EG_OK;
}
// The contest proofs' scalars (c, v) x ncn at sc: range flags -> okc, the exponents -L_k c -> negL
static void contest_scalars(eg_ctx* c, const ManShape& M, const ContestTabs& T, uint8_t* sc, size_t ncn, uint8_t* negL,
                            uint8_t* okc) {
  if (M.uniform)
    hipLaunchKernelGGL(k_scalar_prep, dim3(cgrid(ncn)), dim3(256), 0, c->stream, c->d_q, sc, (uint32_t)ncn, 2u, 0u,
                       M.ulimit, negL, okc, c->resp_plus, 0x1u);
  else
    hipLaunchKernelGGL(k_scalar_prep_tab, dim3(cgrid(ncn)), dim3(256), 0, c->stream, c->d_q, sc, (uint32_t)ncn, 2u, 0u,
                       T.limit, (uint32_t)M.nc, negL, okc, c->resp_plus, 0x1u);
}
// (A, B) flags per contest: the AND of its selections' range + residue flags
static void contest_flags(eg_ctx* c, const ManShape& M, const ContestTabs& T, const uint8_t* ltp, size_t ncn,
                          uint8_t* crf) {
  if (M.uniform)
    hipLaunchKernelGGL(k_contest_flags, dim3(cgrid(ncn * 2)), dim3(256), 0, c->stream, ltp, (uint32_t)ncn, M.uspc,
                       crf);
  else
    hipLaunchKernelGGL(k_contest_flags_seg, dim3(cgrid(ncn * 2)), dim3(256), 0, c->stream, ltp, (uint32_t)ncn,
                       (uint32_t)M.nc, (uint32_t)M.nsel, T.first, T.spc, crf);
}
// the sum of each contest's selection nonces R (the encryptor's scalars sc) -> rsum
static void nonce_sums(eg_ctx* c, const ManShape& M, const ContestTabs& T, const uint8_t* sc, size_t ncn,
                       uint8_t* rsum) {
  if (M.uniform)
    hipLaunchKernelGGL(k_enc_rsum, dim3(cgrid(ncn)), dim3(256), 0, c->stream, c->d_q, sc, (uint32_t)ncn, M.uspc, rsum);
  else
    hipLaunchKernelGGL(k_enc_rsum_seg, dim3(cgrid(ncn)), dim3(256), 0, c->stream, c->d_q, sc, (uint32_t)ncn,
                       (uint32_t)M.nc, (uint32_t)M.nsel, T.first, T.spc, rsum);
}
// products over the nbc ballots with cast[b] != 0 (all: cast == nullptr) of every real
// selection's (alpha, beta) -> out[nreal * 2]
static int chunk_tally(eg_ctx* c, const ManShape& M, const ContestTabs& T, size_t nbc, const uint32_t* elems,
                       uint32_t* out, const uint8_t* d_cast) {
  if (M.uniform)
    return run_prod(c, elems, GroupMap{2, M.uspc - M.uph, 1, 2, 2 * M.uspc}, M.nreal * 2, nbc, M.nsel * 2, out, d_cast);
  return run_prod_tab(c, elems, T.tally, M.nreal * 2, 0, M.nreal * 2, nbc, M.nsel * 2, out, nullptr, 0, d_cast);
}

// ---------------------------------------------------------------------------------
// verification + tally
// ---------------------------------------------------------------------------------
// The verifier's scalar space (32-byte rows): the range proofs (c0, v0, c1, v1) x ns, the contest
// proofs (c, v) x ncn, then the derived exponents -c1 x ns and -L c x ncn.  Elements: the
// ciphertexts (ns x 2), then the aggregates (ncn x 2); commitments: ns x 4, then ncn x 2.
struct VerifyLayout {
  size_t ns, ncn, off_c, off_neg, off_negL;
  VerifyLayout(const ManShape& M, size_t nbc)
      : ns(nbc * M.nsel), ncn(nbc * M.nc), off_c(ns * 4), off_neg(off_c + ncn * 2), off_negL(off_neg + ns) {}
};
// the alpha (beta == false) or beta jobs of ns selections
static std::vector<PowJob> verify_sel_jobs(const VerifyLayout& V, bool beta) {
  auto J = new_jobs(V.ns);
  for (size_t i = 0; i < V.ns; ++i) {
    PowJob& x = J[i];
    const uint32_t c0 = (uint32_t)(i * 4), v0 = c0 + 1, c1 = c0 + 2, v1 = c0 + 3, e = beta ? 1u : 0u;
    x.base = (uint32_t)(i * 2) + e; x.exp[0] = c0; x.exp[1] = c1; x.out[0] = c0 + e; x.out[1] = c1 + e;
    x.fb[0][0] = v0; x.fb[1][0] = v1;
    if (beta) x.fb[1][1] = (uint32_t)(V.off_neg + i);
  }
  return J;
}
// the contest a (b == false) or contest b jobs of class C, ballot-major: job bi * C.n + mi
static std::vector<PowJob> verify_contest_jobs(const ManShape& M, const ManShape::Class& C, const VerifyLayout& V,
                                                 size_t nbc, bool b) {
  auto J = new_jobs(nbc * C.n);
  for (size_t bi = 0; bi < nbc; ++bi)
    for (size_t mi = 0; mi < C.n; ++mi) {
      const uint32_t k = M.member(C, mi), e = b ? 1u : 0u;
      const size_t j = bi * M.nc + k;  // the contest's place in every ballot-major array
      PowJob& x = J[bi * C.n + mi];
      const uint32_t cc = (uint32_t)(V.off_c + j * 2);
      x.base = (uint32_t)(V.ns * 2 + j * 2) + e; x.exp[0] = cc; x.out[0] = (uint32_t)(V.ns * 4 + j * 2) + e;
      x.fb[0][0] = cc + 1;
      if (b) x.fb[0][1] = (uint32_t)(V.off_negL + j);
      x.gather_src() = (uint32_t)(bi * M.nsel + M.first_of(k));  // the contest's first selection job (y_k source)
    }
  return J;
}

// One launch_pow call of the contest populations: a main part and up to two tails.
struct PowLaunch {
  PowPop main;
  std::vector<PowPop> tails;
};
// The verifier's k_pow launches.  Launch 1 is alpha with the first xb beta jobs as its tail,
// launch 2 the other betas with `l2` as tails, then `later`, one launch_pow call each.
struct VerifyPlan {
  size_t xb = 0;
  std::vector<PowPop> l2;
  std::vector<PowLaunch> later;
};

// The beta head: x0 beta jobs (rounded to whole workgroups) plus as many as fill launch 1's last
// round of `slots` resident workgroups.
static size_t beta_head(size_t ns, size_t slots, size_t x0) {
  if (!slots) return 0;
  auto last_blocks = [](size_t n) {  // workgroups of the last k_pow sub-launch of n jobs
    return n ? (size_t)grid_for(n - (n - 1) / kPowMaxJobs * kPowMaxJobs) : 0;
  };
  x0 = std::min(ns, (x0 + kGroupsPerBlock - 1) / kGroupsPerBlock * kGroupsPerBlock);
  // the beta head rides with alpha's last sub-launch: keep that launch within
  // kPowTailJobs jobs (its k_pow scratch, 40 KB per job; a 120-selection chunk would
  // otherwise put 1.8M beta jobs there), the rest of contest b then stays in launch 3
  const size_t a_last = ns ? ns - (ns - 1) / kPowMaxJobs * kPowMaxJobs : 0;
  const size_t cap = a_last < kPowTailJobs ? (kPowTailJobs - a_last) / kGroupsPerBlock * kGroupsPerBlock : 0;
  x0 = std::min(x0, cap);
  // then fill launch 1's last round (the beta part rides with alpha's last sub-launch)
  const size_t used = last_blocks(ns) + x0 / kGroupsPerBlock;
  const size_t fill1 = (slots - used % slots) % slots;
  return std::min(ns, x0 + fill1 * kGroupsPerBlock);
}

// pa / pb: the contest a = A^c g^v populations (need the alpha y_k: any launch after 1) and the
// contest b = B^c K^v g^-Lc populations (need the beta y_k: any launch after 2), one per class.
// Two rules, because the uniform entry points' plan is the measured one of the benchmark:
//   * uniform: three launches.  Launch 2 takes EVERY contest-a job as one tail, whatever their
//     number (a 16,384 x 20-contest chunk's 327,680 ride as one), launch 3 is contest b.  With
//     EG_CB_EARLY=1 (opt-in, measured slower) launch 1 also takes the betas of every contest
//     whose contest-b job can then ride in launch 2, so launch 3 shrinks to EG_L3_WAVES waves per
//     SIMD.  In an interleaved A/B on one box (four rounds, MM per shader clock from the
//     in-kernel clock) it ran 0.4-0.5% SLOWER than the default split, although it cuts launch 3
//     from 10.8 to ~5 ms (profiles/r03n_ab_l3clock.log).
//   * table-addressed: launch 2 takes up to two contest-a populations as its tails; what is left
//     of contest a and every contest-b population follow three to a launch.  A tail is never
//     split into sub-launches, so only populations of at most kPowMaxJobs jobs ride as one.  At
//     most 2 + (C - 2) + C <= 2 + 2 C launch_pow calls for C classes.  EG_CB_EARLY is ignored.
static VerifyPlan plan_pow_launches(const eg_ctx* c, const ManShape& M, size_t ns, size_t ncn,
                                    const std::vector<PowPop>& pa, const std::vector<PowPop>& pb) {
  VerifyPlan P;
  size_t slots = c->pow_slots;
  if (const char* ov = getenv("EG_POW_SLOTS")) slots = (size_t)strtoull(ov, nullptr, 10);  // test override
  const char* dbg = getenv("EG_DEBUG_SCHED");
  const bool debug = dbg && dbg[0] == '1';
  if (M.uniform) {
    const char* cbe = getenv("EG_CB_EARLY");
    const bool cb_early = cbe && cbe[0] == '1';
    // launch 3 (contest b after the contests launch 1 covers) within two waves per SIMD
    // (EG_L3_WAVES, 1 .. the occupancy; a lone round of 172-MM jobs at 3 waves/SIMD takes
    // ~5 ms, at 2 its jobs finish in about two thirds of that): at least (ncn - that many
    // jobs) contests' betas in launch 1
    size_t x0 = 0;
    if (slots && cb_early) {
      uint32_t l3w = std::min(2u, c->pow_wps);
      if (const char* lw = getenv("EG_L3_WAVES")) l3w = (uint32_t)std::max(1, std::min((int)c->pow_wps, atoi(lw)));
      const size_t l3_jobs = slots * kGroupsPerBlock * l3w / c->pow_wps;
      if (ncn > l3_jobs) x0 = (ncn - l3_jobs) * M.uspc;
    }
    P.xb = beta_head(ns, slots, x0);
    const size_t jc = cb_early ? std::min(ncn, P.xb / M.uspc) : 0;  // contests whose betas all run in launch 1
    if (debug)
      fprintf(stderr, "eg verify schedule: ns %zu ncn %zu slots %zu waves/SIMD %u: beta head %zu, early contest b %zu\n",
              ns, ncn, slots, c->pow_wps, P.xb, jc);
    P.l2 = {pa[0], pb[0].part(0, jc)};
    if (jc < ncn) P.later.push_back(PowLaunch{pb[0].part(jc, ncn - jc), {}});
    return P;
  }
  P.xb = beta_head(ns, slots, 0);
  std::vector<PowPop> rest;
  for (const PowPop& p : pa) {
    if (P.l2.size() < 2 && p.njobs <= kPowMaxJobs) P.l2.push_back(p);
    else rest.push_back(p);
  }
  if (debug)
    fprintf(stderr, "eg verify schedule (manifest): ns %zu ncn %zu classes %zu slots %zu: beta head %zu, "
                    "contest a in launch 2: %zu\n", ns, ncn, M.cls.size(), slots, P.xb, P.l2.size());
  rest.insert(rest.end(), pb.begin(), pb.end());
  for (size_t i = 0; i < rest.size();) {
    PowLaunch L{rest[i++], {}};
    while (L.tails.size() < 2 && i < rest.size() && rest[i].njobs <= kPowMaxJobs) L.tails.push_back(rest[i++]);
    P.later.push_back(std::move(L));
  }
  return P;
}

// One chunk of <= ballot_chunk(nsel) ballots: every proof of ballots [0, nbc) of the given device
// arrays, and (tally != nullptr) their per-selection products, written to tally (first
// chunk) or multiplied into it.  d_qbar and the key tables are set by the caller.
// cast (optional, nbc bytes on the device): only ballots with cast[b] != 0 enter the tally; the
// others (spoiled ballots, RunRemoteDecryptor.java:264-269) are verified but not tallied.
static int verify_chunk_locked(eg_ctx* c, const ManShape& M, size_t nbc, const uint8_t* cts, const uint8_t* d_rproof,
                               const uint8_t* d_cproof, const uint8_t* d_cast, uint8_t* d_ok_sel, uint8_t* d_ok_con,
                               uint32_t* tally, bool first) {
  const FbTab G = c->gtab->tab(), K = c->Ktab->tab();
  const VerifyLayout V(M, nbc);
  const size_t ns = V.ns, ncn = V.ncn, nreal = M.nreal, ncls = M.cls.size();
  int rc;
  uint32_t *E = nullptr, *COMM = nullptr;
  uint8_t *LTP = nullptr, *SC = nullptr, *OKR = nullptr, *OKC = nullptr, *COMM_BE = nullptr, *CP_BE = nullptr;
  if ((rc = ws_get(c, W_E0, (ns * 2 + ncn * 2) * kW * 4, (void**)&E))) return rc;
  if ((rc = ws_get(c, W_E1, (ns * 4 + ncn * 2) * kW * 4, (void**)&COMM))) return rc;
  if ((rc = ws_get(c, W_FLAGS, ns * 2, (void**)&LTP))) return rc;
  if ((rc = ws_get(c, W_SCAL, (V.off_negL + ncn) * 32, (void**)&SC))) return rc;
  if ((rc = ws_get(c, W_OK0, ns, (void**)&OKR))) return rc;
  if ((rc = ws_get(c, W_OK1, ncn, (void**)&OKC))) return rc;
  if ((rc = ws_get(c, W_BE0, (ns * 4 + ncn * 2) * 512, (void**)&COMM_BE))) return rc;
  if ((rc = ws_get(c, W_BE1, ncn * 2 * 512, (void**)&CP_BE))) return rc;
  // The chunk's tables, one cached set (a second set could be freed by the first's cache_bound):
  // the contest layer's, the selection jobs, and per class the contest jobs.
  ContestTabs T(M);
  const uint32_t *jA = nullptr, *jB = nullptr;
  std::vector<const uint32_t*> jCA(ncls, nullptr), jCB(ncls, nullptr);
  TableList L;
  add_contest_tables(L, M, T, true);
  L.add("A", &jA, [&]() { return verify_sel_jobs(V, false); });
  L.add("B", &jB, [&]() { return verify_sel_jobs(V, true); });
  for (size_t ci = 0; ci < ncls; ++ci) {
    const ManShape::Class& C = M.cls[ci];
    add_class_tables(L, M, T, ci);
    L.add("CA" + C.tag, &jCA[ci], [&M, &C, &V, nbc]() { return verify_contest_jobs(M, C, V, nbc, false); });
    L.add("CB" + C.tag, &jCB[ci], [&M, &C, &V, nbc]() { return verify_contest_jobs(M, C, V, nbc, true); });
  }
  if ((rc = fetch_tables(c, M.fam + "v/" + std::to_string(nbc) + "/" + M.key, L))) return rc;
  // 1. import ciphertexts (range flags alpha, beta < p)
  if ((rc = launch_import(c, cts, ns * 2, E, LTP))) return rc;
  // 2. scalars: proofs + derived exponents (-c1, -L c) + range flags
  HIPCHK(hipMemcpyAsync(SC, d_rproof, ns * 128, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(SC + V.off_c * 32, d_cproof, ncn * 64, hipMemcpyDeviceToDevice, c->stream));
  // plus convention: c0, c1 and c negated in place (the comb exponents), the g terms take +c1, +L c
  hipLaunchKernelGGL(k_scalar_prep, dim3(cgrid(ns)), dim3(256), 0, c->stream, c->d_q, SC, (uint32_t)ns, 4u, 2u, 1u,
                     SC + V.off_neg * 32, OKR, c->resp_plus, 0x5u);
  contest_scalars(c, M, T, SC + V.off_c * 32, ncn, SC + V.off_negL * 32, OKC);
  HIPCHK(hipGetLastError());
  // 3. contest aggregates A = prod alpha, B = prod beta -> E[ns*2 + j*2 + {0,1}]
  uint32_t* CP = E + ns * 2 * kW;
  if ((rc = contest_aggregates(c, M, T, nbc, E, CP))) return rc;
  // 4. commitments
  // The selection jobs keep their comb powers y_k = alpha^(2^(52k)) (YA, YB); the contest
  // aggregates A = prod alpha, B = prod beta then get theirs as products over the contest
  // (4 x (spc-1) MM instead of 208 squarings; the contest comb costs ~150 MM, not 329).
  // The alpha / beta jobs always run the comb (two column blocks): its squaring chain to
  // B^(2^234) runs on to the residue test's B^(2^256) (EG_NO_COMB only switches the contest
  // and trustee jobs to the 4-bit window).
  const bool gat = c->use_comb != 0;
  uint32_t *YA = nullptr, *YB = nullptr, *RZ = nullptr;
  if (gat) {
    if ((rc = ws_get(c, W_YA, ns * (kCombH - 1) * kW * 4, (void**)&YA))) return rc;
    if ((rc = ws_get(c, W_YB, ns * (kCombH - 1) * kW * 4, (void**)&YB))) return rc;
  }
  // residue-test pairs (z, w) of every alpha, then every beta (4 device elements per selection)
  if ((rc = ws_get(c, W_RZ, ns * 4 * kW * 4, (void**)&RZ))) return rc;
  // the selection jobs' comb: 4 rows x 3 blocks (22 columns, three 16-entry tables: 33 subset
  // products, 21 squarings + 63 multiplies per exponent) or, with EG_SEL_COMB=52, round 2's
  // 5 rows x 2 blocks (26 columns, two 32-entry tables: 52 + 2 x (25 + 51)); every block's
  // bases come from the residue chain.  4 x 3 is 3 MM fewer per job, 0.4% more ballots per
  // shader clock and a 0.6% higher clock (25% less comb-table traffic) in a same-box A/B
  // (profiles/r03r_ab_sel43.log)
  const uint32_t srows = c->sel_rows, sblocks = c->sel_blocks;
  // alpha: a0 = alpha^c0 g^v0, a1 = alpha^c1 g^v1; beta: b0 = beta^c0 K^v0, b1 = beta^c1 K^v1 g^-c1
  // (one comb shared by c0, c1 each)
  const PowPop PA{pow_sel_pair(false, srows, sblocks), jA, ns, YA, nullptr, RZ};
  const PowPop PB{pow_sel_pair(true, srows, sblocks), jB, ns, YB, nullptr, RZ + ns * 2 * kW};
  std::vector<PowPop> pa, pb;
  for (size_t ci = 0; ci < ncls; ++ci) {
    const uint32_t gather = gat ? M.cls[ci].spc : 0u;
    const size_t n = nbc * M.cls[ci].n;
    // contest a = A^c g^v, contest b = B^c K^v g^-Lc
    pa.push_back(PowPop{pow_sel_gather(false, gather), jCA[ci], n, nullptr, YA});
    pb.push_back(PowPop{pow_sel_gather(true, gather), jCB[ci], n, nullptr, YB});
  }
  const VerifyPlan P = plan_pow_launches(c, M, ns, ncn, pa, pb);
  const size_t xb = P.xb;
  auto launch = [&](const PowPop& main, const std::vector<PowPop>& tl) {
    return launch_pow(c, main, E, SC, COMM, G, K, {tl.size() > 0 ? tl[0] : PowPop{}, tl.size() > 1 ? tl[1] : PowPop{}});
  };
  // the first xb beta jobs fill launch 1's last round
  if ((rc = launch(PA, {PB.part(0, xb)}))) return rc;
  if ((rc = launch(PB.part(xb, ns - xb), P.l2))) return rc;
  // alpha^q == 1 and beta^q == 1 (valid residues) fold into the range flags the hash check reads
  LAUNCH_F(c, k_resid_check, dim3(grid_for(ns)), c->d, RZ, (uint32_t)ns, LTP, 2u);
  LAUNCH_F(c, k_resid_check, dim3(grid_for(ns)), c->d, RZ + ns * 2 * kW, (uint32_t)ns, LTP + 1, 2u);
  HIPCHK(hipGetLastError());
  // The contest proof's message (A, B) = (prod alpha, prod beta) is valid when every selection's
  // alpha (beta) is: the AND of the selections' range + residue flags, no products -- a contest
  // holding an invalid selection is rejected together with it.
  uint8_t* CRF = nullptr;
  if ((rc = ws_get(c, W_CRF, ncn * 2, (void**)&CRF))) return rc;
  contest_flags(c, M, T, LTP, ncn, CRF);
  HIPCHK(hipGetLastError());
  for (const PowLaunch& l : P.later)
    if ((rc = launch(l.main, l.tails))) return rc;
  // 5. canonical bytes of commitments and contest aggregates
  if ((rc = launch_export(c, COMM, ns * 4 + ncn * 2, COMM_BE))) return rc;
  if ((rc = launch_export(c, CP, ncn * 2, CP_BE))) return rc;
  // 6. Fiat-Shamir checks
  // (the challenges come from the caller's proofs: SC's may be negated, EG_RESPONSE_PLUS)
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
  // 7. tally over this chunk's cast ballots (real selections only)
  if (tally) {
    uint32_t* TP = first ? tally : tally + nreal * 2 * kW;
    if ((rc = chunk_tally(c, M, T, nbc, E, TP, d_cast))) return rc;
    if (!first) {
      LAUNCH_F(c, k_mul, dim3(grid_for(nreal * 2)), c->d, tally, 1u, TP, 1u, (uint32_t)(nreal * 2), tally, 1u);
      HIPCHK(hipGetLastError());
    }
  }
  return EG_OK;
}

// The key a ballot call uses is set under the same lock as the call itself (a ctx is shared by
// every thread of a process, productionGroup): K's table is kept when it matches (no work),
// else rebuilt at the window width of the table the ctx holds (eg_set_election_key picks it).
static int use_key_locked(eg_ctx* c, const uint8_t* K_be) {
  for (size_t i = 0; i < c->keys.size(); ++i)
    if (std::memcmp(c->keys[i].K.data(), K_be, 512) == 0) {  // a cached table of K, whatever its width
      key_front(c, i);
      return EG_OK;
    }
  const int wb = c->Ktab ? c->Ktab->wbits : c->gtab->wbits;
  return set_key_locked(c, K_be, wb, false);
}

// an all-ones tally (the empty product) in wire form
static void ones_be(uint8_t* out, size_t n) {
  std::memset(out, 0, n * 512);
  for (size_t i = 0; i < n; ++i) out[i * 512 + 511] = 1;
}

// The drivers below run under the caller's lock, after its argument checks and use_key_locked.
// Device pointers in and out, chunk by chunk on the ctx stream.
static int verify_dev_locked(eg_ctx* c, const ManShape& M, const uint8_t* qbar_be, size_t nb, const uint8_t* d_cts,
                             const uint8_t* d_rproof, const uint8_t* d_cproof, const uint8_t* d_cast,
                             uint8_t* d_ok_sel, uint8_t* d_ok_con, uint8_t* d_tally_be) {
  int rc;
  const size_t nc = M.nc, nsel = M.nsel, nreal = M.nreal;
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
    if ((rc = verify_chunk_locked(c, M, nbc, d_cts + b0 * nsel * 1024, d_rproof + b0 * nsel * 128,
                                  d_cproof + b0 * nc * 64, d_cast ? d_cast + b0 : nullptr, d_ok_sel + b0 * nsel,
                                  d_ok_con + b0 * nc, tally, b0 == 0)))
      return rc;
  }
  return d_tally_be ? launch_export(c, tally, nreal * 2, d_tally_be) : EG_OK;
}

// the ctx's copy stream and its two pairs of events (created on first use, under the lock)
static int ensure_copy_stream(eg_ctx* c) {
  if (c->copy) return EG_OK;
  HIPCHK(hipStreamCreateWithFlags(&c->copy, hipStreamNonBlocking));
  for (int i = 0; i < 2; ++i) {
    HIPCHK(hipEventCreateWithFlags(&c->up_ev[i], hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->done_ev[i], hipEventDisableTiming));
  }
  return EG_OK;
}

// Host pointers, streamed in ballot_chunk(nsel)-ballot chunks through two upload buffers: chunk
// k+1's wire input goes up on the ctx's copy stream while chunk k verifies on the ctx stream, so
// the device holds two chunks of input (about 2 x 400 MB at 4x(5+1)) however many ballots the
// caller passes.  Verdicts stay on the device until the end (a pageable D2H per chunk would block
// the host before it can start the next upload).
static int verify_host_locked(eg_ctx* c, const ManShape& M, const uint8_t* qbar_be, size_t nb, const uint8_t* cts,
                              const uint8_t* rproof, const uint8_t* cproof, const uint8_t* cast, uint8_t* ok_sel,
                              uint8_t* ok_con, uint8_t* tally_be) {
  int rc;
  const size_t nc = M.nc, nsel = M.nsel, nreal = M.nreal;
  if (!nb) {
    if (tally_be) ones_be(tally_be, nreal * 2);
    return EG_OK;
  }
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
    if ((rc = verify_chunk_locked(c, M, nbc, up[u][0], up[u][1], up[u][2], d_cast ? d_cast + b0 : nullptr,
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

extern "C" int eg_verify_ballots_dev(eg_ctx* c, const uint8_t K_be[512], const uint8_t qbar_be[32], size_t nb,
                                     size_t nc, size_t spc, size_t ph, uint32_t limit, const uint8_t* d_cts,
                                     const uint8_t* d_rproof, const uint8_t* d_cproof, const uint8_t* d_cast,
                                     uint8_t* d_ok_sel, uint8_t* d_ok_con, uint8_t* d_tally_be) {
  if (!c || !K_be || !qbar_be || (nb && (!d_cts || !d_rproof || !d_cproof || !d_ok_sel || !d_ok_con)))
    return fail(EG_ERR_ARG, "null argument");
  if (!manifest_ok(nc, spc) || ph >= spc) return fail(EG_ERR_ARG, "bad manifest shape");
  const ManShape M = uniform_shape(nc, spc, ph, limit);
  Locked L(c);
  int rc;
  if ((rc = use_key_locked(c, K_be))) return rc;
  return verify_dev_locked(c, M, qbar_be, nb, d_cts, d_rproof, d_cproof, d_cast, d_ok_sel, d_ok_con, d_tally_be);
}

extern "C" int eg_verify_ballots(eg_ctx* c, const uint8_t K_be[512], const uint8_t qbar_be[32], size_t nb, size_t nc,
                                 size_t spc, size_t ph, uint32_t limit, const uint8_t* cts, const uint8_t* rproof,
                                 const uint8_t* cproof, const uint8_t* cast, uint8_t* ok_sel, uint8_t* ok_con,
                                 uint8_t* tally_be) {
  if (!c || !K_be || !qbar_be || (nb && (!cts || !rproof || !cproof || !ok_sel || !ok_con)))
    return fail(EG_ERR_ARG, "null argument");
  if (!manifest_ok(nc, spc) || ph >= spc) return fail(EG_ERR_ARG, "bad manifest shape");
  const ManShape M = uniform_shape(nc, spc, ph, limit);
  Locked L(c);
  int rc;
  if ((rc = use_key_locked(c, K_be))) return rc;
  return verify_host_locked(c, M, qbar_be, nb, cts, rproof, cproof, cast, ok_sel, ok_con, tally_be);
}

// ---------------------------------------------------------------------------------
// encryption with injected nonces (known-nonce disjunctive + constant proofs)
// ---------------------------------------------------------------------------------
// The radix tables one encryption call uses: g's and K's (the ctx's K must be current), or in
// constant-time mode their ct_window-bit tables (kCtEncWindow = 6: 1.76 MB each), built once per key.
static int enc_tables_locked(eg_ctx* c, FbTab* G, FbTab* K) {
  if (!c->ct_encrypt) {
    *G = c->gtab->tab();
    *K = c->Ktab->tab();
    return EG_OK;
  }
  int rc;
  if (!c->g_ct && (rc = fb_create_locked(c, c->g_be, c->ct_window, &c->g_ct))) return rc;
  eg_ctx::KeyTabs& cur = c->keys.front();  // the call's key (use_key_locked made it current)
  if (!cur.ct && (rc = fb_create_locked(c, cur.K.data(), c->ct_window, &cur.ct))) return rc;
  *G = c->g_ct->tab();
  *K = cur.ct->tab();
  return EG_OK;
}

extern "C" int eg_ctx_set_ct_encrypt(eg_ctx* c, int on) {
  if (!c) return fail(EG_ERR_ARG, "null ctx");
  Locked L(c);
  c->ct_encrypt = on ? 1u : 0u;
  return EG_OK;
}

// The encryptor's scalar space (32-byte rows): the selection nonces (R, u, cf, vf) x ns, the
// contest nonces x ncn, the derived (m, sf, sg) x ns, then the nonce sums x ncn.  One element
// space: the ciphertexts (ns x 2), the selection commitments (ns x 4), the aggregates A, B
// (ncn x 2), then the contest commitments a, b (ncn x 2).
struct EncryptLayout {
  size_t ns, ncn, off_cn, off_der, off_rs, nscal, oCM, oCP, oCC, nU;
  static constexpr size_t oCT = 0;  // the ciphertexts lead the element space
  EncryptLayout(const ManShape& M, size_t nb)
      : ns(nb * M.nsel), ncn(nb * M.nc), off_cn(ns * 4), off_der(off_cn + ncn), off_rs(off_der + ns * 3),
        nscal(off_rs + ncn), oCM(ns * 2), oCP(oCM + ns * 4), oCC(oCP + ncn * 2), nU(oCC + ncn * 2) {}
};
// the selection jobs (a selection job does not know its contest), which:
//   1  alpha = g^R ; a_real = g^u                -> slot 0
//   2  beta = K^R g^m ; b_real = K^u             -> slot 1
//   3  a_fake = g^sf ; b_fake = K^sf g^sg       -> slots 2, 3
static std::vector<PowJob> encrypt_sel_jobs(const EncryptLayout& V, int which) {
  auto J = new_jobs(V.ns);
  for (size_t i = 0; i < V.ns; ++i) {
    const uint32_t R = (uint32_t)(i * 4), u = R + 1;
    const uint32_t dm = (uint32_t)(V.off_der + i * 3), sf = dm + 1, sg = dm + 2;
    const uint32_t cm = (uint32_t)(V.oCM + i * 4);
    PowJob& x = J[i];
    if (which == 1) {
      x.out[0] = (uint32_t)(V.oCT + i * 2); x.out[1] = cm; x.fb[0][0] = R; x.fb[1][0] = u;
    } else if (which == 2) {
      x.out[0] = (uint32_t)(V.oCT + i * 2 + 1); x.out[1] = cm + 1; x.fb[0][0] = R; x.fb[0][1] = dm; x.fb[1][0] = u;
    } else {
      x.out[0] = cm + 2; x.out[1] = cm + 3; x.fb[0][0] = sf; x.fb[1][0] = sf; x.fb[1][1] = sg;
    }
  }
  return J;
}
// the contest commitments a = g^u_c ; b = K^u_c (they do not depend on the contests' sizes)
static std::vector<PowJob> encrypt_contest_jobs(const EncryptLayout& V) {
  auto J = new_jobs(V.ncn);
  for (size_t j = 0; j < V.ncn; ++j) {
    PowJob& a = J[j];
    a.out[0] = (uint32_t)(V.oCC + j * 2); a.out[1] = (uint32_t)(V.oCC + j * 2 + 1);
    a.fb[0][0] = (uint32_t)(V.off_cn + j); a.fb[1][0] = (uint32_t)(V.off_cn + j);
  }
  return J;
}

// One chunk of <= ballot_chunk(nsel) ballots, enqueued on the ctx stream (c->d_qbar already holds
// Q-bar; the caller holds the lock).  d_votes, the nonces and (when given) the outputs are device
// pointers; the wire outputs land in output set `set` (two sets, so the caller can copy one
// chunk's outputs back while the next chunk computes): *d_cts (ns*1024 B), *d_rp (ns*128),
// *d_cp (ncn*64).  A caller whose outputs live in device memory passes their addresses in
// *d_cts / *d_rproof / *d_cproof and the kernels write there (no device-to-device copy).
// The job tables do not depend on the votes: every selection computes its real branch into
// commitment slots 0-1 and its simulated branch into 2-3, and k_enc_order swaps the pairs of the
// selections voted 1 with masks.  So they are cached per chunk shape, the host never reads a
// vote, and with eg_ctx_set_ct_encrypt (k_pow<F, true>, masked scans of 64-entry table columns)
// neither addresses nor the schedule depend on a nonce or a vote.
static int encrypt_chunk_locked(eg_ctx* c, const ManShape& M, size_t nb, const uint8_t* d_votes,
                                const uint8_t* sel_nonces, const uint8_t* contest_nonces, bool dev_nonces, int set,
                                const uint8_t** d_cts, const uint8_t** d_rproof, const uint8_t** d_cproof) {
  int rc;
  FbTab G{}, K{};
  if ((rc = enc_tables_locked(c, &G, &K))) return rc;
  const bool ct = c->ct_encrypt != 0;
  const EncryptLayout V(M, nb);
  const size_t ns = V.ns, ncn = V.ncn, oCT = V.oCT, oCM = V.oCM, oCP = V.oCP, oCC = V.oCC, nU = V.nU;
  uint8_t *SC = nullptr, *CH = nullptr, *CHC = nullptr, *d_rp = nullptr, *d_cp = nullptr;
  uint8_t* UBE = nullptr;
  uint32_t* U = nullptr;
  if ((rc = ws_get(c, W_SCAL, V.nscal * 32, (void**)&SC))) return rc;
  if ((rc = ws_get(c, W_E0, nU * kW * 4, (void**)&U))) return rc;
  ContestTabs T(M);
  const uint32_t *j1 = nullptr, *j2 = nullptr, *j3 = nullptr, *j4 = nullptr;
  TableList L;
  add_contest_tables(L, M, T, false);
  L.add("1", &j1, [&V]() { return encrypt_sel_jobs(V, 1); });
  L.add("2", &j2, [&V]() { return encrypt_sel_jobs(V, 2); });
  L.add("3", &j3, [&V]() { return encrypt_sel_jobs(V, 3); });
  L.add("4", &j4, [&V]() { return encrypt_contest_jobs(V); });
  for (size_t ci = 0; ci < M.cls.size(); ++ci) add_class_tables(L, M, T, ci);
  if ((rc = fetch_tables(c, M.fam + "e/" + std::to_string(nb) + "/" + M.key, L))) return rc;
  const hipMemcpyKind nk = dev_nonces ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  HIPCHK(hipMemcpyAsync(SC, sel_nonces, ns * 128, nk, c->stream));
  HIPCHK(hipMemcpyAsync(SC + V.off_cn * 32, contest_nonces, ncn * 32, nk, c->stream));
  hipLaunchKernelGGL(k_enc_prep, dim3(cgrid(ns)), dim3(256), 0, c->stream, c->d_q, d_votes, SC, (uint32_t)ns,
                     SC + V.off_der * 32, c->resp_plus);
  nonce_sums(c, M, T, SC, ncn, SC + V.off_rs * 32);
  HIPCHK(hipGetLastError());
  // All four job populations are fixed-base only and independent of each other (j1: alpha and
  // the real-branch a; j2: beta and the real-branch b; j3: the simulated branch; j4: the contest
  // commitments), so they run as two two-part launches whose second part fills the first's
  // last round; the contest aggregates (products of j1/j2's ciphertexts) follow.  g^m (m the
  // vote, 0 or 1) takes radix window 0 only: one multiply instead of a full fixed-base term.
  {
    PowShape S = pow_fb_pair(false);
    S.tab[1][0] = 0;  // g^R ; g^u: both from g's table
    if ((rc = launch_pow(c, {S, j1, ns}, U, SC, U, G, K, {{pow_fb_pair(false), j4, ncn}, {}, ct}))) return rc;
  }
  {
    PowShape S = pow_fb_pair(false);  // K^R g^m ; K^u
    S.nfb[0] = 2; S.tab[0][0] = 1; S.fb_small[0][1] = 1;
    if ((rc = launch_pow(c, {S, j2, ns}, U, SC, U, G, K, {{pow_fb_pair(true), j3, ns}, {}, ct}))) return rc;
  }
  hipLaunchKernelGGL(k_enc_order, dim3(cgrid(ns * (2 * kW / 4))), dim3(256), 0, c->stream, U + oCM * kW, d_votes,
                     (uint32_t)ns);
  HIPCHK(hipGetLastError());
  if ((rc = contest_aggregates(c, M, T, nb, U + oCT * kW, U + oCP * kW))) return rc;
  uint8_t* const want_cts = const_cast<uint8_t*>(*d_cts);
  uint8_t* const want_rp = const_cast<uint8_t*>(*d_rproof);
  uint8_t* const want_cp = const_cast<uint8_t*>(*d_cproof);
  if ((rc = ws_get(c, set ? W_EB0 : W_BE0, nU * 512, (void**)&UBE))) return rc;
  if (want_cts) {  // the ciphertexts (elements [oCT, oCM)) straight into the caller's buffer
    static_assert(EncryptLayout::oCT == 0, "ciphertexts lead the element space");
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
  // set 0's contest proofs get their own slot: W_TMP is the product tree's scratch, and the next
  // chunk's products may run while this chunk's proofs are still being copied back (ADVICE r01)
  if (want_cp) d_cp = want_cp;
  else if ((rc = ws_get(c, set ? W_EB2 : W_EA2, ncn * 64 + 64, (void**)&d_cp))) return rc;
  hipLaunchKernelGGL(k_enc_finish, dim3(cgrid(ns)), dim3(256), 0, c->stream, c->d_q, d_votes, SC, CH, (uint32_t)ns,
                     d_rp, c->resp_plus);
  hipLaunchKernelGGL(k_response, dim3(cgrid(ncn)), dim3(256), 0, c->stream, c->d_q, SC + V.off_cn * 32, CHC,
                     SC + V.off_rs * 32, 32u, (uint32_t)ncn, d_cp, c->resp_plus);
  HIPCHK(hipGetLastError());
  *d_cts = CT_BE;
  *d_rproof = d_rp;
  *d_cproof = d_cp;
  return EG_OK;
}

// Ballots are encrypted in the verifier's chunks (ballot_chunk: 16,384 ballots for the configs'
// manifests): the device working set is ~184 KB per 4x(5+1) ballot, so a 1M-ballot batch
// (configs[2]) runs in 1.7 GB chunks instead of one ~180 GB element space.  Output is
// independent of the chunking (nonces injected).  Both drivers run under the caller's lock,
// after its argument checks and use_key_locked.
// Host pointers, a software pipeline: chunk k computes on the ctx stream while chunk k-1's
// outputs go back on the copy stream (two output sets; a pageable D2H blocks the host, so it is
// issued only after chunk k is enqueued).  The votes go up once for the whole batch.
static int encrypt_host_locked(eg_ctx* c, const ManShape& M, const uint8_t* qbar_be, size_t nb, const uint8_t* votes,
                               const uint8_t* sel_nonces, const uint8_t* contest_nonces, uint8_t* cts,
                               uint8_t* rproof, uint8_t* cproof) {
  int rc;
  HIPCHK(hipMemcpyAsync(c->d_qbar, qbar_be, 32, hipMemcpyHostToDevice, c->stream));
  if ((rc = ensure_copy_stream(c))) return rc;
  const size_t nc = M.nc, nsel = M.nsel, chunk = host_chunk(nb, nsel);
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
    if ((rc = encrypt_chunk_locked(c, M, n, d_votes + b0 * nsel, sel_nonces + b0 * nsel * 128,
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

// device pointers in and out: the kernels write the caller's device buffers directly
static int encrypt_dev_locked(eg_ctx* c, const ManShape& M, const uint8_t* qbar_be, size_t nb, const uint8_t* d_votes,
                              const uint8_t* d_sel_nonces, const uint8_t* d_contest_nonces, uint8_t* d_cts,
                              uint8_t* d_rproof, uint8_t* d_cproof) {
  int rc;
  const size_t nc = M.nc, nsel = M.nsel, chunk = ballot_chunk(nsel);
  HIPCHK(hipMemcpyAsync(c->d_qbar, qbar_be, 32, hipMemcpyHostToDevice, c->stream));
  size_t k = 0;
  for (size_t b0 = 0; b0 < nb; b0 += chunk, ++k) {
    const size_t n = std::min(chunk, nb - b0);
    const uint8_t *o_cts = d_cts + b0 * nsel * 1024, *o_rp = d_rproof + b0 * nsel * 128,
                  *o_cp = d_cproof + b0 * nc * 64;
    if ((rc = encrypt_chunk_locked(c, M, n, d_votes + b0 * nsel, d_sel_nonces + b0 * nsel * 128,
                                   d_contest_nonces + b0 * nc * 32, true, (int)(k & 1), &o_cts, &o_rp, &o_cp)))
      return rc;
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  return EG_OK;
}

extern "C" int eg_encrypt_ballots(eg_ctx* c, const uint8_t K_be[512], const uint8_t qbar_be[32], size_t nb, size_t nc,
                                  size_t spc, const uint8_t* votes, const uint8_t* sel_nonces,
                                  const uint8_t* contest_nonces, uint8_t* cts, uint8_t* rproof, uint8_t* cproof) {
  if (!c || !K_be || !qbar_be || (nb && (!votes || !sel_nonces || !contest_nonces || !cts || !rproof || !cproof)))
    return fail(EG_ERR_ARG, "null argument");
  if (!nb) return EG_OK;
  if (!manifest_ok(nc, spc)) return fail(EG_ERR_ARG, "bad manifest shape");
  const ManShape M = uniform_shape(nc, spc, 0, 0);
  Locked L(c);
  int rc;
  if ((rc = use_key_locked(c, K_be))) return rc;
  return encrypt_host_locked(c, M, qbar_be, nb, votes, sel_nonces, contest_nonces, cts, rproof, cproof);
}

extern "C" int eg_encrypt_ballots_dev(eg_ctx* c, const uint8_t K_be[512], const uint8_t qbar_be[32], size_t nb,
                                      size_t nc, size_t spc, const uint8_t* d_votes, const uint8_t* d_sel_nonces,
                                      const uint8_t* d_contest_nonces, uint8_t* d_cts, uint8_t* d_rproof,
                                      uint8_t* d_cproof) {
  if (!c || !K_be || !qbar_be ||
      (nb && (!d_votes || !d_sel_nonces || !d_contest_nonces || !d_cts || !d_rproof || !d_cproof)))
    return fail(EG_ERR_ARG, "null argument");
  if (!nb) return EG_OK;
  if (!manifest_ok(nc, spc)) return fail(EG_ERR_ARG, "bad manifest shape");
  const ManShape M = uniform_shape(nc, spc, 0, 0);
  Locked L(c);
  int rc;
  if ((rc = use_key_locked(c, K_be))) return rc;
  return encrypt_dev_locked(c, M, qbar_be, nb, d_votes, d_sel_nonces, d_contest_nonces, d_cts, d_rproof, d_cproof);
}

// ---------------------------------------------------------------------------------
// trustee shares
// ---------------------------------------------------------------------------------
// Comb subset table of g (the 32 products of y_k = g^(2^(52k))), built once per ctx by one
// comb job with no outputs and kept for the trustee's constant-time a = g^u.
static int g_comb_table(eg_ctx* c, const uint32_t** out) {
  if (!c->d_gcomb) {
    uint32_t *d_g = nullptr, *tab = nullptr;
    auto build = [&]() -> int {
      int rc = import_one(c, c->g_be, &d_g);
      if (rc) return rc;
      // a workgroup's idle groups recompute job 0 into their own table slots: room for all of them
      HIPCHK(hipMalloc(&tab, (size_t)kGroupsPerBlock * (1 << kCombH) * kW * 4));
      auto J = new_jobs(1);
      J[0].base = 0;
      // no output: only the comb's precompute runs
      PowShape S = pow_var(0);
      S.comb = 1;
      const FbTab G = c->gtab->tab();
      // the job's subset table is written straight into `tab` (its scratch, job 0 of the launch)
      PowOpts o;
      o.scratch = tab;
      if ((rc = launch_pow_jobs(c, W_JOBS, S, J, d_g, nullptr, nullptr, G, G, o))) return rc;
      HIPCHK(hipStreamSynchronize(c->stream));
      return EG_OK;
    };
    const int rc = build();
    if (d_g) hipFree(d_g);
    if (rc) {
      if (tab) hipFree(tab);
      return rc;
    }
    c->d_gcomb = tab;
  }
  *out = c->d_gcomb;
  return EG_OK;
}

// The trustee's launch, under k_pow<F, true> (fixed schedule, every table read a masked scan of
// the column block's whole table: 16 entries for the pair's 4-row comb, 32 for g's shared table),
// the only place the secret share and the proof nonces go.  E: the imported pads, pad i at element
// i * pad_stride; SC: the scalars [secret][nonce x n]; gc: g's shared comb table.  O, 3 per item:
//   O[3 i] = pad^secret, O[3 i + 2] = pad^nonce   one comb per pad, shared by both exponents
//   O[3 i + 1] = g^nonce                          from gc: the short jobs fill the pair launch's tail
static int trustee_pair_launch(eg_ctx* c, const uint32_t* gc, const uint32_t* E, size_t pad_stride, const uint8_t* SC,
                               size_t n, uint32_t* O) {
  int rc;
  auto JA = new_jobs(n), JB = new_jobs(n);
  for (size_t i = 0; i < n; ++i) {
    PowJob& a = JA[i];
    a.base = (uint32_t)(i * pad_stride); a.exp[0] = 0; a.exp[1] = (uint32_t)(1 + i);
    a.out[0] = (uint32_t)(i * 3); a.out[1] = (uint32_t)(i * 3 + 2);
    PowJob& b = JB[i];
    b.base = 0; b.exp[0] = (uint32_t)(1 + i); b.out[0] = (uint32_t)(i * 3 + 1);
  }
  const uint32_t *ja, *jb;
  if ((rc = upload_jobs(c, W_JOBS, JA, &ja)) || (rc = upload_jobs(c, W_H1, JB, &jb))) return rc;
  const FbTab G = c->gtab->tab();
  PowOpts o;
  o.tail = PowPop{pow_shared_comb(), jb, n};
  o.tail.ctab = gc;
  o.ct = true;
  return launch_pow(c, {pow_ct_pair(c->ct_rows), ja, n}, E, SC, O, G, G, o);
}

extern "C" int eg_trustee_decrypt_batch(eg_ctx* c, const uint8_t secret_be[32], const uint8_t qbar_be[32],
                                        const uint8_t* texts, const uint8_t* nonces, size_t n, uint8_t* out_M,
                                        uint8_t* out_proof) {
  if (!c || !secret_be || !qbar_be || (n && (!texts || !nonces || !out_M || !out_proof)))
    return fail(EG_ERR_ARG, "null argument");
  if (!n) return EG_OK;
  if (n > kMaxBatch / 2) return fail(EG_ERR_ARG, "batch too large");
  Locked L(c);
  int rc;
  // g's shared comb table first: building it (once per ctx) runs its own job through the
  // W_JOBS / W_SCR workspaces, which this batch's jobs reuse below
  const uint32_t* gc = nullptr;
  if ((rc = g_comb_table(c, &gc))) return rc;
  // EG_PREIMAGE_WITH_KEY hashes the guardian's public key K_i = g^s (the recovery key g^P_l(x_i) of a
  // compensated share): one more job on g's shared comb table, constant-time like every other use of
  // the secret (k_pow<F, true> below), written into W_KBE before this batch takes the workspaces
  uint8_t* d_Ki = nullptr;
  if (c->pre_order == EG_PREIMAGE_WITH_KEY) {
    uint8_t* d_s = nullptr;
    uint32_t* d_o = nullptr;
    auto JK = new_jobs(1);
    JK[0].exp[0] = 0;  // the secret (row 0 of d_s)
    JK[0].out[0] = 0;
    PowPop PK{pow_shared_comb(), nullptr, 1};
    PK.ctab = gc;
    const FbTab G0 = c->gtab->tab();
    if ((rc = upload(c, W_SCAL, secret_be, 32, (void**)&d_s)) || (rc = ws_get(c, W_E1, kW * 4, (void**)&d_o)) ||
        (rc = upload_jobs(c, W_JOBS, JK, &PK.jobs)) || (rc = launch_pow(c, PK, nullptr, d_s, d_o, G0, G0, pow_ct(true))) ||
        (rc = ws_get(c, W_KBE, 512, (void**)&d_Ki)) || (rc = launch_export(c, d_o, 1, d_Ki)))
      return rc;
    HIPCHK(hipStreamSynchronize(c->stream));  // the batch below may grow (reallocate) the slots it used
  }
  HIPCHK(hipMemcpyAsync(c->d_qbar, qbar_be, 32, hipMemcpyHostToDevice, c->stream));
  uint8_t *d_t = nullptr, *SC = nullptr, *OBE = nullptr, *CH = nullptr, *PR = nullptr;
  uint32_t *E = nullptr, *O = nullptr;
  if ((rc = upload(c, W_H0, texts, n * 1024, (void**)&d_t))) return rc;
  if ((rc = ws_get(c, W_SCAL, (n + 1) * 32, (void**)&SC))) return rc;
  HIPCHK(hipMemcpyAsync(SC, secret_be, 32, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(SC + 32, nonces, n * 32, hipMemcpyHostToDevice, c->stream));
  if ((rc = ws_get(c, W_E0, n * 2 * kW * 4, (void**)&E))) return rc;
  if ((rc = launch_import(c, d_t, n * 2, E, nullptr))) return rc;
  if ((rc = ws_get(c, W_E1, n * 3 * kW * 4, (void**)&O))) return rc;
  // M = pad^s, a = g^u, b = pad^u of the share s (or P_l(x_i)) and the proof nonces u
  if ((rc = trustee_pair_launch(c, gc, E, 2, SC, n, O))) return rc;
  if ((rc = ws_get(c, W_BE0, n * 3 * 512, (void**)&OBE))) return rc;
  if ((rc = launch_export(c, O, n * 3, OBE))) return rc;
  if ((rc = ws_get(c, W_OK0, n * 32, (void**)&CH))) return rc;
  if ((rc = launch_hash(c, (uint32_t)n,
                        preimage(c, {HashSrc{d_t, 512, 1024}, HashSrc{d_t + 512, 512, 1024}},
                                 {HashSrc{OBE + 512, 512, 1536}, HashSrc{OBE + 1024, 512, 1536}},
                                 HashSrc{d_Ki, 512, 0}, {HashSrc{OBE, 512, 1536}}),
                        nullptr, 0, 0, kNone, nullptr, nullptr, 0, nullptr, CH)))
    return rc;
  if ((rc = ws_get(c, W_OK1, n * 64, (void**)&PR))) return rc;
  hipLaunchKernelGGL(k_response, dim3(cgrid(n)), dim3(256), 0, c->stream, c->d_q, SC + 32, CH, SC, 0u, (uint32_t)n, PR,
                     c->resp_plus);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy2DAsync(out_M, 512, OBE, 1536, 512, n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(out_proof, PR, n * 64, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return EG_OK;
}

// Fixed-base table of one guardian key K_i (w = 12: 22 windows, 57 MB), cached per ctx for the
// mediator's per-trustee share batches.  Building it costs ~0.1 M Montgomery ops plus a
// 264-step squaring chain, so only batches of >= kShareTableMin shares use it.
static constexpr size_t kShareTableMin = 8192;
static constexpr size_t kShareTableCache = 8;
static int share_key_table(eg_ctx* c, const uint8_t K_be[512], eg_fixed_base** out) {
  for (size_t i = 0; i < c->share_keys.size(); ++i)
    if (std::memcmp(c->share_keys[i].first.data(), K_be, 512) == 0) {
      std::rotate(c->share_keys.begin(), c->share_keys.begin() + i, c->share_keys.begin() + i + 1);
      *out = c->share_keys.front().second;
      return EG_OK;
    }
  eg_fixed_base* fb = nullptr;
  int rc = fb_create_locked(c, K_be, 12, &fb);
  if (rc) return rc;
  if (c->share_keys.size() >= kShareTableCache) {
    HIPCHK(hipStreamSynchronize(c->stream));
    eg_fixed_base_destroy(c->share_keys.back().second);
    c->share_keys.pop_back();
  }
  std::array<uint8_t, 512> key;
  std::memcpy(key.data(), K_be, 512);
  c->share_keys.insert(c->share_keys.begin(), {key, fb});
  *out = fb;
  return EG_OK;
}

// The commitments a Chaum-Pedersen proof (c, v) of M = A^x under X = g^x answers for:
//   a = g^v X^c,  b = A^v M^c
// for n items j = t k + i (text t, key i; k = 1: one key per item or one for all), recomputed
// from imported elements E and 32-byte scalars SC into O and exported to OBE.
struct CpLayout {
  size_t n, k;
  uint32_t eX, nX;    // X_j = element eX + j % nX (unused with tables)
  uint32_t eA, eM;    // text t's (A, B) = elements eA + 2 t, + 1;  M_j = element eM + j
  uint32_t sC, sV, ds;  // c_j = scalar sC + ds j, v_j = scalar sV + ds j
  uint32_t sNeg;      // kNone, or -c_j = scalar sNeg + j, which then stands in c_j's place
  uint32_t so;        // a_j -> output so j, b_j -> so j + 1; the first so n outputs are exported
  uint32_t oT, dT;    // the factors A^v, M^c of b_j -> outputs oT + dT j, + 1
  // none: X_j is a variable base.  Else k radix tables, key i's X from tabs[i] next to g's: the
  // jobs of a are key-major and every table takes one launch (k = 1: one table, one launch)
  std::vector<FbTab> tabs;
};
static int cp_recompute(eg_ctx* c, const CpLayout& L, const uint32_t* E, const uint8_t* SC, uint32_t* O, uint8_t* OBE) {
  int rc;
  const size_t n = L.n, k = L.k, m = n / k;
  const bool tabs = !L.tabs.empty();
  if (tabs ? L.tabs.size() != k : !L.nX) return fail(EG_ERR_ARG, "Chaum-Pedersen layout: k tables, or nX variable bases");
  auto JA = new_jobs(n), JB = new_jobs(n), JC = new_jobs(n);
  for (size_t j = 0; j < n; ++j) {
    const size_t t = j / k, i = j % k;
    const uint32_t vv = L.sV + L.ds * (uint32_t)j, cc = L.sNeg != kNone ? L.sNeg + (uint32_t)j : L.sC + L.ds * (uint32_t)j;
    PowJob& a = JA[tabs ? i * m + t : j];  // a = X^c g^v
    a.out[0] = L.so * (uint32_t)j; a.fb[0][0] = vv;
    if (tabs) a.fb[0][1] = cc;
    else a.base = L.eX + (uint32_t)(j % L.nX), a.exp[0] = cc;
    PowJob& b = JB[j];  // A^v
    b.base = L.eA + 2 * (uint32_t)t; b.exp[0] = vv; b.out[0] = L.oT + L.dT * (uint32_t)j;
    PowJob& d = JC[j];  // M^c
    d.base = L.eM + (uint32_t)j; d.exp[0] = cc; d.out[0] = L.oT + L.dT * (uint32_t)j + 1;
  }
  const uint32_t *ja, *jb, *jc;
  if ((rc = upload_jobs(c, W_JOBS, JA, &ja)) || (rc = upload_jobs(c, W_H1, JB, &jb)) ||
      (rc = upload_jobs(c, W_H2, JC, &jc)))
    return rc;
  const FbTab G = c->gtab->tab();
  if (tabs) {  // g^v (fb0) * X^c (fb1)
    const PowPop A{pow_two_table(), ja, n};
    for (size_t i = 0; i < k; ++i)
      if ((rc = launch_pow(c, A.part(i * m, m), E, SC, O, G, L.tabs[i]))) return rc;
  } else if ((rc = launch_pow(c, {pow_var(1, 32, 1), ja, n}, E, SC, O, G, G))) {
    return rc;
  }
  if ((rc = launch_pow(c, {pow_var(), jb, n}, E, SC, O, G, G))) return rc;
  if ((rc = launch_pow(c, {pow_var(), jc, n}, E, SC, O, G, G))) return rc;
  LAUNCH_F(c, k_mul, dim3(grid_for(n)), c->d, O + L.oT * kW, L.dT, O + (L.oT + 1) * kW, L.dT, (uint32_t)n, O + kW, L.so);
  HIPCHK(hipGetLastError());
  return launch_export(c, O, n * L.so, OBE);
}

extern "C" int eg_verify_shares(eg_ctx* c, const uint8_t qbar_be[32], const uint8_t* Ki_be, const uint8_t* texts,
                                const uint8_t* M_be, const uint8_t* proof, size_t n, uint8_t* ok) {
  if (!c || !qbar_be || (n && (!Ki_be || !texts || !M_be || !proof || !ok))) return fail(EG_ERR_ARG, "null argument");
  if (!n) return EG_OK;
  if (n > kMaxBatch / 4) return fail(EG_ERR_ARG, "batch too large");
  Locked L(c);
  int rc;
  HIPCHK(hipMemcpyAsync(c->d_qbar, qbar_be, 32, hipMemcpyHostToDevice, c->stream));
  // element input: [Ki (n)][pad,data (2n)][M (n)]
  uint8_t *IN = nullptr, *SC = nullptr, *OBE = nullptr, *OKR = nullptr, *d_ok = nullptr, *NEG = nullptr;
  uint32_t *E = nullptr, *O = nullptr;
  if ((rc = ws_get(c, W_H0, n * 4 * 512, (void**)&IN))) return rc;
  HIPCHK(hipMemcpyAsync(IN, Ki_be, n * 512, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(IN + n * 512, texts, n * 1024, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(IN + n * 1536, M_be, n * 512, hipMemcpyHostToDevice, c->stream));
  // scalars: [proofs (c, v) x n][-c x n] (the plus convention raises K_i and M to -c)
  if ((rc = ws_get(c, W_SCAL, n * 96, (void**)&SC))) return rc;
  HIPCHK(hipMemcpyAsync(SC, proof, n * 64, hipMemcpyHostToDevice, c->stream));
  if ((rc = ws_get(c, W_E0, n * 4 * kW * 4, (void**)&E))) return rc;
  if ((rc = launch_import(c, IN, n * 4, E, nullptr))) return rc;
  if ((rc = ws_get(c, W_OK0, n, (void**)&OKR))) return rc;
  NEG = SC + n * 64;
  hipLaunchKernelGGL(k_scalar_prep, dim3(cgrid(n)), dim3(256), 0, c->stream, c->d_q, SC, (uint32_t)n, 2u, 0u, 1u,
                     NEG, OKR, 0u, 0u);
  HIPCHK(hipGetLastError());
  if ((rc = ws_get(c, W_E1, n * 4 * kW * 4, (void**)&O))) return rc;
  // one K_i for the whole (large) batch -> a = g^v K_i^c from two radix tables, no window
  eg_fixed_base* kt = nullptr;
  if (n >= kShareTableMin) {
    bool same = true;
    for (size_t i = 1; i < n && same; ++i) same = std::memcmp(Ki_be, Ki_be + i * 512, 512) == 0;
    if (same && (rc = share_key_table(c, Ki_be, &kt))) return rc;
  }
  if ((rc = ws_get(c, W_BE0, n * 4 * 512, (void**)&OBE))) return rc;
  // elements [K_i (n)][pad, data (2 n)][M (n)], scalars [c, v (2 n)][-c (n): the plus convention
  // raises K_i and M to -c]; rows of four outputs (a, b, pad^v, M^c)
  CpLayout CP{};
  CP.n = n; CP.k = 1;
  CP.eX = 0; CP.nX = (uint32_t)n; CP.eA = (uint32_t)n; CP.eM = (uint32_t)(3 * n);
  CP.sC = 0; CP.sV = 1; CP.ds = 2; CP.sNeg = c->resp_plus ? (uint32_t)(2 * n) : kNone;
  CP.so = 4; CP.oT = 2; CP.dT = 4;
  if (kt) CP.tabs = {kt->tab()};
  if ((rc = cp_recompute(c, CP, E, SC, O, OBE))) return rc;
  if ((rc = ws_get(c, W_OK1, n, (void**)&d_ok))) return rc;
  const uint8_t* pads = IN + n * 512;
  if ((rc = launch_hash(c, (uint32_t)n,
                        preimage(c, {HashSrc{pads, 512, 1024}, HashSrc{pads + 512, 512, 1024}},
                                 {HashSrc{OBE, 512, 2048}, HashSrc{OBE + 512, 512, 2048}}, HashSrc{IN, 512, 512},
                                 {HashSrc{IN + n * 1536, 512, 512}}),
                        SC, 2, 0, kNone, OKR, nullptr, 0, d_ok, nullptr)))
    return rc;
  HIPCHK(hipMemcpyAsync(ok, d_ok, n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return EG_OK;
}
