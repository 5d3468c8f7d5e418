// eg_capi_prodpow.inc — multi-exponentiation out[r] = PROD_i B[r,i]^{e_i} with one exponent vector
// shared by every row (include/eg_hip_prodpow.h; DESIGN.md §17; included by eg_capi.hip after the
// other families, none of whose code or workspace slots it shares).  Kernels: eg_prodpow.hpp.  The
// entry point and its _dev twin are one body taking `bool host`: a loop over row chunks and term
// chunks, each step one staged run (eg_stage.hpp) of the chunk function on the step's terms.

static int pp_fail(const std::string& msg) { return fail(EG_ERR_ARG, "prod_pow: " + msg); }

// ---------------------------------------------------------------------------------
// the plan: the cost model the dispatcher chooses by (pure host)
// ---------------------------------------------------------------------------------
// Upper bound on the Montgomery multiplies of one row over one term chunk of m terms.
static double pp_chunk_cost(int method, int w, size_t m) {
  const double R = (double)((256 + w - 1) / w);
  if (method == EG_PRODPOW_INTERLEAVED) return w * (R - 1) + (double)m * ((double)(1u << w) - 2 + R);
  return R * (double)m + R * w * ((double)(1u << (w - 1)) - 1) + 511;
}

static size_t pp_term_chunk(int method) { return method == EG_PRODPOW_INTERLEAVED ? kPpInterTerms : kPpBucketTerms; }

// ... of one row over all n terms: the chunks' bounds and one multiply per further chunk
static double pp_row_cost(int method, int w, size_t n) {
  const size_t tc = pp_term_chunk(method);
  const size_t full = n / tc, rest = n % tc;
  const double chunks = (double)(full + (rest ? 1 : 0));
  return full * pp_chunk_cost(method, w, tc) + (rest ? pp_chunk_cost(method, w, rest) : 0) + (chunks - 1);
}

static int pp_limits(size_t rows, size_t n) {
  if (n > EG_PRODPOW_MAX_TERMS) return pp_fail("more than 2^20 terms");
  if (rows > EG_PRODPOW_MAX_ROWS) return pp_fail("more than 2^16 rows");
  if (rows * n > EG_PRODPOW_MAX_ITEMS) return pp_fail("rows * n exceeds 2^24");
  return EG_OK;
}

extern "C" int eg_prod_pow_plan(size_t rows, size_t n, int method, int window_bits, int* method_out, int* window_out,
                                double* mont_ops) {
  int rc;
  if ((rc = pp_limits(rows, n))) return rc;
  if (method < EG_PRODPOW_AUTO || method > EG_PRODPOW_BUCKETS) return pp_fail("unknown method");
  const int wmax = method == EG_PRODPOW_INTERLEAVED ? 5 : 13;
  if (window_bits < 0 || window_bits > wmax) return pp_fail("window_bits out of range for the method");
  int bm = 0, bw = 0;
  double best = 0;
  for (int mt = EG_PRODPOW_INTERLEAVED; mt <= EG_PRODPOW_BUCKETS; ++mt) {
    if (method != EG_PRODPOW_AUTO && method != mt) continue;
    const int top = mt == EG_PRODPOW_INTERLEAVED ? 5 : 13;
    for (int w = 1; w <= top; ++w) {
      if (window_bits && window_bits != w) continue;
      const double cost = n ? pp_row_cost(mt, w, n) : 0;
      if (!bm || cost < best) bm = mt, bw = w, best = cost;
    }
  }
  if (method_out) *method_out = bm;
  if (window_out) *window_out = bw;
  if (mont_ops) *mont_ops = best * (double)rows;
  return EG_OK;
}

// ---------------------------------------------------------------------------------
// chunks
// ---------------------------------------------------------------------------------
// bytes of per-row workspace of a chunk of m terms (the arrays that scale with the rows of a chunk)
constexpr size_t kPpRowBudget = (size_t)3 << 29;   // 1.5 GiB of per-row arrays per row chunk
constexpr size_t kPpSpanElems = (size_t)1 << 17;   // host mode: terms uploaded per step (64 MiB)

struct PpShape {
  int method, w;
  uint32_t nwin, seg, segmax, ch, nch;  // buckets: windows, segment length, segment slots per window, bit chunks
  size_t per_row(size_t m) const {
    const size_t E = (size_t)kW * 4;
    if (method == EG_PRODPOW_INTERLEAVED) return m * ((1u << w) - 1u) * E + E;
    const size_t bits = (size_t)nwin * w * nch;
    return (m + std::max((size_t)nwin * segmax, bits) + ((size_t)nwin << w) + (size_t)nwin * w + 1) * E;
  }
};

static PpShape pp_shape(int method, int w, size_t m) {
  PpShape S{};
  S.method = method;
  S.w = w;
  if (method == EG_PRODPOW_BUCKETS) {
    S.nwin = (256u + w - 1u) / w;
    S.seg = pp_segment((uint32_t)m);
    S.segmax = (uint32_t)std::min<size_t>(m, (m + S.seg - 1) / S.seg + ((size_t)1 << w) - 1);
    S.ch = 1u << (w / 2);  // of the 2^(w-1) buckets of a bit: ch * nch = 2^(w-1), both powers of two
    S.nch = (1u << (w - 1)) / S.ch;
  }
  return S;
}

// One chunk on device pointers (the caller holds the lock): rows x m terms at d_bases with the
// call's strides, m exponents at d_exps; the product goes into (first) or is multiplied into the
// rows' accumulators in W_PP_ACC.
static int pp_chunk_locked(eg_ctx* c, const PpShape& S, const uint8_t* d_bases, size_t rs, size_t ts,
                           const uint8_t* d_exps, size_t rows, size_t m, bool first) {
  int rc;
  const size_t E = (size_t)kW * 4;
  const uint32_t R = (uint32_t)rows, M = (uint32_t)m;
  uint32_t* acc = nullptr;
  if ((rc = ws_get(c, W_PP_ACC, rows * E, (void**)&acc))) return rc;
  if (S.method == EG_PRODPOW_INTERLEAVED) {
    const uint32_t tw = (1u << S.w) - 1u;
    uint32_t* tab = nullptr;
    if ((rc = ws_get(c, W_PP_E, rows * m * tw * E, (void**)&tab))) return rc;
    LAUNCH_F(c, k_pp_import, dim3(grid_for(rows * m)), c->d, d_bases, (uint64_t)rs, (uint64_t)ts, R, M, tw, tab);
    HIPCHK(hipGetLastError());
    LAUNCH_F(c, k_pp_inter, dim3(grid_for(rows)), c->d, tab, d_exps, R, M, (uint32_t)S.w, first ? 1u : 0u, acc);
    HIPCHK(hipGetLastError());
    return EG_OK;
  }
  const uint32_t cb = (uint32_t)S.w, W = S.nwin;
  const size_t WB = (size_t)W << cb;
  uint32_t *el = nullptr, *sort = nullptr, *part = nullptr, *bk = nullptr, *Q = nullptr;
  if ((rc = ws_get(c, W_PP_E, rows * m * E, (void**)&el))) return rc;
  // cnt, fill (zeroed together), start: W 2^c each; segoff: W (2^c + 1); perm: W m
  if ((rc = ws_get(c, W_PP_SORT, (3 * WB + (WB + W) + (size_t)W * m) * 4, (void**)&sort))) return rc;
  uint32_t *cnt = sort, *fill = cnt + WB, *start = fill + WB, *segoff = start + WB, *perm = segoff + WB + W;
  const size_t nbits = (size_t)rows * W * cb;
  if ((rc = ws_get(c, W_PP_PART, rows * std::max((size_t)W * S.segmax, (size_t)W * cb * S.nch) * E, (void**)&part)))
    return rc;
  if ((rc = ws_get(c, W_PP_BK, rows * WB * E, (void**)&bk))) return rc;
  if ((rc = ws_get(c, W_PP_Q, nbits * E, (void**)&Q))) return rc;
  LAUNCH_F(c, k_pp_import, dim3(grid_for(rows * m)), c->d, d_bases, (uint64_t)rs, (uint64_t)ts, R, M, 1u, el);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemsetAsync(cnt, 0, 2 * WB * 4, c->stream));
  hipLaunchKernelGGL(k_pp_hist, dim3(cgrid((size_t)W * m)), dim3(256), 0, c->stream, d_exps, M, cb, W, cnt);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_pp_scan, dim3(W), dim3(256), 0, c->stream, cnt, cb, S.seg, start, segoff);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_pp_scatter, dim3(cgrid((size_t)W * m)), dim3(256), 0, c->stream, d_exps, M, cb, W, start, fill,
                     perm);
  HIPCHK(hipGetLastError());
  LAUNCH_F(c, k_pp_seg, dim3(grid_for((size_t)W * S.segmax * rows)), c->d, el, cnt, start, segoff, perm, R, M, cb,
           S.seg, S.segmax, W, part);
  HIPCHK(hipGetLastError());
  LAUNCH_F(c, k_pp_bucket, dim3(grid_for(WB * rows)), c->d, part, segoff, R, cb, S.segmax, W, bk);
  HIPCHK(hipGetLastError());
  // the segment products are dead: their slot takes the bit products' partial runs
  LAUNCH_F(c, k_pp_bits, dim3(grid_for(nbits * S.nch)), c->d, bk, R, cb, W, S.ch, S.nch, S.nch == 1 ? Q : part);
  HIPCHK(hipGetLastError());
  if (S.nch > 1 && (rc = run_prod(c, part, GroupMap{1, 1, 0, 0, S.nch}, nbits, S.nch, 1, Q))) return rc;
  LAUNCH_F(c, k_pp_horner, dim3(grid_for(rows)), c->d, Q, R, W * cb, first ? 1u : 0u, acc);
  HIPCHK(hipGetLastError());
  return EG_OK;
}

// out[r] = 1 for rows elements (the caller holds the lock)
static int pp_ones(eg_ctx* c, bool host, uint8_t* out, size_t rows) {
  if (host) {
    std::memset(out, 0, rows * 512);
    for (size_t r = 0; r < rows; ++r) out[r * 512 + 511] = 1;
    return EG_OK;
  }
  HIPCHK(hipMemsetAsync(out, 0, rows * 512, c->stream));
  HIPCHK(hipMemset2DAsync(out + 511, 512, 1, 1, rows, c->stream));
  return EG_OK;
}

static int pp_run(eg_ctx* c, bool host, const uint8_t* bases, size_t rs, size_t ts, const uint8_t* exps, size_t rows,
                  size_t n, int method, int window_bits, uint8_t* out) {
  int rc;
  if (!c) return pp_fail("null context");
  if ((rc = pp_limits(rows, n))) return rc;
  if (rows && !out) return pp_fail("null output");
  if (rows && n && (!bases || !exps)) return pp_fail("null bases or exponents");
  if ((rows > 1 && !rs) || (n > 1 && !ts)) return pp_fail("a stride of 0 over more than one element");
  if (!host && !aligned16({bases, exps, out})) return pp_fail("device pointer not 16-byte aligned");
  int mt = 0, w = 0;
  if ((rc = eg_prod_pow_plan(rows, n, method, window_bits, &mt, &w, nullptr))) return rc;
  Locked lk(c);
  if (c->ct_pow)
    return fail(EG_ERR_STATE, "prod_pow is variable time and eg_ctx_set_ct_pow is on: use eg_powp_batch and "
                              "eg_prod_reduce for secret exponents");
  if (!rows) return EG_OK;
  if (!n) return pp_ones(c, host, out, rows);
  // term chunks of the method's size (the plan counts them); row chunks within the per-row budget,
  // in host mode also within the staging bound
  const size_t tc = std::min(n, pp_term_chunk(mt));
  size_t rcn = std::max<size_t>(1, std::min(rows, kPpRowBudget / pp_shape(mt, w, tc).per_row(tc)));
  if (host) rcn = std::max<size_t>(1, std::min(rcn, kPpSpanElems / tc));
  std::vector<uint8_t> pack;  // host mode: a step's terms, row-major, when the caller's are not
  for (size_t r0 = 0; r0 < rows; r0 += rcn) {
    const size_t rr = std::min(rcn, rows - r0);
    for (size_t t0 = 0; t0 < n; t0 += tc) {
      const size_t m = std::min(tc, n - t0);
      const bool last = t0 + m == n;
      const PpShape S = pp_shape(mt, w, m);
      const uint8_t* b = bases + (r0 * rs + t0 * ts) * 512;
      size_t brs = rs, bts = ts;
      if (host && !((ts == 1 || m == 1) && (rr == 1 || rs == m))) {
        pack.resize(rr * m * 512);
        for (size_t r = 0; r < rr; ++r)
          for (size_t i = 0; i < m; ++i) std::memcpy(&pack[(r * m + i) * 512], b + (r * rs + i * ts) * 512, 512);
        b = pack.data();
        brs = m, bts = 1;
      }
      const uint8_t* e = exps + t0 * 32;
      uint8_t* o = last ? out + r0 * 512 : nullptr;
      Stage st(c, host, 1, 1);
      st.in(b, (host ? rr * m : 1) * 512);  // device mode binds the pointer: the stride is not used
      st.in(e, m * 32);
      st.out(o, rr * 512);
      rc = st.run([&](size_t) {
        int rc2;
        if ((rc2 = pp_chunk_locked(c, S, b, brs, bts, e, rr, m, t0 == 0))) return rc2;
        if (!last) return (int)EG_OK;
        uint32_t* acc = nullptr;
        if ((rc2 = ws_get(c, W_PP_ACC, rr * (size_t)kW * 4, (void**)&acc))) return rc2;
        return launch_export(c, acc, rr, o);
      });
      if (rc) return rc;
    }
  }
  return EG_OK;
}

extern "C" int eg_prod_pow_dev(eg_ctx* c, const uint8_t* d_bases_be, size_t row_stride, size_t term_stride,
                               const uint8_t* d_exps_be, size_t rows, size_t n, int method, int window_bits,
                               uint8_t* d_out_be) {
  return pp_run(c, false, d_bases_be, row_stride, term_stride, d_exps_be, rows, n, method, window_bits, d_out_be);
}

extern "C" int eg_prod_pow(eg_ctx* c, const uint8_t* bases_be, size_t row_stride, size_t term_stride,
                           const uint8_t* exps_be, size_t rows, size_t n, int method, int window_bits,
                           uint8_t* out_be) {
  return pp_run(c, true, bases_be, row_stride, term_stride, exps_be, rows, n, method, window_bits, out_be);
}
