// eg_capi_decode.inc — decoding decrypted texts on the device: the batch inverse and the discrete
// logarithm to the base g (include/eg_hip_decode.h; DESIGN.md §20; included by eg_capi.hip after
// eg_capi_shuffle.inc: the job helpers are eg_capi_ballot.inc's).  Kernels: eg_decode.hpp, k_pow,
// k_import, k_export, k_mul.  Each entry point and its _dev twin are one body taking `bool host`;
// the host variants upload the whole arrays into the family's own workspace slots.

static int dc_fail(const std::string& msg) { return fail(EG_ERR_ARG, "decode: " + msg); }

// ---------------------------------------------------------------------------------
// the plan (pure host)
// ---------------------------------------------------------------------------------
constexpr double kDcPowOps = 5129;  // a^(p-2) on the 4-bit window: 14 for the table, 1,023 x (4 + 1)

// the inversion of n elements: segment length, levels, elements left for a^(p-2)
struct DcInv {
  uint32_t seg, levels, jobs;
};
static DcInv dc_inv_plan(size_t n) {
  DcInv v{4, 0, 0};
  while ((size_t)v.seg * EG_DECODE_STOP < n && v.seg < 16) v.seg *= 2;
  size_t left = n;
  while (left > EG_DECODE_STOP) {
    left = (left + v.seg - 1) / v.seg;
    ++v.levels;
  }
  v.jobs = (uint32_t)left;
  return v;
}

static uint64_t dc_isqrt(uint64_t x) {
  uint64_t r = 0;  // x <= 2^32: the root has at most 17 bits
  for (uint64_t bit = (uint64_t)1 << 16; bit; bit >>= 1)
    if ((r + bit) * (r + bit) <= x) r += bit;
  return r;
}

static int dc_limits(size_t n, uint64_t max_count) {
  if (n > EG_DECODE_MAX_TEXTS) return dc_fail("more than 2^24 elements");
  if (max_count > EG_DECODE_MAX_COUNT) return dc_fail("max_count exceeds 2^32");
  return EG_OK;
}

extern "C" int eg_decode_plan(size_t n, uint64_t max_count, uint32_t* seg_len, uint32_t* levels, uint32_t* pow_jobs,
                              uint32_t* m_out, uint32_t* slots_out, double* load, double* inv_ops, double* mont_ops) {
  int rc;
  if ((rc = dc_limits(n, max_count))) return rc;
  const DcInv v = dc_inv_plan(n);
  const uint32_t m = (uint32_t)dc_isqrt(max_count) + 1;
  uint32_t slots = 16;
  while (slots < 2 * (uint64_t)m) slots *= 2;
  const double inv = 3.0 * (double)(n - v.jobs) + kDcPowOps * v.jobs;
  if (seg_len) *seg_len = v.seg;
  if (levels) *levels = v.levels;
  if (pow_jobs) *pow_jobs = v.jobs;
  if (m_out) *m_out = m;
  if (slots_out) *slots_out = slots;
  if (load) *load = (double)m / slots;
  if (inv_ops) *inv_ops = inv;
  if (mont_ops) *mont_ops = inv + (double)n + (double)n * m;
  return EG_OK;
}

// ---------------------------------------------------------------------------------
// the batch inverse
// ---------------------------------------------------------------------------------
// X[i] <- X[i]^-1 for n Montgomery elements in HBM, 0 -> 0 (the caller holds the lock).  Fully
// asynchronous; workspace: W_DC_CONST, W_DC_Z, W_DC_P, W_DC_LV, W_DC_O, W_DC_JOBS.
static int dc_invert_locked(eg_ctx* c, uint32_t* X, size_t n) {
  int rc;
  const size_t E = (size_t)kW * 4;
  const DcInv v = dc_inv_plan(n);
  // the shared exponent p - 2: p is odd and > 2, so the subtraction ends in the low bytes
  std::array<uint8_t, 512> e;
  std::memcpy(e.data(), c->p_be, 512);
  for (int i = 511, borrow = 2; borrow && i >= 0; --i) {
    const int b = e[i] - borrow;
    e[i] = (uint8_t)b;
    borrow = b < 0 ? 1 : 0;
  }
  uint8_t* d_exp = nullptr;
  if ((rc = upload(c, W_DC_CONST, e.data(), 512, (void**)&d_exp))) return rc;
  // level l inverts lv[l].n elements at lv[l].X with prefix products at lv[l].P; level 0 is the caller's
  struct Level {
    uint32_t *X, *P;
    size_t n;
  };
  std::vector<Level> lv(v.levels + 1);
  lv[0] = Level{X, nullptr, n};
  size_t lower = 0;
  for (uint32_t l = 1; l <= v.levels; ++l) {
    lv[l].n = (lv[l - 1].n + v.seg - 1) / v.seg;
    lower += 2 * lv[l].n;
  }
  uint8_t* zero = nullptr;
  if (v.levels) {
    uint32_t* at = nullptr;
    if ((rc = ws_get(c, W_DC_Z, n, (void**)&zero))) return rc;
    if ((rc = ws_get(c, W_DC_P, n * E, (void**)&lv[0].P))) return rc;
    if ((rc = ws_get(c, W_DC_LV, lower * E, (void**)&at))) return rc;
    for (uint32_t l = 1; l <= v.levels; ++l) {
      lv[l].X = at;
      lv[l].P = at + lv[l].n * kW;
      at += 2 * lv[l].n * kW;
    }
  }
  for (uint32_t l = 0; l < v.levels; ++l) {
    const size_t nseg = lv[l + 1].n;
    LAUNCH_F(c, k_dc_fwd, dim3(grid_for(nseg)), c->d, lv[l].X, (uint32_t)lv[l].n, v.seg, l ? nullptr : zero, lv[l].P,
             lv[l + 1].X);
    HIPCHK(hipGetLastError());
  }
  // the elements left: a^(p-2), every job reading the one 512-byte exponent (0^(p-2) = 0)
  const Level& last = lv[v.levels];
  uint32_t* O = nullptr;
  if ((rc = ws_get(c, W_DC_O, last.n * E, (void**)&O))) return rc;
  auto J = new_jobs(last.n);
  for (size_t i = 0; i < last.n; ++i) {
    PowJob& a = J[i];
    a.base = (uint32_t)i; a.exp[0] = 0; a.out[0] = (uint32_t)i;
  }
  const FbTab Gt = c->gtab->tab();
  if ((rc = launch_pow_jobs(c, W_DC_JOBS, pow_var(1, 512), J, last.X, d_exp, O, Gt, Gt))) return rc;
  if (!v.levels) {
    HIPCHK(hipMemcpyAsync(X, O, n * E, hipMemcpyDeviceToDevice, c->stream));
    return EG_OK;
  }
  for (uint32_t l = v.levels; l-- > 0;) {
    const uint32_t* tinv = l + 1 == v.levels ? O : lv[l + 1].X;
    LAUNCH_F(c, k_dc_bwd, dim3(grid_for(lv[l + 1].n)), c->d, lv[l].X, (uint32_t)lv[l].n, v.seg,
             l ? (const uint8_t*)nullptr : (const uint8_t*)zero, (const uint32_t*)lv[l].P, tinv);
    HIPCHK(hipGetLastError());
  }
  return EG_OK;
}

static int dc_inverse(eg_ctx* c, bool host, const uint8_t* a, uint8_t* out, size_t n) {
  int rc;
  if (!c) return dc_fail("null context");
  if ((rc = dc_limits(n, 0))) return rc;
  if (n && (!a || !out)) return dc_fail("null input or output");
  if (!host && !aligned16({a, out})) return dc_fail("device pointer not 16-byte aligned");
  if (!n) return EG_OK;
  Locked lk(c);
  if (c->ct_pow)
    return fail(EG_ERR_STATE, "decode: batch_inverse is variable time and eg_ctx_set_ct_pow is on: use "
                              "eg_multinv_batch for secret values");
  const size_t E = (size_t)kW * 4;
  uint8_t* d_be = nullptr;
  uint32_t* X = nullptr;
  if (host && (rc = upload(c, W_DC_BE, a, n * 512, (void**)&d_be))) return rc;
  if ((rc = ws_get(c, W_DC_X, n * E, (void**)&X))) return rc;
  if ((rc = launch_import(c, host ? d_be : a, n, X, nullptr))) return rc;  // a value >= p is reduced
  if ((rc = dc_invert_locked(c, X, n))) return rc;
  if ((rc = launch_export(c, X, n, host ? d_be : out))) return rc;  // the input bytes are dead
  if (host) {
    HIPCHK(hipMemcpyAsync(out, d_be, n * 512, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  return EG_OK;
}

extern "C" int eg_batch_inverse_dev(eg_ctx* c, const uint8_t* d_a_be, uint8_t* d_out_be, size_t n) {
  return dc_inverse(c, false, d_a_be, d_out_be, n);
}

extern "C" int eg_batch_inverse(eg_ctx* c, const uint8_t* a_be, uint8_t* out_be, size_t n) {
  return dc_inverse(c, true, a_be, out_be, n);
}

// ---------------------------------------------------------------------------------
// the table
// ---------------------------------------------------------------------------------
struct eg_decode_table {
  eg_ctx* ctx = nullptr;
  uint64_t max_count = 0;
  uint32_t m = 0, fp_bits = 64, slots = 0;
  uint32_t* d_baby = nullptr;  // m canonical baby steps, then the step g^(-m) (Montgomery form)
  uint32_t* d_j = nullptr;     // slots baby-step indices, kDcEmpty where free
  uint64_t* d_fp = nullptr;    // slots fingerprints
};

extern "C" int eg_decode_table_destroy(eg_decode_table* t) {
  if (!t) return EG_OK;
  if (t->d_baby) hipFree(t->d_baby);
  if (t->d_j) hipFree(t->d_j);
  if (t->d_fp) hipFree(t->d_fp);
  delete t;
  return EG_OK;
}

static int dc_table_build(eg_ctx* c, eg_decode_table* t) {
  int rc;
  const size_t E = (size_t)kW * 4;
  const uint32_t m = t->m;
  // the scalars 0 .. m-1 and q - m (q > m is checked by the caller)
  std::vector<uint8_t> sc((size_t)(m + 1) * 32, 0);
  for (uint32_t j = 0; j < m; ++j)
    for (int b = 0; b < 4; ++b) sc[(size_t)j * 32 + 31 - b] = (uint8_t)(j >> (8 * b));
  uint8_t* neg = &sc[(size_t)m * 32];
  std::memcpy(neg, c->q_be, 32);
  for (int i = 31, borrow = 0, b = 0; i >= 0; --i, ++b) {
    const int d = neg[i] - (b < 4 ? (int)((m >> (8 * b)) & 0xFF) : 0) - borrow;
    neg[i] = (uint8_t)d;
    borrow = d < 0 ? 1 : 0;
  }
  uint8_t* SC = nullptr;
  if ((rc = upload(c, W_DC_BE, sc.data(), sc.size(), (void**)&SC))) return rc;
  HIPCHK(hipMalloc(&t->d_baby, (size_t)(m + 1) * E));
  HIPCHK(hipMalloc(&t->d_j, (size_t)t->slots * 4));
  HIPCHK(hipMalloc(&t->d_fp, (size_t)t->slots * 8));
  auto J = new_jobs(m + 1);
  for (uint32_t j = 0; j <= m; ++j) {
    PowJob& a = J[j];
    a.fb[0][0] = j; a.out[0] = j;
  }
  const FbTab Gt = c->gtab->tab();
  if ((rc = launch_pow_jobs(c, W_DC_JOBS, pow_fb_one(), J, nullptr, SC, t->d_baby, Gt, Gt))) return rc;
  LAUNCH_F(c, k_dc_canon, dim3(grid_for(m + 1)), c->d, t->d_baby, m + 1);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemsetAsync(t->d_j, 0xFF, (size_t)t->slots * 4, c->stream));
  HIPCHK(hipMemsetAsync(t->d_fp, 0, (size_t)t->slots * 8, c->stream));
  hipLaunchKernelGGL(k_dc_insert, dim3(cgrid(m)), dim3(256), 0, c->stream, t->d_baby, m, t->fp_bits, t->slots - 1,
                     t->d_j, t->d_fp);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  return EG_OK;
}

extern "C" int eg_decode_table_create(eg_ctx* c, uint64_t max_count, int fp_bits, eg_decode_table** tab_out) {
  int rc;
  if (!c) return dc_fail("null context");
  if (!tab_out) return dc_fail("null table pointer");
  if ((rc = dc_limits(0, max_count))) return rc;
  if (fp_bits != 0 && (fp_bits < 8 || fp_bits > 64)) return dc_fail("fp_bits is 0 or in 8..64");
  *tab_out = nullptr;
  uint32_t m = 0, slots = 0;
  eg_decode_plan(0, max_count, nullptr, nullptr, nullptr, &m, &slots, nullptr, nullptr, nullptr);
  Locked lk(c);
  bool q_small = true;  // q <= m: g^(-m) would not be g^(q-m)
  for (int i = 0; i < 28; ++i) q_small &= c->q_be[i] == 0;
  if (q_small) {
    const uint32_t ql = (uint32_t)c->q_be[28] << 24 | (uint32_t)c->q_be[29] << 16 | (uint32_t)c->q_be[30] << 8 | c->q_be[31];
    if (ql <= m) return dc_fail("q is not above floor(sqrt(max_count)) + 1");
  }
  auto* t = new eg_decode_table();
  t->ctx = c;
  t->max_count = max_count;
  t->m = m;
  t->fp_bits = fp_bits ? (uint32_t)fp_bits : 64u;
  t->slots = slots;
  if ((rc = dc_table_build(c, t))) {
    eg_decode_table_destroy(t);
    return rc;
  }
  *tab_out = t;
  return EG_OK;
}

// ---------------------------------------------------------------------------------
// the decode
// ---------------------------------------------------------------------------------
static int dc_counts(eg_decode_table* t, bool host, const uint8_t* B, const uint8_t* Mb, size_t n, int64_t* counts) {
  int rc;
  if (!t) return dc_fail("null table");
  if ((rc = dc_limits(n, 0))) return rc;
  if (n && (!B || !counts)) return dc_fail("null texts or counts");
  if (!host && !aligned16({B, Mb, counts})) return dc_fail("device pointer not 16-byte aligned");
  if (!n) return EG_OK;
  eg_ctx* c = t->ctx;
  Locked lk(c);
  const size_t E = (size_t)kW * 4;
  uint8_t *d_b = nullptr, *d_m = nullptr;
  uint32_t *Y = nullptr, *X = nullptr;
  long long* d_cnt = nullptr;
  if (host) {
    if ((rc = upload(c, W_DC_BE, B, n * 512, (void**)&d_b))) return rc;
    if (Mb && (rc = upload(c, W_DC_BE2, Mb, n * 512, (void**)&d_m))) return rc;
    if ((rc = ws_get(c, W_DC_CNT, n * 8, (void**)&d_cnt))) return rc;
  }
  if ((rc = ws_get(c, W_DC_Y, n * E, (void**)&Y))) return rc;
  if ((rc = launch_import(c, host ? d_b : B, n, Y, nullptr))) return rc;
  if (Mb) {  // y = B * M^-1 (0 for M = 0)
    if ((rc = ws_get(c, W_DC_X, n * E, (void**)&X))) return rc;
    if ((rc = launch_import(c, host ? d_m : Mb, n, X, nullptr))) return rc;
    if ((rc = dc_invert_locked(c, X, n))) return rc;
    LAUNCH_F(c, k_mul, dim3(grid_for(n)), c->d, Y, 1u, X, 1u, (uint32_t)n, Y, 1u);
    HIPCHK(hipGetLastError());
  }
  LAUNCH_F(c, k_dc_giant, dim3(grid_for(n)), c->d, Y, (uint32_t)n, t->d_baby, t->m, t->max_count, t->fp_bits,
           t->slots - 1, t->d_j, t->d_fp, host ? d_cnt : reinterpret_cast<long long*>(counts));
  HIPCHK(hipGetLastError());
  if (host) {
    HIPCHK(hipMemcpyAsync(counts, d_cnt, n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  return EG_OK;
}

extern "C" int eg_decode_counts_dev(eg_decode_table* tab, const uint8_t* d_B_be, const uint8_t* d_M_be, size_t n,
                                    int64_t* d_counts) {
  return dc_counts(tab, false, d_B_be, d_M_be, n, d_counts);
}

extern "C" int eg_decode_counts(eg_decode_table* tab, const uint8_t* B_be, const uint8_t* M_be, size_t n,
                                int64_t* counts) {
  return dc_counts(tab, true, B_be, M_be, n, counts);
}
