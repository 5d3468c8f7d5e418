// eg_capi_coalesce.inc — per-element group operations behind the C ABI (included by eg_capi.hip).
//
// The reference drives the group one element at a time: upstream's ElementModP.powP / times and
// GroupContext.gPowP, and the accelerated election key's K.powP, called from 11 encryptor /
// verifier threads (RunRemoteWorkflowTest.java:140-141,179-181) on the context
// KUtils.productionGroup() injects (KUtils.java:10-12).  One 4096-bit exponentiation is ~314
// Montgomery multiplies in sequence, so a GPU call per element would leave the chip idle; instead
// every submitted element is a JOB (eg_mexp_submit: a product of bases, raised to an optional
// exponent, times up to two fixed-base powers) that joins the ctx's open batch, and a dispatcher
// thread runs the batch as ONE launch of the per-wave job kernel (eg_pow16.hip k_wave_job: one job
// per wave, every kind of job side by side) when
//   * the GPU (the ctx lock) is free and the oldest job has waited its window (counted from the end
//     of the previous dispatch for jobs that queued while it ran): by default ADAPTIVE, half as long
//     as the previous batch ran within [20 us, 100 us] (a short fixed-base batch does not wait out a
//     long exponentiation's window); exactly `window_us` when the caller set one
//     (eg_ctx_set_coalescing with window_us > 0, or EG_COALESCE_WINDOW_US), or
//   * as many jobs are pending as the previous dispatch took (the callers that were served last
//     time have all come back: a single blocking caller is served at once, 11 blocking threads
//     wait for each other at most `window_us`), or
//   * the batch holds `max_batch` jobs.
// While a batch runs, new jobs gather into the next one, so under load the batch size follows the
// arrival rate.  A batch's inputs travel in one pinned host-to-device copy and its results in one
// copy back.  Large batches of one plain kind (powP, one fixed-base table, times) keep the
// throughput layouts (the 16- or 8-lane k_pow, k_mul).  eg_*_submit returns at once with a
// ticket; eg_ticket_wait blocks until the job's batch has run, its result is in the caller's
// `out`, and returns the batch's status.  eg_*_one = submit + wait (the blocking call).

struct CoJob {
  uint32_t base, nbase;   // rows in the batch's `bases`
  uint32_t exp;           // row in `exps` or kWaveNone
  uint32_t fexp[2];       // rows in `exps` of the fixed-base terms
  eg_fixed_base* fb[2];   // nullptr: no term
  uint8_t* out;           // the caller's 512 bytes
};
struct CoBatch {
  std::vector<uint8_t> bases, exps;  // packed inputs, 512 / 32 bytes per row
  std::vector<CoJob> jobs;
  // eg_ctx_set_ct_pow as it was when the batch's jobs were SUBMITTED: a batch never mixes modes, and
  // a job submitted with the constant-time switch on runs constant-time even if the switch is turned
  // off before its batch is dispatched (ADVICE r05)
  bool ct = false;
  // completion: each batch has its own lock and condition, so a finished batch wakes only its own
  // callers (one shared condition woke every waiting thread on every batch: with hundreds of caller
  // threads that thundering herd, all queueing on the coalescer's lock, cut the per-element rate
  // 3-14x above 32-128 threads, profiles/r06c_percall_threads.json)
  std::mutex dm;
  std::condition_variable dcv;
  bool done = false;
  int rc = EG_OK;
  std::string err;
};

struct Coalescer {
  std::mutex m;
  std::condition_variable cv_work;
  std::shared_ptr<CoBatch> open;
  std::chrono::steady_clock::time_point first{};  // arrival of the oldest pending job
  size_t max_batch = 16384;
  uint32_t window_us = 100;
  bool window_fixed = false;  // window_us set by the caller: honoured exactly (no adaptive wait)
  // batches closed early because a job came in the other constant-time mode: dispatched first, in order
  std::deque<std::shared_ptr<CoBatch>> sealed;
  size_t last_n = 1;  // jobs the previous dispatch took (its callers' return ends the wait)
  // end of the previous dispatch: the window of jobs that queued while the GPU was busy starts
  // here, not at their arrival, so the callers that batch released can still join them
  std::chrono::steady_clock::time_point last_done{};
  // how long the previous batch held the GPU: the wait for stragglers is at most half of it (short
  // fixed-base batches do not wait a long job's window), within [20 us, window_us]
  uint32_t last_dur_us = 0;
  bool stop = false;
  std::thread th;
  // EG_COALESCE_STATS=1: batch statistics printed to stderr when the dispatcher stops
  bool stats = false;
  uint64_t st_batches = 0, st_jobs = 0, st_max = 0, st_run_us = 0, st_queue_us = 0, st_sealed = 0;
  // pinned staging of the dispatcher (its thread only): inputs up, results down
  uint8_t* h_in = nullptr;
  size_t h_in_bytes = 0;
  uint8_t* h_out = nullptr;
  size_t h_out_bytes = 0;
};

struct eg_ticket {
  std::shared_ptr<CoBatch> b;
  std::shared_ptr<Coalescer> co;  // keeps the dispatcher state alive past eg_ctx_destroy
};

static int identity_pow_jobs(eg_ctx* c, size_t n, bool fbonly, const uint32_t** out);  // eg_capi.hip

// A small variable-base batch on a latency-shaped layout (eg_pow16.hip); host in, host out.
//   * up to one element per SIMD: one element per wave (k_wave_job, 48 lanes x 3 limbs);
//   * up to half a resident round of 16-lane groups (larger ones run faster on 8-lane groups):
//     the 16-lane layout, the same 4-bit window op program and identity job records as pow_host,
//     elements of 192 words.
static bool latency_shaped(const eg_ctx* c, size_t n) {
  return (c->latw && n <= c->latw_jobs) || (c->lat && n <= c->lat_jobs);
}

static int pow_latency(eg_ctx* c, const uint8_t* base_be, const uint8_t* exp_be, uint8_t* out_be, size_t n) {
  int rc;
  const bool ct = c->ct_pow != 0;
  if (c->latw && n <= c->latw_jobs) {
    uint8_t *d_base = nullptr, *d_exp = nullptr, *d_out = nullptr;
    if ((rc = upload(c, W_IN0, base_be, n * 512, (void**)&d_base))) return rc;
    if ((rc = upload(c, W_EXP, exp_be, n * 32, (void**)&d_exp))) return rc;
    if ((rc = ws_get(c, W_OUT, n * 512, (void**)&d_out))) return rc;
    std::string err;
    if (powwave_powp(c->latw, c->h.friendly != 0, ct, n <= c->r2l_max, c->stream, d_base, d_exp, d_out, n, &err))
      return fail(EG_ERR_HIP, err);
    HIPCHK(hipMemcpyAsync(out_be, d_out, n * 512, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return EG_OK;
  }
  const PowShape S = pow_var();  // pow16_powp's shape
  const FbTab G = c->gtab->tab();
  const uint32_t *sched = nullptr, *jobs = nullptr;
  uint8_t *d_base = nullptr, *d_exp = nullptr, *d_out = nullptr;
  uint32_t *el = nullptr, *ou = nullptr, *scr = nullptr;
  if ((rc = pow_schedule_dev(c, S, G, G, &sched, nullptr))) return rc;
  if ((rc = identity_pow_jobs(c, n, false, &jobs))) return rc;
  if ((rc = upload(c, W_IN0, base_be, n * 512, (void**)&d_base))) return rc;
  if ((rc = upload(c, W_EXP, exp_be, n * 32, (void**)&d_exp))) return rc;
  if ((rc = ws_get(c, W_E0, n * pow16_elem_bytes(), (void**)&el))) return rc;
  if ((rc = ws_get(c, W_E1, n * pow16_elem_bytes(), (void**)&ou))) return rc;
  if ((rc = ws_get(c, W_SCR, pow16_scratch_bytes(n), (void**)&scr))) return rc;
  if ((rc = ws_get(c, W_OUT, n * 512, (void**)&d_out))) return rc;
  std::string err;
  if (pow16_powp(c->lat, c->h.friendly != 0, ct, c->stream, sched, jobs, d_base, d_exp, d_out, n, el, ou, scr, &err))
    return fail(EG_ERR_HIP, err);
  HIPCHK(hipMemcpyAsync(out_be, d_out, n * 512, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return EG_OK;
}

// A small fixed-base batch (up to one element per SIMD) on the per-wave kernel; host in, host out.
static int fb_latency(eg_ctx* c, const FbTab& t, const uint8_t* exp_be, uint8_t* out_be, size_t n) {
  int rc;
  uint8_t *d_exp = nullptr, *d_out = nullptr;
  if ((rc = upload(c, W_EXP, exp_be, n * 32, (void**)&d_exp))) return rc;
  if ((rc = ws_get(c, W_OUT, n * 512, (void**)&d_out))) return rc;
  std::string err;
  if (powwave_fbpow(c->latw, c->h.friendly != 0, c->ct_pow != 0, c->stream, WaveTab{t.data, t.wbits, t.nwin}, d_exp,
                    d_out, n, &err))
    return fail(EG_ERR_HIP, err);
  HIPCHK(hipMemcpyAsync(out_be, d_out, n * 512, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return EG_OK;
}

static size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

static int pinned(uint8_t** p, size_t* have, size_t want) {
  if (*have >= want) return EG_OK;
  if (*p) hipHostFree(*p);
  *p = nullptr;
  *have = 0;
  want = std::max(want, (size_t)1 << 20);
  if (hipHostMalloc((void**)p, want, hipHostMallocDefault) != hipSuccess) {
    *p = nullptr;
    return fail(EG_ERR_NOMEM, "hipHostMalloc of the coalescer's staging failed");
  }
  *have = want;
  return EG_OK;
}

// One batch of mixed jobs on the per-wave kernel: the job records, the table descriptors, the
// exponents and the bases go up in ONE pinned copy, the results come back in one.  Results land in
// co->h_out (n x 512 bytes).  Caller holds the ctx lock.
static int run_wave_batch(eg_ctx* c, Coalescer* co, const CoBatch& b) {
  const size_t n = b.jobs.size();
  int rc;
  // distinct fixed-base tables of the batch (eg_ctx_set_ct_pow: their constant-time companions)
  std::vector<eg_fixed_base*> fbs;
  std::vector<WaveTab> tabs;
  std::vector<WaveJob> wj(n);
  for (size_t i = 0; i < n; ++i) {
    const CoJob& j = b.jobs[i];
    WaveJob& w = wj[i];
    w.base = j.base;
    w.nbase = j.nbase;
    w.exp = j.exp;
    w.out = (uint32_t)i;
    for (int t = 0; t < 2; ++t) {
      w.tab[t] = kWaveNone;
      w.fexp[t] = kWaveNone;
      if (!j.fb[t]) continue;
      size_t k = 0;
      while (k < fbs.size() && fbs[k] != j.fb[t]) ++k;
      if (k == fbs.size()) {
        FbTab ft = j.fb[t]->tab();
        if (c->ct_pow && (rc = ct_table_locked(c, j.fb[t], &ft))) return rc;
        fbs.push_back(j.fb[t]);
        tabs.push_back(WaveTab{ft.data, ft.wbits, ft.nwin});
      }
      w.tab[t] = (uint32_t)k;
      w.fexp[t] = j.fexp[t];
    }
  }
  const size_t o_tabs = align16(n * sizeof(WaveJob));
  const size_t o_exps = align16(o_tabs + tabs.size() * sizeof(WaveTab));
  const size_t o_bases = align16(o_exps + b.exps.size());
  const size_t total = o_bases + b.bases.size();
  if ((rc = pinned(&co->h_in, &co->h_in_bytes, total))) return rc;
  if ((rc = pinned(&co->h_out, &co->h_out_bytes, n * 512))) return rc;
  std::memcpy(co->h_in, wj.data(), n * sizeof(WaveJob));
  if (!tabs.empty()) std::memcpy(co->h_in + o_tabs, tabs.data(), tabs.size() * sizeof(WaveTab));
  if (!b.exps.empty()) std::memcpy(co->h_in + o_exps, b.exps.data(), b.exps.size());
  if (!b.bases.empty()) std::memcpy(co->h_in + o_bases, b.bases.data(), b.bases.size());
  uint8_t *d_in = nullptr, *d_out = nullptr;
  // the kernel writes its results straight into the pinned staging (host memory the GPU maps) instead of
  // a device buffer and a copy back (EG_COALESCE_ZC: "out" the default, "in" / "inout" also read the
  // inputs from it, "0" neither; profiles/r05zi_ab_percall_builds.log)
  if (c->co_zc & 1) {
    HIPCHK(hipHostGetDevicePointer((void**)&d_in, co->h_in, 0));
  } else {
    if ((rc = ws_get(c, W_IN1, total, (void**)&d_in))) return rc;
    HIPCHK(hipMemcpyAsync(d_in, co->h_in, total, hipMemcpyHostToDevice, c->stream));
  }
  if (c->co_zc & 2) {
    HIPCHK(hipHostGetDevicePointer((void**)&d_out, co->h_out, 0));
  } else if ((rc = ws_get(c, W_OUT, n * 512, (void**)&d_out))) {
    return rc;
  }
  std::string err;
  const WaveJob none{0, 0, kWaveNone, {kWaveNone, kWaveNone}, {kWaveNone, kWaveNone}, 0};
  // jobs with fixed-base terms split their windows over 4 waves (EG_WAVE_SPLIT=0: one wave per job), over 8
  // up to one job per CU when no job has a variable exponent; up to one job per CU, the variable parts run
  // right to left over the 4 waves as well (in both modes)
  bool any_fixed = false, any_exp = false;
  for (const CoJob& j : b.jobs) {
    any_fixed |= j.fb[0] != nullptr;
    any_exp |= j.nbase > 0 && j.exp != kWaveNone;
  }
  const bool r2l = any_exp && n <= c->r2l_max;
  int waves = ((any_fixed && c->wave_split) || r2l) ? 4 : 1;
  if (!r2l && any_fixed && c->wave_split && n <= c->w8_max) waves = 8;  // two waves per SIMD, one job per CU
  if (powwave_jobs(c->latw, c->h.friendly != 0, c->ct_pow != 0, waves, r2l, c->stream, (const WaveJob*)d_in, none, (uint32_t)n,
                   (const WaveTab*)(d_in + o_tabs), WaveTab{nullptr, 0, 0}, d_in + o_bases, d_in + o_exps, d_out, &err))
    return fail(EG_ERR_HIP, err);
  if (!(c->co_zc & 2)) HIPCHK(hipMemcpyAsync(co->h_out, d_out, n * 512, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return EG_OK;
}

// jobs of one plain kind, for the throughput layouts of a large batch
enum CoPlain { PLAIN_NONE, PLAIN_POWP, PLAIN_FB, PLAIN_MULTP };
static CoPlain plain_kind(const CoBatch& b) {
  CoPlain k = PLAIN_NONE;
  for (size_t i = 0; i < b.jobs.size(); ++i) {
    const CoJob& j = b.jobs[i];
    CoPlain kj = PLAIN_NONE;
    if (j.nbase == 1 && j.exp != kWaveNone && !j.fb[0] && !j.fb[1]) kj = PLAIN_POWP;
    else if (j.nbase == 0 && j.exp == kWaveNone && j.fb[0] && !j.fb[1] && j.fb[0] == b.jobs[0].fb[0]) kj = PLAIN_FB;
    else if (j.nbase == 2 && j.exp == kWaveNone && !j.fb[0] && !j.fb[1]) kj = PLAIN_MULTP;
    if (kj == PLAIN_NONE || (i && kj != k)) return PLAIN_NONE;
    k = kj;
  }
  return k;
}

static int run_batch(eg_ctx* c, Coalescer* co, const CoBatch& b) {
  const size_t n = b.jobs.size();
  if (c->latw && n <= c->wave_max) return run_wave_batch(c, co, b);
  // a large batch of one plain kind: rows were appended in job order, so the inputs are contiguous
  const CoPlain k = plain_kind(b);
  int rc;
  if ((rc = pinned(&co->h_out, &co->h_out_bytes, n * 512))) return rc;
  if (k == PLAIN_POWP) {
    if (latency_shaped(c, n)) return pow_latency(c, b.bases.data(), b.exps.data(), co->h_out, n);
    return pow_host(c, b.bases.data(), b.exps.data(), 32, false, co->h_out, n, nullptr);
  }
  if (k == PLAIN_FB) {
    FbTab t = b.jobs[0].fb[0]->tab();
    if (c->ct_pow && (rc = ct_table_locked(c, b.jobs[0].fb[0], &t))) return rc;
    return pow_host(c, nullptr, b.exps.data(), 32, false, co->h_out, n, &t);
  }
  if (k == PLAIN_MULTP) {
    std::vector<uint8_t> a(n * 512), bb(n * 512);
    for (size_t i = 0; i < n; ++i) {
      std::memcpy(&a[i * 512], &b.bases[(size_t)b.jobs[i].base * 512], 512);
      std::memcpy(&bb[i * 512], &b.bases[((size_t)b.jobs[i].base + 1) * 512], 512);
    }
    return multp_host(c, a.data(), bb.data(), co->h_out, n);
  }
  if (!c->latw) return fail(EG_ERR_STATE, "mixed per-element jobs need the per-wave kernel (EG_LATENCY_POW=0 disables it)");
  return run_wave_batch(c, co, b);
}

static void coalescer_loop(eg_ctx* c, Coalescer* co) {
  std::unique_lock<std::mutex> lk(co->m);
  for (;;) {
    co->cv_work.wait(lk, [&] { return co->stop || co->open || !co->sealed.empty(); });
    if (!co->open && co->sealed.empty()) break;  // stop requested and nothing left
    while (!co->stop && co->sealed.empty() && co->open->jobs.size() < co->max_batch) {
      if (co->open->jobs.size() >= co->last_n) break;
      const uint32_t win = co->window_fixed ? co->window_us
                                            : std::min<uint32_t>(co->window_us, std::max<uint32_t>(20u, co->last_dur_us / 2));
      const auto window_end = std::max(co->first, co->last_done) + std::chrono::microseconds(win);
      if (std::chrono::steady_clock::now() >= window_end) break;
      co->cv_work.wait_until(lk, window_end);  // submits wake it
    }
    lk.unlock();
    std::shared_ptr<CoBatch> take;
    std::chrono::steady_clock::time_point t_run{};
    {
      Locked L(c);  // wait for the GPU; the batch stays open meanwhile
      t_run = std::chrono::steady_clock::now();
      lk.lock();
      if (!co->sealed.empty()) {  // batches closed by a mode switch go first, in submission order
        take = std::move(co->sealed.front());
        co->sealed.pop_front();
        ++co->st_sealed;
      } else {
        take.swap(co->open);
        co->st_queue_us += (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(t_run - co->first).count();
      }
      co->last_n = std::max<size_t>(1, take->jobs.size());
      lk.unlock();
      CoBatch* b = take.get();
      const size_t n = b->jobs.size();
      int rc;
      // the batch runs in the constant-time mode its jobs were submitted in (the ctx lock is held, so
      // no other call sees the temporary value; eg_ctx_set_ct_pow takes the same lock)
      const uint32_t ct_saved = c->ct_pow;
      c->ct_pow = b->ct ? 1u : 0u;
      try {  // an exception must not end this thread (std::terminate): it fails the batch
        rc = run_batch(c, co, *b);
        if (!rc)
          for (size_t i = 0; i < n; ++i) std::memcpy(b->jobs[i].out, co->h_out + i * 512, 512);
      } catch (const std::bad_alloc&) {
        rc = fail(EG_ERR_NOMEM, "coalesced batch: out of host memory");
      }
      c->ct_pow = ct_saved;
      {
        std::lock_guard<std::mutex> dl(b->dm);
        b->rc = rc;
        if (rc) b->err = g_err;
      }
      for (const CoJob& j : b->jobs)  // the batch no longer reads its tables
        for (eg_fixed_base* f : j.fb)
          if (f) f->queued.fetch_sub(1, std::memory_order_release);
    }
    {
      std::lock_guard<std::mutex> dl(take->dm);
      take->done = true;
    }
    take->dcv.notify_all();  // this batch's callers only
    lk.lock();
    co->last_done = std::chrono::steady_clock::now();
    co->last_dur_us = (uint32_t)std::min<int64_t>(
        1000000, std::chrono::duration_cast<std::chrono::microseconds>(co->last_done - t_run).count());
    ++co->st_batches;
    co->st_jobs += take->jobs.size();
    co->st_max = std::max<uint64_t>(co->st_max, take->jobs.size());
    co->st_run_us += (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(co->last_done - t_run).count();
  }
}

// EG_COALESCE_STATS=1: one JSON line of batch statistics on stderr (at eg_ctx_destroy, and at each
// eg_ctx_set_coalescing, which then starts a new count: a caller marks its phases that way)
static void coalescer_stats_locked(Coalescer* co) {
  if (!co->stats || !co->st_batches) return;
  fprintf(stderr,
          "{\"coalescer\": {\"batches\": %llu, \"jobs\": %llu, \"mean_batch\": %.1f, \"max_batch\": %llu, "
          "\"mean_run_us\": %.1f, \"mean_first_job_wait_us\": %.1f, \"sealed\": %llu}}\n",
          (unsigned long long)co->st_batches, (unsigned long long)co->st_jobs, (double)co->st_jobs / co->st_batches,
          (unsigned long long)co->st_max, (double)co->st_run_us / co->st_batches,
          (double)co->st_queue_us / co->st_batches, (unsigned long long)co->st_sealed);
  co->st_batches = co->st_jobs = co->st_max = co->st_run_us = co->st_queue_us = co->st_sealed = 0;
}

static std::shared_ptr<Coalescer> coalescer_of(eg_ctx* c) {
  std::lock_guard<std::mutex> g(c->co_mu);
  if (!c->co && !c->co_closed) {
    auto co = std::make_shared<Coalescer>();
    if (const char* st = getenv("EG_COALESCE_STATS")) co->stats = st[0] == '1';
    if (const char* w = getenv("EG_COALESCE_WINDOW_US")) {
      co->window_us = (uint32_t)std::max(0L, atol(w));
      co->window_fixed = true;
    }
    co->th = std::thread(coalescer_loop, c, co.get());
    c->co = std::move(co);
  }
  return c->co;
}

static void coalescer_stop(eg_ctx* c) {
  std::shared_ptr<Coalescer> co;
  {
    std::lock_guard<std::mutex> g(c->co_mu);
    co.swap(c->co);
    c->co_closed = true;  // a submit racing eg_ctx_destroy fails instead of starting a new dispatcher
  }
  if (!co) return;
  {
    std::lock_guard<std::mutex> lk(co->m);
    co->stop = true;
  }
  co->cv_work.notify_all();
  co->th.join();  // every batch has run; tickets not yet waited keep co and their batch alive
  coalescer_stats_locked(co.get());
  hipSetDevice(c->device);
  if (co->h_in) hipHostFree(co->h_in);
  if (co->h_out) hipHostFree(co->h_out);
  co->h_in = co->h_out = nullptr;
}

// Queue one job (see eg_mexp_submit).  Inputs are copied: nothing but `out` is retained.
static int co_submit(eg_ctx* c, const uint8_t* bases, size_t nbase, const uint8_t* exp, eg_fixed_base* fb0,
                     const uint8_t* e0, eg_fixed_base* fb1, const uint8_t* e1, uint8_t* out, eg_ticket** t) {
  if (!c || !out || !t || (nbase && !bases) || (fb0 && !e0) || (fb1 && !e1)) return fail(EG_ERR_ARG, "null argument");
  if (nbase > kWaveMaxBases) return fail(EG_ERR_ARG, "a job multiplies at most 16 bases (eg_prod_reduce for more)");
  if ((fb0 && fb0->ctx != c) || (fb1 && fb1->ctx != c)) return fail(EG_ERR_ARG, "fixed-base table of another context");
  std::shared_ptr<Coalescer> co = coalescer_of(c);
  if (!co) return fail(EG_ERR_STATE, "context is being destroyed");
  std::shared_ptr<CoBatch> batch;
  bool wake = false;
  const bool ct = c->ct_pow_submit.load(std::memory_order_acquire) != 0;  // the mode at submission
  {
    std::lock_guard<std::mutex> lk(co->m);
    if (co->stop) return fail(EG_ERR_STATE, "context is being destroyed");
    if (co->open && co->open->ct != ct) {  // never mix modes: close the open batch, start one in this mode
      co->sealed.push_back(std::move(co->open));
      co->open.reset();
      wake = true;
    }
    if (!co->open) {
      co->open = std::make_shared<CoBatch>();
      co->open->ct = ct;
      co->first = std::chrono::steady_clock::now();
      wake = true;
    }
    CoBatch& b = *co->open;
    CoJob j{};
    j.base = (uint32_t)(b.bases.size() / 512);
    j.nbase = (uint32_t)nbase;
    if (nbase) b.bases.insert(b.bases.end(), bases, bases + nbase * 512);
    auto put_exp = [&](const uint8_t* e) {
      const uint32_t row = (uint32_t)(b.exps.size() / 32);
      b.exps.insert(b.exps.end(), e, e + 32);
      return row;
    };
    j.exp = exp ? put_exp(exp) : kWaveNone;
    j.fb[0] = fb0;
    j.fb[1] = fb1;
    j.fexp[0] = fb0 ? put_exp(e0) : kWaveNone;
    j.fexp[1] = fb1 ? put_exp(e1) : kWaveNone;
    j.out = out;
    b.jobs.push_back(j);
    for (eg_fixed_base* f : j.fb)  // held until the batch has run (eg_fixed_base_destroy waits)
      if (f) f->queued.fetch_add(1, std::memory_order_relaxed);
    batch = co->open;
    wake |= b.jobs.size() >= co->max_batch || b.jobs.size() >= co->last_n;
  }
  if (wake) co->cv_work.notify_one();
  *t = new eg_ticket{std::move(batch), std::move(co)};
  return EG_OK;
}

extern "C" int eg_ticket_wait(eg_ticket* t) {
  if (!t) return fail(EG_ERR_ARG, "null ticket");
  int rc;
  {
    std::unique_lock<std::mutex> lk(t->b->dm);
    t->b->dcv.wait(lk, [&] { return t->b->done; });
    rc = t->b->rc;
    if (rc) g_err = t->b->err;
  }
  delete t;
  return rc;
}

extern "C" int eg_ctx_set_coalescing(eg_ctx* c, size_t max_batch, uint32_t window_us) {
  if (!c || max_batch == 0 || max_batch > kMaxBatch) return fail(EG_ERR_ARG, "max_batch must be in [1, 2^31]");
  std::shared_ptr<Coalescer> co = coalescer_of(c);
  if (!co) return fail(EG_ERR_STATE, "context is being destroyed");
  std::lock_guard<std::mutex> lk(co->m);
  coalescer_stats_locked(co.get());
  co->max_batch = max_batch;
  // window_us > 0: honoured exactly; 0: the adaptive default (half the previous batch, in [20, 100] us)
  co->window_fixed = window_us > 0;
  co->window_us = window_us > 0 ? window_us : 100;
  co->last_n = max_batch;  // the next batch waits for max_batch jobs or the window, then adapts again
  return EG_OK;
}

extern "C" int eg_mexp_submit(eg_ctx* c, const uint8_t* bases_be, size_t nbases, const uint8_t* exp_be,
                              eg_fixed_base* fb0, const uint8_t* e0_be, eg_fixed_base* fb1, const uint8_t* e1_be,
                              uint8_t* out_be, eg_ticket** t) {
  return co_submit(c, bases_be, nbases, exp_be, fb0, e0_be, fb1, e1_be, out_be, t);
}
extern "C" int eg_powp_submit(eg_ctx* c, const uint8_t base_be[512], const uint8_t exp_be[32], uint8_t out_be[512],
                              eg_ticket** t) {
  if (!base_be || !exp_be) return fail(EG_ERR_ARG, "null argument");
  return co_submit(c, base_be, 1, exp_be, nullptr, nullptr, nullptr, nullptr, out_be, t);
}
extern "C" int eg_gpowp_submit(eg_ctx* c, const uint8_t exp_be[32], uint8_t out_be[512], eg_ticket** t) {
  if (!c || !exp_be) return fail(EG_ERR_ARG, "null argument");
  return co_submit(c, nullptr, 0, nullptr, c->gtab, exp_be, nullptr, nullptr, out_be, t);
}
extern "C" int eg_fb_pow_submit(eg_fixed_base* fb, const uint8_t exp_be[32], uint8_t out_be[512], eg_ticket** t) {
  if (!fb || !exp_be) return fail(EG_ERR_ARG, "null argument");
  return co_submit(fb->ctx, nullptr, 0, nullptr, fb, exp_be, nullptr, nullptr, out_be, t);
}
extern "C" int eg_multp_submit(eg_ctx* c, const uint8_t a_be[512], const uint8_t b_be[512], uint8_t out_be[512],
                               eg_ticket** t) {
  if (!a_be || !b_be) return fail(EG_ERR_ARG, "null argument");
  uint8_t ab[1024];
  std::memcpy(ab, a_be, 512);
  std::memcpy(ab + 512, b_be, 512);
  return co_submit(c, ab, 2, nullptr, nullptr, nullptr, nullptr, nullptr, out_be, t);
}

static int submit_wait(int rc, eg_ticket* t) { return rc ? rc : eg_ticket_wait(t); }
extern "C" int eg_mexp_one(eg_ctx* c, const uint8_t* bases_be, size_t nbases, const uint8_t* exp_be, eg_fixed_base* fb0,
                           const uint8_t* e0_be, eg_fixed_base* fb1, const uint8_t* e1_be, uint8_t* out_be) {
  eg_ticket* t = nullptr;
  return submit_wait(eg_mexp_submit(c, bases_be, nbases, exp_be, fb0, e0_be, fb1, e1_be, out_be, &t), t);
}
extern "C" int eg_powp_one(eg_ctx* c, const uint8_t base_be[512], const uint8_t exp_be[32], uint8_t out_be[512]) {
  eg_ticket* t = nullptr;
  return submit_wait(eg_powp_submit(c, base_be, exp_be, out_be, &t), t);
}
extern "C" int eg_gpowp_one(eg_ctx* c, const uint8_t exp_be[32], uint8_t out_be[512]) {
  eg_ticket* t = nullptr;
  return submit_wait(eg_gpowp_submit(c, exp_be, out_be, &t), t);
}
extern "C" int eg_fb_pow_one(eg_fixed_base* fb, const uint8_t exp_be[32], uint8_t out_be[512]) {
  eg_ticket* t = nullptr;
  return submit_wait(eg_fb_pow_submit(fb, exp_be, out_be, &t), t);
}
extern "C" int eg_multp_one(eg_ctx* c, const uint8_t a_be[512], const uint8_t b_be[512], uint8_t out_be[512]) {
  eg_ticket* t = nullptr;
  return submit_wait(eg_multp_submit(c, a_be, b_be, out_be, &t), t);
}

extern "C" int eg_ctx_set_ct_pow(eg_ctx* c, int on) {
  if (!c) return fail(EG_ERR_ARG, "null ctx");
  Locked L(c);  // no batch runs while the mode changes
  c->ct_pow = on ? 1u : 0u;
  c->ct_pow_submit.store(on ? 1u : 0u, std::memory_order_release);  // what later submits record
  return EG_OK;
}
