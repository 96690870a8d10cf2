// part of nagp_api.hip: objective and gradient of the GPPAD envelope inference, GPModelFast/GetGPObjFast.m (see include/nagp.h,
// nagp_gppad.hpp): the resident handle, the one-shot call on top of it, the twiddle tables.
constexpr size_t GPPAD_BUDGET_BYTES = (size_t)1 << 30;    // device memory of the per-evaluation buffers: the problems run in device batches under it
static thread_local double g_gppad_ms = 0.0;

struct nagp_gppad {
  int device = 0, n = 0, nb = 0, N1 = 1, N2 = 1, lcb = 0, nwg = 1, nt = 64;
  int64_t T = 0, Tx = 0, vary_stride = 0, ic_stride = 0;
  size_t lds = 0;
  DevBlock res, bat;          // resident / per device batch (with the two events), laid out by r / b
  GppadRes r{}; GppadBat b{};
  const double2* tw = nullptr;
};

// exp(-2 pi i m / Tx), m < Tx, in long double through the octant of m (the argument of sinl / cosl stays inside [0, pi/4]); one table
// per (device, Tx), kept for the life of the process
static int gppad_twiddles(int device, int64_t Tx, const double2** out) {
  static std::mutex mu;
  static std::map<std::pair<int, int64_t>, double2*> cache;
  std::lock_guard<std::mutex> lk(mu);
  auto it = cache.find({device, Tx});
  if (it != cache.end()) { *out = it->second; return NAGP_OK; }
  std::vector<double2> h((size_t)Tx);
  const long double pi = 3.14159265358979323846264338327950288L;
  for (int64_t m = 0; m < Tx; ++m) {
    // angle 2 pi m / Tx = (o + r) pi / 4 with octant o = floor(8 m / Tx) and r in [0, 1): exact integer reduction
    const int64_t e = 8 * m, o = e / Tx, rem = e % Tx;
    long double cs, sn;
    if (o & 1) { const long double a = pi / 4 * ((long double)(Tx - rem) / (long double)Tx); cs = sinl(a); sn = cosl(a); }     // pi/2 - a' within the quadrant
    else { const long double a = pi / 4 * ((long double)rem / (long double)Tx); cs = cosl(a); sn = sinl(a); }
    // quadrant (o / 2) rotates (cs, sn) of the angle inside [0, pi/2)
    long double c, s;
    switch ((o >> 1) & 3) {
      case 0: c = cs; s = sn; break;
      case 1: c = -sn; s = cs; break;
      case 2: c = -cs; s = -sn; break;
      default: c = sn; s = -cs; break;
    }
    h[(size_t)m] = make_double2((double)c, (double)(-s));
  }
  double2* d = nullptr;
  HIP_TRY(hipMalloc(&d, (size_t)Tx * sizeof(double2)));
  hipError_t e = hipMemcpy(d, h.data(), (size_t)Tx * sizeof(double2), hipMemcpyHostToDevice);
  if (e != hipSuccess) { (void)hipFree(d); HIP_TRY(e); }
  cache[{device, Tx}] = d;
  *out = d;
  return NAGP_OK;
}

extern "C" int nagp_gppad_timings(double* ms) { return timings_out(ms, &g_gppad_ms, 1); }
extern "C" void nagp_gppad_destroy(nagp_gppad* h) { delete h; }

static GppadPar gppad_par(const nagp_gppad* h) {
  GppadPar pp{};
  pp.T = h->T; pp.Tx = h->Tx; pp.N1 = h->N1; pp.N2 = h->N2; pp.lcb = h->lcb; pp.nwg = h->nwg; pp.tw = h->tw;
  pp.vary_stride = h->vary_stride; pp.ic_stride = h->ic_stride;
  return pp;
}

extern "C" int nagp_gppad_create(nagp_gppad** handle, int32_t n_problems, int64_t T, int64_t Tx, const double* y, const double* vary, int64_t vary_stride,
                                 const double* len, const double* fftCov, int64_t cov_stride, const double* varx, const double* mux, const double* varc,
                                 int32_t device) {
  if (handle) *handle = nullptr;
  if (!handle || !y || !vary || !varx || !mux || !varc) FAIL(NAGP_EINVAL, "null argument");
  if (n_problems < 1 || T < 1) FAIL(NAGP_EINVAL, "bad sizes (n_problems=%d T=%lld)", n_problems, (long long)T);
  if ((len != nullptr) == (fftCov != nullptr)) FAIL(NAGP_EINVAL, "exactly one of len and fftCov is given");
  if (Tx < 2 || Tx > ((int64_t)1 << GPPAD_LOG_MAX) || (Tx & (Tx - 1))) FAIL(NAGP_EUNSUPPORTED, "Tx=%lld: a power of two from 2 to 2^%d", (long long)Tx, GPPAD_LOG_MAX);
  if (T > Tx) FAIL(NAGP_EINVAL, "T=%lld > Tx=%lld", (long long)T, (long long)Tx);
  if (vary_stride != 0 && vary_stride != T) FAIL(NAGP_EINVAL, "vary_stride = %lld: 0 (one per problem) or T", (long long)vary_stride);
  if (fftCov && cov_stride != 0 && cov_stride != Tx) FAIL(NAGP_EINVAL, "cov_stride = %lld: 0 (shared) or Tx", (long long)cov_stride);
  const size_t nz = (size_t)n_problems, Tz = (size_t)T, Txz = (size_t)Tx;
  for (size_t e = 0; e < nz * Tz; ++e) if (!std::isfinite(y[e])) FAIL(NAGP_EINVAL, "y[%zu] = %g", e, y[e]);
  for (size_t e = 0, m = vary_stride ? nz * Tz : nz; e < m; ++e)
    if (!std::isfinite(vary[e]) || vary[e] < 0.0) FAIL(NAGP_EINVAL, "vary[%zu] = %g: finite and >= 0", e, vary[e]);
  for (size_t q = 0; q < nz; ++q) {
    if (!std::isfinite(varx[q]) || !(varx[q] > 0.0)) FAIL(NAGP_EINVAL, "varx[%zu] = %g: finite and > 0", q, varx[q]);
    if (!std::isfinite(varc[q]) || !(varc[q] > 0.0)) FAIL(NAGP_EINVAL, "varc[%zu] = %g: finite and > 0", q, varc[q]);
    if (!std::isfinite(mux[q])) FAIL(NAGP_EINVAL, "mux[%zu] = %g", q, mux[q]);
    if (len && (!std::isfinite(len[q]) || !(len[q] > 0.0))) FAIL(NAGP_EINVAL, "len[%zu] = %g: finite and > 0", q, len[q]);
  }
  if (fftCov)
    for (size_t e = 0, m = cov_stride ? nz * Txz : Txz; e < m; ++e)
      if (!std::isfinite(fftCov[e]) || !(fftCov[e] > 0.0)) FAIL(NAGP_EINVAL, "fftCov[%zu] = %g: finite and > 0", e, fftCov[e]);
  const DevSwitches dev_sw = read_dev_switches();
  std::unique_ptr<nagp_gppad> h(new nagp_gppad());      // released to the caller at the end; every return before that frees it
  h->device = device; h->n = n_problems; h->T = T; h->Tx = Tx; h->vary_stride = vary_stride;
  h->ic_stride = (fftCov && cov_stride == 0) ? 0 : Tx;
  if (Tx > GPPAD_TILE) { h->N2 = GPPAD_TILE; h->N1 = (int)(Tx / GPPAD_TILE); h->lcb = GPPAD_LOG_TILE - gp_log2(h->N1); h->nwg = h->N1; }
  else { h->N1 = 1; h->N2 = (int)Tx; h->lcb = 0; h->nwg = 1; }
  h->nt = gppad_threads(Tx); h->lds = gppad_lds_bytes(Tx);
  // the budget rule of include/nagp.h
  const bool four = h->N1 > 1;
  const size_t per_problem = 8 * (2 * Txz + (four ? 2 * Txz : 0) + 2 * (size_t)h->nwg + 1);
  const size_t budget = budget_bytes(dev_sw.budget_mb[DevSwitches::GPPAD], GPPAD_BUDGET_BYTES);
  const BatchPlan bp = batch_plan(nz, budget, 0, per_problem);
  if (!bp.ok) FAIL(NAGP_EUNSUPPORTED, "one problem takes %zu B of device memory per evaluation (budget %zu B)", per_problem, budget);
  h->nb = (int)bp.nb;
  if (hipSetDevice(device) != hipSuccess) FAIL(NAGP_EHIP, "hipSetDevice(%d)", device);
  const size_t n_vy = vary_stride ? nz * Tz : nz, n_ic = h->ic_stride ? nz * Txz : Txz;
  h->r = gppad_res(nz, Tz, Txz, vary_stride != 0, h->ic_stride != 0);
  h->b = gppad_bat(Txz, four, (size_t)h->nwg, bp.nb);
  API_ALLOC(h->res, device, h->r.total);
  API_ALLOC(h->bat, device, h->b.total);
  double* const res = h->res.p; double* const bat = h->bat.p;
  int st = gppad_twiddles(device, Tx, &h->tw);
  if (st == NAGP_OK) st = set_lds(gppad_lds_kernel<0>, h->lds);
  if (st == NAGP_OK) st = set_lds(gppad_colf_kernel<0>, h->lds);
  if (st == NAGP_OK) st = set_lds(gppad_row_kernel<0>, h->lds);
  if (st == NAGP_OK) st = set_lds(gppad_coli_kernel<0>, h->lds);
  API_HIP(nagp_gppad_create, h->bat.events(2));
  API_HIP(nagp_gppad_create, hipMemcpy(res + h->r.y, y, nz * Tz * 8, hipMemcpyHostToDevice));
  API_HIP(nagp_gppad_create, hipMemcpy(res + h->r.vy, vary, n_vy * 8, hipMemcpyHostToDevice));
  API_HIP(nagp_gppad_create, hipMemcpy(res + h->r.vx, varx, nz * 8, hipMemcpyHostToDevice));
  API_HIP(nagp_gppad_create, hipMemcpy(res + h->r.mu, mux, nz * 8, hipMemcpyHostToDevice));
  API_HIP(nagp_gppad_create, hipMemcpy(res + h->r.vc, varc, nz * 8, hipMemcpyHostToDevice));
  if (fftCov) {                                            // 1 / (c Tx) in the order the forward transform leaves
    std::vector<double> ic(n_ic);
    const double invT = 1.0 / (double)Tx;
    for (size_t q = 0, nq = cov_stride ? nz : 1; q < nq; ++q)
      for (size_t e = 0; e < Txz; ++e) ic[q * Txz + e] = (1.0 / fftCov[q * Txz + (size_t)gppad_freq_at((int64_t)e, h->N1, h->N2)]) * invT;
    API_HIP(nagp_gppad_create, hipMemcpy(res + h->r.ic, ic.data(), n_ic * 8, hipMemcpyHostToDevice));
  } else {                                                 // GetFFTCovFast.m:10-16 on the device (len goes through the head of the batch block)
    run_batches("nagp_gppad_create", st, n_problems, h->nb, nullptr, 0, nullptr,
      [&](int i0, int nbk) { API_HIP(nagp_gppad_create, hipMemcpy(bat, len + i0, (size_t)nbk * 8, hipMemcpyHostToDevice)); },
      [&](int i0, int nbk, int) {
        GppadPar pp = gppad_par(h.get());
        pp.len = bat; pp.ic_out = res + h->r.ic + (size_t)i0 * Txz;
        hipLaunchKernelGGL(gppad_cov_kernel<0>, dim3((unsigned)((Tx + 255) / 256), (unsigned)nbk), dim3(256), 0, 0, pp);
      }, [](int, int) {});
  }
  if (st == NAGP_OK) *handle = h.release();
  return st;
}

extern "C" int nagp_gppad_eval(nagp_gppad* h, const double* x, double* Obj, double* dObj) {
  g_gppad_ms = 0.0;                                         // a call that is refused or fails reports no time of an earlier one
  if (!h || !x || !Obj) FAIL(NAGP_EINVAL, "null argument");
  if (hipSetDevice(h->device) != hipSuccess) FAIL(NAGP_EHIP, "hipSetDevice(%d)", h->device);
  const size_t Txz = (size_t)h->Tx, Tz = (size_t)h->T;
  double* const res = h->res.p; double* const bat = h->bat.p;
  const GppadRes& r = h->r; const GppadBat& b = h->b;
  int st = NAGP_OK;
  run_batches("nagp_gppad_eval", st, h->n, h->nb, h->bat.ev, 2, &g_gppad_ms,
    [&](int i0, int nbk) { API_HIP(nagp_gppad_eval, hipMemcpy(bat + b.x, x + (size_t)i0 * Txz, (size_t)nbk * Txz * 8, hipMemcpyHostToDevice)); },
    [&](int i0, int nbk, int) {
      GppadPar pp = gppad_par(h);
      pp.grad = dObj ? 1 : 0;
      pp.x = bat + b.x; pp.dObj = bat + b.dg; pp.work = reinterpret_cast<double2*>(bat + b.wk); pp.part = bat + b.pt; pp.Obj = bat + b.ob;
      pp.y = res + r.y + (size_t)i0 * Tz; pp.vary = res + r.vy + (h->vary_stride ? (size_t)i0 * Tz : (size_t)i0);
      pp.ic = res + r.ic + (h->ic_stride ? (size_t)i0 * Txz : 0);
      pp.varx = res + r.vx + i0; pp.mux = res + r.mu + i0; pp.varc = res + r.vc + i0;
      if (h->N1 == 1) hipLaunchKernelGGL(gppad_lds_kernel<0>, dim3((unsigned)nbk), dim3(h->nt), h->lds, 0, pp);
      else {
        const dim3 grid((unsigned)h->N1, (unsigned)nbk);
        hipLaunchKernelGGL(gppad_colf_kernel<0>, grid, dim3(h->nt), h->lds, 0, pp);
        hipLaunchKernelGGL(gppad_row_kernel<0>, grid, dim3(h->nt), h->lds, 0, pp);
        hipLaunchKernelGGL(gppad_coli_kernel<0>, grid, dim3(h->nt), h->lds, 0, pp);
      }
      hipLaunchKernelGGL(gppad_finish_kernel<0>, dim3((unsigned)((nbk + 63) / 64)), dim3(64), 0, 0, pp, nbk);
    }, [&](int i0, int nbk) {
      API_HIP(nagp_gppad_eval, hipMemcpy(Obj + i0, bat + b.ob, (size_t)nbk * 8, hipMemcpyDeviceToHost));
      if (dObj) API_HIP(nagp_gppad_eval, hipMemcpy(dObj + (size_t)i0 * Txz, bat + b.dg, (size_t)nbk * Txz * 8, hipMemcpyDeviceToHost));
    });
  return st;
}

extern "C" int nagp_gppad_obj(int32_t n_problems, int64_t T, int64_t Tx, const double* x, const double* y, const double* vary, int64_t vary_stride,
                              const double* len, const double* fftCov, int64_t cov_stride, const double* varx, const double* mux, const double* varc,
                              double* Obj, double* dObj, int32_t device) {
  g_gppad_ms = 0.0;
  if (!x || !Obj) FAIL(NAGP_EINVAL, "null argument");
  nagp_gppad* h = nullptr;
  const int st = nagp_gppad_create(&h, n_problems, T, Tx, y, vary, vary_stride, len, fftCov, cov_stride, varx, mux, varc, device);
  const std::unique_ptr<nagp_gppad> owner(h);
  return st != NAGP_OK ? st : nagp_gppad_eval(h, x, Obj, dObj);
}
