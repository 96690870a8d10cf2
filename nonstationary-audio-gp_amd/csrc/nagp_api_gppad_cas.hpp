// part of nagp_api.hip: objective and gradient of the GPPAD cascade, Cascade/GetObjCasGPFAST.m (see include/nagp.h, nagp_gppad.hpp): the
// resident handle and the one-shot call on top of it.  The transforms, the twiddle tables, the budget rule and the developer switch slot are
// those of nagp_api_gppad.hpp; a cascade of M columns is M "problems" of its kernels.
static thread_local double g_gppad_cas_ms = 0.0;

struct nagp_gppad_cas {
  int device = 0, n = 0, M = 1, nb = 0, N1 = 1, N2 = 1, lcb = 0, nwg = 1, nwgA = 1, nt = 64;
  int64_t T = 0, Tx = 0, ic_stride = 0;
  size_t lds = 0;
  DevBlock res, bat;          // resident / per device batch (with the two events), laid out by r / b
  GppadCasRes r{}; GppadCasBat b{};
  const double2* tw = nullptr;
};

extern "C" int nagp_gppad_cas_timings(double* ms) { return timings_out(ms, &g_gppad_cas_ms, 1); }
extern "C" void nagp_gppad_cas_destroy(nagp_gppad_cas* h) { delete h; }

static GppadPar gppad_cas_par(const nagp_gppad_cas* h) {
  GppadPar pp{};
  pp.T = h->T; pp.Tx = h->Tx; pp.N1 = h->N1; pp.N2 = h->N2; pp.lcb = h->lcb; pp.nwg = h->nwg; pp.tw = h->tw;
  pp.ic_stride = h->ic_stride; pp.M = h->M; pp.nwgA = h->nwgA;
  return pp;
}

extern "C" int nagp_gppad_cas_create(nagp_gppad_cas** handle, int32_t n_problems, int32_t M, int64_t T, int64_t Tx, const double* y, const double* len,
                                     const double* fftCovs, int64_t cov_stride, const double* varx, const double* mux, const double* varc, int32_t device) {
  if (handle) *handle = nullptr;
  if (!handle || !y || !varx || !mux || !varc) FAIL(NAGP_EINVAL, "null argument");
  if (n_problems < 1 || T < 1) FAIL(NAGP_EINVAL, "bad sizes (n_problems=%d T=%lld)", n_problems, (long long)T);
  if (M < 1 || M > GPPAD_CAS_MAX_M) FAIL(NAGP_EUNSUPPORTED, "M=%d: a cascade has 1 to %d modulators", M, GPPAD_CAS_MAX_M);
  if ((len != nullptr) == (fftCovs != nullptr)) FAIL(NAGP_EINVAL, "exactly one of len and fftCovs is given");
  if (Tx < 2 || Tx > ((int64_t)1 << GPPAD_LOG_MAX) || (Tx & (Tx - 1))) FAIL(NAGP_EUNSUPPORTED, "Tx=%lld: a power of two from 2 to 2^%d", (long long)Tx, GPPAD_LOG_MAX);
  if (T > Tx) FAIL(NAGP_EINVAL, "T=%lld > Tx=%lld", (long long)T, (long long)Tx);
  if (fftCovs && cov_stride != 0 && cov_stride != (int64_t)M * Tx) FAIL(NAGP_EINVAL, "cov_stride = %lld: 0 (shared) or M Tx", (long long)cov_stride);
  const size_t nz = (size_t)n_problems, Mz = (size_t)M, Tz = (size_t)T, Txz = (size_t)Tx;
  for (size_t e = 0; e < nz * Tz; ++e) if (!std::isfinite(y[e])) FAIL(NAGP_EINVAL, "y[%zu] = %g", e, y[e]);
  for (size_t q = 0; q < nz * Mz; ++q) {
    if (!std::isfinite(varx[q]) || !(varx[q] > 0.0)) FAIL(NAGP_EINVAL, "varx[%zu] = %g: finite and > 0", q, varx[q]);
    if (!std::isfinite(mux[q])) FAIL(NAGP_EINVAL, "mux[%zu] = %g", q, mux[q]);
    if (len && (!std::isfinite(len[q]) || !(len[q] > 0.0))) FAIL(NAGP_EINVAL, "len[%zu] = %g: finite and > 0", q, len[q]);
  }
  for (size_t q = 0; q < nz; ++q)
    if (!std::isfinite(varc[q]) || !(varc[q] > 0.0)) FAIL(NAGP_EINVAL, "varc[%zu] = %g: finite and > 0", q, varc[q]);
  if (fftCovs)
    for (size_t e = 0, m = (cov_stride ? nz : 1) * Mz * Txz; e < m; ++e)
      if (!std::isfinite(fftCovs[e]) || !(fftCovs[e] > 0.0)) FAIL(NAGP_EINVAL, "fftCovs[%zu] = %g: finite and > 0", e, fftCovs[e]);
  const DevSwitches dev_sw = read_dev_switches();
  std::unique_ptr<nagp_gppad_cas> h(new nagp_gppad_cas());      // released to the caller at the end; every return before that frees it
  h->device = device; h->n = n_problems; h->M = M; h->T = T; h->Tx = Tx;
  h->ic_stride = (fftCovs && cov_stride == 0) ? 0 : Tx;          // per "problem" (column of a cascade); 0: the M spectra are shared
  if (Tx > GPPAD_TILE) { h->N2 = GPPAD_TILE; h->N1 = (int)(Tx / GPPAD_TILE); h->lcb = GPPAD_LOG_TILE - gp_log2(h->N1); h->nwg = h->N1; }
  else { h->N1 = 1; h->N2 = (int)Tx; h->lcb = 0; h->nwg = 1; }
  h->nwgA = gppad_cas_nwg(T);
  h->nt = gppad_threads(Tx); h->lds = gppad_lds_bytes(Tx);
  // the budget rule of include/nagp.h
  const bool four = h->N1 > 1;
  const size_t per_cascade = 8 * (Mz * (2 * Txz + (four ? 2 * Txz : 0) + 2 * (size_t)h->nwg) + Tz + 2 * (size_t)h->nwgA + 1);
  const size_t budget = budget_bytes(dev_sw.budget_mb[DevSwitches::GPPAD], GPPAD_BUDGET_BYTES);
  const BatchPlan bp = batch_plan(nz, budget, 0, per_cascade);
  if (!bp.ok) FAIL(NAGP_EUNSUPPORTED, "one cascade takes %zu B of device memory per evaluation (budget %zu B)", per_cascade, budget);
  h->nb = (int)std::min(bp.nb, BATCH_MAX / Mz);                  // nb M "problems" on the y extent of a grid
  if (hipSetDevice(device) != hipSuccess) FAIL(NAGP_EHIP, "hipSetDevice(%d)", device);
  const size_t n_ic = (h->ic_stride ? nz : 1) * Mz * Txz;
  h->r = gppad_cas_res(nz, Mz, Tz, Txz, h->ic_stride != 0);
  h->b = gppad_cas_bat(Mz, Tz, Txz, four, (size_t)h->nwg, (size_t)h->nwgA, (size_t)h->nb);
  API_ALLOC(h->res, device, h->r.total);
  API_ALLOC(h->bat, device, h->b.total);
  double* const res = h->res.p; double* const bat = h->bat.p;
  int st = gppad_twiddles(device, Tx, &h->tw);
  if (st == NAGP_OK) st = set_lds(gppad_lds_kernel<1>, h->lds);
  if (st == NAGP_OK) st = set_lds(gppad_colf_kernel<0>, h->lds);
  if (st == NAGP_OK) st = set_lds(gppad_row_kernel<1>, h->lds);
  if (st == NAGP_OK) st = set_lds(gppad_coli_kernel<1>, h->lds);
  API_HIP(nagp_gppad_cas_create, h->bat.events(2));
  API_HIP(nagp_gppad_cas_create, hipMemcpy(res + h->r.y, y, nz * Tz * 8, hipMemcpyHostToDevice));
  API_HIP(nagp_gppad_cas_create, hipMemcpy(res + h->r.vx, varx, nz * Mz * 8, hipMemcpyHostToDevice));
  API_HIP(nagp_gppad_cas_create, hipMemcpy(res + h->r.mu, mux, nz * Mz * 8, hipMemcpyHostToDevice));
  API_HIP(nagp_gppad_cas_create, hipMemcpy(res + h->r.vc, varc, nz * 8, hipMemcpyHostToDevice));
  if (fftCovs) {                                           // 1 / (c Tx) in the order the forward transform leaves
    std::vector<double> ic(n_ic);
    const double invT = 1.0 / (double)Tx;
    for (size_t q = 0, nq = n_ic / Txz; q < nq; ++q)
      for (size_t e = 0; e < Txz; ++e) ic[q * Txz + e] = (1.0 / fftCovs[q * Txz + (size_t)gppad_freq_at((int64_t)e, h->N1, h->N2)]) * invT;
    API_HIP(nagp_gppad_cas_create, hipMemcpy(res + h->r.ic, ic.data(), n_ic * 8, hipMemcpyHostToDevice));
  } else {                                                 // GetFFTCovFast.m:10-16 on the device (len goes through the head of the batch block)
    run_batches("nagp_gppad_cas_create", st, n_problems, h->nb, nullptr, 0, nullptr,
      [&](int i0, int nbk) { API_HIP(nagp_gppad_cas_create, hipMemcpy(bat, len + (size_t)i0 * Mz, (size_t)nbk * Mz * 8, hipMemcpyHostToDevice)); },
      [&](int i0, int nbk, int) {
        GppadPar pp = gppad_cas_par(h.get());
        pp.len = bat; pp.ic_out = res + h->r.ic + (size_t)i0 * Mz * Txz;
        hipLaunchKernelGGL(gppad_cov_kernel<0>, dim3((unsigned)((Tx + 255) / 256), (unsigned)(nbk * M)), dim3(256), 0, 0, pp);
      }, [](int, int) {});
  }
  if (st == NAGP_OK) *handle = h.release();
  return st;
}

extern "C" int nagp_gppad_cas_eval(nagp_gppad_cas* h, const double* x, double* Obj, double* dObj) {
  g_gppad_cas_ms = 0.0;                                     // a call that is refused or fails reports no time of an earlier one
  if (!h || !x || !Obj) FAIL(NAGP_EINVAL, "null argument");
  if (hipSetDevice(h->device) != hipSuccess) FAIL(NAGP_EHIP, "hipSetDevice(%d)", h->device);
  const size_t Txz = (size_t)h->Tx, Tz = (size_t)h->T, Mz = (size_t)h->M;
  double* const res = h->res.p; double* const bat = h->bat.p;
  const GppadCasRes& r = h->r; const GppadCasBat& b = h->b;
  int st = NAGP_OK;
  run_batches("nagp_gppad_cas_eval", st, h->n, h->nb, h->bat.ev, 2, &g_gppad_cas_ms,
    [&](int i0, int nbk) { API_HIP(nagp_gppad_cas_eval, hipMemcpy(bat + b.x, x + (size_t)i0 * Mz * Txz, (size_t)nbk * Mz * Txz * 8, hipMemcpyHostToDevice)); },
    [&](int i0, int nbk, int) {
      GppadPar pp = gppad_cas_par(h);
      pp.grad = dObj ? 1 : 0;
      pp.x = bat + b.x; pp.dObj = bat + b.dg; pp.work = reinterpret_cast<double2*>(bat + b.wk); pp.part = bat + b.pt; pp.Obj = bat + b.ob;
      pp.D = bat + b.d; pp.partA = bat + b.pa;
      pp.y = res + r.y + (size_t)i0 * Tz;
      pp.ic = res + r.ic + (h->ic_stride ? (size_t)i0 * Mz * Txz : 0);
      pp.varx = res + r.vx + (size_t)i0 * Mz; pp.mux = res + r.mu + (size_t)i0 * Mz; pp.varc = res + r.vc + i0;
      const unsigned nq = (unsigned)(nbk * h->M);             // the columns of the batch's cascades: the "problems" of the transform kernels
      hipLaunchKernelGGL(gppad_cas_pre_kernel<1>, dim3((unsigned)h->nwgA, (unsigned)nbk), dim3(GPPAD_CAS_NT), 0, 0, pp);
      if (h->N1 == 1) hipLaunchKernelGGL(gppad_lds_kernel<1>, dim3(nq), dim3(h->nt), h->lds, 0, pp);
      else {
        const dim3 grid((unsigned)h->N1, nq);
        hipLaunchKernelGGL(gppad_colf_kernel<0>, grid, dim3(h->nt), h->lds, 0, pp);
        hipLaunchKernelGGL(gppad_row_kernel<1>, grid, dim3(h->nt), h->lds, 0, pp);
        hipLaunchKernelGGL(gppad_coli_kernel<1>, grid, dim3(h->nt), h->lds, 0, pp);
      }
      hipLaunchKernelGGL(gppad_cas_finish_kernel<1>, dim3((unsigned)((nbk + 63) / 64)), dim3(64), 0, 0, pp, nbk);
    }, [&](int i0, int nbk) {
      API_HIP(nagp_gppad_cas_eval, hipMemcpy(Obj + i0, bat + b.ob, (size_t)nbk * 8, hipMemcpyDeviceToHost));
      if (dObj) API_HIP(nagp_gppad_cas_eval, hipMemcpy(dObj + (size_t)i0 * Mz * Txz, bat + b.dg, (size_t)nbk * Mz * Txz * 8, hipMemcpyDeviceToHost));
    });
  return st;
}

extern "C" int nagp_gppad_cas_obj(int32_t n_problems, int32_t M, int64_t T, int64_t Tx, const double* x, const double* y, const double* len,
                                  const double* fftCovs, int64_t cov_stride, const double* varx, const double* mux, const double* varc,
                                  double* Obj, double* dObj, int32_t device) {
  g_gppad_cas_ms = 0.0;
  if (!x || !Obj) FAIL(NAGP_EINVAL, "null argument");
  nagp_gppad_cas* h = nullptr;
  const int st = nagp_gppad_cas_create(&h, n_problems, M, T, Tx, y, len, fftCovs, cov_stride, varx, mux, varc, device);
  const std::unique_ptr<nagp_gppad_cas> owner(h);
  return st != NAGP_OK ? st : nagp_gppad_cas_eval(h, x, Obj, dObj);
}
