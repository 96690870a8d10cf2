// part of nagp_api.hip: the Laplace step of GPPAD (GPModelFast/Laplace: GetHessian.m, SigDSigTimesV.m, LanczosGPPAD.m, GetErrorBarGPPAD.m,
// GetLaplaceObjGPPADOneChunk.m; see include/nagp.h, nagp_gppad_lap.hpp): the resident handle and the batched eigen-solve.  The Lanczos
// control (nagp_tridiag.hpp) runs here on the host; per step alpha and beta (and h1 when a problem reorthogonalises) cross the bus, the
// basis never does.  The twiddle tables, the budget and its developer switch are those of nagp_api_gppad.hpp.
static thread_local double g_gppad_lap_ms = 0.0;

struct nagp_gppad_lap {
  int device = 0, n = 0, nb = 0, N1 = 1, N2 = 1, lcb = 0, nwe = 1, np = 1, nt = 64, jmax = 0;
  int64_t T = 0, Tx = 0, vary_stride = 0;
  size_t lds = 0;
  bool has_x = false, has_eig = false;
  DevBlock res, bat;
  LapRes r{}; LapBat b{};
  const double2* tw = nullptr;
  std::vector<double> varx, lmb;      // lmb: n x jmax of the last eigen-solve, NaN beyond nconv
  std::vector<int> nconv;
};

extern "C" int nagp_gppad_lap_timings(double* ms) { return timings_out(ms, &g_gppad_lap_ms, 1); }
extern "C" void nagp_gppad_lap_destroy(nagp_gppad_lap* h) { delete h; }

// the parameters of the kernels for the problems [i0, i0 + nbk) of the handle
static LapPar lap_par(const nagp_gppad_lap* h, int i0, int nbk) {
  LapPar pp{};
  double* const res = h->res.p; double* const bat = h->bat.p;
  pp.T = h->T; pp.Tx = h->Tx; pp.N1 = h->N1; pp.N2 = h->N2; pp.lcb = h->lcb; pp.nb = nbk; pp.jmax = h->jmax; pp.np = 1; pp.ss = 1; pp.lev = 1.0;
  pp.vary_stride = h->vary_stride; pp.tw = h->tw;
  pp.flag = bat + h->b.fl; pp.g = res + h->r.g + (size_t)i0 * h->Tx; pp.work = reinterpret_cast<double2*>(bat + h->b.wk);
  pp.d = res + h->r.d + (size_t)i0 * h->T; pp.part = bat + h->b.pt; pp.h1 = bat + h->b.h1; pp.S = bat + h->b.S; pp.q = bat + h->b.V;
  pp.x = res + h->r.x + (size_t)i0 * h->Tx; pp.y = res + h->r.y + (size_t)i0 * h->T;
  pp.vary = res + h->r.vy + (h->vary_stride ? (size_t)i0 * h->T : (size_t)i0);
  pp.varx = res + h->r.vx + i0; pp.varc = res + h->r.vc + i0;
  return pp;
}

// one sandwich of pp.in into pp.out with the epilogue E
template <int E>
static void lap_sandwich(const nagp_gppad_lap* h, const LapPar& pp, int i0, int nbk) {
  if (h->N1 == 1) { hipLaunchKernelGGL(lap_lds_kernel<E>, dim3((unsigned)nbk), dim3(h->nt), h->lds, 0, pp); return; }
  GppadPar gp{};                                                   // the forward column kernel and the row kernel of nagp_gppad.hpp: mux = 0, g for 1 / (c Tx)
  gp.T = h->T; gp.Tx = h->Tx; gp.N1 = h->N1; gp.N2 = h->N2; gp.lcb = h->lcb; gp.nwg = h->N1; gp.tw = h->tw;
  gp.x = pp.in; gp.mux = h->res.p + h->r.ze + i0; gp.ic = pp.g; gp.ic_stride = h->Tx; gp.work = pp.work;
  const dim3 grid((unsigned)h->N1, (unsigned)nbk);
  hipLaunchKernelGGL(gppad_colf_kernel<0>, grid, dim3(h->nt), h->lds, 0, gp);
  hipLaunchKernelGGL(gppad_row_kernel<0>, grid, dim3(h->nt), h->lds, 0, gp);
  hipLaunchKernelGGL(lap_coli_kernel<E>, grid, dim3(h->nt), h->lds, 0, pp);
}

extern "C" int nagp_gppad_lap_create(nagp_gppad_lap** handle, int32_t n_problems, int64_t T, int64_t Tx, const double* y, const double* vary, int64_t vary_stride,
                                     const double* len, const double* varx, const double* mux, const double* varc, int32_t jmax, int32_t device) {
  if (handle) *handle = nullptr;
  if (!handle || !y || !vary || !len || !varx || !mux || !varc) FAIL(NAGP_EINVAL, "null argument");
  if (n_problems < 1 || T < 1) FAIL(NAGP_EINVAL, "bad sizes (n_problems=%d T=%lld)", n_problems, (long long)T);
  if (Tx < 2 || Tx > ((int64_t)1 << GPPAD_LOG_MAX) || (Tx & (Tx - 1))) FAIL(NAGP_EUNSUPPORTED, "Tx=%lld: a power of two from 2 to 2^%d", (long long)Tx, GPPAD_LOG_MAX);
  if (T > Tx) FAIL(NAGP_EINVAL, "T=%lld > Tx=%lld", (long long)T, (long long)Tx);
  if (vary_stride != 0 && vary_stride != T) FAIL(NAGP_EINVAL, "vary_stride = %lld: 0 (one per problem) or T", (long long)vary_stride);
  if (jmax < 1 || jmax > Tx || jmax > 4096) FAIL(NAGP_EINVAL, "jmax = %d: 1 to min(Tx, 4096) Lanczos steps", jmax);
  const size_t nz = (size_t)n_problems, Tz = (size_t)T, Txz = (size_t)Tx, jz = (size_t)jmax;
  for (size_t e = 0; e < nz * Tz; ++e) if (!std::isfinite(y[e])) FAIL(NAGP_EINVAL, "y[%zu] = %g", e, y[e]);
  for (size_t e = 0, m = vary_stride ? nz * Tz : nz; e < m; ++e)
    if (!std::isfinite(vary[e]) || vary[e] < 0.0) FAIL(NAGP_EINVAL, "vary[%zu] = %g: finite and >= 0", e, vary[e]);
  for (size_t q = 0; q < nz; ++q) {
    if (!std::isfinite(varx[q]) || !(varx[q] > 0.0)) FAIL(NAGP_EINVAL, "varx[%zu] = %g: finite and > 0", q, varx[q]);
    if (!std::isfinite(varc[q]) || !(varc[q] > 0.0)) FAIL(NAGP_EINVAL, "varc[%zu] = %g: finite and > 0", q, varc[q]);
    if (!std::isfinite(mux[q])) FAIL(NAGP_EINVAL, "mux[%zu] = %g", q, mux[q]);
    if (!std::isfinite(len[q]) || !(len[q] > 0.0)) FAIL(NAGP_EINVAL, "len[%zu] = %g: finite and > 0", q, len[q]);
  }
  const DevSwitches dev_sw = read_dev_switches();
  std::unique_ptr<nagp_gppad_lap> h(new nagp_gppad_lap());
  h->device = device; h->n = n_problems; h->T = T; h->Tx = Tx; h->vary_stride = vary_stride; h->jmax = jmax;
  if (Tx > GPPAD_TILE) { h->N2 = GPPAD_TILE; h->N1 = (int)(Tx / GPPAD_TILE); h->lcb = GPPAD_LOG_TILE - gp_log2(h->N1); }
  else { h->N1 = 1; h->N2 = (int)Tx; h->lcb = 0; }
  h->nwe = lap_nwe(Tx); h->np = std::max(h->nwe, h->N1);
  h->nt = gppad_threads(Tx); h->lds = gppad_lds_bytes(Tx);
  h->varx.assign(varx, varx + nz);
  // the budget rule of include/nagp.h
  const bool four = h->N1 > 1;
  const size_t per_problem = 8 * lap_bat_per_problem(Txz, jz, four, (size_t)h->np);
  const size_t budget = budget_bytes(dev_sw.budget_mb[DevSwitches::GPPAD], GPPAD_BUDGET_BYTES);
  const BatchPlan bp = batch_plan(nz, budget, 0, per_problem);
  if (!bp.ok) FAIL(NAGP_EUNSUPPORTED, "one problem takes %zu B of device memory per eigen-solve (budget %zu B)", per_problem, budget);
  h->nb = (int)bp.nb;
  if (hipSetDevice(device) != hipSuccess) FAIL(NAGP_EHIP, "hipSetDevice(%d)", device);
  h->r = lap_res(nz, Tz, Txz, vary_stride != 0);
  h->b = lap_bat(Txz, jz, four, (size_t)h->np, bp.nb);
  API_ALLOC(h->res, device, h->r.total);
  API_ALLOC(h->bat, device, h->b.total);
  double* const res = h->res.p; double* const bat = h->bat.p;
  int st = gppad_twiddles(device, Tx, &h->tw);
  if (st == NAGP_OK) st = set_lds(lap_lds_kernel<0>, h->lds);
  if (st == NAGP_OK) st = set_lds(lap_lds_kernel<1>, h->lds);
  if (st == NAGP_OK) st = set_lds(lap_lds_kernel<2>, h->lds);
  if (st == NAGP_OK) st = set_lds(lap_lds_kernel<3>, h->lds);
  if (st == NAGP_OK) st = set_lds(lap_coli_kernel<0>, h->lds);
  if (st == NAGP_OK) st = set_lds(lap_coli_kernel<1>, h->lds);
  if (st == NAGP_OK) st = set_lds(lap_coli_kernel<2>, h->lds);
  if (st == NAGP_OK) st = set_lds(lap_coli_kernel<3>, h->lds);
  if (st == NAGP_OK) st = set_lds(gppad_lds_kernel<0>, h->lds);
  if (st == NAGP_OK) st = set_lds(gppad_colf_kernel<0>, h->lds);
  if (st == NAGP_OK) st = set_lds(gppad_row_kernel<0>, h->lds);
  if (st == NAGP_OK) st = set_lds(gppad_coli_kernel<0>, h->lds);
  const size_t n_vy = vary_stride ? nz * Tz : nz;
  API_HIP(nagp_gppad_lap_create, h->bat.events(2));
  API_HIP(nagp_gppad_lap_create, hipMemcpy(res + h->r.y, y, nz * Tz * 8, hipMemcpyHostToDevice));
  API_HIP(nagp_gppad_lap_create, hipMemcpy(res + h->r.vy, vary, n_vy * 8, hipMemcpyHostToDevice));
  API_HIP(nagp_gppad_lap_create, hipMemcpy(res + h->r.vx, varx, nz * 8, hipMemcpyHostToDevice));
  API_HIP(nagp_gppad_lap_create, hipMemcpy(res + h->r.mu, mux, nz * 8, hipMemcpyHostToDevice));
  API_HIP(nagp_gppad_lap_create, hipMemcpy(res + h->r.vc, varc, nz * 8, hipMemcpyHostToDevice));
  API_HIP(nagp_gppad_lap_create, hipMemset(res + h->r.ze, 0, nz * 8));
  // g = sqrt(c varx) / Tx and 1 / (c Tx), both in position order, on the device (len goes through the head of the batch block)
  run_batches("nagp_gppad_lap_create", st, n_problems, h->nb, nullptr, 0, nullptr,
    [&](int i0, int nbk) { API_HIP(nagp_gppad_lap_create, hipMemcpy(bat, len + i0, (size_t)nbk * 8, hipMemcpyHostToDevice)); },
    [&](int i0, int nbk, int) {
      const dim3 grid((unsigned)h->nwe, (unsigned)nbk);
      LapPar pp = lap_par(h.get(), i0, nbk);
      pp.len = bat; pp.out = res + h->r.g + (size_t)i0 * Txz;
      hipLaunchKernelGGL(lap_sample_kernel<0>, grid, dim3(LAP_NT), 0, 0, pp);
      GppadPar gp{};
      gp.Tx = Tx; gp.N1 = h->N1; gp.N2 = h->N2; gp.len = bat; gp.ic_out = res + h->r.ic + (size_t)i0 * Txz;
      hipLaunchKernelGGL(gppad_cov_kernel<0>, grid, dim3(256), 0, 0, gp);
    }, [](int, int) {});
  if (st == NAGP_OK) *handle = h.release();
  return st;
}

extern "C" int nagp_gppad_lap_hess(nagp_gppad_lap* h, const double* x, double* d) {
  if (!h || !x) FAIL(NAGP_EINVAL, "null argument");
  if (hipSetDevice(h->device) != hipSuccess) FAIL(NAGP_EHIP, "hipSetDevice(%d)", h->device);
  const size_t Txz = (size_t)h->Tx, Tz = (size_t)h->T;
  double* const res = h->res.p;
  int st = NAGP_OK;
  h->has_x = false; h->has_eig = false;
  API_HIP(nagp_gppad_lap_hess, hipMemcpy(res + h->r.x, x, (size_t)h->n * Txz * 8, hipMemcpyHostToDevice));
  run_batches("nagp_gppad_lap_hess", st, h->n, h->nb, nullptr, 0, nullptr, [](int, int) {},
    [&](int i0, int nbk, int) {
      LapPar pp = lap_par(h, i0, nbk);
      pp.out = res + h->r.d + (size_t)i0 * Tz;
      hipLaunchKernelGGL(lap_sample_kernel<1>, dim3((unsigned)((h->T + LAP_NT - 1) / LAP_NT), (unsigned)nbk), dim3(LAP_NT), 0, 0, pp);
    }, [](int, int) {});
  if (d) API_HIP(nagp_gppad_lap_hess, hipMemcpy(d, res + h->r.d, (size_t)h->n * Tz * 8, hipMemcpyDeviceToHost));
  h->has_x = st == NAGP_OK;
  return st;
}

static int lap_set_flags(nagp_gppad_lap* h, const std::vector<double>& f) {
  int st = NAGP_OK;
  API_HIP(nagp_gppad_lap, hipMemcpy(h->bat.p + h->b.fl, f.data(), f.size() * 8, hipMemcpyHostToDevice));
  return st;
}

extern "C" int nagp_gppad_lap_apply(nagp_gppad_lap* h, const double* v, double* Av) {
  if (!h || !v || !Av) FAIL(NAGP_EINVAL, "null argument");
  if (!h->has_x) FAIL(NAGP_EINVAL, "nagp_gppad_lap_hess sets the point first");
  if (hipSetDevice(h->device) != hipSuccess) FAIL(NAGP_EHIP, "hipSetDevice(%d)", h->device);
  const size_t Txz = (size_t)h->Tx;
  double* const bat = h->bat.p;
  int st = NAGP_OK;
  run_batches("nagp_gppad_lap_apply", st, h->n, h->nb, nullptr, 0, nullptr,
    [&](int i0, int nbk) {
      API_HIP(nagp_gppad_lap_apply, hipMemcpy(bat + h->b.r, v + (size_t)i0 * Txz, (size_t)nbk * Txz * 8, hipMemcpyHostToDevice));
      if (st == NAGP_OK) st = lap_set_flags(h, std::vector<double>((size_t)nbk, 1.0));
    },
    [&](int i0, int nbk, int) {
      LapPar pp = lap_par(h, i0, nbk);
      pp.in = bat + h->b.r; pp.out = bat + h->b.tmp;
      lap_sandwich<1>(h, pp, i0, nbk);
      pp.in = bat + h->b.tmp; pp.out = bat + h->b.r;
      lap_sandwich<0>(h, pp, i0, nbk);
    },
    [&](int i0, int nbk) { API_HIP(nagp_gppad_lap_apply, hipMemcpy(Av + (size_t)i0 * Txz, bat + h->b.r, (size_t)nbk * Txz * 8, hipMemcpyDeviceToHost)); });
  return st;
}

// Varx of the batch [i0, i0 + nbk) from the Ritz vectors in the xv slots: Varx = varx, then one sandwich per Ritz vector, k ascending.
// lam (K x nbk, slot-major) holds max(lambda, 0), NaN where problem q has no k-th pair.
static int lap_varx_batch(nagp_gppad_lap* h, int i0, int nbk, int K, const std::vector<double>& lam) {
  const size_t Txz = (size_t)h->Tx;
  double* const res = h->res.p; double* const bat = h->bat.p;
  int st = NAGP_OK;
  std::vector<double> v0((size_t)nbk * Txz);
  for (int q = 0; q < nbk; ++q) std::fill(v0.begin() + (size_t)q * Txz, v0.begin() + (size_t)(q + 1) * Txz, h->varx[(size_t)(i0 + q)]);
  API_HIP(nagp_gppad_lap_varx, hipMemcpy(res + h->r.var + (size_t)i0 * Txz, v0.data(), v0.size() * 8, hipMemcpyHostToDevice));
  if (K > 0) API_HIP(nagp_gppad_lap_varx, hipMemcpy(bat + h->b.lam, lam.data(), (size_t)K * nbk * 8, hipMemcpyHostToDevice));
  for (int k = 0; k < K && st == NAGP_OK; ++k) {
    LapPar pp = lap_par(h, i0, nbk);
    pp.in = bat + h->b.xv + (size_t)k * nbk * Txz; pp.out = res + h->r.var + (size_t)i0 * Txz; pp.sc = bat + h->b.lam + (size_t)k * nbk;
    lap_sandwich<3>(h, pp, i0, nbk);
  }
  API_HIP(nagp_gppad_lap_varx, hipGetLastError());
  API_HIP(nagp_gppad_lap_varx, hipDeviceSynchronize());
  return st;
}

extern "C" int nagp_gppad_lap_eig(nagp_gppad_lap* h, int32_t nev, double tresh, double tolconv, const double* vstart, double* lmb, int32_t* nconv,
                                  int32_t* info, double* anorm, double* xv) {
  g_gppad_lap_ms = 0.0;
  if (!h || !vstart || !lmb || !nconv) FAIL(NAGP_EINVAL, "null argument");
  if (!h->has_x) FAIL(NAGP_EINVAL, "nagp_gppad_lap_hess sets the point first");
  if (nev < 1) FAIL(NAGP_EINVAL, "nev = %d", nev);
  if (!(tresh > 0.0) || !(tolconv > 0.0)) FAIL(NAGP_EINVAL, "tresh = %g, tolconv = %g: > 0", tresh, tolconv);
  if (hipSetDevice(h->device) != hipSuccess) FAIL(NAGP_EHIP, "hipSetDevice(%d)", h->device);
  const size_t Txz = (size_t)h->Tx, jz = (size_t)h->jmax;
  const int jmax = h->jmax;
  double* const bat = h->bat.p;
  const LapBat& b = h->b;
  h->has_eig = false;
  h->lmb.assign((size_t)h->n * jz, NAN); h->nconv.assign((size_t)h->n, 0);
  int st = NAGP_OK;
  for (int i0 = 0; i0 < h->n && st == NAGP_OK; i0 += h->nb) {
    const int nbk = std::min(h->nb, h->n - i0);
    const size_t slot = (size_t)nbk * Txz;
    const dim3 ge((unsigned)h->nwe, (unsigned)nbk), g1((unsigned)((nbk + 63) / 64));
    std::vector<LanczosControl> ctl((size_t)nbk);
    std::vector<double> flag((size_t)nbk, 1.0), al((size_t)nbk), be((size_t)nbk), h1((size_t)nbk * jz * 2);
    API_HIP(nagp_gppad_lap_eig, hipMemcpy(bat + b.r, vstart + (size_t)i0 * Txz, slot * 8, hipMemcpyHostToDevice));
    if (st == NAGP_OK) st = lap_set_flags(h, flag);
    if (st != NAGP_OK) break;
    (void)hipEventRecord(h->bat.ev[0], 0);
    auto norm_of_r = [&](LapPar pp) {                                    // the |r|^2 partials of the update kernel, then beta = sqrt of their sum
      pp.out = bat + b.r; pp.np = h->nwe;
      hipLaunchKernelGGL(lap_update_kernel<0>, ge, dim3(LAP_NT), 0, 0, pp);
      pp.root = 1; pp.res = bat + b.be;
      hipLaunchKernelGGL(lap_finish_kernel<0>, g1, dim3(64), 0, 0, pp, nbk);
    };
    { LapPar pp = lap_par(h, i0, nbk); pp.j = -1; norm_of_r(pp); }
    API_HIP(nagp_gppad_lap_eig, hipMemcpy(be.data(), bat + b.be, (size_t)nbk * 8, hipMemcpyDeviceToHost));
    for (int q = 0; q < nbk; ++q) ctl[(size_t)q].start(nev, jmax, tresh, tolconv, be[(size_t)q]);
    for (int step = 0; step < jmax && st == NAGP_OK; ++step) {
      double* const vj = bat + b.V + (size_t)step * slot;
      LapPar pp = lap_par(h, i0, nbk);
      pp.in = bat + b.r; pp.out = vj; pp.sc = bat + b.be;                // v_j = r / beta_j
      hipLaunchKernelGGL(lap_sample_kernel<2>, ge, dim3(LAP_NT), 0, 0, pp);
      pp.in = vj; pp.out = bat + b.tmp;
      lap_sandwich<1>(h, pp, i0, nbk);
      pp.in = bat + b.tmp; pp.out = bat + b.r; pp.j = step; pp.va = vj; pp.vb = step ? vj - slot : vj;
      lap_sandwich<2>(h, pp, i0, nbk);
      pp.np = h->N1; pp.root = 0; pp.res = bat + b.al;                   // alpha_j = r . v_j
      hipLaunchKernelGGL(lap_finish_kernel<0>, g1, dim3(64), 0, 0, pp, nbk);
      pp.sc = bat + b.al;                                                // r -= alpha_j v_j, beta_{j+1} = |r|
      norm_of_r(pp);
      API_HIP(nagp_gppad_lap_eig, hipGetLastError());
      API_HIP(nagp_gppad_lap_eig, hipMemcpy(al.data(), bat + b.al, (size_t)nbk * 8, hipMemcpyDeviceToHost));
      API_HIP(nagp_gppad_lap_eig, hipMemcpy(be.data(), bat + b.be, (size_t)nbk * 8, hipMemcpyDeviceToHost));
      if (st != NAGP_OK) break;
      bool any = false;
      for (int q = 0; q < nbk; ++q)
        if (flag[(size_t)q] >= 1.0 && ctl[(size_t)q].step(al[(size_t)q], be[(size_t)q])) { flag[(size_t)q] = 2.0; any = true; }
      if (any) {                                                         // LanczosGPPAD.m:55-63 for the problems with flag 2
        st = lap_set_flags(h, flag);
        LapPar rp = lap_par(h, i0, nbk);
        rp.j = step; rp.va = vj; rp.in = bat + b.r; rp.out = bat + b.r; rp.res = bat + b.h1; rp.lev = 2.0;
        if (step > 0 && st == NAGP_OK) {
          hipLaunchKernelGGL(lap_h1_kernel<0>, dim3((unsigned)step, (unsigned)nbk), dim3(LAP_NT), 0, 0, rp);
          hipLaunchKernelGGL(lap_sample_kernel<3>, ge, dim3(LAP_NT), 0, 0, rp);
          API_HIP(nagp_gppad_lap_eig, hipMemcpy(h1.data(), bat + b.h1, h1.size() * 8, hipMemcpyDeviceToHost));
          bool again = false;
          for (int q = 0; q < nbk && st == NAGP_OK; ++q)
            if (flag[(size_t)q] == 2.0 && norm2_two_columns(h1.data() + (size_t)q * jz * 2, step) > 10.0 * std::sqrt(2.220446049250313e-16)) { flag[(size_t)q] = 3.0; again = true; }
          if (again && st == NAGP_OK) {
            st = lap_set_flags(h, flag);
            rp.lev = 3.0;
            hipLaunchKernelGGL(lap_h1_kernel<0>, dim3((unsigned)step, (unsigned)nbk), dim3(LAP_NT), 0, 0, rp);
            hipLaunchKernelGGL(lap_sample_kernel<3>, ge, dim3(LAP_NT), 0, 0, rp);
            rp.lev = 2.0;
          }
        }
        // r -= v_j (v_j' r): the two dot products of "basis vector" v_j land in sc[2 q], sc[2 q + 1]
        rp.q = vj; rp.jmax = 1; rp.res = bat + b.sc;
        hipLaunchKernelGGL(lap_h1_kernel<0>, dim3(1, (unsigned)nbk), dim3(LAP_NT), 0, 0, rp);
        rp.sc = bat + b.sc + 1; rp.ss = 2; rp.np = h->nwe;
        hipLaunchKernelGGL(lap_update_kernel<0>, ge, dim3(LAP_NT), 0, 0, rp);
        for (int q = 0; q < nbk; ++q) if (flag[(size_t)q] >= 2.0) { ctl[(size_t)q].after_reorth(); flag[(size_t)q] = 1.0; }
      }
      bool left = false;
      for (int q = 0; q < nbk; ++q) {
        if (flag[(size_t)q] < 1.0) continue;
        ctl[(size_t)q].finish_step();
        if (ctl[(size_t)q].done) flag[(size_t)q] = 0.0; else left = true;
      }
      if (st == NAGP_OK) st = lap_set_flags(h, flag);
      if (!left) break;
    }
    if (st != NAGP_OK) break;
    // the Ritz pairs: s on the host, xv = V s on the device, then Varx
    std::vector<double> S((size_t)nbk * jz * jz, 0.0), steps((size_t)nbk), lam;
    int K = 0;
    for (int q = 0; q < nbk; ++q) {
      LanczosControl& c = ctl[(size_t)q];
      std::vector<double> l;
      if (!c.ritz(l, S.data() + (size_t)q * jz * jz, jmax)) { c.status = LAP_NO_QL; l.clear(); }
      const size_t p = (size_t)(i0 + q);
      h->nconv[p] = (int)l.size();
      std::copy(l.begin(), l.end(), h->lmb.begin() + p * jz);
      flag[(size_t)q] = (double)l.size(); steps[(size_t)q] = (double)c.j;
      K = std::max(K, (int)l.size());
      if (info) { info[3 * p] = c.j; info[3 * p + 1] = c.reorths; info[3 * p + 2] = c.status; }
      if (anorm) anorm[p] = c.anorm;
    }
    lam.assign((size_t)std::max(K, 1) * nbk, NAN);
    for (int q = 0; q < nbk; ++q)
      for (int k = 0; k < h->nconv[(size_t)(i0 + q)]; ++k) lam[(size_t)k * nbk + q] = std::max(h->lmb[(size_t)(i0 + q) * jz + k], 0.0);
    if (K > 0) {
      st = lap_set_flags(h, flag);
      API_HIP(nagp_gppad_lap_eig, hipMemcpy(bat + b.S, S.data(), S.size() * 8, hipMemcpyHostToDevice));
      API_HIP(nagp_gppad_lap_eig, hipMemcpy(bat + b.sc, steps.data(), (size_t)nbk * 8, hipMemcpyHostToDevice));
      if (st == NAGP_OK) {
        LapPar pp = lap_par(h, i0, nbk);
        pp.sc = bat + b.sc; pp.out = bat + b.xv;
        hipLaunchKernelGGL(lap_ritz_kernel<0>, dim3((unsigned)h->nwe, (unsigned)((K + LAP_KT - 1) / LAP_KT), (unsigned)nbk), dim3(LAP_NT), 0, 0, pp);
      }
    }
    if (st == NAGP_OK) st = lap_varx_batch(h, i0, nbk, K, lam);
    (void)hipEventRecord(h->bat.ev[1], 0);
    API_HIP(nagp_gppad_lap_eig, hipEventSynchronize(h->bat.ev[1]));
    { float t = 0.f; if (st == NAGP_OK && hipEventElapsedTime(&t, h->bat.ev[0], h->bat.ev[1]) == hipSuccess) g_gppad_lap_ms += t; }
    if (xv)
      for (int q = 0; q < nbk && st == NAGP_OK; ++q)
        if (h->nconv[(size_t)(i0 + q)] > 0)
          API_HIP(nagp_gppad_lap_eig, hipMemcpy2D(xv + (size_t)(i0 + q) * jz * Txz, Txz * 8, bat + b.xv + (size_t)q * Txz, slot * 8, Txz * 8, (size_t)h->nconv[(size_t)(i0 + q)], hipMemcpyDeviceToHost));
  }
  if (st != NAGP_OK) return st;
  std::copy(h->lmb.begin(), h->lmb.end(), lmb);
  for (int p = 0; p < h->n; ++p) nconv[p] = h->nconv[(size_t)p];
  h->has_eig = true;
  return st;
}

extern "C" int nagp_gppad_lap_varx(nagp_gppad_lap* h, int32_t K, const double* xv, const double* lmb, double* Varx, int64_t* n_negative) {
  if (!h || !Varx) FAIL(NAGP_EINVAL, "null argument");
  if ((xv != nullptr) != (lmb != nullptr)) FAIL(NAGP_EINVAL, "xv and lmb are given together");
  if (xv && (K < 0 || K > h->jmax)) FAIL(NAGP_EINVAL, "K = %d: 0 to jmax = %d pairs", K, h->jmax);
  if (!xv && !h->has_eig) FAIL(NAGP_EINVAL, "nagp_gppad_lap_eig leaves the Ritz pairs first");
  if (hipSetDevice(h->device) != hipSuccess) FAIL(NAGP_EHIP, "hipSetDevice(%d)", h->device);
  const size_t Txz = (size_t)h->Tx;
  int st = NAGP_OK;
  if (xv) {
    h->has_eig = false;                                                  // the resident Varx is no longer that of the eigen-solve
    for (int i0 = 0; i0 < h->n && st == NAGP_OK; i0 += h->nb) {
      const int nbk = std::min(h->nb, h->n - i0);
      std::vector<double> lam((size_t)std::max(K, 1) * nbk, NAN);
      for (int q = 0; q < nbk; ++q) {
        for (int k = 0; k < K; ++k) { const double l = lmb[(size_t)(i0 + q) * K + k]; lam[(size_t)k * nbk + q] = l < 0.0 ? 0.0 : l; }
        if (K > 0) API_HIP(nagp_gppad_lap_varx, hipMemcpy2D(h->bat.p + h->b.xv + (size_t)q * Txz, (size_t)nbk * Txz * 8, xv + (size_t)(i0 + q) * K * Txz, Txz * 8, Txz * 8, (size_t)K, hipMemcpyHostToDevice));
      }
      if (st == NAGP_OK) st = lap_varx_batch(h, i0, nbk, K, lam);
    }
  }
  API_HIP(nagp_gppad_lap_varx, hipMemcpy(Varx, h->res.p + h->r.var, (size_t)h->n * Txz * 8, hipMemcpyDeviceToHost));
  if (n_negative && st == NAGP_OK)
    for (int p = 0; p < h->n; ++p) {
      int64_t c = 0;
      for (size_t e = 0; e < Txz; ++e) c += Varx[(size_t)p * Txz + e] < 0.0;
      n_negative[p] = c;
    }
  return st;
}

extern "C" int nagp_gppad_lap_obj(nagp_gppad_lap* h, double* Obj) {
  if (!h || !Obj) FAIL(NAGP_EINVAL, "null argument");
  if (!h->has_x) FAIL(NAGP_EINVAL, "nagp_gppad_lap_hess sets the point first");
  if (hipSetDevice(h->device) != hipSuccess) FAIL(NAGP_EHIP, "hipSetDevice(%d)", h->device);
  const size_t Txz = (size_t)h->Tx, jz = (size_t)h->jmax;
  double* const res = h->res.p; double* const bat = h->bat.p;
  int st = NAGP_OK;
  run_batches("nagp_gppad_lap_obj", st, h->n, h->nb, nullptr, 0, nullptr, [](int, int) {},
    [&](int i0, int nbk, int) {                                          // GetGPObjFast.m's two sums by the kernels of nagp_gppad.hpp, without the gradient
      GppadPar gp{};
      gp.T = h->T; gp.Tx = h->Tx; gp.N1 = h->N1; gp.N2 = h->N2; gp.lcb = h->lcb; gp.nwg = h->N1; gp.tw = h->tw; gp.vary_stride = h->vary_stride; gp.ic_stride = h->Tx;
      gp.x = res + h->r.x + (size_t)i0 * Txz; gp.y = res + h->r.y + (size_t)i0 * h->T; gp.vary = res + h->r.vy + (h->vary_stride ? (size_t)i0 * h->T : (size_t)i0);
      gp.ic = res + h->r.ic + (size_t)i0 * Txz; gp.varx = res + h->r.vx + i0; gp.mux = res + h->r.mu + i0; gp.varc = res + h->r.vc + i0;
      gp.work = reinterpret_cast<double2*>(bat + h->b.wk); gp.part = bat + h->b.pt;
      if (h->N1 == 1) hipLaunchKernelGGL(gppad_lds_kernel<0>, dim3((unsigned)nbk), dim3(h->nt), h->lds, 0, gp);
      else {
        const dim3 grid((unsigned)h->N1, (unsigned)nbk);
        hipLaunchKernelGGL(gppad_colf_kernel<0>, grid, dim3(h->nt), h->lds, 0, gp);
        hipLaunchKernelGGL(gppad_row_kernel<0>, grid, dim3(h->nt), h->lds, 0, gp);
        hipLaunchKernelGGL(gppad_coli_kernel<0>, grid, dim3(h->nt), h->lds, 0, gp);
      }
      LapPar pp = lap_par(h, i0, nbk);
      pp.np = h->N1; pp.res = bat + h->b.ob;
      hipLaunchKernelGGL(lap_finish_kernel<1>, dim3((unsigned)((nbk + 63) / 64)), dim3(64), 0, 0, pp, nbk);
    },
    [&](int i0, int nbk) { API_HIP(nagp_gppad_lap_obj, hipMemcpy(Obj + (size_t)i0 * 3, bat + h->b.ob, (size_t)nbk * 3 * 8, hipMemcpyDeviceToHost)); });
  for (int p = 0; p < h->n && st == NAGP_OK; ++p) {                      // Obj0 = -1/2 sum_k log|1 + max(lmb_k, 0)|, k ascending; NaN before an eigen-solve
    double s = 0.0;
    for (int k = 0; h->has_eig && k < h->nconv[(size_t)p]; ++k) s += std::log(std::fabs(1.0 + std::max(h->lmb[(size_t)p * jz + k], 0.0)));
    Obj[(size_t)p * 3] = h->has_eig ? -0.5 * s : NAN;
  }
  return st;
}
