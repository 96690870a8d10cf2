// part of nagp_api.hip: the squared-exponential basis-function convolution of basis2SEGP.m and the three objectives on top of it --
// getObj_fitSE_basis_func.m (nagp_sebf_fit_*), getObj_nmf_log_norm.m and getObj_nmf_log_norm_inf.m (nagp_tnmf_*) -- see include/nagp.h and
// nagp_sebf.hpp: the resident handles and the one-shot calls on top of them.  The row arithmetic of nagp_tnmf is that of nagp_nmf_temp
// without a prior on logH := conv(X) + mux: its two kernels run on the device-resident array as they are.
constexpr size_t SEBF_BUDGET_BYTES = (size_t)1 << 30;     // device memory of the per-evaluation buffers: the problems run in device batches under it
static thread_local double g_sebf_ms[3] = {0.0, 0.0, 0.0};

typedef void (*SebfFn)(SebfPar);

// the basis of a handle: taps built on the host (once), uploaded with their offsets, tau and the per-column constant
struct SebfBasis {
  DevBlock blk; SebfRes r{}; int n_tc = 0;
  const double* taps() const { return blk.p + r.tp; }
  const int64_t* off() const { return reinterpret_cast<const int64_t*>(blk.p + r.of); }
  const int* tau() const { return reinterpret_cast<const int*>(blk.p + r.ta); }
  const double* c() const { return blk.p + r.c; }
  double* e() const { return blk.p + r.e; }
};

static int sebf_basis_upload(const char* fn, SebfBasis& b, int device, size_t n_tc, size_t n_taps, const double* lenx, const double* varx, const int64_t* tau,
                             const double* c, size_t n_targets) {
  b.n_tc = (int)n_tc; b.r = sebf_res(n_taps, n_tc, n_targets);
  API_ALLOC(b.blk, device, b.r.total);
  std::vector<double> taps; std::vector<int64_t> off; std::vector<int> ta;
  try { taps.resize(n_taps); off.resize(n_tc); ta.resize(n_tc); }
  catch (const std::bad_alloc&) { FAIL(NAGP_ENOMEM, "%s: host memory for %zu taps", fn, n_taps); }
  size_t at = 0;
  for (size_t k = 0; k < n_tc; ++k) {
    off[k] = (int64_t)at; ta[k] = (int)tau[k];
    sebf_build_taps(lenx[k], varx[k], tau[k], taps.data() + at);
    at += (size_t)(2 * tau[k] + 1);
  }
  int st = NAGP_OK;
  API_HIP_S(fn, hipMemcpy(b.blk.p + b.r.tp, taps.data(), n_taps * 8, hipMemcpyHostToDevice));
  API_HIP_S(fn, hipMemcpy(b.blk.p + b.r.of, off.data(), n_tc * 8, hipMemcpyHostToDevice));
  API_HIP_S(fn, hipMemcpy(b.blk.p + b.r.ta, ta.data(), n_tc * 4, hipMemcpyHostToDevice));
  if (c) API_HIP_S(fn, hipMemcpy(b.blk.p + b.r.c, c, n_tc * 8, hipMemcpyHostToDevice));
  return st;
}

// columns [q0, q0 + n_cols) of the handle's batch buffers; tap columns from tc0 on (tmod = 0) or shared (tmod = kc)
static void sebf_launch(SebfFn k, const SebfBasis& b, int64_t T, int ntile, int n_cols, int kc, int64_t ldp, int tmod, int tc0, const double* Z, const double* E, double* Y) {
  SebfPar p{};
  p.T = T; p.ntile = ntile; p.kc = kc; p.ldp = ldp; p.tmod = tmod; p.tau = b.tau() + tc0; p.off = b.off() + tc0; p.taps = b.taps(); p.c = b.c() + tc0;
  p.Z = Z; p.E = E; p.Y = Y;
  hipLaunchKernelGGL(k, dim3((unsigned)n_cols * (unsigned)ntile), dim3(SEBF_NT), 0, 0, p);
}

extern "C" int nagp_tnmf_timings(double* ms) { return timings_out(ms, g_sebf_ms, 3); }

// ---------------------------------------------------------------------------------------------------------------- basis2SEGP
extern "C" int nagp_sebf_conv(int32_t n_cols, int64_t T, const double* Z, const double* lenx, const double* varx, double tol, double* Y, int32_t device) {
  g_sebf_ms[0] = g_sebf_ms[1] = g_sebf_ms[2] = 0.0;
  const DevSwitches dev_sw = read_dev_switches();
  const size_t budget = budget_bytes(dev_sw.budget_mb[DevSwitches::SEBF], SEBF_BUDGET_BYTES);
  SebfShape sh;
  const std::unique_ptr<int64_t[]> tau(new (std::nothrow) int64_t[n_cols > 0 ? (size_t)n_cols : 1]);
  if (!tau) FAIL(NAGP_ENOMEM, "host memory for %d values of tau", n_cols);
  {
    char msg[512];
    const int chk = sebf_conv_check(n_cols, T, Z, lenx, varx, tol, Y, budget, &sh, tau.get(), msg, sizeof msg);
    if (chk != SEBF_OK) { g_last_error = msg; return chk; }
  }
  const BatchPlan bp = batch_plan((size_t)n_cols, budget, 0, sh.per_problem);
  if (hipSetDevice(device) != hipSuccess) FAIL(NAGP_EHIP, "hipSetDevice(%d)", device);
  SebfBasis b;
  int st = sebf_basis_upload("nagp_sebf_conv", b, device, (size_t)n_cols, sh.n_taps, lenx, varx, tau.get(), nullptr, 0);
  if (st != NAGP_OK) return st;
  const SebfBat o = sebf_conv_bat((size_t)T, bp.nb);
  DevBlock bat;
  API_ALLOC(bat, device, o.total);
  API_HIP(nagp_sebf_conv, bat.events(2));
  run_batches("nagp_sebf_conv", st, n_cols, (int)bp.nb, bat.ev, 2, g_sebf_ms,
    [&](int i0, int nbk) { API_HIP(nagp_sebf_conv, hipMemcpy(bat.p + o.x, Z + (size_t)i0 * T, (size_t)nbk * T * 8, hipMemcpyHostToDevice)); },
    [&](int i0, int nbk, int) { sebf_launch(sebf_conv_kernel<SEBF_CONV>, b, T, sh.ntile, nbk, 1, T, 0, i0, bat.p + o.x, nullptr, bat.p + o.out); },
    [&](int i0, int nbk) { API_HIP(nagp_sebf_conv, hipMemcpy(Y + (size_t)i0 * T, bat.p + o.out, (size_t)nbk * T * 8, hipMemcpyDeviceToHost)); });
  return st;
}

// ---------------------------------------------------------------------------------------------------------------- getObj_fitSE_basis_func
struct nagp_sebf_fit {
  int device = 0, n = 0, nb = 0, ntile = 1;
  int64_t T = 0;
  SebfBasis basis; DevBlock bat; SebfBat b{};
};

extern "C" void nagp_sebf_fit_destroy(nagp_sebf_fit* h) { delete h; }

extern "C" int nagp_sebf_fit_create(nagp_sebf_fit** handle, int32_t n_problems, int64_t T, const double* x, const double* lenx, const double* varx, double tol,
                                    int32_t device) {
  if (handle) *handle = nullptr;
  if (!handle) FAIL(NAGP_EINVAL, "null argument");
  static_assert(SEBF_EINVAL == NAGP_EINVAL && SEBF_EUNSUPPORTED == NAGP_EUNSUPPORTED && SEBF_OK == NAGP_OK, "status codes of nagp_sebf_check.hpp");
  const DevSwitches dev_sw = read_dev_switches();
  const size_t budget = budget_bytes(dev_sw.budget_mb[DevSwitches::SEBF], SEBF_BUDGET_BYTES);
  SebfShape sh;
  const std::unique_ptr<int64_t[]> tau(new (std::nothrow) int64_t[n_problems > 0 ? (size_t)n_problems : 1]);
  if (!tau) FAIL(NAGP_ENOMEM, "host memory for %d values of tau", n_problems);
  {
    char msg[512];
    const int chk = sebf_fit_check(n_problems, T, x, lenx, varx, tol, budget, &sh, tau.get(), msg, sizeof msg);
    if (chk != SEBF_OK) { g_last_error = msg; return chk; }
  }
  std::unique_ptr<nagp_sebf_fit> h(new nagp_sebf_fit());
  h->device = device; h->n = n_problems; h->T = T; h->ntile = sh.ntile;
  const BatchPlan bp = batch_plan((size_t)n_problems, budget, 0, sh.per_problem);
  h->nb = (int)bp.nb;
  if (hipSetDevice(device) != hipSuccess) FAIL(NAGP_EHIP, "hipSetDevice(%d)", device);
  int st = sebf_basis_upload("nagp_sebf_fit_create", h->basis, device, (size_t)n_problems, sh.n_taps, lenx, varx, tau.get(), nullptr, (size_t)n_problems * T);
  if (st != NAGP_OK) return st;
  h->b = sebf_fit_bat((size_t)T, bp.nb);
  API_ALLOC(h->bat, device, h->b.total);
  API_HIP(nagp_sebf_fit_create, h->bat.events(4));
  API_HIP(nagp_sebf_fit_create, hipMemcpy(h->basis.e(), x, (size_t)n_problems * T * 8, hipMemcpyHostToDevice));
  if (st == NAGP_OK) *handle = h.release();
  return st;
}

extern "C" int nagp_sebf_fit_eval(nagp_sebf_fit* h, const double* z, double* Obj, double* dObj) {
  g_sebf_ms[0] = g_sebf_ms[1] = g_sebf_ms[2] = 0.0;
  if (!h || !z || !Obj) FAIL(NAGP_EINVAL, "null argument");
  if (hipSetDevice(h->device) != hipSuccess) FAIL(NAGP_EHIP, "hipSetDevice(%d)", h->device);
  const int64_t T = h->T;
  double* const bat = h->bat.p; const SebfBat& b = h->b;
  int st = NAGP_OK;
  run_batches("nagp_sebf_fit_eval", st, h->n, h->nb, h->bat.ev, 4, g_sebf_ms,
    [&](int i0, int nbk) { API_HIP(nagp_sebf_fit_eval, hipMemcpy(bat + b.x, z + (size_t)i0 * T, (size_t)nbk * T * 8, hipMemcpyHostToDevice)); },
    [&](int i0, int nbk, int s) {
      if (s == 0) sebf_launch(sebf_conv_kernel<SEBF_SUBE>, h->basis, T, h->ntile, nbk, 1, T, 0, i0, bat + b.x, h->basis.e() + (size_t)i0 * T, bat + b.lh);   // dx = xHat - x
      if (s == 1) {
        SebfSumPar sp{};
        sp.T = T; sp.n1 = T; sp.n2 = T; sp.ld1 = T; sp.ld2 = T; sp.a1 = bat + b.lh; sp.a2 = bat + b.x; sp.Obj = bat + b.ob;
        hipLaunchKernelGGL(sebf_sumsq_kernel<SEBF_SS_FIT>, dim3((unsigned)nbk), dim3(SEBF_NT), 0, 0, sp);
      }
      if (s == 2 && dObj) sebf_launch(sebf_conv_kernel<SEBF_ADDE_T>, h->basis, T, h->ntile, nbk, 1, T, 0, i0, bat + b.lh, bat + b.x, bat + b.out);   // (conv(dx) + z) / T
    }, [&](int i0, int nbk) {
      API_HIP(nagp_sebf_fit_eval, hipMemcpy(Obj + i0, bat + b.ob, (size_t)nbk * 8, hipMemcpyDeviceToHost));
      if (dObj) API_HIP(nagp_sebf_fit_eval, hipMemcpy(dObj + (size_t)i0 * T, bat + b.out, (size_t)nbk * T * 8, hipMemcpyDeviceToHost));
    });
  return st;
}

extern "C" int nagp_sebf_fit_obj(int32_t n_problems, int64_t T, const double* z, const double* x, const double* lenx, const double* varx, double tol, double* Obj,
                                 double* dObj, int32_t device) {
  g_sebf_ms[0] = g_sebf_ms[1] = g_sebf_ms[2] = 0.0;
  if (!z || !Obj) FAIL(NAGP_EINVAL, "null argument");
  nagp_sebf_fit* h = nullptr;
  const int st = nagp_sebf_fit_create(&h, n_problems, T, x, lenx, varx, tol, device);
  const std::unique_ptr<nagp_sebf_fit> owner(h);
  return st != NAGP_OK ? st : nagp_sebf_fit_eval(h, z, Obj, dObj);
}

// ---------------------------------------------------------------------------------------------------------------- getObj_nmf_log_norm(_inf)
struct nagp_tnmf {
  int device = 0, n = 0, nb = 0, D = 0, K = 0, learn = 0, nwg = 1, ntile = 1, has_vary = 0;
  int64_t T = 0;
  size_t nx = 0;
  SebfBasis basis; DevBlock res, bat;
  NmftRes r{}; SebfBat b{};
};

extern "C" void nagp_tnmf_destroy(nagp_tnmf* h) { delete h; }

extern "C" int nagp_tnmf_create(nagp_tnmf** handle, int32_t n_problems, int64_t T, int32_t D, int32_t K, const double* A, const double* vary, const double* W,
                                const double* lenx, const double* mux, const double* varx, double tol, int32_t device) {
  if (handle) *handle = nullptr;
  if (!handle) FAIL(NAGP_EINVAL, "null argument");
  const DevSwitches dev_sw = read_dev_switches();
  const size_t budget = budget_bytes(dev_sw.budget_mb[DevSwitches::SEBF], SEBF_BUDGET_BYTES);
  SebfShape sh;
  int64_t tau[16];
  {
    char msg[512];
    const int chk = tnmf_host_check(n_problems, T, D, K, A, vary, W, lenx, mux, varx, tol, budget, &sh, tau, msg, sizeof msg);
    if (chk != SEBF_OK) { g_last_error = msg; return chk; }
  }
  const size_t TD = (size_t)T * D, KD = (size_t)K * D, nz = (size_t)n_problems;
  std::unique_ptr<nagp_tnmf> h(new nagp_tnmf());
  h->device = device; h->n = n_problems; h->T = T; h->D = D; h->K = K; h->learn = sh.learn; h->has_vary = vary ? 1 : 0;
  h->nwg = sh.nwg; h->ntile = sh.ntile; h->nx = sh.nx;
  const BatchPlan bp = batch_plan(nz, budget, 0, sh.per_problem);
  h->nb = (int)bp.nb;
  if (hipSetDevice(device) != hipSuccess) FAIL(NAGP_EHIP, "hipSetDevice(%d)", device);
  int st = sebf_basis_upload("nagp_tnmf_create", h->basis, device, (size_t)K, sh.n_taps, lenx, varx, tau, mux, 0);
  if (st != NAGP_OK) return st;
  h->r = nmft_res(nz, (size_t)T, (size_t)D, (size_t)K, vary != nullptr, W != nullptr);
  h->b = tnmf_bat(h->nx, (size_t)D, (size_t)K, h->learn != 0, (size_t)h->nwg, bp.nb);
  API_ALLOC(h->res, device, h->r.total);
  API_ALLOC(h->bat, device, h->b.total);
  double* const res = h->res.p;
  st = set_lds(nmft_pass_tab[h->learn ? 1 : 0][K], nmft_pass_lds_doubles(K, D, h->learn) * sizeof(double));
  if (st == NAGP_OK) st = h->learn ? set_lds(nmft_finish_kernel<true>, nmft_finish_lds_doubles(K, D) * sizeof(double))
                                   : set_lds(nmft_finish_kernel<false>, nmft_finish_lds_doubles(K, D) * sizeof(double));
  API_HIP(nagp_tnmf_create, h->bat.events(4));
  API_HIP(nagp_tnmf_create, hipMemcpy(res + h->r.a, A, TD * 8, hipMemcpyHostToDevice));
  if (vary) API_HIP(nagp_tnmf_create, hipMemcpy(res + h->r.vy, vary, TD * 8, hipMemcpyHostToDevice));
  if (W) API_HIP(nagp_tnmf_create, hipMemcpy(res + h->r.w, W, nz * KD * 8, hipMemcpyHostToDevice));
  API_HIP(nagp_tnmf_create, hipMemset(res + h->r.pr, 0, 3 * (size_t)K * 8));
  if (st == NAGP_OK) *handle = h.release();
  return st;
}

extern "C" int nagp_tnmf_eval(nagp_tnmf* h, const double* x, double* Obj, double* dObj) {
  g_sebf_ms[0] = g_sebf_ms[1] = g_sebf_ms[2] = 0.0;
  if (!h || !x || !Obj) FAIL(NAGP_EINVAL, "null argument");
  if (hipSetDevice(h->device) != hipSuccess) FAIL(NAGP_EHIP, "hipSetDevice(%d)", h->device);
  const int K = h->K, D = h->D;
  const int64_t T = h->T, nx = (int64_t)h->nx;
  const size_t KD = (size_t)K * D, TK = (size_t)T * K;
  const NmftFn kp = nmft_pass_tab[h->learn ? 1 : 0][K];
  const NmftFn kfin = h->learn ? nmft_finish_kernel<true> : nmft_finish_kernel<false>;
  const size_t lds_p = nmft_pass_lds_doubles(K, D, h->learn && dObj) * sizeof(double), lds_f = nmft_finish_lds_doubles(K, D) * sizeof(double);
  double* const res = h->res.p; double* const bat = h->bat.p;
  const NmftRes& r = h->r; const SebfBat& b = h->b;
  NmftPar pp{};                                             // the row kernels of nagp_nmf_temp.hpp on logH = conv(X) + mux, no prior
  pp.T = T; pp.D = D; pp.K = K; pp.nwg = h->nwg; pp.prior = NMFT_NONE; pp.grad = dObj ? 1 : 0; pp.nx = nx;
  pp.A = res + r.a; pp.vary = h->has_vary ? res + r.vy : nullptr; pp.x = bat + b.lh;
  pp.prm = res + r.pr; pp.dObj = bat + b.dg; pp.pw = bat + b.pw; pp.po = bat + b.po; pp.Obj = bat + b.ob;
  int st = NAGP_OK;
  run_batches("nagp_tnmf_eval", st, h->n, h->nb, h->bat.ev, 4, g_sebf_ms,
    [&](int i0, int nbk) { API_HIP(nagp_tnmf_eval, hipMemcpy(bat + b.x, x + (size_t)i0 * h->nx, (size_t)nbk * h->nx * 8, hipMemcpyHostToDevice)); },
    [&](int i0, int nbk, int s) {
      if (s == 0) {                                         // logH = conv(X) + mux; log W rides along
        sebf_launch(sebf_conv_kernel<SEBF_ADDC>, h->basis, T, h->ntile, nbk * K, K, nx, K, 0, bat + b.x, nullptr, bat + b.lh);
        if (h->learn) API_HIP(nagp_tnmf_eval, hipMemcpy2DAsync(bat + b.lh + TK, h->nx * 8, bat + b.x + TK, h->nx * 8, KD * 8, (size_t)nbk, hipMemcpyDeviceToDevice, 0));
      }
      if (s == 1) {
        pp.Wg = h->learn ? nullptr : res + r.w + (size_t)i0 * KD;
        hipLaunchKernelGGL(kp, dim3((unsigned)h->nwg, (unsigned)nbk), dim3(NMFT_NT), lds_p, 0, pp);
        hipLaunchKernelGGL(kfin, dim3((unsigned)nbk), dim3(NMFT_FIN_NT), lds_f, 0, pp);
      }
      if (s == 2) {                                         // Obj += 1/2 sum X^2 / T;  dX = conv(dlogh) + X / T; dlogw as the row kernels left it
        SebfSumPar sp{};
        sp.T = T; sp.n1 = (int64_t)TK; sp.ld1 = nx; sp.a1 = bat + b.x; sp.Obj = bat + b.ob;
        hipLaunchKernelGGL(sebf_sumsq_kernel<SEBF_SS_TNMF>, dim3((unsigned)nbk), dim3(SEBF_NT), 0, 0, sp);
        if (dObj) {
          sebf_launch(sebf_conv_kernel<SEBF_ADD_ET>, h->basis, T, h->ntile, nbk * K, K, nx, K, 0, bat + b.dg, bat + b.x, bat + b.out);
          if (h->learn) API_HIP(nagp_tnmf_eval, hipMemcpy2DAsync(bat + b.out + TK, h->nx * 8, bat + b.dg + TK, h->nx * 8, KD * 8, (size_t)nbk, hipMemcpyDeviceToDevice, 0));
        }
      }
    }, [&](int i0, int nbk) {
      API_HIP(nagp_tnmf_eval, hipMemcpy(Obj + i0, bat + b.ob, (size_t)nbk * 8, hipMemcpyDeviceToHost));
      if (dObj) API_HIP(nagp_tnmf_eval, hipMemcpy(dObj + (size_t)i0 * h->nx, bat + b.out, (size_t)nbk * h->nx * 8, hipMemcpyDeviceToHost));
    });
  return st;
}

extern "C" int nagp_tnmf_obj(int32_t n_problems, int64_t T, int32_t D, int32_t K, const double* x, const double* A, const double* vary, const double* W,
                             const double* lenx, const double* mux, const double* varx, double tol, double* Obj, double* dObj, int32_t device) {
  g_sebf_ms[0] = g_sebf_ms[1] = g_sebf_ms[2] = 0.0;
  if (!x || !Obj) FAIL(NAGP_EINVAL, "null argument");
  nagp_tnmf* h = nullptr;
  const int st = nagp_tnmf_create(&h, n_problems, T, D, K, A, vary, W, lenx, mux, varx, tol, device);
  const std::unique_ptr<nagp_tnmf> owner(h);
  return st != NAGP_OK ? st : nagp_tnmf_eval(h, x, Obj, dObj);
}
