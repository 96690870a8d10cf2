// part of nagp_api.hip: objective and gradient of the conjugate-gradient NMF with temporal priors, experiments/nmf/getObj_nmf_temp.m
// and getObj_nmf_temp_inf.m (see include/nagp.h, nagp_nmf_temp.hpp): the resident handle and the one-shot call on top of it.
constexpr size_t NMFT_BUDGET_BYTES = (size_t)1 << 30;     // device memory of the per-evaluation buffers: the problems run in device batches under it
static thread_local double g_nmft_ms = 0.0;

struct nagp_nmf_temp {
  int device = 0, n = 0, nb = 0, D = 0, K = 0, prior = 0, learn = 0, nwg = 1, n_po = 1, has_vary = 0, valu = 0;
  int64_t T = 0;
  size_t nx = 0;
  DevBlock res, bat;          // resident / per device batch (with the two events), laid out by r / b
  NmftRes r{}; NmftBat b{};
};

typedef void (*NmftFn)(NmftPar);
#define NMFT_ROW(L, M) {nullptr, nmft_pass_kernel<1, L, M>, nmft_pass_kernel<2, L, M>, nmft_pass_kernel<3, L, M>, nmft_pass_kernel<4, L, M>, nmft_pass_kernel<5, L, M>, \
  nmft_pass_kernel<6, L, M>, nmft_pass_kernel<7, L, M>, nmft_pass_kernel<8, L, M>, nmft_pass_kernel<9, L, M>, nmft_pass_kernel<10, L, M>, nmft_pass_kernel<11, L, M>,       \
  nmft_pass_kernel<12, L, M>, nmft_pass_kernel<13, L, M>, nmft_pass_kernel<14, L, M>, nmft_pass_kernel<15, L, M>, nmft_pass_kernel<16, L, M>}
static const NmftFn nmft_pass_tab[3][17] = {NMFT_ROW(false, true), NMFT_ROW(true, true), NMFT_ROW(true, false)};   // inference, learning, learning on the VALU
#undef NMFT_ROW

extern "C" int nagp_nmf_temp_timings(double* ms) { return timings_out(ms, &g_nmft_ms, 1); }
extern "C" void nagp_nmf_temp_destroy(nagp_nmf_temp* h) { delete h; }

extern "C" int nagp_nmf_temp_create(nagp_nmf_temp** handle, int32_t n_problems, int64_t T, int32_t D, int32_t K, int32_t prior, const double* A,
                                    const double* vary, const double* W, const double* muinf, const double* varinf, const double* lam, int32_t device) {
  if (handle) *handle = nullptr;
  if (!handle) FAIL(NAGP_EINVAL, "null argument");
  static_assert(NMFT_EINVAL == NAGP_EINVAL && NMFT_EUNSUPPORTED == NAGP_EUNSUPPORTED && NMFT_OK == NAGP_OK, "status codes of nagp_nmf_temp_check.hpp");
  static_assert(NMFT_NONE == NAGP_NMFT_NONE && NMFT_TG == NAGP_NMFT_TG && NMFT_IG == NAGP_NMFT_IG, "prior codes of nagp_nmf_temp.hpp");
  const DevSwitches dev_sw = read_dev_switches();
  const size_t budget = budget_bytes(dev_sw.budget_mb[DevSwitches::NMFT], NMFT_BUDGET_BYTES);
  NmftShape sh;
  {   // every check of include/nagp.h and the budget rule: nagp_nmf_temp_check.hpp
    char msg[512];
    const int chk = nmft_host_check(n_problems, T, D, K, prior, A, vary, W, muinf, varinf, lam, budget, &sh, msg, sizeof msg);
    if (chk != NMFT_OK) { g_last_error = msg; return chk; }
  }
  const size_t TD = (size_t)T * D, KD = (size_t)K * D, nz = (size_t)n_problems;
  std::unique_ptr<nagp_nmf_temp> h(new nagp_nmf_temp());      // released to the caller at the end; every return before that frees it
  h->device = device; h->n = n_problems; h->T = T; h->D = D; h->K = K; h->prior = prior; h->learn = sh.learn; h->has_vary = vary ? 1 : 0;
  h->valu = dev_sw.nmft_valu ? 1 : 0;
  h->nwg = sh.nwg; h->n_po = sh.n_po; h->nx = sh.nx;
  const BatchPlan bp = batch_plan(nz, budget, 0, sh.per_problem);      // (nmft_host_check has refused a problem over the budget)
  h->nb = (int)bp.nb;
  if (hipSetDevice(device) != hipSuccess) FAIL(NAGP_EHIP, "hipSetDevice(%d)", device);
  h->r = nmft_res(nz, (size_t)T, (size_t)D, (size_t)K, vary != nullptr, W != nullptr);
  h->b = nmft_bat(h->nx, (size_t)D, (size_t)K, h->learn != 0, (size_t)h->nwg, (size_t)h->n_po, bp.nb);
  API_ALLOC(h->res, device, h->r.total);
  API_ALLOC(h->bat, device, h->b.total);
  double* const res = h->res.p;
  int st = NAGP_OK;
  const int row = h->learn ? (h->valu ? 2 : 1) : 0;
  st = set_lds(nmft_pass_tab[row][K], nmft_pass_lds_doubles(K, D, h->learn) * sizeof(double));
  if (st == NAGP_OK) st = h->learn ? set_lds(nmft_finish_kernel<true>, nmft_finish_lds_doubles(K, D) * sizeof(double))
                                   : set_lds(nmft_finish_kernel<false>, nmft_finish_lds_doubles(K, D) * sizeof(double));
  API_HIP(nagp_nmf_temp_create, h->bat.events(2));
  API_HIP(nagp_nmf_temp_create, hipMemcpy(res + h->r.a, A, TD * 8, hipMemcpyHostToDevice));
  if (vary) API_HIP(nagp_nmf_temp_create, hipMemcpy(res + h->r.vy, vary, TD * 8, hipMemcpyHostToDevice));
  if (W) API_HIP(nagp_nmf_temp_create, hipMemcpy(res + h->r.w, W, nz * KD * 8, hipMemcpyHostToDevice));
  std::vector<double> prm(3 * (size_t)K, 0.0);
  for (int k = 0; k < K; ++k) {
    if (prior == NAGP_NMFT_IG) prm[k] = muinf[k];
    if (prior != NAGP_NMFT_NONE) { prm[K + k] = varinf[k]; prm[2 * K + k] = lam[k]; }
  }
  API_HIP(nagp_nmf_temp_create, hipMemcpy(res + h->r.pr, prm.data(), prm.size() * 8, hipMemcpyHostToDevice));
  if (st == NAGP_OK) *handle = h.release();
  return st;
}

extern "C" int nagp_nmf_temp_eval(nagp_nmf_temp* h, const double* x, double* Obj, double* dObj) {
  g_nmft_ms = 0.0;                                          // a call that is refused or fails reports no time of an earlier one
  if (!h || !x || !Obj) FAIL(NAGP_EINVAL, "null argument");
  if (hipSetDevice(h->device) != hipSuccess) FAIL(NAGP_EHIP, "hipSetDevice(%d)", h->device);
  const int K = h->K, D = h->D;
  const size_t KD = (size_t)K * D;
  const NmftFn kp = nmft_pass_tab[h->learn ? (h->valu ? 2 : 1) : 0][K];
  const NmftFn kfin = h->learn ? nmft_finish_kernel<true> : nmft_finish_kernel<false>;
  const size_t lds_p = nmft_pass_lds_doubles(K, D, h->learn && dObj) * sizeof(double), lds_f = nmft_finish_lds_doubles(K, D) * sizeof(double);
  double* const res = h->res.p; double* const bat = h->bat.p;
  const NmftRes& r = h->r; const NmftBat& b = h->b;
  NmftPar pp{};
  pp.T = h->T; pp.D = D; pp.K = K; pp.nwg = h->nwg; pp.prior = h->prior; pp.grad = dObj ? 1 : 0; pp.nx = (int64_t)h->nx;
  pp.A = res + r.a; pp.vary = h->has_vary ? res + r.vy : nullptr; pp.x = bat + b.x;
  pp.prm = res + r.pr; pp.dObj = bat + b.dg; pp.pw = bat + b.pw; pp.po = bat + b.po; pp.Obj = bat + b.ob;
  int st = NAGP_OK;
  run_batches("nagp_nmf_temp_eval", st, h->n, h->nb, h->bat.ev, 2, &g_nmft_ms,
    [&](int i0, int nbk) { API_HIP(nagp_nmf_temp_eval, hipMemcpy(bat + b.x, x + (size_t)i0 * h->nx, (size_t)nbk * h->nx * 8, hipMemcpyHostToDevice)); },
    [&](int i0, int nbk, int) {
      pp.Wg = h->learn ? nullptr : res + r.w + (size_t)i0 * KD;
      hipLaunchKernelGGL(kp, dim3((unsigned)h->nwg, (unsigned)nbk), dim3(NMFT_NT), lds_p, 0, pp);
      hipLaunchKernelGGL(kfin, dim3((unsigned)nbk), dim3(NMFT_FIN_NT), lds_f, 0, pp);
    }, [&](int i0, int nbk) {
      API_HIP(nagp_nmf_temp_eval, hipMemcpy(Obj + i0, bat + b.ob, (size_t)nbk * 8, hipMemcpyDeviceToHost));
      if (dObj) API_HIP(nagp_nmf_temp_eval, hipMemcpy(dObj + (size_t)i0 * h->nx, bat + b.dg, (size_t)nbk * h->nx * 8, hipMemcpyDeviceToHost));
    });
  return st;
}

extern "C" int nagp_nmf_temp_obj(int32_t n_problems, int64_t T, int32_t D, int32_t K, int32_t prior, const double* x, const double* A, const double* vary,
                                 const double* W, const double* muinf, const double* varinf, const double* lam, double* Obj, double* dObj, int32_t device) {
  g_nmft_ms = 0.0;
  if (!x || !Obj) FAIL(NAGP_EINVAL, "null argument");
  nagp_nmf_temp* h = nullptr;
  const int st = nagp_nmf_temp_create(&h, n_problems, T, D, K, prior, A, vary, W, muinf, varinf, lam, device);
  const std::unique_ptr<nagp_nmf_temp> owner(h);
  return st != NAGP_OK ? st : nagp_nmf_temp_eval(h, x, Obj, dObj);
}
