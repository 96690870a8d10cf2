// part of nagp_api.hip: objective and gradient of the conjugate-gradient NMF with temporal priors, experiments/nmf/getObj_nmf_temp.m
// and getObj_nmf_temp_inf.m (see include/nagp.h, nagp_nmf_temp.hpp): the resident handle and the one-shot call on top of it.
constexpr size_t NMFT_BUDGET_BYTES = (size_t)1 << 30;     // device memory of the per-evaluation buffers: the problems run in device batches under it
static thread_local double g_nmft_ms = 0.0;
#define NMFT_HIP(fn, x) do { if (st == NAGP_OK) { hipError_t _e = (x); if (_e != hipSuccess) { g_last_error = std::string(#fn ": " #x " -> ") + hipGetErrorString(_e); (void)hipGetLastError(); st = NAGP_EHIP; } } } while (0)

struct nagp_nmf_temp {
  int device = 0, n = 0, nb = 0, D = 0, K = 0, prior = 0, learn = 0, nwg = 1, n_po = 1, has_vary = 0, valu = 0;
  int64_t T = 0;
  size_t nx = 0;
  double* res = nullptr;      // resident: A | vary | W (inference form) | muinf, varinf, lam
  double* bat = nullptr;      // per device batch: x | dObj | pw | po | Obj
  size_t o_vy = 0, o_w = 0, o_pr = 0, o_dg = 0, o_pw = 0, o_po = 0, o_ob = 0;
  hipEvent_t ev[2] = {nullptr, nullptr};
};

typedef void (*NmftFn)(NmftPar);
#define NMFT_ROW(L, M) {nullptr, nmft_pass_kernel<1, L, M>, nmft_pass_kernel<2, L, M>, nmft_pass_kernel<3, L, M>, nmft_pass_kernel<4, L, M>, nmft_pass_kernel<5, L, M>, \
  nmft_pass_kernel<6, L, M>, nmft_pass_kernel<7, L, M>, nmft_pass_kernel<8, L, M>, nmft_pass_kernel<9, L, M>, nmft_pass_kernel<10, L, M>, nmft_pass_kernel<11, L, M>,       \
  nmft_pass_kernel<12, L, M>, nmft_pass_kernel<13, L, M>, nmft_pass_kernel<14, L, M>, nmft_pass_kernel<15, L, M>, nmft_pass_kernel<16, L, M>}
static const NmftFn nmft_pass_tab[3][17] = {NMFT_ROW(false, true), NMFT_ROW(true, true), NMFT_ROW(true, false)};   // inference, learning, learning on the VALU
#undef NMFT_ROW

extern "C" int nagp_nmf_temp_timings(double* ms) {
  if (!ms) FAIL(NAGP_EINVAL, "null argument");
  ms[0] = g_nmft_ms;
  return NAGP_OK;
}

extern "C" void nagp_nmf_temp_destroy(nagp_nmf_temp* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  for (int i = 0; i < 2; ++i) if (h->ev[i]) (void)hipEventDestroy(h->ev[i]);
  if (h->res) (void)hipFree(h->res);
  if (h->bat) (void)hipFree(h->bat);
  delete h;
}

extern "C" int nagp_nmf_temp_create(nagp_nmf_temp** handle, int32_t n_problems, int64_t T, int32_t D, int32_t K, int32_t prior, const double* A,
                                    const double* vary, const double* W, const double* muinf, const double* varinf, const double* lam, int32_t device) {
  if (handle) *handle = nullptr;
  if (!handle) FAIL(NAGP_EINVAL, "null argument");
  static_assert(NMFT_EINVAL == NAGP_EINVAL && NMFT_EUNSUPPORTED == NAGP_EUNSUPPORTED && NMFT_OK == NAGP_OK, "status codes of nagp_nmf_temp_check.hpp");
  static_assert(NMFT_NONE == NAGP_NMFT_NONE && NMFT_TG == NAGP_NMFT_TG && NMFT_IG == NAGP_NMFT_IG, "prior codes of nagp_nmf_temp.hpp");
  const DevSwitches dev_sw = read_dev_switches();
  const size_t budget = dev_sw.nmft_budget_mb ? (size_t)dev_sw.nmft_budget_mb << 20 : NMFT_BUDGET_BYTES;
  NmftShape sh;
  {   // every check of include/nagp.h and the budget rule: nagp_nmf_temp_check.hpp
    char msg[512];
    const int chk = nmft_host_check(n_problems, T, D, K, prior, A, vary, W, muinf, varinf, lam, budget, &sh, msg, sizeof msg);
    if (chk != NMFT_OK) { g_last_error = msg; return chk; }
  }
  const size_t TD = (size_t)T * D, KD = (size_t)K * D, nz = (size_t)n_problems, per_problem = sh.per_problem;
  nagp_nmf_temp* h = new nagp_nmf_temp();
  h->device = device; h->n = n_problems; h->T = T; h->D = D; h->K = K; h->prior = prior; h->learn = sh.learn; h->has_vary = vary ? 1 : 0;
  h->valu = dev_sw.nmft_valu ? 1 : 0;
  h->nwg = sh.nwg; h->n_po = sh.n_po; h->nx = sh.nx;
  h->nb = (int)std::min<size_t>({nz, budget / per_problem, (size_t)32768});
  if (hipSetDevice(device) != hipSuccess) { delete h; FAIL(NAGP_EHIP, "hipSetDevice(%d)", device); }
  const size_t nbz = (size_t)h->nb;
  h->o_vy = TD; h->o_w = h->o_vy + (vary ? TD : 0); h->o_pr = h->o_w + (W ? nz * KD : 0);
  const size_t res_total = h->o_pr + 3 * (size_t)K + 2;
  h->o_dg = nbz * h->nx; h->o_pw = h->o_dg + nbz * h->nx; h->o_po = h->o_pw + (h->learn ? nbz * h->nwg * KD : 0); h->o_ob = h->o_po + nbz * h->nwg * h->n_po;
  const size_t bat_total = h->o_ob + nbz + 2;
  if (hipMalloc(&h->res, res_total * 8) != hipSuccess) { (void)hipGetLastError(); delete h; FAIL(NAGP_ENOMEM, "hipMalloc(%zu)", res_total * 8); }
  if (hipMalloc(&h->bat, bat_total * 8) != hipSuccess) { (void)hipGetLastError(); nagp_nmf_temp_destroy(h); FAIL(NAGP_ENOMEM, "hipMalloc(%zu)", bat_total * 8); }
  int st = NAGP_OK;
  const int row = h->learn ? (h->valu ? 2 : 1) : 0;
  st = set_lds(nmft_pass_tab[row][K], nmft_pass_lds_doubles(K, D, h->learn) * sizeof(double));
  if (st == NAGP_OK) st = h->learn ? set_lds(nmft_finish_kernel<true>, nmft_finish_lds_doubles(K, D) * sizeof(double))
                                   : set_lds(nmft_finish_kernel<false>, nmft_finish_lds_doubles(K, D) * sizeof(double));
  for (int i = 0; i < 2; ++i) NMFT_HIP(nagp_nmf_temp_create, hipEventCreate(&h->ev[i]));
  NMFT_HIP(nagp_nmf_temp_create, hipMemcpy(h->res, A, TD * 8, hipMemcpyHostToDevice));
  if (vary) NMFT_HIP(nagp_nmf_temp_create, hipMemcpy(h->res + h->o_vy, vary, TD * 8, hipMemcpyHostToDevice));
  if (W) NMFT_HIP(nagp_nmf_temp_create, hipMemcpy(h->res + h->o_w, W, nz * KD * 8, hipMemcpyHostToDevice));
  std::vector<double> prm(3 * (size_t)K, 0.0);
  for (int k = 0; k < K; ++k) {
    if (prior == NAGP_NMFT_IG) prm[k] = muinf[k];
    if (prior != NAGP_NMFT_NONE) { prm[K + k] = varinf[k]; prm[2 * K + k] = lam[k]; }
  }
  NMFT_HIP(nagp_nmf_temp_create, hipMemcpy(h->res + h->o_pr, prm.data(), prm.size() * 8, hipMemcpyHostToDevice));
  if (st != NAGP_OK) { nagp_nmf_temp_destroy(h); return st; }
  *handle = h;
  return NAGP_OK;
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
  int st = NAGP_OK;
  for (int i0 = 0; i0 < h->n && st == NAGP_OK; i0 += h->nb) {
    const int nbk = std::min(h->nb, h->n - i0);
    NMFT_HIP(nagp_nmf_temp_eval, hipMemcpy(h->bat, x + (size_t)i0 * h->nx, (size_t)nbk * h->nx * 8, hipMemcpyHostToDevice));
    NmftPar pp{};
    pp.T = h->T; pp.D = D; pp.K = K; pp.nwg = h->nwg; pp.prior = h->prior; pp.grad = dObj ? 1 : 0; pp.nx = (int64_t)h->nx;
    pp.A = h->res; pp.vary = h->has_vary ? h->res + h->o_vy : nullptr; pp.x = h->bat; pp.Wg = h->learn ? nullptr : h->res + h->o_w + (size_t)i0 * KD;
    pp.prm = h->res + h->o_pr; pp.dObj = h->bat + h->o_dg; pp.pw = h->bat + h->o_pw; pp.po = h->bat + h->o_po; pp.Obj = h->bat + h->o_ob;
    if (st == NAGP_OK) {
      (void)hipEventRecord(h->ev[0], 0);
      hipLaunchKernelGGL(kp, dim3((unsigned)h->nwg, (unsigned)nbk), dim3(NMFT_NT), lds_p, 0, pp);
      hipLaunchKernelGGL(kfin, dim3((unsigned)nbk), dim3(NMFT_FIN_NT), lds_f, 0, pp);
      (void)hipEventRecord(h->ev[1], 0);
    }
    NMFT_HIP(nagp_nmf_temp_eval, hipGetLastError());
    NMFT_HIP(nagp_nmf_temp_eval, hipDeviceSynchronize());
    if (st == NAGP_OK) { float ms = 0.f; if (hipEventElapsedTime(&ms, h->ev[0], h->ev[1]) == hipSuccess) g_nmft_ms += ms; }
    NMFT_HIP(nagp_nmf_temp_eval, hipMemcpy(Obj + i0, h->bat + h->o_ob, (size_t)nbk * 8, hipMemcpyDeviceToHost));
    if (dObj) NMFT_HIP(nagp_nmf_temp_eval, hipMemcpy(dObj + (size_t)i0 * h->nx, h->bat + h->o_dg, (size_t)nbk * h->nx * 8, hipMemcpyDeviceToHost));
  }
  return st;
}

extern "C" int nagp_nmf_temp_obj(int32_t n_problems, int64_t T, int32_t D, int32_t K, int32_t prior, const double* x, const double* A, const double* vary,
                                 const double* W, const double* muinf, const double* varinf, const double* lam, double* Obj, double* dObj, int32_t device) {
  g_nmft_ms = 0.0;
  if (!x || !Obj) FAIL(NAGP_EINVAL, "null argument");
  nagp_nmf_temp* h = nullptr;
  int st = nagp_nmf_temp_create(&h, n_problems, T, D, K, prior, A, vary, W, muinf, varinf, lam, device);
  if (st != NAGP_OK) return st;
  st = nagp_nmf_temp_eval(h, x, Obj, dObj);
  nagp_nmf_temp_destroy(h);
  return st;
}
#undef NMFT_HIP
