// part of nagp_api.hip: fixed-point NMF of experiments/nmf/nmf_fp.m / nmf_inf_fp.m, a batch of problems on one data matrix (see include/nagp.h, nagp_nmf.hpp)
constexpr size_t NMF_BUDGET_BYTES = (size_t)8 << 30;      // device memory of one call: the problems run in device batches under it
static thread_local double g_nmf_ms = 0.0;

typedef void (*NmfFn)(NmfPar);
static const NmfFn nmf_pass_tab[17] = {nullptr, nmf_pass_kernel<1>, nmf_pass_kernel<2>, nmf_pass_kernel<3>, nmf_pass_kernel<4>, nmf_pass_kernel<5>,
                                       nmf_pass_kernel<6>, nmf_pass_kernel<7>, nmf_pass_kernel<8>, nmf_pass_kernel<9>, nmf_pass_kernel<10>,
                                       nmf_pass_kernel<11>, nmf_pass_kernel<12>, nmf_pass_kernel<13>, nmf_pass_kernel<14>, nmf_pass_kernel<15>,
                                       nmf_pass_kernel<16>};

extern "C" int nagp_nmf_timings(double* ms) { return timings_out(ms, &g_nmf_ms, 1); }

extern "C" int nagp_nmf_fp(int32_t n_problems, int64_t T, int32_t D, int32_t K, const double* A, const double* vary, const double* W0,
                           const double* H0, int32_t n_its, int32_t update_w, double* W, double* H, double* Obj, int32_t device) {
  g_nmf_ms = 0.0;                                           // a call that is refused or fails reports no time of an earlier one
  if (!A || !W0 || !H0) FAIL(NAGP_EINVAL, "null argument");
  if (n_problems < 1 || T < 1 || D < 1 || K < 1 || n_its < 0) FAIL(NAGP_EINVAL, "bad sizes (n_problems=%d T=%lld D=%d K=%d n_its=%d)", n_problems, (long long)T, D, K, n_its);
  if (D > 64) FAIL(NAGP_EUNSUPPORTED, "D=%d: at most 64 channels", D);
  if (K > 16) FAIL(NAGP_EUNSUPPORTED, "K=%d: at most 16 components", K);
  const size_t TD = (size_t)T * D, TK = (size_t)T * K, KD = (size_t)K * D;
  for (size_t e = 0; e < TD; ++e) {
    if (!std::isfinite(A[e]) || A[e] < 0.0) FAIL(NAGP_EINVAL, "A[%zu] = %g: the data must be finite and >= 0", e, A[e]);
    if (vary && (!std::isfinite(vary[e]) || vary[e] < 0.0)) FAIL(NAGP_EINVAL, "vary[%zu] = %g: the noise must be finite and >= 0", e, vary[e]);
  }
  for (size_t e = 0, n = (size_t)n_problems * TK; e < n; ++e)
    if (!std::isfinite(H0[e]) || !(H0[e] > 0.0)) FAIL(NAGP_EINVAL, "H0[%zu] = %g: the activations must be finite and > 0", e, H0[e]);
  for (int q = 0; q < n_problems; ++q) {
    const double* w = W0 + (size_t)q * KD;
    bool row[16] = {false, false, false, false, false, false, false, false, false, false, false, false, false, false, false, false};
    for (int d = 0; d < D; ++d) {
      bool col = false;
      for (int k = 0; k < K; ++k) {
        const double x = w[k + (size_t)d * K];
        if (!std::isfinite(x) || x < 0.0) FAIL(NAGP_EINVAL, "W0(%d, %d) of problem %d = %g: the weights must be finite and >= 0", k, d, q, x);
        if (x > 0.0) { col = true; row[k] = true; }
      }
      if (!col) FAIL(NAGP_EINVAL, "column %d of W0 of problem %d is all zero", d, q);
    }
    for (int k = 0; k < K; ++k)
      if (!row[k]) FAIL(NAGP_EINVAL, "row %d of W0 of problem %d is all zero", k, q);
  }
  const int n_obj = (update_w ? 2 : 1) * n_its;
  if (n_its == 0) {                                         // the inputs go through
    if (W) memcpy(W, W0, (size_t)n_problems * KD * sizeof(double));
    if (H) memcpy(H, H0, (size_t)n_problems * TK * sizeof(double));
    return NAGP_OK;
  }
  const DevSwitches dev_sw = read_dev_switches();
  const int nwg = (int)((T + NMF_NT - 1) / NMF_NT);
  // the budget rule of include/nagp.h
  const size_t fixed = 8 * (vary ? 2 : 1) * TD + 4096;
  const size_t per_problem = 8 * (TK + KD + (size_t)nwg * (2 * KD + 2) + (size_t)n_obj);
  const size_t budget = budget_bytes(dev_sw.budget_mb[DevSwitches::NMF], NMF_BUDGET_BYTES);
  const BatchPlan bp = batch_plan((size_t)n_problems, budget, fixed, per_problem);
  if (!bp.ok) FAIL(NAGP_ENOMEM, "one problem takes %zu B of device memory (budget %zu B)", fixed + per_problem, budget);
  if (hipSetDevice(device) != hipSuccess) FAIL(NAGP_EHIP, "hipSetDevice(%d)", device);
  const NmfBlock o = nmf_block((size_t)T, (size_t)D, (size_t)K, (size_t)nwg, (size_t)n_obj, vary != nullptr, bp.nb);
  DevBlock blk;
  API_ALLOC(blk, device, o.total); double* const dev = blk.p;
  int st = NAGP_OK;
  API_HIP(nagp_nmf_fp, hipMemcpy(dev + o.a, A, TD * 8, hipMemcpyHostToDevice));
  if (vary) API_HIP(nagp_nmf_fp, hipMemcpy(dev + o.v, vary, TD * 8, hipMemcpyHostToDevice));
  const NmfFn kp = nmf_pass_tab[K], kfin = update_w ? nmf_finish_kernel<true> : nmf_finish_kernel<false>;
  const size_t lds_p = nmf_pass_lds_doubles(K, D) * sizeof(double), lds_f = nmf_finish_lds_doubles(K, D) * sizeof(double);
  if (st == NAGP_OK) st = set_lds(kp, lds_p);
  if (st == NAGP_OK) st = set_lds(kfin, lds_f);
  API_HIP(nagp_nmf_fp, blk.events(2));
  NmfPar np{};
  np.T = T; np.D = D; np.K = K; np.nwg = nwg; np.A = dev + o.a; np.vary = vary ? dev + o.v : nullptr;
  np.W = dev + o.w; np.H = dev + o.h; np.pw = dev + o.pw; np.po = dev + o.po; np.Obj = dev + o.ob; np.n_obj = n_obj;
  run_batches("nagp_nmf_fp", st, n_problems, (int)bp.nb, blk.ev, 2, &g_nmf_ms,
    [&](int i0, int nbk) {
      API_HIP(nagp_nmf_fp, hipMemcpy(dev + o.w, W0 + (size_t)i0 * KD, (size_t)nbk * KD * 8, hipMemcpyHostToDevice));
      API_HIP(nagp_nmf_fp, hipMemcpy(dev + o.h, H0 + (size_t)i0 * TK, (size_t)nbk * TK * 8, hipMemcpyHostToDevice));
    }, [&](int, int nbk, int) {
      // every iteration is one pass and one finish; with update_w the second objective of iteration l is formed by the pass of
      // iteration l + 1 and that of the last iteration by a closing pass.  Nothing waits on the host until all of it is enqueued.
      for (int l = 0; l <= n_its; ++l) {
        const bool closing = l == n_its;
        if (closing && !update_w) break;
        np.update_h = closing ? 0 : 1;
        np.update_w = (update_w && !closing) ? 1 : 0;
        np.obj_prev = (update_w && l > 0) ? 2 * (l - 1) + 1 : -1;
        np.obj_new = closing ? -1 : (update_w ? 2 * l : l);
        hipLaunchKernelGGL(kp, dim3((unsigned)nwg, (unsigned)nbk), dim3(NMF_NT), lds_p, 0, np);
        hipLaunchKernelGGL(kfin, dim3((unsigned)nbk), dim3(NMF_FIN_NT), lds_f, 0, np);
      }
    }, [&](int i0, int nbk) {
      if (W) API_HIP(nagp_nmf_fp, hipMemcpy(W + (size_t)i0 * KD, dev + o.w, (size_t)nbk * KD * 8, hipMemcpyDeviceToHost));
      if (H) API_HIP(nagp_nmf_fp, hipMemcpy(H + (size_t)i0 * TK, dev + o.h, (size_t)nbk * TK * 8, hipMemcpyDeviceToHost));
      if (Obj) API_HIP(nagp_nmf_fp, hipMemcpy(Obj + (size_t)i0 * n_obj, dev + o.ob, (size_t)nbk * n_obj * 8, hipMemcpyDeviceToHost));
    });
  return st;
}
