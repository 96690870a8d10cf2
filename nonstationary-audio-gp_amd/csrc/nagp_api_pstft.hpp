// part of nagp_api.hip: objective and gradient of the filterbank spectrum fit, get_Obj_pSTFT_{exp,matern32,matern52,all}.m (see include/nagp.h, nagp_pstft.hpp)
constexpr size_t PSTFT_BUDGET_BYTES = (size_t)1 << 30;    // device memory of one call: the problems run in device batches under it
static thread_local double g_pstft_ms = 0.0;

typedef void (*PstftFn)(PstftPar);
static const PstftFn pstft_pass_tab[4] = {pstft_pass_kernel<1>, pstft_pass_kernel<2>, pstft_pass_kernel<3>, pstft_pass_kernel<4>};
static const PstftFn pstft_finish_tab[4] = {pstft_finish_kernel<1>, pstft_finish_kernel<2>, pstft_finish_kernel<3>, pstft_finish_kernel<4>};

extern "C" int nagp_pstft_timings(double* ms) { return timings_out(ms, &g_pstft_ms, 1); }

extern "C" int nagp_pstft_obj(int32_t n_problems, int32_t kernel, int32_t form, int32_t D, int64_t N, const double* theta, const double* specTar,
                              int64_t spec_stride, const double* vary, const double* bet, const double* minVar, const double* limOm,
                              const double* limLam, double* Obj, double* dObj, int32_t device) {
  g_pstft_ms = 0.0;                                         // a call that is refused or fails reports no time of an earlier one
  if (!theta || !specTar || !vary || !bet || !minVar || !limOm || !limLam || !Obj) FAIL(NAGP_EINVAL, "null argument");
  if (n_problems < 1 || D < 1) FAIL(NAGP_EINVAL, "bad sizes (n_problems=%d D=%d)", n_problems, D);
  if (kernel < NAGP_PSTFT_EXP || kernel > NAGP_PSTFT_MATERN72) FAIL(NAGP_EUNSUPPORTED, "kernel %d: exp, matern32, matern52 and matern72 are served (se is not)", kernel);
  if (form != 0 && form != 1) FAIL(NAGP_EINVAL, "form = %d: 0 (closed) or 1 (generic)", form);
  if (form == 0 && kernel == NAGP_PSTFT_MATERN72) FAIL(NAGP_EUNSUPPORTED, "matern72 has no closed-form file: use form = 1 (get_Obj_pSTFT_all)");
  if (D > PSTFT_MAXD) FAIL(NAGP_EUNSUPPORTED, "D=%d: at most %d components", D, PSTFT_MAXD);
  if (N < 4) FAIL(NAGP_EINVAL, "N=%lld: at least 4 frequencies", (long long)N);
  if (spec_stride != 0 && spec_stride != N) FAIL(NAGP_EINVAL, "spec_stride = %lld: 0 (shared) or N", (long long)spec_stride);
  for (int d = 0; d < D; ++d) {
    if (!std::isfinite(minVar[d]) || minVar[d] < 0.0) FAIL(NAGP_EINVAL, "minVar[%d] = %g: finite and >= 0", d, minVar[d]);
    if (!std::isfinite(limOm[d]) || !std::isfinite(limOm[D + d]) || !(limOm[D + d] > limOm[d])) FAIL(NAGP_EINVAL, "limOm(%d, :) = [%g, %g]: finite, upper > lower", d, limOm[d], limOm[D + d]);
    if (!std::isfinite(limLam[d]) || !std::isfinite(limLam[D + d]) || !(limLam[D + d] > limLam[d])) FAIL(NAGP_EINVAL, "limLam(%d, :) = [%g, %g]: finite, upper > lower", d, limLam[d], limLam[D + d]);
    if (limLam[d] < 0.0 || limLam[D + d] > 1.0) FAIL(NAGP_EINVAL, "limLam(%d, :) = [%g, %g]: inside [0, 1], where every component's spectrum is >= 0", d, limLam[d], limLam[D + d]);
  }
  for (size_t e = 0, n = (size_t)n_problems * 3 * D; e < n; ++e)
    if (!std::isfinite(theta[e])) FAIL(NAGP_EINVAL, "theta[%zu] = %g", e, theta[e]);
  for (size_t e = 0, n = spec_stride ? (size_t)n_problems * N : (size_t)N; e < n; ++e)
    if (!std::isfinite(specTar[e]) || specTar[e] < 0.0) FAIL(NAGP_EINVAL, "specTar[%zu] = %g: the target spectrum must be finite and >= 0", e, specTar[e]);
  for (int q = 0; q < n_problems; ++q) {
    if (!std::isfinite(vary[q]) || vary[q] < 0.0) FAIL(NAGP_EINVAL, "vary[%d] = %g: finite and >= 0", q, vary[q]);
    if (!std::isfinite(bet[q])) FAIL(NAGP_EINVAL, "bet[%d] = %g", q, bet[q]);
    if (vary[q] == 0.0) {                                   // spec = 0 at every frequency unless one component has 0 < lam < 1
      bool pos = false;
      for (int d = 0; d < D && !pos; ++d) {
        const double lam = limLam[d] + (limLam[D + d] - limLam[d]) / (1.0 + std::exp(-theta[(size_t)q * 3 * D + 2 * D + d]));
        pos = lam > 0.0 && lam < 1.0;
      }
      if (!pos) FAIL(NAGP_EINVAL, "problem %d: vary = 0 and no component with 0 < lam < 1: the model spectrum is zero", q);
    }
  }
  const DevSwitches dev_sw = read_dev_switches();
  const int grad = dObj ? 1 : 0, n_out = grad ? 3 * D + 2 : 2;
  const int64_t nwg64 = (N + PSTFT_NT - 1) / PSTFT_NT;
  if (nwg64 > 0x7fffffff / n_out) FAIL(NAGP_EUNSUPPORTED, "N=%lld: too many frequencies", (long long)N);
  const int nwg = (int)nwg64;
  // the budget rule of include/nagp.h
  const size_t fixed = 8 * ((spec_stride ? 0 : (size_t)N) + 5 * (size_t)D) + 4096;
  const size_t per_problem = 8 * ((spec_stride ? (size_t)N : 0) + (size_t)nwg * n_out + 6 * (size_t)D + 3);
  const size_t budget = budget_bytes(dev_sw.budget_mb[DevSwitches::PSTFT], PSTFT_BUDGET_BYTES);
  const BatchPlan bp = batch_plan((size_t)n_problems, budget, fixed, per_problem);
  if (!bp.ok) FAIL(NAGP_EUNSUPPORTED, "one problem takes %zu B of device memory (budget %zu B)", fixed + per_problem, budget);
  if (hipSetDevice(device) != hipSuccess) FAIL(NAGP_EHIP, "hipSetDevice(%d)", device);
  const size_t Dz = (size_t)D, Nz = (size_t)N;
  const PstftBlock o = pstft_block(Dz, Nz, spec_stride != 0, (size_t)nwg, (size_t)n_out, bp.nb);
  DevBlock blk;
  API_ALLOC(blk, device, o.total); double* const dev = blk.p;
  int st = NAGP_OK;
  API_HIP(nagp_pstft_obj, hipMemcpy(dev + o.mv, minVar, Dz * 8, hipMemcpyHostToDevice));
  API_HIP(nagp_pstft_obj, hipMemcpy(dev + o.lo, limOm, 2 * Dz * 8, hipMemcpyHostToDevice));
  API_HIP(nagp_pstft_obj, hipMemcpy(dev + o.ll, limLam, 2 * Dz * 8, hipMemcpyHostToDevice));
  if (!spec_stride) API_HIP(nagp_pstft_obj, hipMemcpy(dev + o.ss, specTar, Nz * 8, hipMemcpyHostToDevice));
  const PstftFn kp = pstft_pass_tab[kernel], kfin = pstft_finish_tab[kernel];
  API_HIP(nagp_pstft_obj, blk.events(2));
  PstftPar pp{};
  pp.N = N; pp.D = D; pp.nwg = nwg; pp.grad = grad; pp.kappa = kernel == NAGP_PSTFT_MATERN72 ? std::sqrt(7.0 / 5.0) : 1.0;
  pp.theta = dev + o.th; pp.specTar = spec_stride ? dev + o.sp : dev + o.ss; pp.spec_stride = spec_stride; pp.vary = dev + o.vy; pp.bet = dev + o.bt;
  pp.minVar = dev + o.mv; pp.limOm = dev + o.lo; pp.limLam = dev + o.ll; pp.part = dev + o.pt; pp.Obj = dev + o.ob; pp.dObj = dev + o.dg;
  run_batches("nagp_pstft_obj", st, n_problems, (int)bp.nb, blk.ev, 2, &g_pstft_ms,
    [&](int i0, int nbk) {
      API_HIP(nagp_pstft_obj, hipMemcpy(dev + o.th, theta + (size_t)i0 * 3 * Dz, (size_t)nbk * 3 * Dz * 8, hipMemcpyHostToDevice));
      API_HIP(nagp_pstft_obj, hipMemcpy(dev + o.vy, vary + i0, (size_t)nbk * 8, hipMemcpyHostToDevice));
      API_HIP(nagp_pstft_obj, hipMemcpy(dev + o.bt, bet + i0, (size_t)nbk * 8, hipMemcpyHostToDevice));
      if (spec_stride) API_HIP(nagp_pstft_obj, hipMemcpy(dev + o.sp, specTar + (size_t)i0 * Nz, (size_t)nbk * Nz * 8, hipMemcpyHostToDevice));
    }, [&](int, int nbk, int) {
      hipLaunchKernelGGL(kp, dim3((unsigned)nwg, (unsigned)nbk), dim3(PSTFT_NT), 0, 0, pp);
      hipLaunchKernelGGL(kfin, dim3((unsigned)nbk), dim3(PSTFT_FIN_NT), 0, 0, pp);
    }, [&](int i0, int nbk) {
      API_HIP(nagp_pstft_obj, hipMemcpy(Obj + i0, dev + o.ob, (size_t)nbk * 8, hipMemcpyDeviceToHost));
      if (grad) API_HIP(nagp_pstft_obj, hipMemcpy(dObj + (size_t)i0 * 3 * Dz, dev + o.dg, (size_t)nbk * 3 * Dz * 8, hipMemcpyDeviceToHost));
    });
  return st;
}
