// part of nagp_api.hip: objective and gradient of the modulator prior fit, toolsGP/getObjSEGP.m on getGPSESpec.m (see include/nagp.h, nagp_segp.hpp)
constexpr size_t SEGP_BUDGET_BYTES = (size_t)1 << 30;     // device memory of one call: the problems run in device batches under it
static thread_local double g_segp_ms = 0.0;

typedef void (*SegpFn)(SegpPar);
static const SegpFn segp_pass_tab[3] = {segp_pass_kernel<1>, segp_pass_kernel<2>, segp_pass_kernel<3>};
static const SegpFn segp_finish_tab[3] = {segp_finish_kernel<1>, segp_finish_kernel<2>, segp_finish_kernel<3>};

extern "C" int nagp_segp_timings(double* ms) { return timings_out(ms, &g_segp_ms, 1); }

extern "C" int nagp_segp_obj(int32_t n_problems, int32_t n_param, int64_t T, const double* param, const double* specy, int64_t spec_stride,
                             const double* vary, const double* varx, double* Obj, double* dObj, int32_t device) {
  g_segp_ms = 0.0;                                          // a call that is refused or fails reports no time of an earlier one
  if (!param || !specy || !Obj) FAIL(NAGP_EINVAL, "null argument");
  if (n_problems < 1) FAIL(NAGP_EINVAL, "bad sizes (n_problems=%d)", n_problems);
  if (n_param < 1 || n_param > 3) FAIL(NAGP_EINVAL, "n_param = %d: 1 (log len), 2 (and log varx) or 3 (and log vary)", n_param);
  if (n_param <= 2 && !vary) FAIL(NAGP_EINVAL, "null vary with n_param = %d", n_param);
  if (n_param == 1 && !varx) FAIL(NAGP_EINVAL, "null varx with n_param = 1");
  if (T < 2) FAIL(NAGP_EINVAL, "T=%lld: at least 2 frequencies", (long long)T);
  if (spec_stride != 0 && spec_stride != T) FAIL(NAGP_EINVAL, "spec_stride = %lld: 0 (shared) or T", (long long)spec_stride);
  for (size_t e = 0, n = (size_t)n_problems * n_param; e < n; ++e)
    if (!std::isfinite(param[e])) FAIL(NAGP_EINVAL, "param[%zu] = %g", e, param[e]);
  for (size_t e = 0, n = spec_stride ? (size_t)n_problems * T : (size_t)T; e < n; ++e)
    if (!std::isfinite(specy[e]) || specy[e] < 0.0) FAIL(NAGP_EINVAL, "specy[%zu] = %g: the spectrum must be finite and >= 0", e, specy[e]);
  for (int q = 0; q < n_problems; ++q) {
    if (n_param <= 2 && (!std::isfinite(vary[q]) || !(vary[q] > 0.0))) FAIL(NAGP_EINVAL, "vary[%d] = %g: finite and > 0", q, vary[q]);
    if (n_param == 1 && (!std::isfinite(varx[q]) || varx[q] < 0.0)) FAIL(NAGP_EINVAL, "varx[%d] = %g: finite and >= 0", q, varx[q]);
  }
  const DevSwitches dev_sw = read_dev_switches();
  const int grad = dObj ? 1 : 0, n_out = grad ? 2 + n_param : 2;
  const int64_t nwg64 = (T + SEGP_NT - 1) / SEGP_NT;
  if (nwg64 > 0x7fffffff / SEGP_MAXOUT) FAIL(NAGP_EUNSUPPORTED, "T=%lld: too many frequencies", (long long)T);
  const int nwg = (int)nwg64;
  // the budget rule of include/nagp.h
  const size_t np = (size_t)n_param, Tz = (size_t)T;
  const size_t fixed = 8 * (spec_stride ? 0 : Tz) + 4096;
  const size_t per_problem = 8 * ((spec_stride ? Tz : 0) + (size_t)nwg * n_out + 2 * np + 3);
  const size_t budget = budget_bytes(dev_sw.budget_mb[DevSwitches::SEGP], SEGP_BUDGET_BYTES);
  const BatchPlan bp = batch_plan((size_t)n_problems, budget, fixed, per_problem);
  if (!bp.ok) FAIL(NAGP_EUNSUPPORTED, "one problem takes %zu B of device memory (budget %zu B)", fixed + per_problem, budget);
  if (hipSetDevice(device) != hipSuccess) FAIL(NAGP_EHIP, "hipSetDevice(%d)", device);
  const SegpBlock o = segp_block(np, Tz, spec_stride != 0, (size_t)nwg, (size_t)n_out, bp.nb);
  DevBlock blk;
  API_ALLOC(blk, device, o.total); double* const dev = blk.p;
  int st = NAGP_OK;
  if (!spec_stride) API_HIP(nagp_segp_obj, hipMemcpy(dev + o.ss, specy, Tz * 8, hipMemcpyHostToDevice));
  const SegpFn kp = segp_pass_tab[n_param - 1], kfin = segp_finish_tab[n_param - 1];
  API_HIP(nagp_segp_obj, blk.events(2));
  SegpPar pp{};
  pp.T = T; pp.nwg = nwg; pp.grad = grad; pp.param = dev + o.pa; pp.specy = spec_stride ? dev + o.sp : dev + o.ss; pp.spec_stride = spec_stride;
  pp.vary = dev + o.vy; pp.varx = dev + o.vx; pp.part = dev + o.pt; pp.Obj = dev + o.ob; pp.dObj = dev + o.dg;
  run_batches("nagp_segp_obj", st, n_problems, (int)bp.nb, blk.ev, 2, &g_segp_ms,
    [&](int i0, int nbk) {
      API_HIP(nagp_segp_obj, hipMemcpy(dev + o.pa, param + (size_t)i0 * np, (size_t)nbk * np * 8, hipMemcpyHostToDevice));
      if (n_param <= 2) API_HIP(nagp_segp_obj, hipMemcpy(dev + o.vy, vary + i0, (size_t)nbk * 8, hipMemcpyHostToDevice));
      if (n_param == 1) API_HIP(nagp_segp_obj, hipMemcpy(dev + o.vx, varx + i0, (size_t)nbk * 8, hipMemcpyHostToDevice));
      if (spec_stride) API_HIP(nagp_segp_obj, hipMemcpy(dev + o.sp, specy + (size_t)i0 * Tz, (size_t)nbk * Tz * 8, hipMemcpyHostToDevice));
    }, [&](int, int nbk, int) {
      hipLaunchKernelGGL(kp, dim3((unsigned)nwg, (unsigned)nbk), dim3(SEGP_NT), 0, 0, pp);
      hipLaunchKernelGGL(kfin, dim3((unsigned)nbk), dim3(SEGP_FIN_NT), 0, 0, pp);
    }, [&](int i0, int nbk) {
      API_HIP(nagp_segp_obj, hipMemcpy(Obj + i0, dev + o.ob, (size_t)nbk * 8, hipMemcpyDeviceToHost));
      if (grad) API_HIP(nagp_segp_obj, hipMemcpy(dObj + (size_t)i0 * np, dev + o.dg, (size_t)nbk * np * 8, hipMemcpyDeviceToHost));
    });
  return st;
}
