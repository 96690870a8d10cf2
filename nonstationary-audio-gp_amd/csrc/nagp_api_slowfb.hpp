// part of nagp_api.hip: stationary filterbank, exact form: Kalman filter / smoother with per-step observation variances (see include/nagp.h, nagp_slowfb.hpp)
constexpr size_t SFB_BUDGET_BYTES = (size_t)48 << 30;     // device memory of one call: the series run in device batches under it
static thread_local double g_sfb_ms[3] = {0.0, 0.0, 0.0};

typedef void (*SfbFn)(SfbPar);
#define SFB_TABLE(name) {nullptr, name<1>, name<2>, name<3>, name<4>, name<5>, name<6>, name<7>, name<8>}
static const SfbFn sfb_forward_tab[9] = SFB_TABLE(sfb_forward_kernel);
static const SfbFn sfb_backward_tab[9] = SFB_TABLE(sfb_backward_kernel);
static const SfbFn sfb_combine_tab[9] = SFB_TABLE(sfb_combine_kernel);
#undef SFB_TABLE

extern "C" int nagp_slowfb_timings(double* ms) { return timings_out(ms, g_sfb_ms, 3); }

extern "C" int nagp_slowfb_run(int32_t S, int32_t block, const double* A, const double* Q, const double* H, const double* P0,
                               int32_t n_series, const double* y, const double* vary, int64_t T, int32_t filter_only,
                               int32_t n_sub, const int32_t* sub_idx, double* lik, double* MS, double* Pdiag, double* Psub,
                               int32_t device) {
  g_sfb_ms[0] = g_sfb_ms[1] = g_sfb_ms[2] = 0.0;            // a call that is refused or fails reports no time of an earlier one
  if (!A || !Q || !H || !P0 || !y || !vary) FAIL(NAGP_EINVAL, "null argument");
  if (S < 1 || T < 1 || n_series < 1) FAIL(NAGP_EINVAL, "bad sizes (S=%d T=%lld n_series=%d)", S, (long long)T, n_series);
  if (block < 1 || S % block != 0) FAIL(NAGP_EINVAL, "block=%d does not divide S=%d", block, S);
  if (n_sub < 0 || (n_sub > 0) != (Psub != nullptr) || (n_sub > 0 && !sub_idx)) FAIL(NAGP_EINVAL, "Psub and n_sub=%d are not consistent", n_sub);
  for (int i = 0; i < n_sub; ++i)
    if (sub_idx[i] < 0 || sub_idx[i] >= S || (i > 0 && sub_idx[i] <= sub_idx[i - 1]))
      FAIL(NAGP_EINVAL, "sub_idx[%d] = %d: the indices must ascend strictly inside [0, S)", i, sub_idx[i]);
  if (!lik && !MS && !Pdiag && !Psub) FAIL(NAGP_EINVAL, "no output requested");
  for (size_t e = 0, n = (size_t)n_series * T; e < n; ++e)
    if (!(vary[e] >= 0.0) || !std::isfinite(vary[e])) FAIL(NAGP_EINVAL, "vary[%zu] = %g: an observation variance must be finite and >= 0", e, vary[e]);
  if (S > 128) FAIL(NAGP_EUNSUPPORTED, "S=%d: the covariance of a series lives in the LDS of one workgroup (S <= 128)", S);
  if (block > 8) FAIL(NAGP_EUNSUPPORTED, "block=%d: blocks of at most 8 states", block);
  for (int j = 0; j < S; ++j)
    for (int i = 0; i < S; ++i)
      if (i / block != j / block && (A[i + (size_t)j * S] != 0.0 || Q[i + (size_t)j * S] != 0.0))
        FAIL(NAGP_EUNSUPPORTED, "A or Q has a non-zero at (%d, %d), outside the blocks of %d states: dense transitions are not served", i, j, block);
  const DevSwitches dev_sw = read_dev_switches();
  const bool fo = filter_only != 0;
  const size_t SS = (size_t)S * S, ns2 = (size_t)n_sub * n_sub;
  const int nblk = S / block, NTL = (S + 15) / 16;
  // the budget rule of include/nagp.h
  const size_t per_series = 8 * (size_t)T * ((fo ? SS + S : 2 * SS + 3 * (size_t)S + 2) + 2 + S + (Pdiag ? S : 0) + ns2);
  const size_t fixed = 8 * (2 * SS + 2 * (size_t)S * block + S) + 4 * (size_t)n_sub + 4096;
  const size_t budget = budget_bytes(dev_sw.budget_mb[DevSwitches::SFB], SFB_BUDGET_BYTES);
  const BatchPlan bp = batch_plan((size_t)n_series, budget, fixed, per_series);
  if (!bp.ok) FAIL(NAGP_ENOMEM, "one series takes %zu B of device memory (budget %zu B)", fixed + per_series, budget);
  if (hipSetDevice(device) != hipSuccess) FAIL(NAGP_EHIP, "hipSetDevice(%d)", device);
  // the diagonal blocks of A and Q; the lower triangle of P0, mirrored
  std::vector<double> hb(2 * (size_t)S * block + SS);
  for (int I = 0; I < nblk; ++I)
    for (int j = 0; j < block; ++j)
      for (int i = 0; i < block; ++i) {
        const size_t src = (size_t)(I * block + i) + (size_t)(I * block + j) * S, dst = (size_t)I * block * block + i + (size_t)j * block;
        hb[dst] = A[src]; hb[(size_t)S * block + dst] = Q[src];
      }
  for (int j = 0; j < S; ++j)
    for (int i = 0; i < S; ++i) hb[2 * (size_t)S * block + i + (size_t)j * S] = (i >= j) ? P0[i + (size_t)j * S] : P0[j + (size_t)i * S];
  const size_t TS = (size_t)T * S;
  const SfbBlock o = sfb_block((size_t)S, (size_t)block, (size_t)T, (size_t)n_sub, fo, Pdiag != nullptr, bp.nb);
  DevBlock blk;
  API_ALLOC(blk, device, o.total); double* const dev = blk.p;
  int st = NAGP_OK;
  API_HIP(nagp_slowfb_run, hipMemcpy(dev + o.ab, hb.data(), hb.size() * 8, hipMemcpyHostToDevice));      // Ab | Qb | P0 are adjacent
  API_HIP(nagp_slowfb_run, hipMemcpy(dev + o.h, H, (size_t)S * 8, hipMemcpyHostToDevice));
  if (n_sub) API_HIP(nagp_slowfb_run, hipMemcpy(dev + o.sub, sub_idx, (size_t)n_sub * 4, hipMemcpyHostToDevice));
  const SfbFn kf = sfb_forward_tab[block], kb = sfb_backward_tab[block], kc = sfb_combine_tab[NTL];
  const size_t lds_s = sfb_seq_lds_doubles(S, block) * sizeof(double), lds_c = sfb_combine_lds_doubles(16 * NTL) * sizeof(double);
  if (st == NAGP_OK) st = set_lds(kf, lds_s);
  if (st == NAGP_OK && !fo) st = set_lds(kb, lds_s);
  if (st == NAGP_OK) st = set_lds(kc, lds_c);
  const int NT = (S > 64) ? 512 : 256;
  API_HIP(nagp_slowfb_run, blk.events(4));
  SfbPar sp{};
  sp.S = S; sp.nblk = nblk; sp.T = T; sp.filter_only = fo ? 1 : 0;
  sp.Ab = dev + o.ab; sp.Qb = dev + o.qb; sp.H = dev + o.h; sp.P0 = dev + o.p0; sp.y = dev + o.y; sp.vary = dev + o.vr;
  sp.pm = dev + o.pm; sp.pP = dev + o.pP; sp.vv = dev + o.v; sp.sinv = dev + o.si; sp.K = dev + o.K; sp.r = dev + o.r; sp.N = dev + o.N;
  sp.lik = dev + o.lik; sp.flag = reinterpret_cast<int*>(dev + o.fl);
  sp.n_sub = n_sub; sp.sub = reinterpret_cast<const int*>(dev + o.sub);
  sp.MS = dev + o.ms; sp.Pdiag = Pdiag ? dev + o.pd : nullptr; sp.Psub = Psub ? dev + o.ps : nullptr;
  const bool post = MS || Pdiag || Psub;                     // lik alone needs neither the backward pass nor the combination
  bool notpd = false;
  run_batches("nagp_slowfb_run", st, n_series, (int)bp.nb, blk.ev, 4, g_sfb_ms,
    [&](int i0, int nbk) {
      API_HIP(nagp_slowfb_run, hipMemcpy(dev + o.y, y + (size_t)i0 * T, (size_t)nbk * T * 8, hipMemcpyHostToDevice));
      API_HIP(nagp_slowfb_run, hipMemcpy(dev + o.vr, vary + (size_t)i0 * T, (size_t)nbk * T * 8, hipMemcpyHostToDevice));
    }, [&](int, int nbk, int seg) {                             // the three timed segments: forward, backward, combination
      if (seg == 0) hipLaunchKernelGGL(kf, dim3(nbk), dim3(NT), lds_s, 0, sp);
      if (seg == 1 && !fo && post) hipLaunchKernelGGL(kb, dim3(nbk), dim3(NT), lds_s, 0, sp);
      if (seg == 2 && post) hipLaunchKernelGGL(kc, dim3((unsigned)T, nbk), dim3(256), lds_c, 0, sp);
    }, [&](int i0, int nbk) {
      std::vector<int> fl((size_t)nbk, 0);
      API_HIP(nagp_slowfb_run, hipMemcpy(fl.data(), dev + o.fl, (size_t)nbk * 4, hipMemcpyDeviceToHost));
      for (int i = 0; i < nbk; ++i) notpd = notpd || fl[i] != 0;
      if (lik) API_HIP(nagp_slowfb_run, hipMemcpy(lik + i0, dev + o.lik, (size_t)nbk * 8, hipMemcpyDeviceToHost));
      if (MS) API_HIP(nagp_slowfb_run, hipMemcpy(MS + (size_t)i0 * TS, dev + o.ms, (size_t)nbk * TS * 8, hipMemcpyDeviceToHost));
      if (Pdiag) API_HIP(nagp_slowfb_run, hipMemcpy(Pdiag + (size_t)i0 * TS, dev + o.pd, (size_t)nbk * TS * 8, hipMemcpyDeviceToHost));
      if (Psub) API_HIP(nagp_slowfb_run, hipMemcpy(Psub + (size_t)i0 * ns2 * T, dev + o.ps, (size_t)nbk * ns2 * T * 8, hipMemcpyDeviceToHost));
    });
  if (st == NAGP_OK && notpd) FAIL(NAGP_ENOTPD, "an innovation variance s <= 0 (possible only with vary = 0): lik of that series is NaN");
  return st;
}
