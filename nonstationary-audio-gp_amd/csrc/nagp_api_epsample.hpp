// part of nagp_api.hip: joint posterior draws of a full-covariance EP run by forward filtering with the returned sites and backward
// sampling (see include/nagp.h, nagp_epsample.hpp)
constexpr size_t EPS_BUDGET_BYTES = (size_t)48 << 30;     // device memory of one call: the draws run in device batches under it
static thread_local double g_eps_ms[3] = {0.0, 0.0, 0.0};

typedef void (*EpsFn)(EpsPar);
static const EpsFn eps_factor_tab[6] = {nullptr, eps_factor_kernel<1>, eps_factor_kernel<2>, eps_factor_kernel<3>, eps_factor_kernel<4>, eps_factor_kernel<5>};
static const EpsFn eps_draw_tab[6] = {nullptr, eps_draw_kernel<1>, eps_draw_kernel<2>, eps_draw_kernel<3>, eps_draw_kernel<4>, eps_draw_kernel<5>};

extern "C" int nagp_ep_sample_timings(double* ms) { return timings_out(ms, g_eps_ms, 3); }

extern "C" int nagp_ep_sample(const nagp_model* model, const double* ttau, const double* tnu, const double* y, int64_t T,
                              int32_t predict_at_k1, int32_t n_draws, uint64_t seed, const double* z, const nagp_epsample_sig* sig,
                              double* Xdraw, double* Fdraw, double* Sdraw, double* MS, int64_t* counters, int32_t device) {
  g_eps_ms[0] = g_eps_ms[1] = g_eps_ms[2] = 0.0;            // a call that is refused or fails reports no time of an earlier one
  if (!model || !ttau || !tnu || !y) FAIL(NAGP_EINVAL, "null argument");
  if (!model->block_offsets || !model->A || !model->Q || !model->Pinf || !model->h_val) FAIL(NAGP_EINVAL, "null argument in the model");
  if (T < 1 || n_draws < 1) FAIL(NAGP_EINVAL, "bad sizes (T=%lld n_draws=%d)", (long long)T, n_draws);
  const int S = model->S, M = model->M;
  if (S < 1 || M < 1 || M > S) FAIL(NAGP_EINVAL, "bad sizes (S=%d M=%d)", S, M);
  if (!Xdraw && !Fdraw && !Sdraw && !MS) FAIL(NAGP_EINVAL, "no output requested");
  if (Sdraw && !sig) FAIL(NAGP_EINVAL, "Sdraw needs sig (Wnmf, amplitude kind, link)");
  int D = 0, N = 0;
  if (sig) {
    D = model->D; N = model->N;
    if (!sig->Wnmf) FAIL(NAGP_EINVAL, "null argument: sig->Wnmf");
    if (D < 1 || N < 1 || D + N != M) FAIL(NAGP_EINVAL, "sig: the model's D=%d and N=%d must add up to M=%d", D, N, M);
    if (sig->amp_kind != NAGP_AMP_LINEAR && sig->amp_kind != NAGP_AMP_SQRT) FAIL(NAGP_EINVAL, "unknown amplitude kind");
    if (sig->link_kind != NAGP_LINK_SOFTPLUS && sig->link_kind != NAGP_LINK_EXP) FAIL(NAGP_EINVAL, "unknown link kind");
    if (!std::isfinite(sig->link_shift)) FAIL(NAGP_EINVAL, "the link shift must be finite");
    for (int e = 0; e < D * N; ++e) if (!std::isfinite(sig->Wnmf[e])) FAIL(NAGP_EINVAL, "sig->Wnmf[%d] is not finite", e);
  }
  const int32_t* bo = model->block_offsets;
  if (bo[0] != 0 || bo[M] != S) FAIL(NAGP_EINVAL, "block_offsets must run from 0 to S");
  int nb2 = 0;
  for (int n = 0; n < M; ++n) {
    const int b = bo[n + 1] - bo[n];
    if (b < 1) FAIL(NAGP_EINVAL, "block_offsets must ascend strictly");
    if (b > EPS_MAXB) FAIL(NAGP_EUNSUPPORTED, "block %d has %d states: blocks of 1 .. %d states are served", n, b, EPS_MAXB);
    nb2 += b * b;
  }
  if (S > EPS_MAXS) FAIL(NAGP_EUNSUPPORTED, "S=%d: the three S x S operands of a step's factorisation live in the 160 KiB LDS of one workgroup (S <= %d)", S, EPS_MAXS);
  const DevSwitches dev_sw = read_dev_switches();
  const size_t budget = budget_bytes(dev_sw.budget_mb[DevSwitches::EPS], EPS_BUDGET_BYTES);
  const size_t SS = (size_t)S * S;
  if ((double)T * (double)(2 * SS) * 8.0 > (double)budget) FAIL(NAGP_ENOMEM, "the per-step storage, %.3g B, is beyond the budget of a call (%zu B); there is no checkpoint scheme", (double)T * (double)(2 * SS) * 8.0, budget);
  const bool want_f = Fdraw || Sdraw;
  const size_t fixed = eps_fixed_bytes((size_t)S, (size_t)M, (size_t)T, (size_t)nb2, (size_t)D * N);
  const size_t per_draw = eps_draw_bytes((size_t)S, (size_t)M, (size_t)T, z != nullptr, Xdraw != nullptr, Fdraw != nullptr, Sdraw != nullptr);
  BatchPlan bp = batch_plan((size_t)n_draws, budget, fixed, per_draw);
  if (!bp.ok) FAIL(NAGP_ENOMEM, "the per-step storage and one draw take %zu B of device memory (budget %zu B); there is no checkpoint scheme", fixed + per_draw, budget);
  if (bp.nb > 16) bp.nb -= bp.nb % 16;                      // whole blocks of 16 draws
  const size_t MT = (size_t)M * T;
  for (size_t e = 0; e < MT; ++e) {
    if (!(ttau[e] >= 0.0) || !std::isfinite(ttau[e])) FAIL(NAGP_EINVAL, "ttau[%zu] = %g: a site precision must be finite and >= 0", e, ttau[e]);
    if (!std::isfinite(tnu[e])) FAIL(NAGP_EINVAL, "tnu[%zu] = %g is not finite", e, tnu[e]);
  }
  if (hipSetDevice(device) != hipSuccess) FAIL(NAGP_EHIP, "hipSetDevice(%d)", device);
  // host packing: dense block-diagonal A, Q, Pinf (only the blocks are read), the packed blocks, the index tables
  std::vector<double> hm(3 * SS + 2 * (size_t)nb2, 0.0);
  std::vector<int> hi(2 * (size_t)M + 2 + S);
  int* h_off = hi.data(); int* h_boff = h_off + M + 1; int* h_blk = h_boff + M + 1;
  int at = 0;
  for (int n = 0; n < M; ++n) {
    const int o = bo[n], b = bo[n + 1] - o;
    h_off[n] = o; h_boff[n] = at;
    for (int j = 0; j < b; ++j) {
      h_blk[o + j] = n;
      for (int i = 0; i < b; ++i) {
        const size_t src = (size_t)(o + i) + (size_t)(o + j) * S;
        hm[src] = model->A[src]; hm[SS + src] = model->Q[src]; hm[2 * SS + src] = model->Pinf[src];
        hm[3 * SS + at + i + j * b] = model->A[src]; hm[3 * SS + nb2 + at + i + j * b] = model->Q[src];
      }
    }
    at += b * b;
  }
  h_off[M] = S; h_boff[M] = nb2;
  const size_t TS = (size_t)T * S;
  const EpsBlock o = eps_block((size_t)S, (size_t)M, (size_t)T, (size_t)nb2, (size_t)D * N, z != nullptr, Xdraw != nullptr, Fdraw != nullptr, Sdraw != nullptr, bp.nb);
  DevBlock blk;
  API_ALLOC(blk, device, o.total); double* const dev = blk.p;
  int st = NAGP_OK;
  API_HIP(nagp_ep_sample, hipMemcpy(dev + o.A, hm.data(), hm.size() * 8, hipMemcpyHostToDevice));           // A | Q | P0 | Ab | Qb are adjacent
  API_HIP(nagp_ep_sample, hipMemcpy(dev + o.h, model->h_val, (size_t)M * 8, hipMemcpyHostToDevice));
  API_HIP(nagp_ep_sample, hipMemcpy(dev + o.idx, hi.data(), hi.size() * 4, hipMemcpyHostToDevice));
  if (sig) API_HIP(nagp_ep_sample, hipMemcpy(dev + o.w, sig->Wnmf, (size_t)D * N * 8, hipMemcpyHostToDevice));
  API_HIP(nagp_ep_sample, hipMemcpy(dev + o.tt, ttau, MT * 8, hipMemcpyHostToDevice));
  API_HIP(nagp_ep_sample, hipMemcpy(dev + o.tn, tnu, MT * 8, hipMemcpyHostToDevice));
  API_HIP(nagp_ep_sample, hipMemcpy(dev + o.y, y, (size_t)T * 8, hipMemcpyHostToDevice));
  API_HIP(nagp_ep_sample, hipMemset(dev + o.cnt, 0, 4 * 8));
  const int NTL = (S + 15) / 16;
  const EpsFn kfac = eps_factor_tab[NTL], kdraw = eps_draw_tab[NTL];
  const EpsFn kfil = (S > 32) ? eps_filter_kernel<512> : eps_filter_kernel<256>;
  const EpsFn ksig = (sig && sig->amp_kind == NAGP_AMP_SQRT) ? eps_signal_kernel<true> : eps_signal_kernel<false>;
  const size_t lds_f = eps_filter_lds_bytes(S, M, nb2), lds_c = eps_factor_lds_bytes(S), lds_d = eps_draw_lds_bytes(16 * NTL);
  if (st == NAGP_OK) st = set_lds(kfil, lds_f);
  if (st == NAGP_OK) st = set_lds(kfac, lds_c);
  if (st == NAGP_OK) st = set_lds(kdraw, lds_d);
  API_HIP(nagp_ep_sample, blk.events(4));
  EpsPar ep{};
  ep.S = S; ep.M = M; ep.D = D; ep.N = N; ep.T = T; ep.predict_at_k1 = predict_at_k1 ? 1 : 0;
  ep.A = dev + o.A; ep.Q = dev + o.Q; ep.P0 = dev + o.p0; ep.Ab = dev + o.ab; ep.Qb = dev + o.qb; ep.hval = dev + o.h;
  ep.off = reinterpret_cast<const int*>(dev + o.idx); ep.boff = ep.off + M + 1; ep.blk = ep.boff + M + 1;
  ep.ttau = dev + o.tt; ep.tnu = dev + o.tn; ep.y = dev + o.y; ep.MF = dev + o.mf; ep.PG = dev + o.pg; ep.Lc = dev + o.lc;
  ep.cnt = reinterpret_cast<unsigned long long*>(dev + o.cnt);
  ep.seed = seed; ep.W = dev + o.w;
  if (sig) { ep.link_kind = sig->link_kind; ep.link_shift = sig->link_shift; }
  if (st == NAGP_OK) {                                      // the filter and the factorisation: once, whatever the draws
    (void)hipEventRecord(blk.ev[0], 0);
    hipLaunchKernelGGL(kfil, dim3(1), dim3(S > 32 ? 512 : 256), lds_f, 0, ep);
    (void)hipEventRecord(blk.ev[1], 0);
    hipLaunchKernelGGL(kfac, dim3((unsigned)T), dim3(256), lds_c, 0, ep);
    (void)hipEventRecord(blk.ev[2], 0);
    API_HIP(nagp_ep_sample, hipGetLastError());
    API_HIP(nagp_ep_sample, hipDeviceSynchronize());
    for (int s = 0; s < 2 && st == NAGP_OK; ++s) { float t = 0.f; if (hipEventElapsedTime(&t, blk.ev[s], blk.ev[s + 1]) == hipSuccess) g_eps_ms[s] += t; }
  }
  const bool draws = Xdraw || want_f;                         // MS alone: one launch of the mean chain, no draw
  run_batches("nagp_ep_sample", st, draws ? n_draws : 1, (int)bp.nb, blk.ev, 2, g_eps_ms + 2,
      [&](int i0, int nbk) {
        if (z && draws) API_HIP(nagp_ep_sample, hipMemcpy(dev + o.z, z + (size_t)i0 * TS, (size_t)nbk * TS * 8, hipMemcpyHostToDevice));
      }, [&](int i0, int nbk, int) {
        EpsPar ed = ep;
        ed.n = draws ? nbk : 0; ed.draw0 = i0; ed.z = z ? dev + o.z : nullptr;
        ed.MSout = (MS && i0 == 0) ? dev + o.ms : nullptr;       // the chain with z = 0 (the RTS means) rides with the first batch
        ed.X = Xdraw ? dev + o.x : nullptr; ed.F = want_f ? dev + o.f : nullptr; ed.Sd = Sdraw ? dev + o.sd : nullptr;
        hipLaunchKernelGGL(kdraw, dim3((ed.n + 15) / 16 + (ed.MSout ? 1 : 0)), dim3(64 * NTL), lds_d, 0, ed);
        if (Sdraw) hipLaunchKernelGGL(ksig, dim3((unsigned)(((size_t)nbk * T + 255) / 256)), dim3(256), 0, 0, ed);
      }, [&](int i0, int nbk) {
        if (MS && i0 == 0) API_HIP(nagp_ep_sample, hipMemcpy(MS, dev + o.ms, TS * 8, hipMemcpyDeviceToHost));
        if (Xdraw) API_HIP(nagp_ep_sample, hipMemcpy(Xdraw + (size_t)i0 * TS, dev + o.x, (size_t)nbk * TS * 8, hipMemcpyDeviceToHost));
        if (Fdraw) API_HIP(nagp_ep_sample, hipMemcpy(Fdraw + (size_t)i0 * MT, dev + o.f, (size_t)nbk * MT * 8, hipMemcpyDeviceToHost));
        if (Sdraw) API_HIP(nagp_ep_sample, hipMemcpy(Sdraw + (size_t)i0 * T, dev + o.sd, (size_t)nbk * T * 8, hipMemcpyDeviceToHost));
      });
  unsigned long long hc[4] = {0, 0, 0, 0};
  API_HIP(nagp_ep_sample, hipMemcpy(hc, dev + o.cnt, 4 * 8, hipMemcpyDeviceToHost));
  if (counters && st == NAGP_OK) { counters[0] = (int64_t)hc[0]; counters[1] = (int64_t)hc[1]; }
  if (st == NAGP_OK && hc[2]) FAIL(NAGP_ENOTPD, "A PF_k A' + Q is not positive definite even with the jitter at %llu step(s): the draws are not usable", hc[2]);
  return st;
}
