// nagp_api_entry.hpp -- part of the ONE translation unit nagp_api.hip (included there, in this order: nagp_api_plan.hpp, nagp_api_sweep.hpp,
// nagp_api_entry.hpp; the plan struct, the error helpers and the developer switches live in nagp_api.hip itself).
// The one-shot entry points (ep / ihgp / giekf run), mom on its own, iekf_update1, the stationary filterbank, nagp_batch_run (RCCL), reconstruction.

// device calls of the per-call entry points: the first failure is kept (st, the text names the entry point), the calls after it are skipped
#define ENTRY_HIP(fn, x) do { if (st == NAGP_OK) { hipError_t _e = (x); if (_e != hipSuccess) { g_last_error = std::string(#fn ": " #x " -> ") + hipGetErrorString(_e); st = NAGP_EHIP; } } } while (0)

// ---------------------------------------------------------------------------------------------
static int run_one(const nagp_model* model, const nagp_ihgp_tables* tables, const double* y, int64_t T,
                   const nagp_opts* opts, nagp_out* out) {
  if (!model || !y || !opts || !out) FAIL(NAGP_EINVAL, "null argument");
  nagp_opts o = *opts;
  if (out->PS) o.flags |= 0x4u;
  nagp_plan* p = nullptr;
  int st = nagp_plan_create(&p, 1, model, tables, T, &o);
  if (st != NAGP_OK) return st;
  const double* ys[1] = {y};
  st = nagp_plan_upload_y(p, ys);
  if (st == NAGP_OK && (o.ttau0 || o.tnu0)) {
    const double* t0[1] = {o.ttau0}; const double* n0[1] = {o.tnu0};
    st = nagp_plan_upload_sites(p, t0, n0);
  }
  if (st == NAGP_OK) st = nagp_plan_execute(p);
  if (st == NAGP_OK) st = nagp_plan_download(p, out);
  nagp_plan_destroy(p);
  return st;
}

extern "C" int nagp_ep_run(const nagp_model* model, const double* y, int64_t T, const nagp_opts* opts, nagp_out* out) {
  if (opts && opts->kind != NAGP_KIND_GF_EP) FAIL(NAGP_EINVAL, "nagp_ep_run needs kind = NAGP_KIND_GF_EP");
  return run_one(model, nullptr, y, T, opts, out);
}
extern "C" int nagp_ihgp_run(const nagp_model* model, const nagp_ihgp_tables* tables, const double* y, int64_t T,
                             const nagp_opts* opts, nagp_out* out) {
  if (opts && opts->kind != NAGP_KIND_IHGP) FAIL(NAGP_EINVAL, "nagp_ihgp_run needs kind = NAGP_KIND_IHGP");
  return run_one(model, tables, y, T, opts, out);
}
extern "C" int nagp_giekf_run(const nagp_model* model, const double* y, int64_t T, const nagp_opts* opts, nagp_out* out) {
  if (opts && opts->kind != NAGP_KIND_GIEKF) FAIL(NAGP_EINVAL, "nagp_giekf_run needs kind = NAGP_KIND_GIEKF");
  return run_one(model, nullptr, y, T, opts, out);
}

// ---------------------------------------------------------------------------------------------
// mom on its own (see include/nagp.h)
extern "C" int nagp_mom_eval(const nagp_opts* o, int32_t D, int32_t N, const double* Wnmf, double lik_param, int64_t n,
                             const double* y, const double* mu, const double* s2, double* lZ, double* dlZ, double* d2lZ) {
  if (!o || !y || !mu || !s2 || !lZ || !dlZ || !d2lZ || n < 0) FAIL(NAGP_EINVAL, "null argument");
  if (o->lik_kind < NAGP_LIK_POWER || o->lik_kind > NAGP_LIK_POWER_NMF_SQRT) FAIL(NAGP_EINVAL, "unknown likelihood");
  const bool power = o->lik_kind == NAGP_LIK_POWER;
  const int M = power ? 2 * D : D + N;
  if (D < 1 || M > MAXM || o->n_pts < 1 || !o->wn || !o->xn_unscaled) FAIL(NAGP_EINVAL, "bad sizes / cubature");
  if (power ? (o->cub_dim != D) : (o->cub_dim != N || N < 1 || N > MOM_MAXCD || !Wnmf)) FAIL(NAGP_EUNSUPPORTED, "cub_dim / N / Wnmf");
  if (n == 0) return NAGP_OK;
  if (hipSetDevice(o->device) != hipSuccess) FAIL(NAGP_EHIP, "hipSetDevice(%d)", o->device);
  std::vector<double> xd;
  std::vector<unsigned char> code((size_t)o->n_pts * o->cub_dim);
  for (int pt = 0; pt < o->n_pts; ++pt)
    for (int j = 0; j < o->cub_dim; ++j) {
      const double v = o->xn_unscaled[j + (size_t)o->cub_dim * pt];
      size_t ci = 0;
      while (ci < xd.size() && xd[ci] != v) ++ci;
      if (ci == xd.size()) {
        if (xd.size() == 64) FAIL(NAGP_EUNSUPPORTED, "sigma-point rule has more than 64 distinct coordinate values");
        xd.push_back(v);
      }
      code[(size_t)pt * o->cub_dim + j] = (unsigned char)ci;
    }
  // one device block: wn | xd | code | W | y | mu | s2 | lZ | dl | d2l
  const size_t n_code = (code.size() + 7) / 8 + 1, nW = power ? 0 : (size_t)D * N;
  const size_t o_wn = 0, o_xd = o_wn + o->n_pts, o_code = o_xd + xd.size(), o_W = o_code + n_code, o_y = o_W + nW,
               o_mu = o_y + n, o_s2 = o_mu + (size_t)n * M, o_lZ = o_s2 + (size_t)n * M, o_dl = o_lZ + n, o_d2 = o_dl + (size_t)n * M,
               total = o_d2 + (size_t)n * M;
  double* dev = nullptr;
  if (hipMalloc(&dev, total * sizeof(double)) != hipSuccess) { (void)hipGetLastError(); FAIL(NAGP_ENOMEM, "hipMalloc(%zu)", total * sizeof(double)); }
  std::vector<double> Wr(nW);
  for (int dd = 0; dd < (power ? 0 : D); ++dd)
    for (int j = 0; j < N; ++j) Wr[(size_t)dd * N + j] = Wnmf[dd + (size_t)D * j];
  int st = NAGP_OK;
  ENTRY_HIP(nagp_mom_eval, hipMemcpy(dev + o_wn, o->wn, (size_t)o->n_pts * 8, hipMemcpyHostToDevice));
  ENTRY_HIP(nagp_mom_eval, hipMemcpy(dev + o_xd, xd.data(), xd.size() * 8, hipMemcpyHostToDevice));
  ENTRY_HIP(nagp_mom_eval, hipMemcpy(dev + o_code, code.data(), code.size(), hipMemcpyHostToDevice));
  if (nW) ENTRY_HIP(nagp_mom_eval, hipMemcpy(dev + o_W, Wr.data(), nW * 8, hipMemcpyHostToDevice));
  ENTRY_HIP(nagp_mom_eval, hipMemcpy(dev + o_y, y, (size_t)n * 8, hipMemcpyHostToDevice));
  ENTRY_HIP(nagp_mom_eval, hipMemcpy(dev + o_mu, mu, (size_t)n * M * 8, hipMemcpyHostToDevice));
  ENTRY_HIP(nagp_mom_eval, hipMemcpy(dev + o_s2, s2, (size_t)n * M * 8, hipMemcpyHostToDevice));
  MomCfg mc{};
  mc.lik_kind = o->lik_kind; mc.link_kind = o->link_kind; mc.link_shift = o->link_shift;
  mc.n_pts = o->n_pts; mc.cdim = o->cub_dim; mc.D = D; mc.nd = (int)xd.size();
  mc.wn = dev + o_wn; mc.xd = dev + o_xd; mc.code = reinterpret_cast<const unsigned char*>(dev + o_code);
  mc.jitter = power ? 1e-8 : 1e-10; mc.stamps = nullptr;
  mc.DG = pick_DG(o->lik_kind, o->n_pts, 256, D, o->cub_dim);
  mc.cache_tabs = 1; mc.store_a = (o->lik_kind == NAGP_LIK_POWER_NMF_SQRT) ? 1 : 0;
  if (momk_lds_doubles(D, power ? D : N, M, mc) * sizeof(double) > 150 * 1024) mc.store_a = 0;
  if (momk_lds_doubles(D, power ? D : N, M, mc) * sizeof(double) > 150 * 1024) mc.cache_tabs = 0;
  const size_t lds = momk_lds_doubles(D, power ? D : N, M, mc) * sizeof(double);
  if (lds > 160 * 1024) { (void)hipFree(dev); FAIL(NAGP_EUNSUPPORTED, "mom workspace of %zu B exceeds the LDS", lds); }
  MomPar mp{D, power ? 0 : N, M, std::exp(lik_param), o->ep_fraction, nW ? dev + o_W : nullptr, dev + o_y, dev + o_mu, dev + o_s2,
            dev + o_lZ, dev + o_dl, dev + o_d2, n};
  const int grid = (int)std::min<int64_t>(n, 1024);
  const MomFn mom = pick_mom(mom_variant(mc));
  if (st == NAGP_OK) st = set_lds(mom, lds);
  if (st == NAGP_OK) hipLaunchKernelGGL(mom, dim3(grid), dim3(256), lds, 0, mc, mp);
#undef LM
  ENTRY_HIP(nagp_mom_eval, hipGetLastError());
  ENTRY_HIP(nagp_mom_eval, hipDeviceSynchronize());
  ENTRY_HIP(nagp_mom_eval, hipMemcpy(lZ, dev + o_lZ, (size_t)n * 8, hipMemcpyDeviceToHost));
  ENTRY_HIP(nagp_mom_eval, hipMemcpy(dlZ, dev + o_dl, (size_t)n * M * 8, hipMemcpyDeviceToHost));
  ENTRY_HIP(nagp_mom_eval, hipMemcpy(d2lZ, dev + o_d2, (size_t)n * M * 8, hipMemcpyDeviceToHost));
  (void)hipFree(dev);
  return st;
}

// ---------------------------------------------------------------------------------------------
// iekf_update1 / ekf_update1 on their own (see include/nagp.h)
extern "C" int nagp_iekf_update1(int32_t S, int32_t D, int32_t N, const int32_t* h_col, const double* h_val, const double* Wnmf,
                                 double R, double y, int32_t iters, double* m, double* P, double* K, double* MU, double* Sinn,
                                 int32_t device) {
  if (!h_col || !h_val || !Wnmf || !m || !P) FAIL(NAGP_EINVAL, "null argument");
  const int M = D + N;
  if (S < 1 || S > 512 || D < 1 || N < 1 || M > S || iters < 1) FAIL(NAGP_EINVAL, "bad sizes (S=%d D=%d N=%d iters=%d)", S, D, N, iters);
  for (int n = 0; n < M; ++n)
    if (h_col[n] < 0 || h_col[n] >= S) FAIL(NAGP_EINVAL, "h_col[%d] = %d outside the state", n, h_col[n]);
  if (hipSetDevice(device) != hipSuccess) FAIL(NAGP_EHIP, "hipSetDevice(%d)", device);
  // one device block: m | P | K | MU,S | hval | W | hcol(int)
  const size_t o_m = 0, o_P = o_m + S, o_K = o_P + (size_t)S * S, o_ms = o_K + S, o_hv = o_ms + 2, o_W = o_hv + M,
               o_hc = o_W + (size_t)D * N, total = o_hc + (M + 1) / 2 + 1;
  double* dev = nullptr;
  if (hipMalloc(&dev, total * sizeof(double)) != hipSuccess) { (void)hipGetLastError(); FAIL(NAGP_ENOMEM, "hipMalloc(%zu)", total * sizeof(double)); }
  std::vector<double> Wr((size_t)D * N);
  for (int dd = 0; dd < D; ++dd)
    for (int j = 0; j < N; ++j) Wr[(size_t)dd * N + j] = Wnmf[dd + (size_t)D * j];
  int st = NAGP_OK;
  ENTRY_HIP(nagp_iekf_update1, hipMemcpy(dev + o_m, m, (size_t)S * 8, hipMemcpyHostToDevice));
  ENTRY_HIP(nagp_iekf_update1, hipMemcpy(dev + o_P, P, (size_t)S * S * 8, hipMemcpyHostToDevice));
  ENTRY_HIP(nagp_iekf_update1, hipMemcpy(dev + o_hv, h_val, (size_t)M * 8, hipMemcpyHostToDevice));
  ENTRY_HIP(nagp_iekf_update1, hipMemcpy(dev + o_W, Wr.data(), Wr.size() * 8, hipMemcpyHostToDevice));
  ENTRY_HIP(nagp_iekf_update1, hipMemcpy(dev + o_hc, h_col, (size_t)M * sizeof(int32_t), hipMemcpyHostToDevice));
  EkfPar ep{S, D, N, iters, R, y, reinterpret_cast<const int*>(dev + o_hc), dev + o_hv, dev + o_W, dev + o_m, dev + o_P, dev + o_K, dev + o_ms};
  const size_t lds = (2 * (size_t)S + 2 * M + 2) * sizeof(double);
  if (st == NAGP_OK) hipLaunchKernelGGL(iekf_update1_kernel, dim3(1), dim3(256), lds, 0, ep);
  ENTRY_HIP(nagp_iekf_update1, hipGetLastError());
  ENTRY_HIP(nagp_iekf_update1, hipDeviceSynchronize());
  double ms[2] = {0, 0};
  ENTRY_HIP(nagp_iekf_update1, hipMemcpy(m, dev + o_m, (size_t)S * 8, hipMemcpyDeviceToHost));
  ENTRY_HIP(nagp_iekf_update1, hipMemcpy(P, dev + o_P, (size_t)S * S * 8, hipMemcpyDeviceToHost));
  if (K) ENTRY_HIP(nagp_iekf_update1, hipMemcpy(K, dev + o_K, (size_t)S * 8, hipMemcpyDeviceToHost));
  ENTRY_HIP(nagp_iekf_update1, hipMemcpy(ms, dev + o_ms, 16, hipMemcpyDeviceToHost));
  if (MU) *MU = ms[0];
  if (Sinn) *Sinn = ms[1];
  (void)hipFree(dev);
  return st;
}

// ---------------------------------------------------------------------------------------------
// stationary filterbank: kernel_ss_kalmanFastFB (see include/nagp.h)
extern "C" int nagp_fastfb_run(int32_t S, const double* A, const double* AKHA, const double* HA, const double* K, const double* G,
                               const double* y, int64_t T, double* MS, double* sum_v2, int32_t device) {
  if (!A || !AKHA || !HA || !K || !y || !MS) FAIL(NAGP_EINVAL, "null argument");
  if (S < 1 || T < 1) FAIL(NAGP_EINVAL, "bad sizes (S=%d T=%lld)", S, (long long)T);
  // S <= 96: both constant S x S matrices of a pass live in the LDS; 96 < S <= 256 (a thread per state): they stay in global memory (L2-resident)
  const int mat_global = (fb_lds_doubles(S) * sizeof(double) > 160 * 1024) ? 1 : 0;
  const size_t lds = fb_lds_doubles(S, mat_global) * sizeof(double);
  if (S > 256) FAIL(NAGP_EUNSUPPORTED, "S=%d: the stationary filterbank runs a thread per state (S <= 256)", S);
  if (hipSetDevice(device) != hipSuccess) FAIL(NAGP_EHIP, "hipSetDevice(%d)", device);
  // spans of the parallel-in-time form (needs two more (S+4) x (S+4) work matrices in LDS: fb_compose_lds_doubles fits 160 KiB up to S = 69); short series run as one span
  const size_t lds_c = fb_compose_lds_doubles(S) * sizeof(double);
  int ns = 1;
  if (lds_c <= 160 * 1024 && T >= 2048 && !read_dev_switches().fb_sequential) ns = (int)std::min<int64_t>(512, T / 128);
  const int64_t L = (T + ns - 1) / ns;
  ns = (int)((T + L - 1) / L);
  const size_t SS = (size_t)S * S, SP = (size_t)S + 4;
  const size_t o_A = 0, o_B = o_A + SS, o_G = o_B + SS, o_ha = o_G + SS, o_k = o_ha + S, o_y = o_k + S, o_ms = o_y + T,
               o_sv = o_ms + (size_t)T * S, o_phi = o_sv + ns + 1, o_st = o_phi + (size_t)ns * S * SP, total = o_st + (size_t)ns * S + 2;
  double* dev = nullptr;
  if (hipMalloc(&dev, total * sizeof(double)) != hipSuccess) { (void)hipGetLastError(); FAIL(NAGP_ENOMEM, "hipMalloc(%zu)", total * sizeof(double)); }
  int st = NAGP_OK;
  ENTRY_HIP(nagp_fastfb_run, hipMemcpy(dev + o_A, A, SS * 8, hipMemcpyHostToDevice));
  ENTRY_HIP(nagp_fastfb_run, hipMemcpy(dev + o_B, AKHA, SS * 8, hipMemcpyHostToDevice));
  if (G) ENTRY_HIP(nagp_fastfb_run, hipMemcpy(dev + o_G, G, SS * 8, hipMemcpyHostToDevice));
  ENTRY_HIP(nagp_fastfb_run, hipMemcpy(dev + o_ha, HA, (size_t)S * 8, hipMemcpyHostToDevice));
  ENTRY_HIP(nagp_fastfb_run, hipMemcpy(dev + o_k, K, (size_t)S * 8, hipMemcpyHostToDevice));
  ENTRY_HIP(nagp_fastfb_run, hipMemcpy(dev + o_y, y, (size_t)T * 8, hipMemcpyHostToDevice));
  const int NT = std::max(64, roundup64(S));
  if (st == NAGP_OK) st = set_lds(fastfb_filter_kernel, lds);
  if (st == NAGP_OK) st = set_lds(fastfb_smoother_kernel, lds);
  if (st == NAGP_OK && ns > 1) st = set_lds(fastfb_compose_kernel<false>, lds_c);
  if (st == NAGP_OK && ns > 1) st = set_lds(fastfb_compose_kernel<true>, lds_c);
  if (st == NAGP_OK) {
    FbPar fp{S, T, dev + o_A, dev + o_B, dev + o_ha, dev + o_k, dev + o_y, dev + o_ms, dev + o_sv, L, ns, dev + o_phi,
             ns > 1 ? dev + o_st : nullptr, mat_global};
    if (ns > 1) {
      hipLaunchKernelGGL(fastfb_compose_kernel<false>, dim3(ns), dim3(256), lds_c, 0, fp);
      hipLaunchKernelGGL(fastfb_boundary_kernel<false>, dim3(1), dim3(256), 0, 0, fp);
    }
    hipLaunchKernelGGL(fastfb_filter_kernel, dim3(ns), dim3(NT), lds, 0, fp);
    if (G && T > 1) {
      fp.B = dev + o_G;
      // the T-1 smoothing steps are partitioned with the same span length
      const int nss = (int)((T - 1 + L - 1) / L);
      fp.ns = nss;
      if (ns > 1) {
        hipLaunchKernelGGL(fastfb_compose_kernel<true>, dim3(nss), dim3(256), lds_c, 0, fp);
        hipLaunchKernelGGL(fastfb_boundary_kernel<true>, dim3(1), dim3(256), 0, 0, fp);
      }
      hipLaunchKernelGGL(fastfb_smoother_kernel, dim3(nss), dim3(NT), lds, 0, fp);
    }
  }
  ENTRY_HIP(nagp_fastfb_run, hipGetLastError());
  ENTRY_HIP(nagp_fastfb_run, hipDeviceSynchronize());
  ENTRY_HIP(nagp_fastfb_run, hipMemcpy(MS, dev + o_ms, (size_t)T * S * 8, hipMemcpyDeviceToHost));
  if (sum_v2) {
    std::vector<double> part((size_t)ns);
    ENTRY_HIP(nagp_fastfb_run, hipMemcpy(part.data(), dev + o_sv, (size_t)ns * 8, hipMemcpyDeviceToHost));
    double acc = 0.0;
    for (int j = 0; j < ns; ++j) acc += part[j];      // fixed order
    *sum_v2 = acc;
  }
  (void)hipFree(dev);
  return st;
}

// ---------------------------------------------------------------------------------------------
// stationary filterbank: joint posterior draws by the simulation smoother (see include/nagp.h, nagp_fbsample.hpp)
constexpr size_t FBS_BUDGET_BYTES = (size_t)8 << 30;      // device memory of one call: the draws run in device batches under it
constexpr int FBS_ONE_SPAN_DRAWS = 256;                   // from this many draws on, one span per draw fills the chip

// M^n of a column-major S x S matrix in the layout of the boundary pass: out[i * (S+4) + l] = (M^n)(i,l)
static void fbs_matrix_power(const double* M, int S, int64_t n, double* out) {
  const size_t SS = (size_t)S * S;
  std::vector<double> r(SS, 0.0), b(SS), t(SS);
  for (int i = 0; i < S; ++i) { r[(size_t)i * S + i] = 1.0; for (int l = 0; l < S; ++l) b[(size_t)i * S + l] = M[i + (size_t)l * S]; }
  auto mul = [&](const std::vector<double>& x, const std::vector<double>& z) {
    std::fill(t.begin(), t.end(), 0.0);
    for (int i = 0; i < S; ++i)
      for (int q = 0; q < S; ++q) { const double xv = x[(size_t)i * S + q]; for (int l = 0; l < S; ++l) t[(size_t)i * S + l] += xv * z[(size_t)q * S + l]; }
  };
  for (; n > 0; n >>= 1) {
    if (n & 1) { mul(r, b); r.swap(t); }
    if (n > 1) { mul(b, b); b.swap(t); }
  }
  for (int i = 0; i < S; ++i) for (int l = 0; l < S + 4; ++l) out[(size_t)i * (S + 4) + l] = l < S ? r[(size_t)i * S + l] : 0.0;
}

extern "C" int nagp_fastfb_sample(int32_t S, const double* A, const double* AKHA, const double* HA, const double* K, const double* G,
                                  const double* H, double R, const double* Lp, const double* Lq, const double* y, int64_t T,
                                  int32_t n_draws, uint64_t seed, double* Ydraw, double* Xdraw, double* MS, int32_t device) {
  if (!A || !AKHA || !HA || !K || !G || !H || !Lp || !Lq || !y) FAIL(NAGP_EINVAL, "null argument (there is no filter-only form: G is required)");
  if (S < 1 || T < 1 || n_draws < 1) FAIL(NAGP_EINVAL, "bad sizes (S=%d T=%lld n_draws=%d)", S, (long long)T, n_draws);
  if (!(R > 0.0) || !std::isfinite(R)) FAIL(NAGP_EINVAL, "the observation variance R must be positive and finite");
  if (!Ydraw && !Xdraw && !MS) FAIL(NAGP_EINVAL, "no output requested");
  if (S > 256) FAIL(NAGP_EUNSUPPORTED, "S=%d: the stationary filterbank runs a thread per state (S <= 256)", S);
  const DevSwitches dev_sw = read_dev_switches();
  const int mat_global = (fb_lds_doubles(S) * sizeof(double) > 160 * 1024) ? 1 : 0;
  const size_t lds = fb_lds_doubles(S, mat_global) * sizeof(double);
  const size_t lds_c = fb_compose_lds_doubles(S) * sizeof(double);
  // spans as in nagp_fastfb_run (the filter's span matrices come from its compose pass); one span per draw for short series and large batches
  int ns = 1;
  if (lds_c <= 160 * 1024 && T >= 2048 && n_draws < FBS_ONE_SPAN_DRAWS && !dev_sw.fb_sequential) ns = (int)std::min<int64_t>(512, T / 128);
  const int64_t L = (T + ns - 1) / ns;
  ns = (int)((T + L - 1) / L);
  const int nss = T > 1 ? (int)((T - 1 + L - 1) / L) : 0;      // spans of the T-1 smoothing steps
  const size_t SS = (size_t)S * S, SP = (size_t)S + 4, TS = (size_t)T * S;
  const size_t budget = dev_sw.fbs_budget_mb ? (size_t)dev_sw.fbs_budget_mb << 20 : FBS_BUDGET_BYTES;
  const size_t fixed = (5 * SS + 3 * (size_t)S + (size_t)T + ((size_t)ns + 3) * S * SP + 8) * sizeof(double);
  const size_t per_draw = (2 * TS + 2 * (size_t)T + 2 * (size_t)ns * S) * sizeof(double);
  if (fixed + per_draw > budget) FAIL(NAGP_ENOMEM, "one draw takes %zu B of device memory (budget %zu B)", fixed + per_draw, budget);
  const int nb = (int)std::min<size_t>({(size_t)n_draws, (budget - fixed) / per_draw, (size_t)32768});
  if (MS) {                                                     // S_y(y): the smoother itself, same launches and bits
    const int st0 = nagp_fastfb_run(S, A, AKHA, HA, K, G, y, T, MS, nullptr, device);
    if (st0 != NAGP_OK) return st0;
  }
  if (!Ydraw && !Xdraw) return NAGP_OK;
  if (hipSetDevice(device) != hipSuccess) FAIL(NAGP_EHIP, "hipSetDevice(%d)", device);
  const size_t o_A = 0, o_B = o_A + SS, o_G = o_B + SS, o_lq = o_G + SS, o_lp = o_lq + SS, o_k = o_lp + SS, o_h = o_k + S, o_ha = o_h + S,
               o_y = o_ha + S, o_phf = o_y + T, o_pha = o_phf + (size_t)ns * S * SP, o_phg = o_pha + S * SP, o_phl = o_phg + S * SP,
               o_xs = o_phl + S * SP + 8, o_ms = o_xs + (size_t)nb * TS, o_d = o_ms + (size_t)nb * TS, o_yd = o_d + (size_t)nb * T,
               o_c = o_yd + (size_t)nb * T, o_st = o_c + (size_t)nb * ns * S, total = o_st + (size_t)nb * ns * S;
  double* dev = nullptr;
  if (hipMalloc(&dev, total * sizeof(double)) != hipSuccess) { (void)hipGetLastError(); FAIL(NAGP_ENOMEM, "hipMalloc(%zu)", total * sizeof(double)); }
  int st = NAGP_OK;
  ENTRY_HIP(nagp_fastfb_sample, hipMemcpy(dev + o_A, A, SS * 8, hipMemcpyHostToDevice));
  ENTRY_HIP(nagp_fastfb_sample, hipMemcpy(dev + o_B, AKHA, SS * 8, hipMemcpyHostToDevice));
  ENTRY_HIP(nagp_fastfb_sample, hipMemcpy(dev + o_G, G, SS * 8, hipMemcpyHostToDevice));
  ENTRY_HIP(nagp_fastfb_sample, hipMemcpy(dev + o_lq, Lq, SS * 8, hipMemcpyHostToDevice));
  ENTRY_HIP(nagp_fastfb_sample, hipMemcpy(dev + o_lp, Lp, SS * 8, hipMemcpyHostToDevice));
  ENTRY_HIP(nagp_fastfb_sample, hipMemcpy(dev + o_k, K, (size_t)S * 8, hipMemcpyHostToDevice));
  ENTRY_HIP(nagp_fastfb_sample, hipMemcpy(dev + o_h, H, (size_t)S * 8, hipMemcpyHostToDevice));
  ENTRY_HIP(nagp_fastfb_sample, hipMemcpy(dev + o_ha, HA, (size_t)S * 8, hipMemcpyHostToDevice));
  ENTRY_HIP(nagp_fastfb_sample, hipMemcpy(dev + o_y, y, (size_t)T * 8, hipMemcpyHostToDevice));
  if (ns > 1) {                                                 // the span matrices that do not depend on y: A^L, G^L, G^(last span)
    std::vector<double> ph(3 * S * SP);
    fbs_matrix_power(A, S, L, ph.data());
    fbs_matrix_power(G, S, L, ph.data() + S * SP);
    fbs_matrix_power(G, S, (T - 1) - (int64_t)(nss - 1) * L, ph.data() + 2 * S * SP);
    ENTRY_HIP(nagp_fastfb_sample, hipMemcpy(dev + o_pha, ph.data(), ph.size() * 8, hipMemcpyHostToDevice));
  }
  const int NT = std::max(64, roundup64(S));
  if (st == NAGP_OK) st = set_lds(fbs_prior_kernel<false>, lds);
  if (st == NAGP_OK) st = set_lds(fbs_filter_kernel<false>, lds);
  if (st == NAGP_OK) st = set_lds(fbs_smoother_kernel<false>, lds);
  if (st == NAGP_OK && ns > 1) st = set_lds(fbs_prior_kernel<true>, lds);
  if (st == NAGP_OK && ns > 1) st = set_lds(fbs_filter_kernel<true>, lds);
  if (st == NAGP_OK && ns > 1) st = set_lds(fbs_smoother_kernel<true>, lds);
  if (st == NAGP_OK && ns > 1) st = set_lds(fastfb_compose_kernel<false>, lds_c);
  if (st == NAGP_OK && ns > 1) {                                // the filter's span matrices: a function of the NaN pattern of y alone
    FbPar cp{S, T, dev + o_A, dev + o_B, dev + o_ha, dev + o_k, dev + o_y, nullptr, nullptr, L, ns, dev + o_phf, nullptr, 0};
    hipLaunchKernelGGL(fastfb_compose_kernel<false>, dim3(ns), dim3(256), lds_c, 0, cp);
  }
  for (int i0 = 0; i0 < n_draws && st == NAGP_OK; i0 += nb) {
    const int nbk = std::min(nb, n_draws - i0);
    FbsPar fq{};
    fq.S = S; fq.T = T; fq.L = L; fq.ns = ns; fq.draw0 = i0; fq.seed = seed; fq.sqrtR = std::sqrt(R);
    fq.A = dev + o_A; fq.Lp = dev + o_lp; fq.H = dev + o_h; fq.K = dev + o_k; fq.y = dev + o_y;
    fq.xs = dev + o_xs; fq.d = dev + o_d; fq.ms = dev + o_ms; fq.yd = dev + o_yd; fq.want_x = Xdraw ? 1 : 0;
    fq.c = dev + o_c; fq.starts = ns > 1 ? dev + o_st : nullptr; fq.mat_global = mat_global;
    // prior draw x*, d = y - y*
    fq.B = dev + o_lq; fq.Phi = dev + o_pha; fq.phi_stride = 0; fq.PhiLast = dev + o_pha;
    if (ns > 1) {
      hipLaunchKernelGGL(fbs_prior_kernel<true>, dim3(ns, nbk), dim3(NT), lds, 0, fq);
      hipLaunchKernelGGL(fbs_boundary_kernel<false>, dim3(nbk), dim3(256), 0, 0, fq);
    }
    hipLaunchKernelGGL(fbs_prior_kernel<false>, dim3(ns, nbk), dim3(NT), lds, 0, fq);
    // filter of d
    fq.B = dev + o_B; fq.Phi = dev + o_phf; fq.phi_stride = (size_t)S * SP; fq.PhiLast = dev + o_phf + (size_t)(ns - 1) * S * SP;
    if (ns > 1) {
      hipLaunchKernelGGL(fbs_filter_kernel<true>, dim3(ns, nbk), dim3(NT), lds, 0, fq);
      hipLaunchKernelGGL(fbs_boundary_kernel<false>, dim3(nbk), dim3(256), 0, 0, fq);
    }
    hipLaunchKernelGGL(fbs_filter_kernel<false>, dim3(ns, nbk), dim3(NT), lds, 0, fq);
    // step T-1, then the T-1 smoothing steps with + x* and the product with H in the replay
    if (Xdraw) hipLaunchKernelGGL(fbs_last_kernel<true>, dim3(nbk), dim3(256), 0, 0, fq);
    else hipLaunchKernelGGL(fbs_last_kernel<false>, dim3(nbk), dim3(256), 0, 0, fq);
    if (T > 1) {
      fq.B = dev + o_G; fq.ns = nss; fq.Phi = dev + o_phg; fq.phi_stride = 0; fq.PhiLast = dev + o_phl;
      if (ns > 1) {
        hipLaunchKernelGGL(fbs_smoother_kernel<true>, dim3(nss, nbk), dim3(NT), lds, 0, fq);
        hipLaunchKernelGGL(fbs_boundary_kernel<true>, dim3(nbk), dim3(256), 0, 0, fq);
      }
      hipLaunchKernelGGL(fbs_smoother_kernel<false>, dim3(nss, nbk), dim3(NT), lds, 0, fq);
    }
    ENTRY_HIP(nagp_fastfb_sample, hipGetLastError());
    ENTRY_HIP(nagp_fastfb_sample, hipDeviceSynchronize());
    if (Ydraw) ENTRY_HIP(nagp_fastfb_sample, hipMemcpy(Ydraw + (size_t)i0 * T, dev + o_yd, (size_t)nbk * T * 8, hipMemcpyDeviceToHost));
    if (Xdraw) ENTRY_HIP(nagp_fastfb_sample, hipMemcpy(Xdraw + (size_t)i0 * TS, dev + o_xs, (size_t)nbk * TS * 8, hipMemcpyDeviceToHost));
  }
  (void)hipFree(dev);
  return st;
}

// ---------------------------------------------------------------------------------------------
// stationary filterbank, exact form: Kalman filter / smoother with per-step observation variances (see include/nagp.h, nagp_slowfb.hpp)
constexpr size_t SFB_BUDGET_BYTES = (size_t)48 << 30;     // device memory of one call: the series run in device batches under it
static thread_local double g_sfb_ms[3] = {0.0, 0.0, 0.0};

typedef void (*SfbFn)(SfbPar);
#define SFB_TABLE(name) {nullptr, name<1>, name<2>, name<3>, name<4>, name<5>, name<6>, name<7>, name<8>}
static const SfbFn sfb_forward_tab[9] = SFB_TABLE(sfb_forward_kernel);
static const SfbFn sfb_backward_tab[9] = SFB_TABLE(sfb_backward_kernel);
static const SfbFn sfb_combine_tab[9] = SFB_TABLE(sfb_combine_kernel);
#undef SFB_TABLE

extern "C" int nagp_slowfb_timings(double* ms) {
  if (!ms) FAIL(NAGP_EINVAL, "null argument");
  for (int i = 0; i < 3; ++i) ms[i] = g_sfb_ms[i];
  return NAGP_OK;
}

extern "C" int nagp_slowfb_run(int32_t S, int32_t block, const double* A, const double* Q, const double* H, const double* P0,
                               int32_t n_series, const double* y, const double* vary, int64_t T, int32_t filter_only,
                               int32_t n_sub, const int32_t* sub_idx, double* lik, double* MS, double* Pdiag, double* Psub,
                               int32_t device) {
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
  const size_t budget = dev_sw.sfb_budget_mb ? (size_t)dev_sw.sfb_budget_mb << 20 : SFB_BUDGET_BYTES;
  if (fixed + per_series > budget) FAIL(NAGP_ENOMEM, "one series takes %zu B of device memory (budget %zu B)", fixed + per_series, budget);
  const int nb = (int)std::min<size_t>({(size_t)n_series, (budget - fixed) / per_series, (size_t)32768});
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
  // one device block (doubles): Ab | Qb | P0 | H | sub (int) | per batch: y | vary | lik | flag (int) | pm | pP | v | 1/s | K | r | N | MS | Pdiag | Psub
  const size_t TS = (size_t)T * S, TSS = (size_t)T * SS, nbz = (size_t)nb;
  const size_t o_ab = 0, o_qb = o_ab + (size_t)S * block, o_p0 = o_qb + (size_t)S * block, o_h = o_p0 + SS, o_sub = o_h + S,
               o_y = o_sub + (size_t)n_sub / 2 + 1, o_vr = o_y + nbz * T, o_lik = o_vr + nbz * T, o_fl = o_lik + nbz, o_pm = o_fl + nbz / 2 + 1,
               o_pP = o_pm + nbz * TS, o_v = o_pP + nbz * TSS, o_si = o_v + (fo ? 0 : nbz * T), o_K = o_si + (fo ? 0 : nbz * T),
               o_r = o_K + (fo ? 0 : nbz * TS), o_N = o_r + (fo ? 0 : nbz * TS), o_ms = o_N + (fo ? 0 : nbz * TSS),
               o_pd = o_ms + nbz * TS, o_ps = o_pd + (Pdiag ? nbz * TS : 0), total = o_ps + nbz * ns2 * T + 2;
  double* dev = nullptr;
  if (hipMalloc(&dev, total * sizeof(double)) != hipSuccess) { (void)hipGetLastError(); FAIL(NAGP_ENOMEM, "hipMalloc(%zu)", total * sizeof(double)); }
  int st = NAGP_OK;
  ENTRY_HIP(nagp_slowfb_run, hipMemcpy(dev + o_ab, hb.data(), hb.size() * 8, hipMemcpyHostToDevice));      // Ab | Qb | P0 are adjacent
  ENTRY_HIP(nagp_slowfb_run, hipMemcpy(dev + o_h, H, (size_t)S * 8, hipMemcpyHostToDevice));
  if (n_sub) ENTRY_HIP(nagp_slowfb_run, hipMemcpy(dev + o_sub, sub_idx, (size_t)n_sub * 4, hipMemcpyHostToDevice));
  const SfbFn kf = sfb_forward_tab[block], kb = sfb_backward_tab[block], kc = sfb_combine_tab[NTL];
  const size_t lds_s = sfb_seq_lds_doubles(S, block) * sizeof(double), lds_c = sfb_combine_lds_doubles(16 * NTL) * sizeof(double);
  if (st == NAGP_OK) st = set_lds(kf, lds_s);
  if (st == NAGP_OK && !fo) st = set_lds(kb, lds_s);
  if (st == NAGP_OK) st = set_lds(kc, lds_c);
  const int NT = (S > 64) ? 512 : 256;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  for (int i = 0; i < 4; ++i) ENTRY_HIP(nagp_slowfb_run, hipEventCreate(&ev[i]));
  g_sfb_ms[0] = g_sfb_ms[1] = g_sfb_ms[2] = 0.0;
  bool notpd = false;
  for (int i0 = 0; i0 < n_series && st == NAGP_OK; i0 += nb) {
    const int nbk = std::min(nb, n_series - i0);
    ENTRY_HIP(nagp_slowfb_run, hipMemcpy(dev + o_y, y + (size_t)i0 * T, (size_t)nbk * T * 8, hipMemcpyHostToDevice));
    ENTRY_HIP(nagp_slowfb_run, hipMemcpy(dev + o_vr, vary + (size_t)i0 * T, (size_t)nbk * T * 8, hipMemcpyHostToDevice));
    SfbPar sp{};
    sp.S = S; sp.nblk = nblk; sp.T = T; sp.filter_only = fo ? 1 : 0;
    sp.Ab = dev + o_ab; sp.Qb = dev + o_qb; sp.H = dev + o_h; sp.P0 = dev + o_p0; sp.y = dev + o_y; sp.vary = dev + o_vr;
    sp.pm = dev + o_pm; sp.pP = dev + o_pP; sp.vv = dev + o_v; sp.sinv = dev + o_si; sp.K = dev + o_K; sp.r = dev + o_r; sp.N = dev + o_N;
    sp.lik = dev + o_lik; sp.flag = reinterpret_cast<int*>(dev + o_fl);
    sp.n_sub = n_sub; sp.sub = reinterpret_cast<const int*>(dev + o_sub);
    sp.MS = dev + o_ms; sp.Pdiag = Pdiag ? dev + o_pd : nullptr; sp.Psub = Psub ? dev + o_ps : nullptr;
    if (st == NAGP_OK) {
      (void)hipEventRecord(ev[0], 0);
      hipLaunchKernelGGL(kf, dim3(nbk), dim3(NT), lds_s, 0, sp);
      (void)hipEventRecord(ev[1], 0);
      if (!fo && (MS || Pdiag || Psub)) hipLaunchKernelGGL(kb, dim3(nbk), dim3(NT), lds_s, 0, sp);      // lik alone needs no backward pass
      (void)hipEventRecord(ev[2], 0);
      if (MS || Pdiag || Psub) hipLaunchKernelGGL(kc, dim3((unsigned)T, nbk), dim3(256), lds_c, 0, sp);
      (void)hipEventRecord(ev[3], 0);
    }
    ENTRY_HIP(nagp_slowfb_run, hipGetLastError());
    ENTRY_HIP(nagp_slowfb_run, hipDeviceSynchronize());
    for (int i = 0; i < 3 && st == NAGP_OK; ++i) { float ms = 0.f; if (hipEventElapsedTime(&ms, ev[i], ev[i + 1]) == hipSuccess) g_sfb_ms[i] += ms; }
    std::vector<int> fl((size_t)nbk, 0);
    ENTRY_HIP(nagp_slowfb_run, hipMemcpy(fl.data(), dev + o_fl, (size_t)nbk * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < nbk; ++i) notpd = notpd || fl[i] != 0;
    if (lik) ENTRY_HIP(nagp_slowfb_run, hipMemcpy(lik + i0, dev + o_lik, (size_t)nbk * 8, hipMemcpyDeviceToHost));
    if (MS) ENTRY_HIP(nagp_slowfb_run, hipMemcpy(MS + (size_t)i0 * TS, dev + o_ms, (size_t)nbk * TS * 8, hipMemcpyDeviceToHost));
    if (Pdiag) ENTRY_HIP(nagp_slowfb_run, hipMemcpy(Pdiag + (size_t)i0 * TS, dev + o_pd, (size_t)nbk * TS * 8, hipMemcpyDeviceToHost));
    if (Psub) ENTRY_HIP(nagp_slowfb_run, hipMemcpy(Psub + (size_t)i0 * ns2 * T, dev + o_ps, (size_t)nbk * ns2 * T * 8, hipMemcpyDeviceToHost));
  }
  for (int i = 0; i < 4; ++i) if (ev[i]) (void)hipEventDestroy(ev[i]);
  (void)hipFree(dev);
  if (st == NAGP_OK && notpd) FAIL(NAGP_ENOTPD, "an innovation variance s <= 0 (possible only with vary = 0): lik of that series is NaN");
  return st;
}

// ---------------------------------------------------------------------------------------------
// fixed-point NMF of experiments/nmf/nmf_fp.m / nmf_inf_fp.m, a batch of problems on one data matrix (see include/nagp.h, nagp_nmf.hpp)
constexpr size_t NMF_BUDGET_BYTES = (size_t)8 << 30;      // device memory of one call: the problems run in device batches under it
static thread_local double g_nmf_ms = 0.0;

typedef void (*NmfFn)(NmfPar);
static const NmfFn nmf_pass_tab[17] = {nullptr, nmf_pass_kernel<1>, nmf_pass_kernel<2>, nmf_pass_kernel<3>, nmf_pass_kernel<4>, nmf_pass_kernel<5>,
                                       nmf_pass_kernel<6>, nmf_pass_kernel<7>, nmf_pass_kernel<8>, nmf_pass_kernel<9>, nmf_pass_kernel<10>,
                                       nmf_pass_kernel<11>, nmf_pass_kernel<12>, nmf_pass_kernel<13>, nmf_pass_kernel<14>, nmf_pass_kernel<15>,
                                       nmf_pass_kernel<16>};

extern "C" int nagp_nmf_timings(double* ms) {
  if (!ms) FAIL(NAGP_EINVAL, "null argument");
  ms[0] = g_nmf_ms;
  return NAGP_OK;
}

extern "C" int nagp_nmf_fp(int32_t n_problems, int64_t T, int32_t D, int32_t K, const double* A, const double* vary, const double* W0,
                           const double* H0, int32_t n_its, int32_t update_w, double* W, double* H, double* Obj, int32_t device) {
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
    g_nmf_ms = 0.0;
    return NAGP_OK;
  }
  const DevSwitches dev_sw = read_dev_switches();
  const int nwg = (int)((T + NMF_NT - 1) / NMF_NT);
  // the budget rule of include/nagp.h
  const size_t fixed = 8 * (vary ? 2 : 1) * TD + 4096;
  const size_t per_problem = 8 * (TK + KD + (size_t)nwg * (2 * KD + 2) + (size_t)n_obj);
  const size_t budget = dev_sw.nmf_budget_mb ? (size_t)dev_sw.nmf_budget_mb << 20 : NMF_BUDGET_BYTES;
  if (fixed + per_problem > budget) FAIL(NAGP_ENOMEM, "one problem takes %zu B of device memory (budget %zu B)", fixed + per_problem, budget);
  const int nb = (int)std::min<size_t>({(size_t)n_problems, (budget - fixed) / per_problem, (size_t)32768});
  if (hipSetDevice(device) != hipSuccess) FAIL(NAGP_EHIP, "hipSetDevice(%d)", device);
  // one device block (doubles): A | vary | per batch: W | H | pw | po | Obj
  const size_t nbz = (size_t)nb;
  const size_t o_a = 0, o_v = o_a + TD, o_w = o_v + (vary ? TD : 0), o_h = o_w + nbz * KD, o_pw = o_h + nbz * TK,
               o_po = o_pw + nbz * nwg * 2 * KD, o_ob = o_po + nbz * nwg * 2, total = o_ob + nbz * n_obj + 2;
  double* dev = nullptr;
  if (hipMalloc(&dev, total * sizeof(double)) != hipSuccess) { (void)hipGetLastError(); FAIL(NAGP_ENOMEM, "hipMalloc(%zu)", total * sizeof(double)); }
  int st = NAGP_OK;
  ENTRY_HIP(nagp_nmf_fp, hipMemcpy(dev + o_a, A, TD * 8, hipMemcpyHostToDevice));
  if (vary) ENTRY_HIP(nagp_nmf_fp, hipMemcpy(dev + o_v, vary, TD * 8, hipMemcpyHostToDevice));
  const NmfFn kp = nmf_pass_tab[K], kfin = update_w ? nmf_finish_kernel<true> : nmf_finish_kernel<false>;
  const size_t lds_p = nmf_pass_lds_doubles(K, D) * sizeof(double), lds_f = nmf_finish_lds_doubles(K, D) * sizeof(double);
  if (st == NAGP_OK) st = set_lds(kp, lds_p);
  if (st == NAGP_OK) st = set_lds(kfin, lds_f);
  hipEvent_t ev[2] = {nullptr, nullptr};
  for (int i = 0; i < 2; ++i) ENTRY_HIP(nagp_nmf_fp, hipEventCreate(&ev[i]));
  g_nmf_ms = 0.0;
  for (int i0 = 0; i0 < n_problems && st == NAGP_OK; i0 += nb) {
    const int nbk = std::min(nb, n_problems - i0);
    ENTRY_HIP(nagp_nmf_fp, hipMemcpy(dev + o_w, W0 + (size_t)i0 * KD, (size_t)nbk * KD * 8, hipMemcpyHostToDevice));
    ENTRY_HIP(nagp_nmf_fp, hipMemcpy(dev + o_h, H0 + (size_t)i0 * TK, (size_t)nbk * TK * 8, hipMemcpyHostToDevice));
    NmfPar np{};
    np.T = T; np.D = D; np.K = K; np.nwg = nwg; np.A = dev + o_a; np.vary = vary ? dev + o_v : nullptr;
    np.W = dev + o_w; np.H = dev + o_h; np.pw = dev + o_pw; np.po = dev + o_po; np.Obj = dev + o_ob; np.n_obj = n_obj;
    if (st == NAGP_OK) {
      // every iteration is one pass and one finish; with update_w the second objective of iteration l is formed by the pass of
      // iteration l + 1 and that of the last iteration by a closing pass.  Nothing waits on the host until all of it is enqueued.
      (void)hipEventRecord(ev[0], 0);
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
      (void)hipEventRecord(ev[1], 0);
    }
    ENTRY_HIP(nagp_nmf_fp, hipGetLastError());
    ENTRY_HIP(nagp_nmf_fp, hipDeviceSynchronize());
    if (st == NAGP_OK) { float ms = 0.f; if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) g_nmf_ms += ms; }
    if (W) ENTRY_HIP(nagp_nmf_fp, hipMemcpy(W + (size_t)i0 * KD, dev + o_w, (size_t)nbk * KD * 8, hipMemcpyDeviceToHost));
    if (H) ENTRY_HIP(nagp_nmf_fp, hipMemcpy(H + (size_t)i0 * TK, dev + o_h, (size_t)nbk * TK * 8, hipMemcpyDeviceToHost));
    if (Obj) ENTRY_HIP(nagp_nmf_fp, hipMemcpy(Obj + (size_t)i0 * n_obj, dev + o_ob, (size_t)nbk * n_obj * 8, hipMemcpyDeviceToHost));
  }
  for (int i = 0; i < 2; ++i) if (ev[i]) (void)hipEventDestroy(ev[i]);
  (void)hipFree(dev);
  return st;
}

// ---------------------------------------------------------------------------------------------
// objective and gradient of the filterbank spectrum fit, get_Obj_pSTFT_{exp,matern32,matern52,all}.m (see include/nagp.h, nagp_pstft.hpp)
constexpr size_t PSTFT_BUDGET_BYTES = (size_t)1 << 30;    // device memory of one call: the problems run in device batches under it
static thread_local double g_pstft_ms = 0.0;

typedef void (*PstftFn)(PstftPar);
static const PstftFn pstft_pass_tab[4] = {pstft_pass_kernel<1>, pstft_pass_kernel<2>, pstft_pass_kernel<3>, pstft_pass_kernel<4>};
static const PstftFn pstft_finish_tab[4] = {pstft_finish_kernel<1>, pstft_finish_kernel<2>, pstft_finish_kernel<3>, pstft_finish_kernel<4>};

extern "C" int nagp_pstft_timings(double* ms) {
  if (!ms) FAIL(NAGP_EINVAL, "null argument");
  ms[0] = g_pstft_ms;
  return NAGP_OK;
}

extern "C" int nagp_pstft_obj(int32_t n_problems, int32_t kernel, int32_t form, int32_t D, int64_t N, const double* theta, const double* specTar,
                              int64_t spec_stride, const double* vary, const double* bet, const double* minVar, const double* limOm,
                              const double* limLam, double* Obj, double* dObj, int32_t device) {
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
  const size_t budget = dev_sw.pstft_budget_mb ? (size_t)dev_sw.pstft_budget_mb << 20 : PSTFT_BUDGET_BYTES;
  if (fixed + per_problem > budget) FAIL(NAGP_EUNSUPPORTED, "one problem takes %zu B of device memory (budget %zu B)", fixed + per_problem, budget);
  const int nb = (int)std::min<size_t>({(size_t)n_problems, (budget - fixed) / per_problem, (size_t)32768});
  if (hipSetDevice(device) != hipSuccess) FAIL(NAGP_EHIP, "hipSetDevice(%d)", device);
  // one device block (doubles): minVar | limOm | limLam | specTar (shared) | per batch: theta | vary | bet | specTar | part | Obj | dObj
  const size_t nbz = (size_t)nb, Dz = (size_t)D, Nz = (size_t)N;
  const size_t o_mv = 0, o_lo = o_mv + Dz, o_ll = o_lo + 2 * Dz, o_ss = o_ll + 2 * Dz, o_th = o_ss + (spec_stride ? 0 : Nz), o_vy = o_th + nbz * 3 * Dz,
               o_bt = o_vy + nbz, o_sp = o_bt + nbz, o_pt = o_sp + (spec_stride ? nbz * Nz : 0), o_ob = o_pt + nbz * nwg * n_out, o_dg = o_ob + nbz,
               total = o_dg + nbz * 3 * Dz + 2;
  double* dev = nullptr;
  if (hipMalloc(&dev, total * sizeof(double)) != hipSuccess) { (void)hipGetLastError(); FAIL(NAGP_ENOMEM, "hipMalloc(%zu)", total * sizeof(double)); }
  int st = NAGP_OK;
  ENTRY_HIP(nagp_pstft_obj, hipMemcpy(dev + o_mv, minVar, Dz * 8, hipMemcpyHostToDevice));
  ENTRY_HIP(nagp_pstft_obj, hipMemcpy(dev + o_lo, limOm, 2 * Dz * 8, hipMemcpyHostToDevice));
  ENTRY_HIP(nagp_pstft_obj, hipMemcpy(dev + o_ll, limLam, 2 * Dz * 8, hipMemcpyHostToDevice));
  if (!spec_stride) ENTRY_HIP(nagp_pstft_obj, hipMemcpy(dev + o_ss, specTar, Nz * 8, hipMemcpyHostToDevice));
  const PstftFn kp = pstft_pass_tab[kernel], kfin = pstft_finish_tab[kernel];
  hipEvent_t ev[2] = {nullptr, nullptr};
  for (int i = 0; i < 2; ++i) ENTRY_HIP(nagp_pstft_obj, hipEventCreate(&ev[i]));
  g_pstft_ms = 0.0;
  for (int i0 = 0; i0 < n_problems && st == NAGP_OK; i0 += nb) {
    const int nbk = std::min(nb, n_problems - i0);
    ENTRY_HIP(nagp_pstft_obj, hipMemcpy(dev + o_th, theta + (size_t)i0 * 3 * Dz, (size_t)nbk * 3 * Dz * 8, hipMemcpyHostToDevice));
    ENTRY_HIP(nagp_pstft_obj, hipMemcpy(dev + o_vy, vary + i0, (size_t)nbk * 8, hipMemcpyHostToDevice));
    ENTRY_HIP(nagp_pstft_obj, hipMemcpy(dev + o_bt, bet + i0, (size_t)nbk * 8, hipMemcpyHostToDevice));
    if (spec_stride) ENTRY_HIP(nagp_pstft_obj, hipMemcpy(dev + o_sp, specTar + (size_t)i0 * Nz, (size_t)nbk * Nz * 8, hipMemcpyHostToDevice));
    PstftPar pp{};
    pp.N = N; pp.D = D; pp.nwg = nwg; pp.grad = grad; pp.kappa = kernel == NAGP_PSTFT_MATERN72 ? std::sqrt(7.0 / 5.0) : 1.0;
    pp.theta = dev + o_th; pp.specTar = spec_stride ? dev + o_sp : dev + o_ss; pp.spec_stride = spec_stride; pp.vary = dev + o_vy; pp.bet = dev + o_bt;
    pp.minVar = dev + o_mv; pp.limOm = dev + o_lo; pp.limLam = dev + o_ll; pp.part = dev + o_pt; pp.Obj = dev + o_ob; pp.dObj = dev + o_dg;
    if (st == NAGP_OK) {
      (void)hipEventRecord(ev[0], 0);
      hipLaunchKernelGGL(kp, dim3((unsigned)nwg, (unsigned)nbk), dim3(PSTFT_NT), 0, 0, pp);
      hipLaunchKernelGGL(kfin, dim3((unsigned)nbk), dim3(PSTFT_FIN_NT), 0, 0, pp);
      (void)hipEventRecord(ev[1], 0);
    }
    ENTRY_HIP(nagp_pstft_obj, hipGetLastError());
    ENTRY_HIP(nagp_pstft_obj, hipDeviceSynchronize());
    if (st == NAGP_OK) { float ms = 0.f; if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) g_pstft_ms += ms; }
    ENTRY_HIP(nagp_pstft_obj, hipMemcpy(Obj + i0, dev + o_ob, (size_t)nbk * 8, hipMemcpyDeviceToHost));
    if (grad) ENTRY_HIP(nagp_pstft_obj, hipMemcpy(dObj + (size_t)i0 * 3 * Dz, dev + o_dg, (size_t)nbk * 3 * Dz * 8, hipMemcpyDeviceToHost));
  }
  for (int i = 0; i < 2; ++i) if (ev[i]) (void)hipEventDestroy(ev[i]);
  (void)hipFree(dev);
  return st;
}

// ---------------------------------------------------------------------------------------------
// objective and gradient of the modulator prior fit, toolsGP/getObjSEGP.m on getGPSESpec.m (see include/nagp.h, nagp_segp.hpp)
constexpr size_t SEGP_BUDGET_BYTES = (size_t)1 << 30;     // device memory of one call: the problems run in device batches under it
static thread_local double g_segp_ms = 0.0;

typedef void (*SegpFn)(SegpPar);
static const SegpFn segp_pass_tab[3] = {segp_pass_kernel<1>, segp_pass_kernel<2>, segp_pass_kernel<3>};
static const SegpFn segp_finish_tab[3] = {segp_finish_kernel<1>, segp_finish_kernel<2>, segp_finish_kernel<3>};

extern "C" int nagp_segp_timings(double* ms) {
  if (!ms) FAIL(NAGP_EINVAL, "null argument");
  ms[0] = g_segp_ms;
  return NAGP_OK;
}

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
  const size_t budget = dev_sw.segp_budget_mb ? (size_t)dev_sw.segp_budget_mb << 20 : SEGP_BUDGET_BYTES;
  if (fixed + per_problem > budget) FAIL(NAGP_EUNSUPPORTED, "one problem takes %zu B of device memory (budget %zu B)", fixed + per_problem, budget);
  const int nb = (int)std::min<size_t>({(size_t)n_problems, (budget - fixed) / per_problem, (size_t)32768});
  if (hipSetDevice(device) != hipSuccess) FAIL(NAGP_EHIP, "hipSetDevice(%d)", device);
  // one device block (doubles): specy (shared) | per batch: param | vary | varx | specy | part | Obj | dObj
  const size_t nbz = (size_t)nb;
  const size_t o_ss = 0, o_pa = o_ss + (spec_stride ? 0 : Tz), o_vy = o_pa + nbz * np, o_vx = o_vy + nbz, o_sp = o_vx + nbz,
               o_pt = o_sp + (spec_stride ? nbz * Tz : 0), o_ob = o_pt + nbz * nwg * n_out, o_dg = o_ob + nbz, total = o_dg + nbz * np + 2;
  double* dev = nullptr;
  if (hipMalloc(&dev, total * sizeof(double)) != hipSuccess) { (void)hipGetLastError(); FAIL(NAGP_ENOMEM, "hipMalloc(%zu)", total * sizeof(double)); }
  int st = NAGP_OK;
  if (!spec_stride) ENTRY_HIP(nagp_segp_obj, hipMemcpy(dev + o_ss, specy, Tz * 8, hipMemcpyHostToDevice));
  const SegpFn kp = segp_pass_tab[n_param - 1], kfin = segp_finish_tab[n_param - 1];
  hipEvent_t ev[2] = {nullptr, nullptr};
  for (int i = 0; i < 2; ++i) ENTRY_HIP(nagp_segp_obj, hipEventCreate(&ev[i]));
  for (int i0 = 0; i0 < n_problems && st == NAGP_OK; i0 += nb) {
    const int nbk = std::min(nb, n_problems - i0);
    ENTRY_HIP(nagp_segp_obj, hipMemcpy(dev + o_pa, param + (size_t)i0 * np, (size_t)nbk * np * 8, hipMemcpyHostToDevice));
    if (n_param <= 2) ENTRY_HIP(nagp_segp_obj, hipMemcpy(dev + o_vy, vary + i0, (size_t)nbk * 8, hipMemcpyHostToDevice));
    if (n_param == 1) ENTRY_HIP(nagp_segp_obj, hipMemcpy(dev + o_vx, varx + i0, (size_t)nbk * 8, hipMemcpyHostToDevice));
    if (spec_stride) ENTRY_HIP(nagp_segp_obj, hipMemcpy(dev + o_sp, specy + (size_t)i0 * Tz, (size_t)nbk * Tz * 8, hipMemcpyHostToDevice));
    SegpPar pp{};
    pp.T = T; pp.nwg = nwg; pp.grad = grad; pp.param = dev + o_pa; pp.specy = spec_stride ? dev + o_sp : dev + o_ss; pp.spec_stride = spec_stride;
    pp.vary = dev + o_vy; pp.varx = dev + o_vx; pp.part = dev + o_pt; pp.Obj = dev + o_ob; pp.dObj = dev + o_dg;
    if (st == NAGP_OK) {
      (void)hipEventRecord(ev[0], 0);
      hipLaunchKernelGGL(kp, dim3((unsigned)nwg, (unsigned)nbk), dim3(SEGP_NT), 0, 0, pp);
      hipLaunchKernelGGL(kfin, dim3((unsigned)nbk), dim3(SEGP_FIN_NT), 0, 0, pp);
      (void)hipEventRecord(ev[1], 0);
    }
    ENTRY_HIP(nagp_segp_obj, hipGetLastError());
    ENTRY_HIP(nagp_segp_obj, hipDeviceSynchronize());
    if (st == NAGP_OK) { float ms = 0.f; if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) g_segp_ms += ms; }
    ENTRY_HIP(nagp_segp_obj, hipMemcpy(Obj + i0, dev + o_ob, (size_t)nbk * 8, hipMemcpyDeviceToHost));
    if (grad) ENTRY_HIP(nagp_segp_obj, hipMemcpy(dObj + (size_t)i0 * np, dev + o_dg, (size_t)nbk * np * 8, hipMemcpyDeviceToHost));
  }
  for (int i = 0; i < 2; ++i) if (ev[i]) (void)hipEventDestroy(ev[i]);
  (void)hipFree(dev);
  return st;
}

// ---------------------------------------------------------------------------------------------
// Multi-GPU batched call (see include/nagp.h): problems round robin over the devices, one host thread + plan per device,
// RCCL all-reduce of the per-sweep nlZ sums.
extern "C" int nagp_batch_partition(int32_t n_problems, int32_t n_gpus, int32_t* dev_of) {
  if (n_problems < 0 || n_gpus < 1 || (n_problems > 0 && !dev_of)) FAIL(NAGP_EINVAL, "bad partition arguments");
  for (int i = 0; i < n_problems; ++i) dev_of[i] = i % n_gpus;      // problem i -> GPU i mod G
  return NAGP_OK;
}

namespace {
struct CommCache {
  std::mutex mu;
  int n = 0;
  std::vector<ncclComm_t> comms;
  std::vector<hipStream_t> streams;
  std::vector<double*> bufs;      // per device: [2 * 64] send | recv
};
CommCache g_cc;

void cc_release_locked() {
  for (size_t d = 0; d < g_cc.comms.size(); ++d) {
    (void)hipSetDevice((int)d);
    if (g_cc.bufs[d]) (void)hipFree(g_cc.bufs[d]);
    if (g_cc.streams[d]) (void)hipStreamDestroy(g_cc.streams[d]);
    if (g_cc.comms[d]) (void)ncclCommDestroy(g_cc.comms[d]);
  }
  g_cc.comms.clear(); g_cc.streams.clear(); g_cc.bufs.clear(); g_cc.n = 0;
}

constexpr int NLZ_MAX = 4096;      // EP sweeps of one call (the reference's drivers use 1 .. 30)
// sum over devices of part[d][0..cnt) with ncclAllReduce; every device ends with the total, device 0's copy is returned
int allreduce_nlz(int G, int cnt, const std::vector<std::vector<double>>& part, std::vector<double>& total) {
  std::lock_guard<std::mutex> lk(g_cc.mu);
  if (cnt > NLZ_MAX) FAIL(NAGP_EUNSUPPORTED, "more than %d EP sweeps in the nlZ reduction", NLZ_MAX);
  if (g_cc.n != G) {
    cc_release_locked();
    g_cc.comms.assign(G, nullptr); g_cc.streams.assign(G, nullptr); g_cc.bufs.assign(G, nullptr);
    std::vector<int> devs(G);
    for (int d = 0; d < G; ++d) devs[d] = d;
    ncclResult_t r = ncclCommInitAll(g_cc.comms.data(), G, devs.data());
    if (r != ncclSuccess) { cc_release_locked(); FAIL(NAGP_ERCCL, "ncclCommInitAll(%d) -> %s", G, ncclGetErrorString(r)); }
    // the cache counts as initialised (g_cc.n = G) only once every per-device stream and buffer exists; a failure on the
    // way releases what was created, so that the next call starts over instead of using null streams / buffers
    for (int d = 0; d < G; ++d) {
      hipError_t e = hipSetDevice(d);
      if (e == hipSuccess) e = hipStreamCreateWithFlags(&g_cc.streams[d], hipStreamNonBlocking);
      if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&g_cc.bufs[d]), 2 * NLZ_MAX * sizeof(double));
      if (e != hipSuccess) {
        cc_release_locked();
        FAIL(e == hipErrorOutOfMemory ? NAGP_ENOMEM : NAGP_EHIP, "per-device resources of the nlZ all-reduce (device %d) -> %s", d, hipGetErrorString(e));
      }
    }
    g_cc.n = G;
  }
  for (int d = 0; d < G; ++d) {
    HIP_TRY(hipSetDevice(d));
    HIP_TRY(hipMemcpyAsync(g_cc.bufs[d], part[d].data(), cnt * sizeof(double), hipMemcpyHostToDevice, g_cc.streams[d]));
  }
  ncclResult_t r = ncclGroupStart();
  for (int d = 0; d < G && r == ncclSuccess; ++d)
    r = ncclAllReduce(g_cc.bufs[d], g_cc.bufs[d] + NLZ_MAX, (size_t)cnt, ncclDouble, ncclSum, g_cc.comms[d], g_cc.streams[d]);
  ncclResult_t r2 = ncclGroupEnd();
  if (r == ncclSuccess) r = r2;
  if (r != ncclSuccess) FAIL(NAGP_ERCCL, "ncclAllReduce -> %s", ncclGetErrorString(r));
  total.assign(cnt, 0.0);
  for (int d = 0; d < G; ++d) {
    HIP_TRY(hipSetDevice(d));
    HIP_TRY(hipStreamSynchronize(g_cc.streams[d]));
  }
  HIP_TRY(hipSetDevice(0));
  HIP_TRY(hipMemcpy(total.data(), g_cc.bufs[0] + NLZ_MAX, cnt * sizeof(double), hipMemcpyDeviceToHost));
  return NAGP_OK;
}
}  // namespace

extern "C" void nagp_shutdown(void) {
  std::lock_guard<std::mutex> lk(g_cc.mu);
  cc_release_locked();
}

extern "C" int nagp_batch_run(int32_t n_problems, const nagp_model* models, const nagp_ihgp_tables* tables, const double* const* ys,
                              int64_t T, const nagp_opts* opts, nagp_out* outs, int32_t n_gpus, double* nlZ_total) {
  if (n_problems < 1 || !models || !ys || !opts || !outs || n_gpus < 1) FAIL(NAGP_EINVAL, "null/empty argument");
  if (opts->kind == NAGP_KIND_IHGP && !tables) FAIL(NAGP_EINVAL, "IHGP tables missing");
  if (opts->ttau0 || opts->tnu0)
    FAIL(NAGP_EINVAL, "nagp_batch_run takes no warm-start sites (opts.ttau0 / tnu0 describe ONE problem): use nagp_plan_create + nagp_plan_upload_sites");
  int ndev = 0, ndev_real = 0;
  if (hipGetDeviceCount(&ndev_real) != hipSuccess) ndev_real = 0;
  (void)hipGetLastError();
  // Test hooks (multi-GPU host logic without the hardware): NAGP_TEST_FAKE_DEVICES=n -- the partition, the per-device threads and the error
  // propagation run for n devices; device d's plan lives on physical device d mod (real devices) (every worker stops at its first device
  // call on a machine without one) and the nlZ sums are added on the host in device order instead of by RCCL (one card cannot hold two
  // ranks of a communicator).  NAGP_TEST_FAIL_DEVICE=d -- worker d reports NAGP_EHIP before it creates its plan.
  // One snapshot of the developer switches for the whole run: the workers' plans are created from it as well.
  const DevSwitches dev = read_dev_switches();
  const int fake = dev.test_fake_devices;
  const int fail_dev = dev.test_fail_device;
  ndev = fake ? fake : ndev_real;
  if (ndev < 1) FAIL(NAGP_ENODEVICE, "no HIP device visible");
  if (n_gpus > ndev) FAIL(NAGP_EINVAL, "n_gpus = %d but %d device(s) visible", n_gpus, ndev);
  const int G = std::min<int>(n_gpus, n_problems);     // a device without a problem takes no part
  const int I = opts->ep_itts;
  if (I < 1) FAIL(NAGP_EINVAL, "ep_itts < 1");
  std::vector<int32_t> dev_of(n_problems);
  (void)nagp_batch_partition(n_problems, G, dev_of.data());
  std::vector<int> status(G, NAGP_OK);
  std::vector<std::string> errs(G);
  std::vector<std::vector<double>> part(G, std::vector<double>(I, 0.0));
  auto worker = [&](int d) {
    std::vector<int> idx;
    for (int i = 0; i < n_problems; ++i) if (dev_of[i] == d) idx.push_back(i);
    std::vector<nagp_model> ms; std::vector<nagp_ihgp_tables> ts; std::vector<const double*> yv; std::vector<nagp_out> os;
    std::vector<std::vector<double>> nlz(idx.size(), std::vector<double>(I, 0.0));
    for (size_t a = 0; a < idx.size(); ++a) {
      ms.push_back(models[idx[a]]);
      if (tables) ts.push_back(tables[idx[a]]);
      yv.push_back(ys[idx[a]]);
      nagp_out o = outs[idx[a]];
      if (!o.nlZ) o.nlZ = nlz[a].data();        // the reduction needs them whether or not the caller wants them
      os.push_back(o);
    }
    nagp_opts o = *opts;
    o.device = fake ? (ndev_real > 0 ? d % ndev_real : 0) : d; o.ttau0 = nullptr; o.tnu0 = nullptr;
    bool wantPS = false;
    for (const nagp_out& q : os) wantPS = wantPS || q.PS;
    if (wantPS) o.flags |= NAGP_FLAG_WANT_PS;
    nagp_plan* p = nullptr;
    int st = NAGP_OK;
    if (d == fail_dev) { g_last_error = "injected failure (NAGP_TEST_FAIL_DEVICE)"; st = NAGP_EHIP; }
    if (st == NAGP_OK) st = plan_create(&p, (int32_t)idx.size(), ms.data(), tables ? ts.data() : nullptr, T, &o, dev);
    if (st == NAGP_OK) st = nagp_plan_upload_y(p, yv.data());
    if (st == NAGP_OK) st = nagp_plan_execute(p);
    if (st == NAGP_OK) st = nagp_plan_download(p, os.data());
    if (st == NAGP_OK)
      for (size_t a = 0; a < idx.size(); ++a)
        for (int i = 0; i < I; ++i) part[d][i] += os[a].nlZ[i];     // fixed order: ascending problem index
    if (st != NAGP_OK) errs[d] = g_last_error;                       // thread-local text of this worker
    nagp_plan_destroy(p);
    status[d] = st;
  };
  if (G == 1) {
    worker(0);
  } else {
    std::vector<std::thread> th;
    for (int d = 0; d < G; ++d) th.emplace_back(worker, d);
    for (auto& t : th) t.join();
  }
  for (int d = 0; d < G; ++d)
    if (status[d] != NAGP_OK) { g_last_error = "device " + std::to_string(d) + ": " + errs[d]; return status[d]; }
  std::vector<double> total(I, 0.0);
  if (fake && G > 1) {
    for (int d = 0; d < G; ++d) for (int i = 0; i < I; ++i) total[i] += part[d][i];
  } else if (G > 1 || dev.force_rccl) {
    const int st = allreduce_nlz(G, I, part, total);
    if (st != NAGP_OK) return st;
  } else {
    total = part[0];
  }
  if (nlZ_total) for (int i = 0; i < I; ++i) nlZ_total[i] = total[i];
  return NAGP_OK;
}

// ---------------------------------------------------------------------------------------------
// posterior reconstruction of the signal and the modulator amplitudes (see include/nagp.h, nagp_recon.hpp)
extern "C" int nagp_reconstruct(int32_t D, int32_t N, int64_t T, const double* Eft, const double* Varft, const double* Wnmf,
                                int32_t link_kind, double link_shift, int32_t n_gh, const double* gh_x, const double* gh_w,
                                int32_t n_samples, uint64_t seed, double* Esig, double* Vsig, double* Eft_mod, double* Varft_mod, int32_t device) {
  if (!Eft || !Varft || !Wnmf || !Esig || !Vsig || !Eft_mod || !Varft_mod) FAIL(NAGP_EINVAL, "null argument");
  if (D < 1 || N < 1 || N > MOM_MAXCD || D + N > MAXM || T < 1) FAIL(NAGP_EINVAL, "bad sizes (D=%d N=%d T=%lld)", D, N, (long long)T);
  if (link_kind != NAGP_LINK_SOFTPLUS && link_kind != NAGP_LINK_EXP) FAIL(NAGP_EINVAL, "unknown link");
  const bool sampling = n_samples > 0;
  if (sampling && n_samples < 2) FAIL(NAGP_EINVAL, "sampling needs at least two draws");
  if (!sampling && link_kind == NAGP_LINK_SOFTPLUS && (n_gh < 1 || n_gh > 256 || !gh_x || !gh_w)) FAIL(NAGP_EINVAL, "Gauss-Hermite rule missing");
  if (hipSetDevice(device) != hipSuccess) FAIL(NAGP_EHIP, "hipSetDevice(%d)", device);
  const int M = D + N;
  const size_t nW = (size_t)D * N, nMT = (size_t)M * T, ngh = sampling ? 0 : (size_t)std::max(n_gh, 0);
  const size_t o_W = 0, o_E = o_W + nW, o_V = o_E + nMT, o_gx = o_V + nMT, o_gw = o_gx + ngh, o_es = o_gw + ngh, o_vs = o_es + T,
               o_em = o_vs + T, o_vm = o_em + (size_t)N * T, total = o_vm + (size_t)N * T;
  double* dev = nullptr;
  if (hipMalloc(&dev, total * sizeof(double)) != hipSuccess) { (void)hipGetLastError(); FAIL(NAGP_ENOMEM, "hipMalloc(%zu)", total * sizeof(double)); }
  std::vector<double> Wr(nW);
  for (int d = 0; d < D; ++d)
    for (int j = 0; j < N; ++j) Wr[(size_t)d * N + j] = Wnmf[d + (size_t)D * j];
  int st = NAGP_OK;
  ENTRY_HIP(nagp_reconstruct, hipMemcpy(dev + o_W, Wr.data(), nW * 8, hipMemcpyHostToDevice));
  ENTRY_HIP(nagp_reconstruct, hipMemcpy(dev + o_E, Eft, nMT * 8, hipMemcpyHostToDevice));      // M x T column-major = [T][M]
  ENTRY_HIP(nagp_reconstruct, hipMemcpy(dev + o_V, Varft, nMT * 8, hipMemcpyHostToDevice));
  if (ngh) { ENTRY_HIP(nagp_reconstruct, hipMemcpy(dev + o_gx, gh_x, ngh * 8, hipMemcpyHostToDevice)); ENTRY_HIP(nagp_reconstruct, hipMemcpy(dev + o_gw, gh_w, ngh * 8, hipMemcpyHostToDevice)); }
  ReconPar rp{D, N, M, T, link_kind, link_shift, dev + o_W, dev + o_E, dev + o_V, (int)ngh, dev + o_gx, dev + o_gw, n_samples, seed,
              dev + o_es, dev + o_vs, dev + o_em, dev + o_vm};
  if (st == NAGP_OK) {
    if (sampling) {
      const unsigned grid = (unsigned)std::min<int64_t>(T, 65536);
      hipLaunchKernelGGL(recon_sample_kernel, dim3(grid), dim3(64), nW * sizeof(double), 0, rp);
    } else {
      hipLaunchKernelGGL(recon_moments_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), (nW + 2 * ngh) * sizeof(double), 0, rp);
    }
  }
  ENTRY_HIP(nagp_reconstruct, hipGetLastError());
  ENTRY_HIP(nagp_reconstruct, hipDeviceSynchronize());
  ENTRY_HIP(nagp_reconstruct, hipMemcpy(Esig, dev + o_es, (size_t)T * 8, hipMemcpyDeviceToHost));
  ENTRY_HIP(nagp_reconstruct, hipMemcpy(Vsig, dev + o_vs, (size_t)T * 8, hipMemcpyDeviceToHost));
  ENTRY_HIP(nagp_reconstruct, hipMemcpy(Eft_mod, dev + o_em, (size_t)N * T * 8, hipMemcpyDeviceToHost));
  ENTRY_HIP(nagp_reconstruct, hipMemcpy(Varft_mod, dev + o_vm, (size_t)N * T * 8, hipMemcpyDeviceToHost));
  (void)hipFree(dev);
  return st;
}

// the experiment scripts' form of the same post-processing: amplitude kind, sources, envelopes (see include/nagp.h, nagp_recon.hpp)
extern "C" int nagp_reconstruct_sources(int32_t D, int32_t N, int64_t T, const double* Eft, const double* Varft, const double* Wnmf,
                                        const nagp_recon_opts* o, nagp_recon_out* out) {
  if (!Eft || !Varft || !Wnmf || !o || !out) FAIL(NAGP_EINVAL, "null argument");
  if (D < 1 || N < 1 || N > MOM_MAXCD || D + N > MAXM || T < 1) FAIL(NAGP_EINVAL, "bad sizes (D=%d N=%d T=%lld)", D, N, (long long)T);
  if (o->amp_kind != NAGP_AMP_LINEAR && o->amp_kind != NAGP_AMP_SQRT) FAIL(NAGP_EINVAL, "unknown amplitude kind");
  if (o->link_kind != NAGP_LINK_SOFTPLUS && o->link_kind != NAGP_LINK_EXP) FAIL(NAGP_EINVAL, "unknown link");
  const int J = o->n_sources;
  if (J < 1 || J > RECON_MAXSRC || J > D) FAIL(NAGP_EINVAL, "bad number of sources (%d)", J);
  if (!o->source_offsets && J > 1) FAIL(NAGP_EINVAL, "source_offsets missing");
  int off[RECON_MAXSRC + 1] = {0};
  off[J] = D;
  if (o->source_offsets) {
    for (int j = 0; j <= J; ++j) off[j] = o->source_offsets[j];
    if (off[0] != 0 || off[J] != D) FAIL(NAGP_EINVAL, "source_offsets must start at 0 and end at D");
    for (int j = 0; j < J; ++j) if (off[j + 1] <= off[j]) FAIL(NAGP_EINVAL, "source_offsets must be strictly ascending");
  }
  if (o->n_samples < 0 || o->n_samples == 1) FAIL(NAGP_EINVAL, "sampling needs at least two draws");
  const bool sampling = o->n_samples > 0, sq = o->amp_kind == NAGP_AMP_SQRT;
  if (!sampling && o->link_kind == NAGP_LINK_SOFTPLUS && (o->n_gh < 1 || o->n_gh > 256 || !o->gh_x || !o->gh_w)) FAIL(NAGP_EINVAL, "Gauss-Hermite rule missing");
  if (!sampling && sq && (o->n_pts < 1 || o->n_pts > (1 << 20) || !o->wn || !o->xn_unscaled)) FAIL(NAGP_EINVAL, "N-dimensional rule missing");
  if (!out->Esig && !out->Vsig && !out->Esrc && !out->Vsrc && !out->Eenv && !out->Eft_mod && !out->Varft_mod) FAIL(NAGP_EINVAL, "no output wanted");
  if (hipSetDevice(o->device) != hipSuccess) FAIL(NAGP_EHIP, "hipSetDevice(%d)", o->device);
  const int M = D + N;
  const size_t nW = (size_t)D * N, nMT = (size_t)M * T, ngh = (!sampling && o->link_kind == NAGP_LINK_SOFTPLUS) ? (size_t)o->n_gh : 0,
               npt = (!sampling && sq) ? (size_t)o->n_pts : 0;
  // outputs that are not wanted get no buffer: the kernels skip a NULL pointer
  const size_t n_es = out->Esig ? T : 0, n_vs = out->Vsig ? T : 0, n_ej = out->Esrc ? (size_t)J * T : 0, n_vj = out->Vsrc ? (size_t)J * T : 0,
               n_en = out->Eenv ? (size_t)D * T : 0, n_em = out->Eft_mod ? (size_t)N * T : 0, n_vm = out->Varft_mod ? (size_t)N * T : 0;
  const size_t o_W = 0, o_E = o_W + nW, o_V = o_E + nMT, o_gx = o_V + nMT, o_gw = o_gx + ngh, o_wn = o_gw + ngh, o_xn = o_wn + npt,
               o_es = o_xn + npt * N, o_vs = o_es + n_es, o_ej = o_vs + n_vs, o_vj = o_ej + n_ej, o_en = o_vj + n_vj, o_em = o_en + n_en,
               o_vm = o_em + n_em, o_off = o_vm + n_vm, total = o_off + (RECON_MAXSRC + 2) / 2;
  double* dev = nullptr;
  if (hipMalloc(&dev, total * sizeof(double)) != hipSuccess) { (void)hipGetLastError(); FAIL(NAGP_ENOMEM, "hipMalloc(%zu)", total * sizeof(double)); }
  std::vector<double> Wr(nW);
  for (int d = 0; d < D; ++d)
    for (int j = 0; j < N; ++j) Wr[(size_t)d * N + j] = Wnmf[d + (size_t)D * j];
  int st = NAGP_OK;
  ENTRY_HIP(nagp_reconstruct_sources, hipMemcpy(dev + o_W, Wr.data(), nW * 8, hipMemcpyHostToDevice));
  ENTRY_HIP(nagp_reconstruct_sources, hipMemcpy(dev + o_E, Eft, nMT * 8, hipMemcpyHostToDevice));      // M x T column-major = [T][M]
  ENTRY_HIP(nagp_reconstruct_sources, hipMemcpy(dev + o_V, Varft, nMT * 8, hipMemcpyHostToDevice));
  ENTRY_HIP(nagp_reconstruct_sources, hipMemcpy(dev + o_off, off, sizeof off, hipMemcpyHostToDevice));
  if (ngh) { ENTRY_HIP(nagp_reconstruct_sources, hipMemcpy(dev + o_gx, o->gh_x, ngh * 8, hipMemcpyHostToDevice)); ENTRY_HIP(nagp_reconstruct_sources, hipMemcpy(dev + o_gw, o->gh_w, ngh * 8, hipMemcpyHostToDevice)); }
  if (npt) { ENTRY_HIP(nagp_reconstruct_sources, hipMemcpy(dev + o_wn, o->wn, npt * 8, hipMemcpyHostToDevice)); ENTRY_HIP(nagp_reconstruct_sources, hipMemcpy(dev + o_xn, o->xn_unscaled, npt * N * 8, hipMemcpyHostToDevice)); }
  auto buf = [&](size_t n, size_t at) -> double* { return n ? dev + at : nullptr; };
  ReconSrcPar rp{D, N, M, J, T, sq ? 1 : 0, o->link_kind, o->link_shift, dev + o_W, dev + o_E, dev + o_V, reinterpret_cast<const int*>(dev + o_off),
                 (int)ngh, dev + o_gx, dev + o_gw, (int)npt, dev + o_wn, dev + o_xn, o->n_samples, o->seed,
                 buf(n_es, o_es), buf(n_vs, o_vs), buf(n_ej, o_ej), buf(n_vj, o_vj), buf(n_en, o_en), buf(n_em, o_em), buf(n_vm, o_vm)};
  if (st == NAGP_OK) {
    const size_t ldsW = (size_t)D * MOM_MAXCD;
    if (sampling) {
      const unsigned grid = (unsigned)std::min<int64_t>(T, 65536);
      hipLaunchKernelGGL(recon_src_sample_kernel, dim3(grid), dim3(64), (ldsW + D + MOM_MAXCD + RECON_MAXSRC) * sizeof(double), 0, rp);
    } else if (sq) {
      const unsigned grid = (unsigned)std::min<int64_t>(T, 65536);
      hipLaunchKernelGGL(recon_src_pop_sqrt_kernel, dim3(grid), dim3(64), (ldsW + 2 * ngh + (size_t)D * 65) * sizeof(double), 0, rp);
    } else {
      hipLaunchKernelGGL(recon_src_moments_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), (ldsW + 2 * ngh) * sizeof(double), 0, rp);
    }
  }
  ENTRY_HIP(nagp_reconstruct_sources, hipGetLastError());
  ENTRY_HIP(nagp_reconstruct_sources, hipDeviceSynchronize());
  if (n_es) ENTRY_HIP(nagp_reconstruct_sources, hipMemcpy(out->Esig, dev + o_es, n_es * 8, hipMemcpyDeviceToHost));
  if (n_vs) ENTRY_HIP(nagp_reconstruct_sources, hipMemcpy(out->Vsig, dev + o_vs, n_vs * 8, hipMemcpyDeviceToHost));
  if (n_ej) ENTRY_HIP(nagp_reconstruct_sources, hipMemcpy(out->Esrc, dev + o_ej, n_ej * 8, hipMemcpyDeviceToHost));      // [T][J] = J x T column-major
  if (n_vj) ENTRY_HIP(nagp_reconstruct_sources, hipMemcpy(out->Vsrc, dev + o_vj, n_vj * 8, hipMemcpyDeviceToHost));
  if (n_en) ENTRY_HIP(nagp_reconstruct_sources, hipMemcpy(out->Eenv, dev + o_en, n_en * 8, hipMemcpyDeviceToHost));
  if (n_em) ENTRY_HIP(nagp_reconstruct_sources, hipMemcpy(out->Eft_mod, dev + o_em, n_em * 8, hipMemcpyDeviceToHost));
  if (n_vm) ENTRY_HIP(nagp_reconstruct_sources, hipMemcpy(out->Varft_mod, dev + o_vm, n_vm * 8, hipMemcpyDeviceToHost));
  (void)hipFree(dev);
  return st;
}

#undef ENTRY_HIP
